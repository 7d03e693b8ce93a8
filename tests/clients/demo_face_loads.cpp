// demo_face_loads.cpp -- the contact load per face of a mesh: spheres dropped onto two fixed meshes, a small lid of 2 triangles
// (loaded first) lying a little above the middle of a plate of 8 x 8 x 2 triangles (loaded second, so its faces do not begin at
// triangle 0).  The scene is run twice, without and with DEMSolver::EnableMeshFaceLoadOutput(), and each run writes the meshes as
// VTK; the second prints, for <mesh> = lid and plate,
//   SLABS <n>                             the slabs the run is decomposed into (1: one domain)
//   FACES <mesh> <n> <n> <n>              entries of the three getters below
//   FACE_SUM <mesh> <x y z>               DEMTracker::GetMeshFaceForces() summed over the faces in double, %a
//   COUNT_SUM <mesh> <n> <loaded>         DEMTracker::GetMeshFaceContactCounts() summed, and the faces with a count > 0
//   OWNER_SUM <mesh> <x y z> <abs> <rows> DEMTracker::GetContactForces() of the mesh (the forces ON it) summed in double, sum of |f_j|
//                                         over all components, and the number of rows
//   PRESSURE <mesh> <min> <max> <finite>  of DEMTracker::GetMeshFacePressures()
//   THROW <msg>                           GetMeshFaceForces() of the clump tracker
// (tests/test_tri_loads_shell.py; DEME_SLABS_PER_DEVICE=2 runs it decomposed)
//
//   ./demo_face_loads <outdir>
#include <DEM/API.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

using namespace deme;

static int run(const std::string& outdir, bool with_loads) {
    DEMSolver DEMSim;
    DEMSim.SetVerbosity("ERROR");
    auto mat = DEMSim.LoadMaterial({{"E", 1e8f}, {"nu", 0.3f}, {"CoR", 0.4f}, {"mu", 0.3f}, {"Crr", 0.0f}});
    DEMSim.InstructBoxDomainDimension({0.f, 0.2f}, {0.f, 0.2f}, {0.f, 0.3f});
    DEMSim.InstructBoxDomainBoundingBC("top_open", mat);

    const int N = 8;
    const float side = 0.14f;
    std::vector<float3> nodes;
    std::vector<std::array<int, 3>> faces;
    for (int i = 0; i <= N; i++)
        for (int j = 0; j <= N; j++)
            nodes.push_back(make_float3(-0.5f * side + side * i / N, -0.5f * side + side * j / N, 0.002f * std::sin(40.f * i / N) * std::cos(30.f * j / N)));
    auto at = [&](int i, int j) { return i * (N + 1) + j; };
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) {
            faces.push_back({at(i, j), at(i + 1, j), at(i + 1, j + 1)});
            faces.push_back({at(i, j), at(i + 1, j + 1), at(i, j + 1)});
        }
    // the lid: two triangles, 3 cm square, 3.2 mm above the plate's mean height (the plate's relief is 2 mm)
    const float lh = 0.015f;
    auto lid = DEMSim.AddMeshObject({{-lh, -lh, 0.f}, {lh, -lh, 0.f}, {lh, lh, 0.f}, {-lh, lh, 0.f}}, {{0, 1, 2}, {0, 2, 3}}, mat);
    lid->SetInitPos(make_float3(0.1f, 0.1f, 0.0532f));
    lid->SetMass(1.f);
    lid->SetMOI(make_float3(1e-2f, 1e-2f, 1e-2f));
    lid->SetFamily(10);
    auto lid_tracker = DEMSim.Track(lid);
    auto plate = DEMSim.AddMeshObject(nodes, faces, mat);
    plate->SetInitPos(make_float3(0.1f, 0.1f, 0.05f));
    plate->SetMass(1.f);
    plate->SetMOI(make_float3(1e-2f, 1e-2f, 1e-2f));
    plate->SetFamily(10);
    DEMSim.SetFamilyFixed(10);
    auto plate_tracker = DEMSim.Track(plate);

    const float r = 0.004f;
    auto ball = DEMSim.LoadSphereType(2.6e3f * 4.f / 3.f * 3.14159265f * r * r * r, r, mat);
    std::vector<float3> xyz;
    for (int k = 0; k < 4; k++)
        for (int j = 0; j < 12; j++)
            for (int i = 0; i < 12; i++)
                xyz.push_back(make_float3(0.05f + i * 0.009f + 0.0003f * ((i * 7 + j * 3 + k) % 5 - 2), 0.05f + j * 0.009f + 0.0003f * ((i + j * 5 + k * 3) % 5 - 2),
                                          0.058f + k * 0.009f));
    auto batch = DEMSim.AddClumps(ball, xyz);
    batch->SetVel(make_float3(0.f, 0.f, -0.3f));
    auto ball_tracker = DEMSim.Track(batch);

    DEMSim.UseFrictionalHertzianModel();
    DEMSim.SetInitTimeStep(5e-6);
    DEMSim.SetGravitationalAcceleration(make_float3(0, 0, -9.81f));
    DEMSim.SetCDUpdateFreq(10);
    DEMSim.SetExpandSafetyAdder(0.3f);
    DEMSim.SetMaxVelocity(10.f);
    DEMSim.SetInitBinSizeAsMultipleOfSmallestSphere(4.f);
    if (with_loads)
        DEMSim.EnableMeshFaceLoadOutput();
    DEMSim.Initialize();

    // a fixed number of frames of 330 steps (both runs must end in the same state; a decomposed run moves clumps between its slabs
    // every 1000 steps and has no per-contact records until the step after): the lowest layer reaches the plate after some 3000
    // steps, and after 0.1 s the four layers have stopped bouncing and lie on it
    for (int frame = 0; frame < 60; frame++)
        DEMSim.DoDynamicsThenSync(330 * 5e-6);
    DEMSim.WriteMeshFile(outdir + (with_loads ? "/meshes_loads.vtk" : "/meshes_plain.vtk"));
    if (!with_loads)
        return 0;

    std::printf("SLABS %u\n", DEMSim.GetNumSlabs());
    const char* names[2] = {"lid", "plate"};
    std::shared_ptr<DEMTracker> trackers[2] = {lid_tracker, plate_tracker};
    for (int m = 0; m < 2; m++) {
        const char* name = names[m];
        auto& tracker = trackers[m];
        const std::vector<float3> ff = tracker->GetMeshFaceForces();
        const std::vector<unsigned int> fc = tracker->GetMeshFaceContactCounts();
        const std::vector<float> fp = tracker->GetMeshFacePressures();
        std::printf("FACES %s %zu %zu %zu\n", name, ff.size(), fc.size(), fp.size());
        double sx = 0, sy = 0, sz = 0;
        for (const float3& f : ff)
            sx += f.x, sy += f.y, sz += f.z;
        std::printf("FACE_SUM %s %a %a %a\n", name, sx, sy, sz);
        unsigned long long cs = 0, loaded = 0;
        for (unsigned int c : fc)
            cs += c, loaded += c > 0;
        std::printf("COUNT_SUM %s %llu %llu\n", name, cs, loaded);
        std::vector<float3> points, forces;
        const size_t rows = tracker->GetContactForces(points, forces);
        double ox = 0, oy = 0, oz = 0, oabs = 0;
        for (const float3& f : forces)
            ox += f.x, oy += f.y, oz += f.z, oabs += std::fabs((double)f.x) + std::fabs((double)f.y) + std::fabs((double)f.z);
        std::printf("OWNER_SUM %s %a %a %a %a %zu\n", name, ox, oy, oz, oabs, rows);
        float pmin = 1e30f, pmax = -1e30f;
        int finite = 1;
        for (float p : fp)
            pmin = std::min(pmin, p), pmax = std::max(pmax, p), finite &= std::isfinite(p) ? 1 : 0;
        std::printf("PRESSURE %s %a %a %d\n", name, pmin, pmax, finite);
    }
    try {
        ball_tracker->GetMeshFaceForces();
        std::printf("NO_THROW\n");
    } catch (const std::exception& e) {
        std::printf("THROW %s\n", e.what());
    }
    std::printf("DEMO_OK contacts=%zu\n", DEMSim.GetNumContacts());
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: demo_face_loads <outdir>\n");
        return 2;
    }
    try {
        if (int rc = run(argv[1], false))
            return rc;
        return run(argv[1], true);
    } catch (const std::exception& e) {
        std::printf("DEMO_FAILED %s\n", e.what());
        return 1;
    }
}
