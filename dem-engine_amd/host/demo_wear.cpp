// demo_wear.cpp -- a wear map of a sliding plate: DEMSolver::EnableMeshWearAccumulation sums, per face and over the run, the contact
// impulse, the normal impulse, the Archard sliding work |Fn| |v_slide| dt and the shear work on the device (deme_tri_wear_*).
//
// Two layers of spheres settle on a flat plate of 8 x 8 x 2 triangles.  The spheres are held in x and y by a prescribed zero velocity
// (they may move along z and spin); after the settling the plate's family is changed to one with a prescribed constant velocity VX
// along x.  Every contact then slides at VX apart from the spheres' spin, so the total sliding work over the plate is close to VX
// times the total normal impulse.  The scene is run twice, without and with the accumulation, and each run writes the mesh as VTK;
// the second run prints
//   SLABS <n>                      the slabs the run is decomposed into (1: one domain)
//   INTERVALS <sampledTime / h>    after a script of 37 + 3 + 60 steps with a sample every 10 steps
//   TOTALS <ix iy iz> <normal> <sliding> <shear> <sampledTime>   the faces' sums over the sliding phase, added in double, %a
//   HOST <normal> <sliding>        the same two integrals on the host road: after every 10 steps the whole contact list is fetched
//                                  (GetContactDetailedInfo) and every sphere-plate row adds w |f_z| and w |f_z| |u_t| in double, u the
//                                  velocity of the sphere's contact point relative to the plate from the trackers' state
//   RATIO <device> <host>          sliding / (VX * normal)
//   FORCE_Z <f_z * sampledTime> <iz>   GetContactForces' z sum on the plate at the end, times the sampled time, beside the z impulse
//   FACE <i> <area> <sliding> <depth> <pressure>   per face: DEMTracker::face_areas, GetMeshFaceSlidingWork, GetMeshFaceWearDepth(K_OVER_H),
//                                  GetMeshFaceMeanPressure
//   THROW <msg>                    GetMeshFaceSlidingWork() of the clump tracker
// (tests/test_tri_wear_shell.py; DEME_SLABS_PER_DEVICE=2 runs it decomposed)
//
//   ./demo_wear <outdir>
#include <DEM/API.h>

#include <array>
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

using namespace deme;

static const double H = 5e-6;
static const float VX = 0.5f;
static const double K_OVER_H = 1e-13;  // Archard's k / H, 1/Pa
static const unsigned EVERY = 10;

static int run(const std::string& outdir, bool with_wear) {
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
            nodes.push_back(make_float3(-0.5f * side + side * i / N, -0.5f * side + side * j / N, 0.f));
    auto at = [&](int i, int j) { return i * (N + 1) + j; };
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) {
            faces.push_back({at(i, j), at(i + 1, j), at(i + 1, j + 1)});
            faces.push_back({at(i, j), at(i + 1, j + 1), at(i, j + 1)});
        }
    auto plate = DEMSim.AddMeshObject(nodes, faces, mat);
    plate->SetInitPos(make_float3(0.1f, 0.1f, 0.05f));
    plate->SetMass(1.f);
    plate->SetMOI(make_float3(1e-2f, 1e-2f, 1e-2f));
    plate->SetFamily(10);
    DEMSim.SetFamilyFixed(10);
    DEMSim.SetFamilyPrescribedLinVel(11, std::to_string(VX), "0", "0");  // the sliding plate: ChangeFamily(10, 11) below
    DEMSim.SetFamilyPrescribedAngVel(11, "0", "0", "0");
    auto plate_tracker = DEMSim.Track(plate);

    const float r = 0.004f;
    auto ball = DEMSim.LoadSphereType(2.6e3f * 4.f / 3.f * 3.14159265f * r * r * r, r, mat);
    std::vector<float3> xyz;
    for (int k = 0; k < 2; k++)
        for (int j = 0; j < 10; j++)
            for (int i = 0; i < 10; i++)
                xyz.push_back(make_float3(0.06f + i * 0.009f + 0.0003f * ((i * 7 + j * 3 + k) % 5 - 2), 0.06f + j * 0.009f + 0.0003f * ((i + j * 5 + k * 3) % 5 - 2),
                                          0.0545f + k * 0.0085f));
    auto batch = DEMSim.AddClumps(ball, xyz);
    batch->SetVel(make_float3(0.f, 0.f, -0.1f));
    batch->SetFamily(1);
    DEMSim.SetFamilyPrescribedLinVel(1, "0", "0", "none", false);  // held in x and y; not dictated: free along z and free to spin
    auto ball_tracker = DEMSim.Track(batch);

    DEMSim.UseFrictionalHertzianModel();
    DEMSim.SetInitTimeStep(H);
    DEMSim.SetGravitationalAcceleration(make_float3(0, 0, -9.81f));
    DEMSim.SetCDUpdateFreq(10);
    DEMSim.SetExpandSafetyAdder(0.3f);
    DEMSim.SetMaxVelocity(10.f);
    DEMSim.SetInitBinSizeAsMultipleOfSmallestSphere(4.f);
    if (with_wear)
        DEMSim.EnableMeshWearAccumulation(EVERY);
    DEMSim.Initialize();

    // 37 + 3 + 60 steps: ten intervals of ten steps whatever the calls were cut into
    DEMSim.DoDynamicsThenSync(37 * H);
    DEMSim.DoDynamicsThenSync(3 * H);
    DEMSim.DoDynamicsThenSync(60 * H);
    if (with_wear)
        std::printf("SLABS %u\nINTERVALS %a\n", DEMSim.GetNumSlabs(), DEMSim.GetMeshWearSampledTime() / H);
    // the bed settles (a decomposed run moves clumps between its slabs every 1000 steps: the sample after that step is carried)
    for (int frame = 0; frame < 30; frame++)
        DEMSim.DoDynamicsThenSync(330 * H);
    if (with_wear)
        DEMSim.ResetMeshWear();
    DEMSim.ChangeFamily(10, 11);

    // the sliding phase, 1200 steps: the plate moves 3 mm.  The host road beside it: the whole list after every interval
    const bodyID_t plate_owner = plate_tracker->GetOwnerID();
    const bodyID_t first_ball = ball_tracker->GetOwnerID(0);
    double host_normal = 0, host_work = 0, host_carry = 0;
    for (int interval = 0; interval < 120; interval++) {
        DEMSim.DoDynamicsThenSync(EVERY * H);
        if (!with_wear)
            continue;
        const double w = EVERY * H + host_carry;
        std::shared_ptr<ContactInfoContainer> info;
        try {
            info = DEMSim.GetContactDetailedInfo(0.f);
        } catch (const std::exception&) {  // the step after a migration: the list is a seed, the shell carries the weight as well
            host_carry = w;
            continue;
        }
        host_carry = 0;
        const std::vector<float3> pos = ball_tracker->Positions();
        const float3 vp = plate_tracker->Vel();
        const auto &oA = info->GetAOwner(), &oB = info->GetBOwner();
        const auto &F = info->GetForce(), &P = info->GetPoint();
        for (size_t c = 0; c < oA.size(); c++) {
            if (oB[c] != plate_owner)
                continue;
            const size_t k = oA[c] - first_ball;
            const float3 v = ball_tracker->Vel(k), om = ball_tracker->AngVelGlobal(k);
            const double rx = (double)P[c].x - pos[k].x, ry = (double)P[c].y - pos[k].y, rz = (double)P[c].z - pos[k].z;
            const double ux = v.x + ((double)om.y * rz - (double)om.z * ry) - vp.x, uy = v.y + ((double)om.z * rx - (double)om.x * rz) - vp.y;
            const double fn = std::fabs((double)F[c].z);  // (the plate is flat and level: its normal is z)
            host_normal += w * fn;
            host_work += w * fn * std::sqrt(ux * ux + uy * uy);
        }
    }
    DEMSim.WriteMeshFile(outdir + (with_wear ? "/mesh_wear.vtk" : "/mesh_plain.vtk"));
    if (!with_wear)
        return 0;

    const std::vector<float3> imp = plate_tracker->GetMeshFaceImpulses();
    const std::vector<double> nrm = plate_tracker->GetMeshFaceNormalImpulses(), work = plate_tracker->GetMeshFaceSlidingWork(),
                              shear = plate_tracker->GetMeshFaceShearWork(), depth = plate_tracker->GetMeshFaceWearDepth(K_OVER_H),
                              pressure = plate_tracker->GetMeshFaceMeanPressure(), area = plate_tracker->face_areas();
    const double t = DEMSim.GetMeshWearSampledTime();
    double ix = 0, iy = 0, iz = 0, sn = 0, sw = 0, ss = 0;
    for (size_t i = 0; i < imp.size(); i++)
        ix += imp[i].x, iy += imp[i].y, iz += imp[i].z, sn += nrm[i], sw += work[i], ss += shear[i];
    std::printf("TOTALS %a %a %a %a %a %a %a\n", ix, iy, iz, sn, sw, ss, t);
    std::printf("HOST %a %a\n", host_normal, host_work);
    std::printf("RATIO %a %a\n", sw / ((double)VX * sn), host_work / ((double)VX * host_normal));
    std::vector<float3> points, forces;
    plate_tracker->GetContactForces(points, forces);
    double fz = 0;
    for (const float3& f : forces)
        fz += f.z;
    std::printf("FORCE_Z %a %a\n", fz * t, iz);
    for (size_t i = 0; i < work.size(); i++)
        std::printf("FACE %zu %a %a %a %a\n", i, area[i], work[i], depth[i], pressure[i]);
    try {
        ball_tracker->GetMeshFaceSlidingWork();
        std::printf("NO_THROW\n");
    } catch (const std::exception& e) {
        std::printf("THROW %s\n", e.what());
    }
    std::printf("DEMO_OK contacts=%zu\n", DEMSim.GetNumContacts());
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: demo_wear <outdir>\n");
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
