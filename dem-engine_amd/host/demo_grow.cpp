// demo_grow.cpp -- radius-expansion packing through the C++ shell: a loose lattice of three-sphere clumps settles in a box while
// ChangeClumpSizes grows every clump a little every few hundred steps (the reference's call sequence for growth and swelling).
// A second, small batch is resized through its tracker; clumps added with UpdateClumps afterwards join at template size while
// the grown ones keep their geometry.
//
//   ./demo_grow <rounds> <outdir>
//     writes <outdir>/spheres_grown.csv after the growth rounds, <outdir>/spheres_updated.csv after UpdateClumps and
//     <outdir>/spheres_resorted.csv after ResortClumps; DEME_SLABS_PER_DEVICE / DEME_SLAB_HALO run it decomposed
#include <DEM/API.h>

#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

using namespace deme;

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: demo_grow rounds outdir\n");
        return 2;
    }
    const int rounds = std::atoi(argv[1]);
    const std::string dir = argv[2];

    DEMSolver DEMSim;
    DEMSim.SetVerbosity("ERROR");
    auto mat = DEMSim.LoadMaterial({{"E", 1e8f}, {"nu", 0.3f}, {"CoR", 0.6f}, {"mu", 0.2f}, {"Crr", 0.0f}});
    DEMSim.InstructBoxDomainDimension({0.f, 0.2f}, {0.f, 0.2f}, {0.f, 0.2f});
    DEMSim.InstructBoxDomainBoundingBC("top_open", mat);

    const float r = 0.004f;
    auto clump3 = DEMSim.LoadClumpType(2.6e3f * 5.5886717f, make_float3(2.928f, 2.6029f, 3.9908f) * 2.6e3f, std::vector<float>{0.8f, 0.8f, 0.8f},
                                       std::vector<float3>{{0.5f, 0.341729f, 0.f}, {0.f, -0.658271f, 0.f}, {-0.5f, 0.341729f, 0.f}}, mat);
    clump3->Scale(r);

    std::vector<float3> xyz;
    const float sep = 4.f * r;
    for (int k = 0; k < 6; k++)
        for (int j = 0; j < 10; j++)
            for (int i = 0; i < 10; i++)
                xyz.push_back(make_float3(0.02f + sep * i + (k % 2) * 0.5f * sep, 0.02f + sep * j, 0.01f + sep * k));
    auto bed = DEMSim.AddClumps(clump3, xyz);
    auto few = DEMSim.AddClumps(clump3, std::vector<float3>{{0.1f, 0.1f, 0.15f}, {0.14f, 0.1f, 0.15f}});
    auto trackBed = DEMSim.Track(bed);
    auto trackFew = DEMSim.Track(few);

    DEMSim.UseFrictionalHertzianModel();
    DEMSim.SetInitTimeStep(5e-6);
    DEMSim.SetGravitationalAcceleration(make_float3(0, 0, -9.81f));
    DEMSim.SetCDUpdateFreq(20);
    DEMSim.SetExpandSafetyAdder(0.5f);
    DEMSim.SetMaxVelocity(5.f);
    DEMSim.SetInitBinSizeAsMultipleOfSmallestSphere(4.f);

    try {  // the engine's arrays exist only after Initialize (API.h:1047)
        DEMSim.ChangeClumpSizes({0}, {1.1f});
        std::printf("NO_THROW\n");
    } catch (const std::exception& e) {
        std::printf("THROW_BEFORE_INIT %s\n", e.what());
    }
    DEMSim.Initialize();

    const float grow = 1.02f;
    for (int round = 0; round < rounds; round++) {
        DEMSim.DoDynamics(200 * 5e-6);
        std::vector<bodyID_t> ids(bed->GetNumClumps());
        for (size_t i = 0; i < ids.size(); i++)
            ids[i] = trackBed->GetOwnerID(i);
        DEMSim.ChangeClumpSizes(ids, std::vector<float>(ids.size(), grow));
        std::printf("round %d contacts=%zu\n", round, DEMSim.GetNumContacts());
    }
    trackFew->ChangeClumpSizes({1}, {1.5f});  // the second clump of the small batch only
    DEMSim.DoDynamicsThenSync(100 * 5e-6);
    DEMSim.WriteSphereFile(dir + "/spheres_grown.csv");

    DEMSim.AddClumps(clump3, std::vector<float3>{{0.1f, 0.1f, 0.18f}});
    DEMSim.UpdateClumps();
    DEMSim.DoDynamicsThenSync(100 * 5e-6);
    DEMSim.WriteSphereFile(dir + "/spheres_updated.csv");
    DEMSim.ResortClumps();
    DEMSim.WriteSphereFile(dir + "/spheres_resorted.csv");
    std::printf("DEMO_OK clumps=%zu contacts=%zu\n", DEMSim.GetNumClumps(), DEMSim.GetNumContacts());
    return 0;
}
