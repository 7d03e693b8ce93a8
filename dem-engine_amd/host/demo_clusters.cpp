// demo_clusters.cpp -- which clumps are joined to which (DEMSolver::CreateClusterInspector): four layers of three-sphere clumps
// settling on a plane and one clump hanging far above them, the connected components of the contact network at the shell's
// threshold and at a threshold in the middle of the clump-clump forces, the table's totals beside GetNumClumps() and the "clump_mass"
// inspector, and the table as a CSV file.  It prints
//   SLABS <n>                          the slabs the run is decomposed into (1: one domain)
//   MIDDLE_FORCE <f> gap=<ratio> of <n> clump-clump contacts   the second threshold and the gap of the forces it lies in
//   THR <t> CLUSTERS <n> SINGLETONS <n> LARGEST <n> LARGEST_LABEL <id> EDGES <n>    once per threshold
//   SIZES <t> <n ints>                 the clusters' sizes, labels ascending
//   LABELS <t> <n ints>                the owners' labels
//   TABLE <t> size=<sum of sizes> mass=<sum of masses, %a> clumps=<GetNumClumps()> clump_mass=<%a>
//   CENTRE <x y z of the largest cluster at the shell's threshold>
// (tests/test_clusters_shell.py; DEME_SLABS_PER_DEVICE=2 runs it decomposed)
//
//   ./demo_clusters [out.csv] [frames]
#include <DEM/API.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

using namespace deme;

static int run(const std::string& csv, int frames) {
    DEMSolver DEMSim;
    DEMSim.SetVerbosity("ERROR");
    auto mat = DEMSim.LoadMaterial({{"E", 1e8f}, {"nu", 0.3f}, {"CoR", 0.4f}, {"mu", 0.3f}, {"Crr", 0.0f}});
    DEMSim.InstructBoxDomainDimension({0.f, 0.2f}, {0.f, 0.2f}, {0.f, 0.2f});
    DEMSim.InstructBoxDomainBoundingBC("top_open", mat);

    const float r = 0.004f;
    auto clump3 = DEMSim.LoadClumpType(2.6e3f * 5.5886717f, make_float3(2.928f, 2.6029f, 3.9908f) * 2.6e3f, std::vector<float>{0.8f, 0.8f, 0.8f},
                                       std::vector<float3>{{0.5f, 0.341729f, 0.f}, {0.f, -0.658271f, 0.f}, {-0.5f, 0.341729f, 0.f}}, mat);
    clump3->Scale(r);

    const float floorZ = 0.01f, sep = 3.2f * r, dz = 1.7f * r;
    const int nx = 9, ny = 9, nz = 4;
    std::vector<float3> xyz;
    for (int k = 0; k < nz; k++)
        for (int j = 0; j < ny; j++)
            for (int i = 0; i < nx; i++)
                xyz.push_back(make_float3(0.03f + sep * i + (k % 2) * 0.5f * sep, 0.03f + sep * j + (k % 2) * 0.3f * sep, floorZ + 0.85f * r + dz * k));
    auto bed = DEMSim.AddClumps(clump3, xyz);
    bed->SetVel(make_float3(0, 0, -0.2f));
    // a clump of a fixed family far above the bed: the rattler no contact ever reaches
    auto lone = DEMSim.AddClumps(clump3, std::vector<float3>{make_float3(0.1f, 0.1f, 0.18f)});
    lone->SetFamily(1);
    DEMSim.SetFamilyFixed(1);
    DEMSim.AddBCPlane(make_float3(0, 0, floorZ), make_float3(0, 0, 1), mat);

    DEMSim.UseFrictionalHertzianModel();
    DEMSim.SetInitTimeStep(5e-6);
    DEMSim.SetGravitationalAcceleration(make_float3(0, 0, -9.81f));
    DEMSim.SetCDUpdateFreq(20);
    DEMSim.SetExpandSafetyAdder(0.5f);
    DEMSim.SetMaxVelocity(5.f);
    DEMSim.SetInitBinSizeAsMultipleOfSmallestSphere(4.f);
    DEMSim.Initialize();

    auto massAll = DEMSim.CreateInspector("clump_mass");
    auto coordAll = DEMSim.CreateInspector("clump_coordination");
    auto clusters = DEMSim.CreateClusterInspector();
    try {
        clusters->GetNumClusters();
        std::printf("NO_THROW\n");
    } catch (const std::exception& e) {
        std::printf("THROW_BEFORE_UPDATE %s\n", e.what());
    }

    // until the bed carries contact forces at the end of a frame (at least `frames` frames of 330 steps: a decomposed run moves
    // clumps between its slabs every 1000 steps and has no per-contact records until the step after)
    int done = 0;
    for (; done < 40; done++) {
        DEMSim.DoDynamicsThenSync(330 * 5e-6);
        if (done + 1 >= frames && coordAll->GetValue() > 0.5f) {
            done++;
            break;
        }
    }
    std::printf("FRAMES %d contacts=%zu\n", done, DEMSim.GetNumContacts());
    std::printf("SLABS %u\n", DEMSim.GetNumSlabs());

    // the second threshold: in the middle of the widest gap among the central third of the sorted clump-clump forces, from the
    // contact list as a script sees it -- about half of the edges go, the bed falls into smaller pieces, and no force lies so
    // close to the threshold that the last digit of a force decides
    const size_t nClumps = DEMSim.GetNumClumps();
    auto info = DEMSim.GetContactDetailedInfo();
    const auto &oA = info->GetAOwner(), &oB = info->GetBOwner();
    const auto& F = info->GetForce();
    std::vector<float> forces;
    for (size_t c = 0; c < oA.size(); c++)
        if (oA[c] < nClumps && oB[c] < nClumps && oA[c] != oB[c])
            forces.push_back(std::sqrt(F[c].x * F[c].x + F[c].y * F[c].y + F[c].z * F[c].z));
    std::sort(forces.begin(), forces.end());
    float middle = 1.f, gap = 1.f;
    for (size_t k = forces.size() / 3; k + 1 < forces.size() && k < 2 * forces.size() / 3; k++)
        if (forces[k] > 0.f && forces[k + 1] / forces[k] > gap)
            gap = forces[k + 1] / forces[k], middle = std::sqrt(forces[k] * forces[k + 1]);
    std::printf("MIDDLE_FORCE %.9g gap=%.6g of %zu clump-clump contacts\n", middle, gap, forces.size());
    const float thresholds[2] = {DEME_TINY_FLOAT_HOST, middle};
    for (int t = 0; t < 2; t++) {
        clusters->Update(thresholds[t]);
        std::printf("THR %d CLUSTERS %zu SINGLETONS %zu LARGEST %zu LARGEST_LABEL %u EDGES %zu\n", t, clusters->GetNumClusters(),
                    clusters->GetNumSingletons(), clusters->GetLargestClusterSize(), (unsigned)clusters->GetLargestClusterLabel(),
                    clusters->GetNumEdges());
        unsigned long long totalSize = 0;
        double totalMass = 0;
        std::printf("SIZES %d", t);
        for (uint32_t n : clusters->GetClusterSizes())
            std::printf(" %u", n), totalSize += n;
        std::printf("\nLABELS %d", t);
        for (uint32_t l : clusters->GetOwnerLabels())
            std::printf(" %u", l);
        for (double m : clusters->GetClusterMasses())
            totalMass += m;
        std::printf("\nTABLE %d size=%llu mass=%a clumps=%zu clump_mass=%a\n", t, totalSize, totalMass, DEMSim.GetNumClumps(),
                    (double)massAll->GetValue());
        if (t == 0) {
            const auto& labels = clusters->GetClusterLabels();
            const auto& centres = clusters->GetClusterCentres();
            for (size_t k = 0; k < labels.size(); k++)
                if (labels[k] == clusters->GetLargestClusterLabel())
                    std::printf("CENTRE %.9g %.9g %.9g\n", centres[3 * k], centres[3 * k + 1], centres[3 * k + 2]);
            clusters->WriteCsv(csv);
            std::printf("CSV %s\n", csv.c_str());
        }
    }
    std::printf("DEMO_OK\n");
    return 0;
}

int main(int argc, char** argv) {
    try {
        return run(argc > 1 ? argv[1] : "clusters.csv", argc > 2 ? std::atoi(argv[2]) : 4);
    } catch (const std::exception& e) {
        std::printf("DEMO_FAILED %s\n", e.what());
        return 1;
    }
}
