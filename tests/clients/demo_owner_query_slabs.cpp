// demo_owner_query_slabs.cpp -- the contact questions a script asks about single owners, on a DECOMPOSED run: a bed of three-sphere
// clumps, long in x, pressed onto a plane and cut into slabs along x (DEME_SLABS_PER_DEVICE, default 2); the tracked clump sits in
// the bottom layer right behind the first cut, so its neighbours are clumps of two slabs; a tracker on the plane, which every slab
// keeps a replica of.  Prints, once settled contacts exist, what demo_contact_query prints --
//   PAIRS a:b ...            DEMSolver::GetClumpContacts, owner pairs of the whole list
//   CLUMP <id> : ...         DEMSolver::GetOwnerContactClumps of the tracked clump
//   PLANE <id> : ...         ... of the plane
//   TRACKER_PLANE : ...      DEMTracker::GetContactClumps of the plane's tracker
//   TRACKER_CLUMP : ...      ... of the clump's tracker
//   SLABS <n>                the slabs the run is decomposed into
//   FORCES <who> <flavour> <count> <sums>   GetContactForces / ...AndGlobalTorque / ...AndLocalTorque of both trackers: the
//                            number of pairs and the running fp32 sums of points, forces and torques, printed with %a
// -- and what the clump's questions moved:
//   LIST_BYTES <n>           56 bytes (key and records) for every listed contact: what one whole-list answer brings to the host
//   CLUMP_BYTES <n>          DEMSolver::GetOwnerQueryHostBytes over the clump's questions alone (0 on the whole-list path)
// (tests/test_owner_query_shell_slabs.py; DEME_QUERY_HOST=1 runs it on the whole-list path)
//
//   ./demo_owner_query_slabs [frames]
#include <DEM/API.h>

#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

using namespace deme;

static float3 sum_of(const std::vector<float3>& v) {
    float3 s = make_float3(0, 0, 0);
    for (const float3& x : v)
        s = s + x;
    return s;
}

static void print_ids(const char* tag, const std::vector<bodyID_t>& ids) {
    std::printf("%s :", tag);
    for (bodyID_t i : ids)
        std::printf(" %u", i);
    std::printf("\n");
}

static size_t print_forces(const char* who, const std::shared_ptr<DEMTracker>& tr) {
    std::vector<float3> p, f, t;
    const size_t n = tr->GetContactForces(p, f);
    float3 sp = sum_of(p), sf = sum_of(f);
    std::printf("FORCES %s plain %zu %a %a %a %a %a %a\n", who, n, sp.x, sp.y, sp.z, sf.x, sf.y, sf.z);
    for (int local = 0; local < 2; local++) {
        const size_t m = local ? tr->GetContactForcesAndLocalTorque(p, f, t) : tr->GetContactForcesAndGlobalTorque(p, f, t);
        sp = sum_of(p), sf = sum_of(f);
        const float3 st = sum_of(t);
        std::printf("FORCES %s %s %zu %a %a %a %a %a %a %a %a %a\n", who, local ? "local" : "global", m, sp.x, sp.y, sp.z, sf.x, sf.y,
                    sf.z, st.x, st.y, st.z);
    }
    return n;
}

static int run(int frames) {
    DEMSolver DEMSim;
    DEMSim.SetVerbosity("ERROR");
    const char* env = std::getenv("DEME_SLABS_PER_DEVICE");
    const int slabs = env && std::atoi(env) > 1 ? std::atoi(env) : 2;
    if (!env)
        DEMSim.SetSlabsPerDevice(2);
    auto mat = DEMSim.LoadMaterial({{"E", 1e8f}, {"nu", 0.3f}, {"CoR", 0.4f}, {"mu", 0.3f}, {"Crr", 0.0f}});
    DEMSim.InstructBoxDomainDimension({0.f, 0.3f}, {0.f, 0.15f}, {0.f, 0.15f});
    DEMSim.InstructBoxDomainBoundingBC("top_open", mat);

    const float r = 0.004f;  // sphere radius 0.8 r, the clump flat in its own xy plane
    auto clump3 = DEMSim.LoadClumpType(2.6e3f * 5.5886717f, make_float3(2.928f, 2.6029f, 3.9908f) * 2.6e3f, std::vector<float>{0.8f, 0.8f, 0.8f},
                                       std::vector<float3>{{0.5f, 0.341729f, 0.f}, {0.f, -0.658271f, 0.f}, {-0.5f, 0.341729f, 0.f}}, mat);
    clump3->Scale(r);

    // three layers a hair apart over a plane at z = 0.01, the layers shifted against each other, 18 columns along x: the slabs are
    // cut along x with as many clumps each, so the first cut falls in front of column nx / slabs; the tracked clump takes the place
    // of the bottom layer's clump of that column
    const float floorZ = 0.01f, sep = 3.2f * r, dz = 1.7f * r;
    const int nx = 18, ny = 6, nz = 3;
    std::vector<float3> xyz;
    float3 mid = make_float3(0, 0, 0);
    for (int k = 0; k < nz; k++)
        for (int j = 0; j < ny; j++)
            for (int i = 0; i < nx; i++) {
                const float3 p = make_float3(0.03f + sep * i + (k % 2) * 0.5f * sep, 0.03f + sep * j + (k % 2) * 0.3f * sep,
                                             floorZ + 0.85f * r + dz * k);
                if (k == 0 && j == ny / 2 && i == nx / slabs)
                    mid = p;
                else
                    xyz.push_back(p);
            }
    auto bed = DEMSim.AddClumps(clump3, xyz);
    bed->SetVel(make_float3(0, 0, -0.2f));
    auto one = DEMSim.AddClumps(clump3, mid);
    one->SetVel(make_float3(0, 0, -0.2f));
    auto plane = DEMSim.AddBCPlane(make_float3(0, 0, floorZ), make_float3(0, 0, 1), mat);
    auto trackClump = DEMSim.Track(one);
    auto trackPlane = DEMSim.Track(plane);

    DEMSim.UseFrictionalHertzianModel();
    DEMSim.SetInitTimeStep(5e-6);
    DEMSim.SetGravitationalAcceleration(make_float3(0, 0, -9.81f));
    DEMSim.SetCDUpdateFreq(20);
    DEMSim.SetExpandSafetyAdder(0.5f);
    DEMSim.SetMaxVelocity(5.f);
    DEMSim.SetInitBinSizeAsMultipleOfSmallestSphere(4.f);
    DEMSim.Initialize();

    const bodyID_t clumpID = trackClump->GetOwnerID(), planeID = trackPlane->GetOwnerID();
    try {
        DEMSim.GetOwnerContactClumps((bodyID_t)(DEMSim.GetNumClumps() + 1000));
        std::printf("NO_THROW\n");
    } catch (const std::exception& e) {
        std::printf("THROW_OUT_OF_RANGE %s\n", e.what());
    }

    // until both the clump and the plane carry contact forces at the end of a frame (at least `frames` frames of 330 steps: the
    // run moves clumps between its slabs every 1000 steps and has no per-contact records until the step after)
    std::vector<float3> p, f;
    int done = 0;
    for (; done < 40; done++) {
        DEMSim.DoDynamicsThenSync(330 * 5e-6);
        if (done + 1 >= frames && trackClump->GetContactForces(p, f) > 0 && trackPlane->GetContactForces(p, f) > 0) {
            done++;
            break;
        }
    }
    std::printf("FRAMES %d contacts=%zu\n", done, DEMSim.GetNumContacts());
    std::printf("SLABS %u\n", DEMSim.GetNumSlabs());

    std::printf("PAIRS");
    for (auto& pr : DEMSim.GetClumpContacts())
        std::printf(" %u:%u", pr.first, pr.second);
    std::printf("\n");
    char tag[64];
    std::snprintf(tag, sizeof tag, "PLANE %u", planeID);
    print_ids(tag, DEMSim.GetOwnerContactClumps(planeID));
    print_ids("TRACKER_PLANE", trackPlane->GetContactClumps());
    const size_t np = print_forces("plane", trackPlane);
    const uint64_t before = DEMSim.GetOwnerQueryHostBytes();
    std::snprintf(tag, sizeof tag, "CLUMP %u", clumpID);
    print_ids(tag, DEMSim.GetOwnerContactClumps(clumpID));
    print_ids("TRACKER_CLUMP", trackClump->GetContactClumps());
    const size_t nc = print_forces("clump", trackClump);
    const uint64_t moved = DEMSim.GetOwnerQueryHostBytes() - before;
    std::printf("LIST_BYTES %zu\n", (size_t)56 * DEMSim.GetNumContacts());
    std::printf("CLUMP_BYTES %llu\n", (unsigned long long)moved);
    std::printf("DEMO_OK clump_pairs=%zu plane_pairs=%zu\n", nc, np);
    return 0;
}

int main(int argc, char** argv) {
    try {
        return run(argc > 1 ? std::atoi(argv[1]) : 9);
    } catch (const std::exception& e) {
        std::printf("DEMO_FAILED %s\n", e.what());
        return 1;
    }
}
