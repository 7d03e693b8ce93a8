// demo_tracker_io.cpp -- a co-simulation script's frame: step, read the tracked owners' state, write some of it back.  A small bed
// of three-sphere clumps over a plane; trackers on one clump, on the plane and on the whole batch of the bed.  Ten frames of
//   DoDynamicsThenSync of 30 steps,
//   every DEMTracker getter that reads pose, velocity or family (Pos, Vel, AngVelLocal, AngVelGlobal, OriQ, GetFamily and the
//   std::vector<float> twins), for every offset,
//   SetVel / SetPos / SetOriQ / SetAngVel / SetFamily on some owners, in the single and the vector forms,
// with every float printed with %a, and what the questions moved on tagged lines:
//   BATCH_GET_BYTES <frame> <n>   DEMSolver::GetOwnerQueryHostBytes over the loop over the batch tracker's offsets alone
//   TOTAL_BYTES <n>               ... over the whole run
// DEME_TRACKER_HOST=1 runs it on the paths that move the whole state (both byte lines 0); DEME_SLABS_PER_DEVICE=S decomposed.
// (tests/test_tracker_io_shell.py)
//
//   ./demo_tracker_io [frames]
#include <DEM/API.h>

#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

using namespace deme;

static void print_owner(const char* tag, int frame, size_t k, const std::shared_ptr<DEMTracker>& tr) {
    const float3 p = tr->Pos(k), v = tr->Vel(k), w = tr->AngVelLocal(k), wg = tr->AngVelGlobal(k);
    const float4 q = tr->OriQ(k);
    std::printf("%s %d %zu id=%u fam=%u pos %a %a %a vel %a %a %a w %a %a %a wg %a %a %a q %a %a %a %a\n", tag, frame, k, tr->GetOwnerID(k),
                tr->GetFamily(k), p.x, p.y, p.z, v.x, v.y, v.z, w.x, w.y, w.z, wg.x, wg.y, wg.z, q.x, q.y, q.z, q.w);
}

static void print_twins(const char* tag, int frame, const std::shared_ptr<DEMTracker>& tr) {
    std::printf("%s %d twins", tag, frame);
    for (const std::vector<float>& v : {tr->GetPos(), tr->GetVel(), tr->GetAngVelLocal(), tr->GetAngVelGlobal(), tr->GetOriQ()})
        for (float x : v)
            std::printf(" %a", x);
    std::printf("\n");
}

static int run(int frames) {
    DEMSolver DEMSim;
    DEMSim.SetVerbosity("ERROR");
    auto mat = DEMSim.LoadMaterial({{"E", 1e8f}, {"nu", 0.3f}, {"CoR", 0.4f}, {"mu", 0.3f}, {"Crr", 0.0f}});
    DEMSim.InstructBoxDomainDimension({0.f, 0.3f}, {0.f, 0.15f}, {0.f, 0.15f});
    DEMSim.InstructBoxDomainBoundingBC("top_open", mat);

    const float r = 0.004f;
    auto clump3 = DEMSim.LoadClumpType(2.6e3f * 5.5886717f, make_float3(2.928f, 2.6029f, 3.9908f) * 2.6e3f, std::vector<float>{0.8f, 0.8f, 0.8f},
                                       std::vector<float3>{{0.5f, 0.341729f, 0.f}, {0.f, -0.658271f, 0.f}, {-0.5f, 0.341729f, 0.f}}, mat);
    clump3->Scale(r);

    // two layers over a plane at z = 0.01, 12 columns along x (a decomposed run is cut along x); the singly tracked clump takes a
    // place in the middle of the bottom layer
    const float floorZ = 0.01f, sep = 3.2f * r, dz = 1.7f * r;
    const int nx = 12, ny = 3, nz = 2;
    std::vector<float3> xyz;
    float3 mid = make_float3(0, 0, 0);
    for (int k = 0; k < nz; k++)
        for (int j = 0; j < ny; j++)
            for (int i = 0; i < nx; i++) {
                const float3 p = make_float3(0.03f + sep * i + (k % 2) * 0.5f * sep, 0.03f + sep * j + (k % 2) * 0.3f * sep,
                                             floorZ + 0.85f * r + dz * k);
                if (k == 0 && j == ny / 2 && i == nx / 2)
                    mid = p;
                else
                    xyz.push_back(p);
            }
    auto bed = DEMSim.AddClumps(clump3, xyz);
    bed->SetVel(make_float3(0, 0, -0.2f));
    auto one = DEMSim.AddClumps(clump3, mid);
    one->SetVel(make_float3(0, 0, -0.2f));
    auto plane = DEMSim.AddBCPlane(make_float3(0, 0, floorZ), make_float3(0, 0, 1), mat);
    auto trackBatch = DEMSim.Track(bed);
    auto trackClump = DEMSim.Track(one);
    auto trackPlane = DEMSim.Track(plane);
    DEMSim.SetFamilyFixed(3);

    DEMSim.UseFrictionalHertzianModel();
    DEMSim.SetInitTimeStep(5e-6);
    DEMSim.SetGravitationalAcceleration(make_float3(0, 0, -9.81f));
    DEMSim.SetCDUpdateFreq(20);
    DEMSim.SetExpandSafetyAdder(0.5f);
    DEMSim.SetMaxVelocity(5.f);
    DEMSim.SetInitBinSizeAsMultipleOfSmallestSphere(4.f);
    DEMSim.Initialize();

    const size_t nb = trackBatch->GetNumOwners();
    std::printf("SLABS %u\nNBATCH %zu\n", DEMSim.GetNumSlabs(), nb);
    const uint64_t bytes0 = DEMSim.GetOwnerQueryHostBytes();
    for (int f = 0; f < frames; f++) {
        DEMSim.DoDynamicsThenSync(30 * 5e-6);
        print_owner("CLUMP", f, 0, trackClump);
        print_twins("CLUMP", f, trackClump);
        print_owner("PLANE", f, 0, trackPlane);
        const uint64_t before = DEMSim.GetOwnerQueryHostBytes();
        for (size_t k = 0; k < nb; k++)
            print_owner("BATCH", f, k, trackBatch);
        std::printf("BATCH_GET_BYTES %d %llu\n", f, (unsigned long long)(DEMSim.GetOwnerQueryHostBytes() - before));
        std::printf("FAMILIES %d", f);
        for (unsigned int fam : trackBatch->GetFamilies())
            std::printf(" %u", fam);
        std::printf("\n");

        // the single forms on the tracked clump (and on one offset of the batch)
        const float3 v = trackClump->Vel(), p = trackClump->Pos();
        trackClump->SetVel(make_float3(0.5f * v.x, 0.5f * v.y, v.z + 0.01f));
        trackClump->SetAngVel(make_float3(0.1f * (float)f, -0.2f, 0.05f));
        if (f % 3 == 1)
            trackClump->SetPos(make_float3(p.x, p.y, p.z + 1e-5f));
        if (f % 4 == 2)
            trackClump->SetOriQ(make_float4(0.f, 0.f, 0.38268343f, 0.92387953f));
        trackBatch->SetVel(make_float3(0.f, 0.01f, -0.1f), (size_t)f);
        if (f == 2)
            trackPlane->SetPos(trackPlane->Pos());
        // the vector forms on the batch: all owners, or its first half
        std::vector<float3> vel(nb), pos(nb / 2), w(nb);
        std::vector<float4> q(nb / 2);
        for (size_t k = 0; k < nb; k++) {
            const float3 vk = trackBatch->Vel(k);
            vel[k] = make_float3(0.9f * vk.x, 0.9f * vk.y, vk.z);
            w[k] = make_float3(0.f, 0.01f * (float)(k % 5), 0.f);
        }
        for (size_t k = 0; k < nb / 2; k++) {
            const float3 pk = trackBatch->Pos(k);
            pos[k] = make_float3(pk.x, pk.y + 2e-5f, pk.z);
            q[k] = make_float4(0.f, 0.f, 0.f, 1.f);
        }
        trackBatch->SetVel(vel);
        if (f % 2 == 0)
            trackBatch->SetAngVel(w);
        if (f == 3 || f == 7)
            trackBatch->SetPos(pos);
        if (f == 5)
            trackBatch->SetOriQ(q);
        if (f == 4)
            trackBatch->SetFamily(1);
        if (f == 6) {
            trackBatch->SetFamily(3, 3);  // fixed from the next step on
            trackClump->SetFamily(2);
        }
        print_owner("CLUMP_SET", f, 0, trackClump);
        print_owner("BATCH_SET", f, (size_t)f, trackBatch);
        print_owner("BATCH_SET", f, nb - 1, trackBatch);
    }
    std::printf("TOTAL_BYTES %llu\n", (unsigned long long)(DEMSim.GetOwnerQueryHostBytes() - bytes0));
    std::printf("DEMO_OK frames=%d contacts=%zu\n", frames, DEMSim.GetNumContacts());
    return 0;
}

int main(int argc, char** argv) {
    try {
        return run(argc > 1 ? std::atoi(argv[1]) : 10);
    } catch (const std::exception& e) {
        std::printf("DEMO_FAILED %s\n", e.what());
        return 1;
    }
}
