// tracker_frame_bench.cpp -- what a co-simulation frame pays for reading and writing tracked owners through the C++ shell
// ("Measured: tracker reads and writes").  A bed of n three-sphere clumps (lattice of spacing 3 r with a seeded jitter
// and random orientations, aspect 1 : 1 : 0.45, in an open-top box over a tracked plane) settles for `settle` steps; then three
// scripts run a warm-up frame and 5 timed frames each:
//   clump   DoDynamicsThenSync(1 step); tracker->Pos(); tracker->SetVel(tracker->Vel())            one clump in the middle of the bed
//   plane   the same for the plane
//   batch   a tracker of 1 000 clumps: Pos and Vel at every offset, then SetVel(vector)
// and a control loop whose frames only read (no write, so no forced detection).  The host clock is taken around the step and
// around the getter + setter part; the median of the 5 with min and max is printed in ms.  The velocities written are the ones
// read, so the bed is not disturbed.  Builds against any commit's shell:
//   g++ -std=c++17 -O2 -I include -I dem-engine_amd/host/include tools/tracker_frame_bench.cpp -L dem-engine_amd/csrc -ldeme_hip
//   ./a.out [n = 1000000] [settle = 30000]         (DEME_TRACKER_HOST=1: the whole-state paths)
#include <DEM/API.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace deme;
using Clock = std::chrono::steady_clock;

static double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

static void report(const char* script, const char* what, std::vector<double> v) {
    std::sort(v.begin(), v.end());
    std::printf("%s %s median %.3f ms (%.3f - %.3f)\n", script, what, v[v.size() / 2], v.front(), v.back());
}

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? (size_t)std::atol(argv[1]) : 1000000;
    const int settle = argc > 2 ? std::atoi(argv[2]) : 30000;
    const size_t nBatch = std::min<size_t>(1000, n / 4);
    try {
        DEMSolver DEMSim;
        DEMSim.SetVerbosity("ERROR");
        auto mat = DEMSim.LoadMaterial({{"E", 1e8f}, {"nu", 0.3f}, {"CoR", 0.6f}, {"mu", 0.2f}, {"Crr", 0.0f}});
        const float r = 0.005f, sep = 3.f * r, pad = 2.f * sep;
        const double side = std::cbrt((double)n / 0.45);  // clumps along x and y; 0.45 of that along z
        const size_t nx = (size_t)std::ceil(side), ny = nx, nz = (n + nx * ny - 1) / (nx * ny);
        DEMSim.InstructBoxDomainDimension({0.f, 2 * pad + sep * nx}, {0.f, 2 * pad + sep * ny}, {0.f, (2 * pad + sep * nz) * 1.3f});
        DEMSim.InstructBoxDomainBoundingBC("top_open", mat);
        auto clump3 = DEMSim.LoadClumpType(2.6e3f * 5.5886717f, make_float3(2.928f, 2.6029f, 3.9908f) * 2.6e3f, std::vector<float>{0.8f, 0.8f, 0.8f},
                                           std::vector<float3>{{0.5f, 0.341729f, 0.f}, {0.f, -0.658271f, 0.f}, {-0.5f, 0.341729f, 0.f}}, mat);
        clump3->Scale(r);

        uint64_t seed = 2024;
        auto rnd = [&]() {  // in [-1, 1)
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            return (float)((double)(seed >> 11) / (double)(1ull << 52) - 1.0);
        };
        std::vector<float3> rest, block;
        std::vector<float4> qRest, qBlock;
        float3 mid = make_float3(0, 0, 0);
        const size_t midAt = (nz / 2) * nx * ny + (ny / 2) * nx + nx / 2, blockFrom = midAt + 1;
        for (size_t i = 0; i < n; i++) {
            const size_t ix = i % nx, iy = (i / nx) % ny, iz = i / (nx * ny);
            const float3 p = make_float3(pad + sep * (ix + 0.5f) + 0.05f * sep * rnd(), pad + sep * (iy + 0.5f) + 0.05f * sep * rnd(),
                                         pad + sep * (iz + 0.5f) + 0.05f * sep * rnd());
            float4 q = make_float4(rnd(), rnd(), rnd(), rnd());
            const float len = std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w) + 1e-9f;
            q = make_float4(q.x / len, q.y / len, q.z / len, q.w / len);
            if (i == midAt)
                mid = p;
            else if (i >= blockFrom && i < blockFrom + nBatch)
                block.push_back(p), qBlock.push_back(q);
            else
                rest.push_back(p), qRest.push_back(q);
        }
        auto bed = DEMSim.AddClumps(clump3, rest);
        bed->SetOriQ(qRest);
        auto some = DEMSim.AddClumps(clump3, block);
        some->SetOriQ(qBlock);
        auto one = DEMSim.AddClumps(clump3, mid);
        auto plane = DEMSim.AddBCPlane(make_float3(0, 0, 0.5f * pad), make_float3(0, 0, 1), mat);
        auto trClump = DEMSim.Track(one), trPlane = DEMSim.Track(plane), trBatch = DEMSim.Track(some);

        DEMSim.UseFrictionalHertzianModel();
        DEMSim.SetInitTimeStep(5e-6);
        DEMSim.SetGravitationalAcceleration(make_float3(0, 0, -9.81f));
        DEMSim.SetCDUpdateFreq(40);
        DEMSim.SetInitBinSizeAsMultipleOfSmallestSphere(5.f);
        DEMSim.Initialize();
        auto t0 = Clock::now();
        DEMSim.DoDynamicsThenSync(settle * 5e-6);
        std::printf("BED clumps=%zu settle_steps=%d settle_s=%.1f contacts=%zu batch=%zu\n", DEMSim.GetNumClumps(), settle, ms_since(t0) / 1e3,
                    DEMSim.GetNumContacts(), trBatch->GetNumOwners());

        float sink = 0;
        for (int script = 0; script < 4; script++) {
            const char* name = script == 0 ? "clump" : script == 1 ? "plane" : script == 2 ? "batch" : "read-only";
            std::vector<double> step, io;
            const uint64_t bytes0 = DEMSim.GetOwnerQueryHostBytes();
            for (int f = 0; f < 6; f++) {
                t0 = Clock::now();
                DEMSim.DoDynamicsThenSync(5e-6);
                const double tStep = ms_since(t0);
                t0 = Clock::now();
                if (script == 0 || script == 1) {
                    auto& tr = script == 0 ? trClump : trPlane;
                    sink += tr->Pos().z;
                    tr->SetVel(tr->Vel());
                } else if (script == 2) {
                    std::vector<float3> v(trBatch->GetNumOwners());
                    for (size_t k = 0; k < v.size(); k++) {
                        sink += trBatch->Pos(k).z;
                        v[k] = trBatch->Vel(k);
                    }
                    trBatch->SetVel(v);
                } else {
                    sink += trClump->Pos().z + trClump->Vel().z;
                }
                const double tIo = ms_since(t0);
                if (f) {  // (frame 0 is the warm-up; its step follows whatever the script before wrote)
                    step.push_back(tStep), io.push_back(tIo);
                }
            }
            report(name, "step", step);
            report(name, "getters+setters", io);
            std::printf("%s bytes_per_frame %llu\n", name, (unsigned long long)((DEMSim.GetOwnerQueryHostBytes() - bytes0) / 6));
        }
        std::printf("BENCH_OK %a\n", sink);
    } catch (const std::exception& e) {
        std::printf("BENCH_FAILED %s\n", e.what());
        return 1;
    }
    return 0;
}
