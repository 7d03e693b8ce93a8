// demo_contact_inspect.cpp -- the two inspectors that look at the contact list, "clump_virial" and "clump_coordination": the bed of
// demo_contact_query.cpp (four layers of three-sphere clumps pressed onto a plane).  Once the bed carries contact forces it prints
//   SLABS <n>                          the slabs the run is decomposed into (1: one domain)
//   CUT <z>                            the region of the second pair of inspectors is "return Z < <z>;"
//   VIRIAL <all|low> <9 values>        DEMInspector("clump_virial" [, region])->GetTensor(), %a
//   COORD <all|low> <value> <sum>      DEMInspector("clump_coordination" [, region])->GetValue() (%a) and the sum of GetValues()
//   OWN_VIRIAL / OWN_COORD             the same sums computed here from GetContactDetailedInfo() (owners, forces and contact points
//                                      in the global frame) and the trackers' positions: arm = point - centre of mass, in fp64
//   OWN_ABS <all|low> <9 values> <3>   sum |arm_i| |f_j|, and sum |f_j|, over the counted sides: what the comparison's bound is made of
//   THROW_VALUE / THROW_TENSOR <msg>   GetValue() of the virial, GetTensor() of "clump_max_z"
// (tests/test_contact_inspect_shell.py; DEME_SLABS_PER_DEVICE=2 runs it decomposed)
//
//   ./demo_contact_inspect [frames]
#include <DEM/API.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

using namespace deme;

struct OwnSums {
    double w[9] = {0}, a[9] = {0}, f[3] = {0};
    unsigned long long sides = 0, clumps = 0;
};

static void print_own(const char* which, const OwnSums& s) {
    std::printf("OWN_VIRIAL %s", which);
    for (double v : s.w)
        std::printf(" %a", v);
    std::printf("\nOWN_ABS %s", which);
    for (double v : s.a)
        std::printf(" %a", v);
    for (double v : s.f)
        std::printf(" %a", v);
    std::printf("\nOWN_COORD %s %a %llu\n", which, s.clumps ? (float)((double)s.sides / (double)s.clumps) : 0.f, s.sides);
}

static void print_inspected(const char* which, const std::shared_ptr<DEMInspector>& virial, const std::shared_ptr<DEMInspector>& coord) {
    std::printf("VIRIAL %s", which);
    for (double v : virial->GetTensor())
        std::printf(" %a", v);
    double sum = 0;
    for (float v : coord->GetValues())
        sum += v;
    std::printf("\nCOORD %s %a %.0f\n", which, coord->GetValue(), sum);
}

static int run(int frames) {
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
    DEMSim.AddBCPlane(make_float3(0, 0, floorZ), make_float3(0, 0, 1), mat);
    auto track = DEMSim.Track(bed);

    DEMSim.UseFrictionalHertzianModel();
    DEMSim.SetInitTimeStep(5e-6);
    DEMSim.SetGravitationalAcceleration(make_float3(0, 0, -9.81f));
    DEMSim.SetCDUpdateFreq(20);
    DEMSim.SetExpandSafetyAdder(0.5f);
    DEMSim.SetMaxVelocity(5.f);
    DEMSim.SetInitBinSizeAsMultipleOfSmallestSphere(4.f);
    DEMSim.Initialize();

    auto virialAll = DEMSim.CreateInspector("clump_virial");
    auto coordAll = DEMSim.CreateInspector("clump_coordination");
    try {
        virialAll->GetValue();
        std::printf("NO_THROW\n");
    } catch (const std::exception& e) {
        std::printf("THROW_VALUE %s\n", e.what());
    }
    try {
        DEMSim.CreateInspector("clump_max_z")->GetTensor();
        std::printf("NO_THROW\n");
    } catch (const std::exception& e) {
        std::printf("THROW_TENSOR %s\n", e.what());
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

    // the clumps' centres; the lower region is the bottom layer: its cut lies in the middle of the widest gap among the heights
    // from the first to the third eighth (the layers above carry their contacts later, and a cut between them would count every side)
    const size_t nC = xyz.size();
    const bodyID_t first = track->GetOwnerID();
    std::vector<float3> pos(nC);
    std::vector<float> zs(nC);
    for (size_t i = 0; i < nC; i++)
        pos[i] = track->Pos(i), zs[i] = pos[i].z;
    std::sort(zs.begin(), zs.end());
    double cut = 0, gap = -1;
    for (size_t i = nC / 8; i + 1 <= 3 * nC / 8; i++)
        if ((double)zs[i + 1] - (double)zs[i] > gap)
            gap = (double)zs[i + 1] - (double)zs[i], cut = 0.5 * ((double)zs[i + 1] + (double)zs[i]);
    char region[96];
    std::snprintf(region, sizeof region, "return Z < %.17g;", cut);
    std::printf("CUT %.17g gap %.3e\n", cut, gap);
    auto virialLow = DEMSim.CreateInspector("clump_virial", region);
    auto coordLow = DEMSim.CreateInspector("clump_coordination", region);

    print_inspected("all", virialAll, coordAll);
    print_inspected("low", virialLow, coordLow);

    // the same from the contact list as a script sees it
    auto info = DEMSim.GetContactDetailedInfo();
    const auto &oA = info->GetAOwner(), &oB = info->GetBOwner();
    const auto &F = info->GetForce(), &P = info->GetPoint();
    OwnSums all, low;
    for (size_t i = 0; i < nC; i++)
        all.clumps++, low.clumps += (double)pos[i].z < cut ? 1 : 0;
    for (size_t c = 0; c < oA.size(); c++) {
        const double fx = F[c].x, fy = F[c].y, fz = F[c].z;
        if (fx * fx + fy * fy + fz * fz < (double)DEME_TINY_FLOAT_HOST * (double)DEME_TINY_FLOAT_HOST)
            continue;
        for (int side = 0; side < 2; side++) {
            const bodyID_t o = side ? oB[c] : oA[c];
            if (o < first || o >= first + nC)
                continue;  // the plane
            const float3 x = pos[o - first];
            const double sgn = side ? -1.0 : 1.0;
            const double arm[3] = {(double)P[c].x - x.x, (double)P[c].y - x.y, (double)P[c].z - x.z}, f[3] = {sgn * fx, sgn * fy, sgn * fz};
            for (OwnSums* s : {&all, &low}) {
                if (s == &low && !((double)x.z < cut))
                    continue;
                for (int i = 0; i < 3; i++)
                    for (int j = 0; j < 3; j++)
                        s->w[3 * i + j] += arm[i] * f[j], s->a[3 * i + j] += std::fabs(arm[i]) * std::fabs(f[j]);
                for (int j = 0; j < 3; j++)
                    s->f[j] += std::fabs(f[j]);
                s->sides++;
            }
        }
    }
    print_own("all", all);
    print_own("low", low);
    std::printf("DEMO_OK sides=%llu\n", all.sides);
    return 0;
}

int main(int argc, char** argv) {
    try {
        return run(argc > 1 ? std::atoi(argv[1]) : 4);
    } catch (const std::exception& e) {
        std::printf("DEMO_FAILED %s\n", e.what());
        return 1;
    }
}
