// demo_fields.cpp -- fields on a grid, cell by cell (DEMSolver::CreateFieldInspector): four layers of three-sphere clumps settling
// on a plane, one Update() of a 4 x 4 x 4 grid over the whole box once the bed carries contact forces, the totals of its columns
// beside what the inspectors of the bed as a whole give, and the grid as a VTK file.  It prints
//   SLABS <n>                          the slabs the run is decomposed into (1: one domain)
//   GRID <nx> <ny> <nz> cells=<n>
//   CELL_CLUMPS / CELL_SIDES <n ints>  the two integer columns, cell by cell
//   CELL_VIRIAL <9 n values>           arm (x) force per cell, %a
//   TOTAL_CLUMPS <n> TOTAL_SIDES <n>
//   MASS <sum over cells> <clump_mass>                                  %a
//   VIRIAL_CELLS / VIRIAL_INSPECTOR <9 values>                          the cells' sum and "clump_virial", %a
//   COORD <total sides / total clumps> <clump_coordination> <its sides> %a
//   OWN_ABS <9 values>                 sum |arm_i| |f_j| over the counted sides, from GetContactDetailedInfo(): what the bound of
//                                      the comparison of the two tensors is made of
//   FIELDS max solid fraction, max granular temperature, min contact stress zz
// (tests/test_fields_shell.py; DEME_SLABS_PER_DEVICE=2 runs it decomposed)
//
//   ./demo_fields [out.vtk] [frames]
#include <DEM/API.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

using namespace deme;

static int run(const std::string& vtk, int frames) {
    DEMSolver DEMSim;
    DEMSim.SetVerbosity("ERROR");
    auto mat = DEMSim.LoadMaterial({{"E", 1e8f}, {"nu", 0.3f}, {"CoR", 0.4f}, {"mu", 0.3f}, {"Crr", 0.0f}});
    DEMSim.InstructBoxDomainDimension({0.f, 0.2f}, {0.f, 0.2f}, {0.f, 0.2f});
    DEMSim.InstructBoxDomainBoundingBC("top_open", mat);

    const float r = 0.004f;
    auto clump3 = DEMSim.LoadClumpType(2.6e3f * 5.5886717f, make_float3(2.928f, 2.6029f, 3.9908f) * 2.6e3f, std::vector<float>{0.8f, 0.8f, 0.8f},
                                       std::vector<float3>{{0.5f, 0.341729f, 0.f}, {0.f, -0.658271f, 0.f}, {-0.5f, 0.341729f, 0.f}}, mat);
    clump3->Scale(r);
    clump3->SetVolume(5.5886717f * r * r * r);

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

    auto massAll = DEMSim.CreateInspector("clump_mass");
    auto virialAll = DEMSim.CreateInspector("clump_virial");
    auto coordAll = DEMSim.CreateInspector("clump_coordination");
    // the bed sits in the lower corner of the box: cells of 2.5 cm over it, the upper ones empty
    const unsigned gx = 4, gy = 4, gz = 4;
    auto fields = DEMSim.CreateFieldInspector(make_float3(0.f, 0.f, 0.f), make_float3(0.05f, 0.05f, 0.025f), gx, gy, gz);
    try {
        fields->GetMass();
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

    fields->Update();
    const size_t nCells = fields->GetNumCells();
    std::printf("GRID %u %u %u cells=%zu\n", gx, gy, gz, nCells);
    const auto& clumps = fields->GetClumpCounts();
    const auto& sides = fields->GetContactSideCounts();
    const auto& mass = fields->GetMass();
    const auto& virial = fields->GetVirial();
    unsigned long long totalClumps = 0, totalSides = 0;
    double totalMass = 0, totalVirial[9] = {0};
    std::printf("CELL_CLUMPS");
    for (size_t c = 0; c < nCells; c++)
        std::printf(" %u", clumps[c]), totalClumps += clumps[c];
    std::printf("\nCELL_SIDES");
    for (size_t c = 0; c < nCells; c++)
        std::printf(" %u", sides[c]), totalSides += sides[c];
    std::printf("\nCELL_VIRIAL");
    for (size_t c = 0; c < nCells; c++) {
        totalMass += mass[c];
        for (int k = 0; k < 9; k++)
            std::printf(" %a", virial[9 * c + k]), totalVirial[k] += virial[9 * c + k];
    }
    std::printf("\nTOTAL_CLUMPS %llu TOTAL_SIDES %llu\n", totalClumps, totalSides);
    std::printf("MASS %a %a\n", totalMass, (double)massAll->GetValue());
    std::printf("VIRIAL_CELLS");
    for (double v : totalVirial)
        std::printf(" %a", v);
    std::printf("\nVIRIAL_INSPECTOR");
    for (double v : virialAll->GetTensor())
        std::printf(" %a", v);
    double inspectorSides = 0;
    for (float v : coordAll->GetValues())
        inspectorSides += v;
    std::printf("\nCOORD %a %a %.0f\n", totalClumps ? (float)((double)totalSides / (double)totalClumps) : 0.f, coordAll->GetValue(), inspectorSides);

    // sum |arm_i| |f_j| over the counted sides, from the contact list as a script sees it
    const size_t nC = xyz.size();
    const bodyID_t first = track->GetOwnerID();
    auto info = DEMSim.GetContactDetailedInfo();
    const auto &oA = info->GetAOwner(), &oB = info->GetBOwner();
    const auto &F = info->GetForce(), &P = info->GetPoint();
    double absSum[9] = {0};
    for (size_t c = 0; c < oA.size(); c++) {
        const double f[3] = {F[c].x, F[c].y, F[c].z};
        if (f[0] * f[0] + f[1] * f[1] + f[2] * f[2] < (double)DEME_TINY_FLOAT_HOST * (double)DEME_TINY_FLOAT_HOST)
            continue;
        for (int side = 0; side < 2; side++) {
            const bodyID_t o = side ? oB[c] : oA[c];
            if (o < first || o >= first + nC)
                continue;  // the plane
            const float3 x = track->Pos(o - first);
            const double arm[3] = {(double)P[c].x - x.x, (double)P[c].y - x.y, (double)P[c].z - x.z};
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++)
                    absSum[3 * i + j] += std::fabs(arm[i]) * std::fabs(f[j]);
        }
    }
    std::printf("OWN_ABS");
    for (double v : absSum)
        std::printf(" %a", v);

    const auto phi = fields->GetSolidFraction(), temp = fields->GetGranularTemperature(), stress = fields->GetContactStress();
    const auto vel = fields->GetMeanVelocity(), coord = fields->GetCoordination(), kin = fields->GetKineticStress();
    double phiMax = 0, tempMax = 0, zzMin = 0;
    bool finite = true;
    for (size_t c = 0; c < nCells; c++) {
        phiMax = std::max(phiMax, phi[c]), tempMax = std::max(tempMax, temp[c]), zzMin = std::min(zzMin, stress[9 * c + 8]);
        finite = finite && std::isfinite(phi[c]) && std::isfinite(temp[c]) && std::isfinite(coord[c]);
        for (int k = 0; k < 3; k++)
            finite = finite && std::isfinite(vel[3 * c + k]);
        for (int k = 0; k < 6; k++)
            finite = finite && std::isfinite(kin[6 * c + k]);
    }
    std::printf("\nFIELDS phi_max=%.6g temperature_max=%.6g contact_zz_min=%.6g finite=%d\n", phiMax, tempMax, zzMin, finite ? 1 : 0);
    fields->WriteVtk(vtk);
    std::printf("VTK %s\n", vtk.c_str());
    std::printf("DEMO_OK sides=%llu\n", totalSides);
    return 0;
}

int main(int argc, char** argv) {
    try {
        return run(argc > 1 ? argv[1] : "fields.vtk", argc > 2 ? std::atoi(argv[2]) : 4);
    } catch (const std::exception& e) {
        std::printf("DEMO_FAILED %s\n", e.what());
        return 1;
    }
}
