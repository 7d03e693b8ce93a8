// deme_fields.h -- per-cell sums on a regular grid, summed on the device (deme_inspect_fields and its deme_multi_ form;
// DEMFieldInspector): clumps, mass, volume, momentum and the kinetic tensor of the owners whose centre of mass lies in a cell, the
// counted sides and the virial of the contact rows those owners take part in.  The reference has no such call.
//
// The statement is in include/deme_hip.h above deme_inspect_fields.  The passes follow deme_tri_loads.h -- select, a stable sort by
// cell, the segmented sum of deme_seg_sum.h:
//   k_field_cells        one thread per owner slot: cellOf[slot], the cell of a counted owner or nCells for any other, and the pair
//                        (cellOf, slot) at position slot
//   deme_radix_sort      the pairs by the key's low bits_for(nCells + 1) bits.  Stable: the slots of a cell stay ascending, the
//                        uncounted owners (key nCells) end up behind every cell
//   k_seg_sums<11> / k_seg_final<11>   FieldOwnerTerm: the 11 fp64 terms of the entry's owner; FieldOwnerOut: the owner columns
//   k_field_side_select  one thread per row: entries 2i and 2i + 1, keyed by the cell of the side's owner if the row is counted
//                        (nCells otherwise), valued 2i + side
//   k_seg_sums<9> / k_seg_final<9>     FieldSideTerm: the 9 terms of contact_side_add, recomputed from the row; FieldSideOut
// Within a cell the owner terms are added slots ascending, the side terms in list order with A before B, down a tree whose shape
// the sorted list fixes (deme_seg_sum.h) -- two calls on one state give the same bits.
#pragma once
#include "deme_contact_inspect.h"
#include "deme_seg_sum.h"

namespace deme_dev {

constexpr int FIELD_OWNER_LANES = 11;  // mass, volume, momentum xyz, kinetic xx yy zz xy xz yz
constexpr int FIELD_SIDE_LANES = 9;    // virial, row-major

struct FieldGridDev {  // DemeFieldGrid of deme_hip.h
    double origin[3], cell[3];
    uint32_t n[3];
};

struct FieldCellArgs {
    uint32_t nSlots, nClumps, nCells;
    const OwnerRec* owners;
    FieldGridDev g;
    uint32_t *cellOf, *key, *slot;  // [nSlots]
};

// the cell of a world-frame point: false outside the grid (a NaN is outside)
__device__ inline bool field_cell_of(const FieldGridDev& g, double X, double Y, double Z, uint32_t& cell) {
    const double ux = (X - g.origin[0]) / g.cell[0], uy = (Y - g.origin[1]) / g.cell[1], uz = (Z - g.origin[2]) / g.cell[2];
    if (!(ux >= 0.0 && ux < (double)g.n[0] && uy >= 0.0 && uy < (double)g.n[1] && uz >= 0.0 && uz < (double)g.n[2]))
        return false;
    cell = (uint32_t)ux + g.n[0] * ((uint32_t)uy + g.n[1] * (uint32_t)uz);
    return true;
}

__global__ __launch_bounds__(256) void k_field_cells(const DevParams p, const FieldCellArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nSlots)
        return;
    uint32_t cell = a.nCells;
    const uint32_t id = p.o2e ? p.o2e[i] : i;  // clumps are the caller's first nClumps owners (k_contact_owner_mask)
    const OwnerRec r = load_owner(a.owners, i);
    if (id < a.nClumps && !ghost_of(r.family)) {
        const d3 P = decode_pos(r.voxelID, r.locX, r.locY, r.locZ, p);
        uint32_t c;
        if (field_cell_of(a.g, P.x + (double)p.LBFX, P.y + (double)p.LBFY, P.z + (double)p.LBFZ, c))
            cell = c;
    }
    a.cellOf[i] = cell, a.key[i] = cell, a.slot[i] = i;
}

struct FieldSideSelectArgs {
    uint32_t n;            // rows of the list
    uint32_t nSlots, nCells;
    const uint64_t* keys;  // the engine's list
    QueryTables t;
    const uint32_t* cellOf;  // per owner slot
    const float* force;      // record 0: 3 floats a row
    double thr2;
    uint32_t *key, *val;  // [2n]
};

__global__ __launch_bounds__(256) void k_field_side_select(const FieldSideSelectArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n)
        return;
    uint32_t kA = a.nCells, kB = a.nCells;
    double fx, fy, fz;
    if (row_force_counted(a.force, i, a.thr2, fx, fy, fz)) {
        uint32_t oA, oB;
        row_owners(a.t, a.keys[i], oA, oB);
        if (oA < a.nSlots)
            kA = a.cellOf[oA];
        if (oB < a.nSlots)
            kB = a.cellOf[oB];
    }
    a.key[2 * i] = kA, a.val[2 * i] = 2 * i;
    a.key[2 * i + 1] = kB, a.val[2 * i + 1] = 2 * i + 1;
}

// ---- owner columns ------------------------------------------------------------------------------------------------------------------
struct FieldOwnerOut {  // nCells entries (times 3 / 6) each
    uint32_t* clumps;
    double *mass, *volume, *momentum, *kinetic;
    __device__ void write(uint32_t cell, const double (&v)[FIELD_OWNER_LANES], uint32_t n) const {
        clumps[cell] = n, mass[cell] = v[0], volume[cell] = v[1];
        for (int j = 0; j < 3; j++)
            momentum[3 * (size_t)cell + j] = v[2 + j];
        for (int j = 0; j < 6; j++)
            kinetic[6 * (size_t)cell + j] = v[5 + j];
    }
};

struct FieldOwnerTerm {  // slots: the sorted owner slots; volumes may be null (the column is then zeros and never asked)
    const uint32_t* slots;
    const OwnerRec* owners;
    const float4* massProps;
    const float* volumes;
    __device__ uint32_t operator()(uint32_t e, double (&v)[FIELD_OWNER_LANES]) const {
        const OwnerRec r = load_owner(owners, slots[e]);  // (a slot of k_field_cells: < nSlots)
        const double m = (double)massProps[r.inertiaOff].x;
        const double vx = (double)r.vx, vy = (double)r.vy, vz = (double)r.vz;
        const double px = m * vx, py = m * vy, pz = m * vz;
        v[0] = m, v[1] = volumes ? (double)volumes[r.inertiaOff] : 0.;
        v[2] = px, v[3] = py, v[4] = pz;
        v[5] = px * vx, v[6] = py * vy, v[7] = pz * vz, v[8] = px * vy, v[9] = px * vz, v[10] = py * vz;
        return 1u;
    }
};

// ---- contact columns ----------------------------------------------------------------------------------------------------------------
struct FieldSideOut {
    uint32_t* sides;
    double* virial;  // 9 a cell, row-major
    __device__ void write(uint32_t cell, const double (&v)[FIELD_SIDE_LANES], uint32_t n) const {
        sides[cell] = n;
        for (int j = 0; j < 9; j++)
            virial[9 * (size_t)cell + j] = v[j];
    }
};

struct FieldSideTerm {  // two sorted entries a row: vals[e] = 2 row + side
    uint32_t nSlots;
    const uint32_t* vals;
    const uint64_t* list;  // the engine's list
    QueryTables t;
    const OwnerRec* owners;
    const float *force, *cpA, *cpB;  // records 0, 2, 3: 3 floats a row
    __device__ uint32_t operator()(uint32_t e, double (&v)[FIELD_SIDE_LANES]) const {
        const uint32_t val = vals[e], row = val >> 1;  // (an entry of k_field_side_select: row < rows of the list)
        const size_t r = (size_t)row * 3;
        const double fx = force[r], fy = force[r + 1], fz = force[r + 2];
        uint32_t oA, oB;
        row_owners(t, list[row], oA, oB);
        const uint32_t o = (val & 1u) ? oB : oA;
        if (o >= nSlots)  // (never: the entry's key came from cellOf[o])
            return 0u;
        if (val & 1u)
            contact_side_add(v, owners, o, cpB + r, -fx, -fy, -fz);
        else
            contact_side_add(v, owners, o, cpA + r, fx, fy, fz);
        return 1u;
    }
};

}  // namespace deme_dev
