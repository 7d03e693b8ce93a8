// deme_fields.h -- per-cell sums on a regular grid, summed on the device (deme_inspect_fields and its deme_multi_ form;
// DEMFieldInspector): clumps, mass, volume, momentum and the kinetic tensor of the owners whose centre of mass lies in a cell, the
// counted sides and the virial of the contact rows those owners take part in.  The reference has no such call.
//
// The statement is in include/deme_hip.h above deme_inspect_fields.  The passes follow deme_tri_loads.h -- select, a stable sort by
// cell, a segmented scan of fixed shape:
//   k_field_cells        one thread per owner slot: cellOf[slot], the cell of a counted owner or nCells for any other, and the pair
//                        (cellOf, slot) at position slot
//   deme_radix_sort      the pairs by the key's low bits_for(nCells + 1) bits.  Stable: the slots of a cell stay ascending, the
//                        uncounted owners (key nCells) end up behind every cell
//   k_field_owner_sums   one workgroup per FIELDS_BLOCK_ROWS sorted entries: the 11 fp64 terms of the entry's owner, a segmented
//                        inclusive scan by cell in LDS.  A run closed inside the block goes straight to the cell's output, the
//                        block's first and last runs go to two partials
//   k_field_owner_final  one workgroup: the same scan over the partials, 256 at a time with the open run carried
//   k_field_side_select  one thread per row: entries 2i and 2i + 1, keyed by the cell of the side's owner if the row is counted
//                        (nCells otherwise), valued 2i + side
//   k_field_side_sums / _final   the same scan with the 9 terms of contact_side_add, recomputed from the row
// No floating-point atomics anywhere, and no workgroup waits for another inside a kernel: within a cell the owner terms are added
// slots ascending, the side terms in list order with A before B, down a tree whose shape the sorted list fixes -- two calls on one
// state give the same bits.
#pragma once
#include "deme_contact_inspect.h"

namespace deme_dev {

constexpr unsigned FIELDS_BLOCK_ROWS = 256;  // sorted entries per workgroup of the segmented sums, one a thread
constexpr int FIELD_OWNER_LANES = 11;        // mass, volume, momentum xyz, kinetic xx yy zz xy xz yz
constexpr int FIELD_SIDE_LANES = 9;          // virial, row-major

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

// the owner slots of both sides of a row, as k_contact_sums looks them up (0xFFFFFFFF: the row names something beyond the tables)
__device__ inline void field_row_owners(const QueryTables& t, uint64_t k, uint32_t& oA, uint32_t& oB) {
    const uint32_t cls = key_class(k), sa = key_a(k), sb = key_b(k);
    oA = oB = 0xFFFFFFFFu;
    if (sa < t.nSpheres)
        oA = load_sphere(t.spheres, sa).owner;
    if (cls == DEME_KEY_CLASS_SS) {
        if (sb < t.nSpheres)
            oB = load_sphere(t.spheres, sb).owner;
    } else if (cls == DEME_KEY_CLASS_SM) {
        if (sb < t.nTri)
            oB = t.tris[sb].owner;
    } else if (sb < t.nAnal) {
        oB = t.anal[sb].owner;
    }
}

__global__ __launch_bounds__(256) void k_field_side_select(const FieldSideSelectArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n)
        return;
    uint32_t kA = a.nCells, kB = a.nCells;
    const size_t r = (size_t)i * 3;
    const double fx = a.force[r], fy = a.force[r + 1], fz = a.force[r + 2];
    if (fx * fx + fy * fy + fz * fz >= a.thr2) {
        uint32_t oA, oB;
        field_row_owners(a.t, a.keys[i], oA, oB);
        if (oA < a.nSlots)
            kA = a.cellOf[oA];
        if (oB < a.nSlots)
            kB = a.cellOf[oB];
    }
    a.key[2 * i] = kA, a.val[2 * i] = 2 * i;
    a.key[2 * i + 1] = kB, a.val[2 * i + 1] = 2 * i + 1;
}

// ---- the segmented sum of L fp64 lanes and one count, by runs of equal keys ---------------------------------------------------------
// The inclusive scan of 256 entries by run of equal keys; the keys ascend, so an equal key d entries back means one run all the way.
// Step d adds the entry d back to every entry of its run: a tree of eight levels, the same for every input.  An array per lane, not
// an array of records: a wavefront's 8-byte accesses then fall on consecutive banks.  256 * (8 L + 8) bytes: 24.6 KB at L = 11.
template <int L>
struct FieldScanLds {
    double v[L][256];
    uint32_t n[256], key[256];
};
template <int L>
struct FieldPartial {  // a block's sum over its first or its last run
    double v[L];
    uint32_t key, n;  // (key >= nCells: the run of the uncounted entries, or an entry past the partials)
};

template <int L>
__device__ inline void field_seg_scan(FieldScanLds<L>& s, uint32_t t, uint32_t key, double (&v)[L], uint32_t& n) {
    s.key[t] = key, s.n[t] = n;
#pragma unroll
    for (int j = 0; j < L; j++)
        s.v[j][t] = v[j];
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const bool add = t >= d && s.key[t - d] == key;
        double av[L];
        uint32_t an = 0;
        if (add) {
#pragma unroll
            for (int j = 0; j < L; j++)
                av[j] = s.v[j][t - d];
            an = s.n[t - d];
        }
        __syncthreads();
        if (add) {
#pragma unroll
            for (int j = 0; j < L; j++) {
                v[j] = av[j] + v[j];  // (the earlier entries first)
                s.v[j][t] = v[j];
            }
            n = an + n;
            s.n[t] = n;
        }
        __syncthreads();
    }
}

template <int L>
__device__ inline FieldPartial<L> field_partial(const double (&v)[L], uint32_t key, uint32_t n) {
    FieldPartial<L> p;
#pragma unroll
    for (int j = 0; j < L; j++)
        p.v[j] = v[j];
    p.key = key, p.n = n;
    return p;
}
template <int L>
__device__ inline FieldPartial<L> field_partial_zero(uint32_t key) {
    FieldPartial<L> p;
#pragma unroll
    for (int j = 0; j < L; j++)
        p.v[j] = 0.;
    p.key = key, p.n = 0u;
    return p;
}

// One block of the first stage, after its threads have loaded their entry (key 0xFFFFFFFF and zeros past the end of the list).  Out:
// write(cell, v, n) stores a finished cell; the outputs were cleared before, so a cell without a run keeps its zeros.
template <int L, class Out>
__device__ inline void field_block_sums(FieldScanLds<L>& s, uint32_t nCells, uint32_t key, double (&v)[L], uint32_t cnt, const Out& out,
                                        FieldPartial<L>* __restrict__ partial) {
    const uint32_t t = threadIdx.x;
    field_seg_scan<L>(s, t, key, v, cnt);
    const uint32_t first = s.key[0], last = s.key[255];
    const bool runEnd = t == 255 || s.key[t + 1] != key;
    if (runEnd && key == first)
        partial[2 * blockIdx.x] = field_partial<L>(v, key, cnt);
    if (t == 255)  // (one run from end to end: its sum is in the first partial, and this one adds nothing to it)
        partial[2 * blockIdx.x + 1] = last != first ? field_partial<L>(v, key, cnt) : field_partial_zero<L>(key);
    if (runEnd && key != first && key != last && key < nCells)
        out.write(key, v, cnt);
}

// the second stage: one workgroup over the partials in workgroup order
template <int L, class Out>
__device__ inline void field_final_sums(FieldScanLds<L>& s, FieldPartial<L>& carryLds, uint32_t nPartials, uint32_t nCells,
                                        const FieldPartial<L>* __restrict__ partial, const Out& out) {
    const uint32_t t = threadIdx.x;
    FieldPartial<L> carry = field_partial_zero<L>(0xFFFFFFFFu);  // the run the round before ended with: the same in every thread
    for (uint32_t base = 0; base < nPartials; base += 256) {
        FieldPartial<L> p = field_partial_zero<L>(0xFFFFFFFFu);
        if (base + t < nPartials)
            p = partial[base + t];
        field_seg_scan<L>(s, t, p.key, p.v, p.n);
        if (s.key[0] >= nCells)  // (the partials ascend: nothing counted from here on)
            break;
        if (p.key == carry.key) {
#pragma unroll
            for (int j = 0; j < L; j++)
                p.v[j] = carry.v[j] + p.v[j];
            p.n = carry.n + p.n;
        } else if (t == 0 && carry.key < nCells) {  // the carried run ended with its round
            out.write(carry.key, carry.v, carry.n);
        }
        if (t < 255 && s.key[t + 1] != p.key && p.key < nCells)
            out.write(p.key, p.v, p.n);
        if (t == 255)
            carryLds = p;
        __syncthreads();
        carry = carryLds;
        __syncthreads();  // (the next round writes s and carryLds again)
    }
    if (t == 0 && carry.key < nCells)
        out.write(carry.key, carry.v, carry.n);
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
using FieldOwnerPartial = FieldPartial<FIELD_OWNER_LANES>;
using FieldSidePartial = FieldPartial<FIELD_SIDE_LANES>;

// keys / slots: the sorted pairs; volumes may be null (the column is then zeros and never asked)
__global__ __launch_bounds__(256) void k_field_owner_sums(uint32_t n, uint32_t nCells, const uint32_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ slots, const OwnerRec* __restrict__ owners,
                                                          const float4* __restrict__ massProps, const float* __restrict__ volumes,
                                                          const FieldOwnerOut out, FieldOwnerPartial* __restrict__ partial) {
    static_assert(FIELDS_BLOCK_ROWS == 256, "one entry a thread of a block of 256");
    __shared__ FieldScanLds<FIELD_OWNER_LANES> s;
    const uint32_t t = threadIdx.x, e = blockIdx.x * FIELDS_BLOCK_ROWS + t;
    if (keys[blockIdx.x * FIELDS_BLOCK_ROWS] >= nCells) {  // behind the counted owners (the block's first entry is one of the list)
        if (t < 2)
            partial[2 * blockIdx.x + t] = field_partial_zero<FIELD_OWNER_LANES>(0xFFFFFFFFu);
        return;
    }
    const uint32_t key = e < n ? keys[e] : 0xFFFFFFFFu;
    double v[FIELD_OWNER_LANES] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
    uint32_t cnt = 0;
    if (key < nCells) {
        const OwnerRec r = load_owner(owners, slots[e]);  // (a slot of k_field_cells: < nSlots)
        const double m = (double)massProps[r.inertiaOff].x;
        const double vx = (double)r.vx, vy = (double)r.vy, vz = (double)r.vz;
        const double px = m * vx, py = m * vy, pz = m * vz;
        v[0] = m, v[1] = volumes ? (double)volumes[r.inertiaOff] : 0.;
        v[2] = px, v[3] = py, v[4] = pz;
        v[5] = px * vx, v[6] = py * vy, v[7] = pz * vz, v[8] = px * vy, v[9] = px * vz, v[10] = py * vz;
        cnt = 1;
    }
    field_block_sums<FIELD_OWNER_LANES>(s, nCells, key, v, cnt, out, partial);
}

__global__ __launch_bounds__(256) void k_field_owner_final(uint32_t nPartials, uint32_t nCells, const FieldOwnerPartial* __restrict__ partial,
                                                           const FieldOwnerOut out) {
    __shared__ FieldScanLds<FIELD_OWNER_LANES> s;
    __shared__ FieldOwnerPartial carryLds;
    field_final_sums<FIELD_OWNER_LANES>(s, carryLds, nPartials, nCells, partial, out);
}

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

struct FieldSideSumArgs {
    uint32_t n;  // sorted entries: two a row
    uint32_t nCells, nSlots;
    const uint32_t *keys, *vals;  // the sorted pairs
    const uint64_t* list;         // the engine's list
    QueryTables t;
    const OwnerRec* owners;
    const float *force, *cpA, *cpB;  // records 0, 2, 3: 3 floats a row
    FieldSideOut out;
    FieldSidePartial* partial;
};

__global__ __launch_bounds__(256) void k_field_side_sums(const FieldSideSumArgs a) {
    __shared__ FieldScanLds<FIELD_SIDE_LANES> s;
    const uint32_t t = threadIdx.x, e = blockIdx.x * FIELDS_BLOCK_ROWS + t;
    if (a.keys[blockIdx.x * FIELDS_BLOCK_ROWS] >= a.nCells) {
        if (t < 2)
            a.partial[2 * blockIdx.x + t] = field_partial_zero<FIELD_SIDE_LANES>(0xFFFFFFFFu);
        return;
    }
    const uint32_t key = e < a.n ? a.keys[e] : 0xFFFFFFFFu;
    double v[FIELD_SIDE_LANES] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
    uint32_t cnt = 0;
    if (key < a.nCells) {
        const uint32_t val = a.vals[e], row = val >> 1;  // (an entry of k_field_side_select: row < rows of the list)
        const size_t r = (size_t)row * 3;
        const double fx = a.force[r], fy = a.force[r + 1], fz = a.force[r + 2];
        uint32_t oA, oB;
        field_row_owners(a.t, a.list[row], oA, oB);
        const uint32_t o = (val & 1u) ? oB : oA;
        if (o < a.nSlots) {  // (always: the entry's key came from cellOf[o])
            if (val & 1u)
                contact_side_add(v, a.owners, o, a.cpB + r, -fx, -fy, -fz);
            else
                contact_side_add(v, a.owners, o, a.cpA + r, fx, fy, fz);
            cnt = 1;
        }
    }
    field_block_sums<FIELD_SIDE_LANES>(s, a.nCells, key, v, cnt, a.out, a.partial);
}

__global__ __launch_bounds__(256) void k_field_side_final(uint32_t nPartials, uint32_t nCells, const FieldSidePartial* __restrict__ partial,
                                                          const FieldSideOut out) {
    __shared__ FieldScanLds<FIELD_SIDE_LANES> s;
    __shared__ FieldSidePartial carryLds;
    field_final_sums<FIELD_SIDE_LANES>(s, carryLds, nPartials, nCells, partial, out);
}

}  // namespace deme_dev
