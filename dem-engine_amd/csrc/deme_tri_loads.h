// deme_tri_loads.h -- the contact load of every mesh triangle, summed on the device (deme_inspect_tri_loads and its deme_multi_ form;
// DEMTracker::GetMeshFaceForces / GetMeshFaceContactCounts / GetMeshFacePressures).  The reference has no such call.
//
// A row of the current list is COUNTED when it is a sphere-mesh row (DEME_KEY_CLASS_SM) whose B is a triangle id < nTri, sphere
// A's owner is no ghost copy, and its recorded force f (record 0) has (double)fx^2 + (double)fy^2 + (double)fz^2 >= (double)thr^2
// -- the test k_contact_sums makes.  A counted row adds -f (the force ON the triangle, world frame) to its triangle in fp64, and 1
// to the triangle's count.
//   k_tri_select      one thread per row: the pair (triangle id, row index) of a counted row, (nTri, row index) of any other --
//                     slot i of the pair list belongs to row i, so nothing depends on which workgroup ran first
//   deme_radix_sort   the pairs by the key's low bits_for(nTri + 1) bits.  The sort is stable: the rows of a triangle stay in list
//                     order and the uncounted rows (key nTri, past every triangle) end up behind them.  The whole list is sorted,
//                     so the number of counted rows never has to come to the host
//   k_tri_seg_sums    one workgroup per BLOCK_ROWS sorted entries: a segmented inclusive scan by triangle, a tree of fixed shape
//                     in LDS (no thread walks a run alone).  A run that neither starts with the block's first entry nor ends with
//                     its last is closed inside the block and goes straight to the triangle's output; the block's first and last
//                     runs go to two partials
//   k_tri_seg_final   one workgroup: the same scan over the partials in workgroup order, 256 at a time with the open run carried
//                     from one round to the next; it ends at the first round that begins behind the counted rows
// No floating-point atomics anywhere, and no workgroup waits for another inside a kernel: the order of every fp64 addition is fixed
// by the list and the grid, so two calls on one state give the same bits.
#pragma once
#include "deme_query.h"

namespace deme_dev {

constexpr unsigned TRI_LOADS_BLOCK_ROWS = 256;  // sorted entries per workgroup of k_tri_seg_sums, one a thread

struct TriPartial {  // a block's sum over its first or its last run
    double x, y, z;
    uint32_t tri, n;  // (tri >= nTri: the run of the uncounted rows, or an entry past the partials)
};
static_assert(sizeof(TriPartial) == 32, "TriPartial is 32 bytes");

struct TriSelectArgs {
    uint32_t n;            // rows of the list
    const uint64_t* keys;  // the engine's list
    const SphereRec* spheres;
    const OwnerRec* owners;
    uint32_t nSpheres, nOwners, nTri;
    const float* force;  // record 0: 3 floats a row
    double thr2;
    uint32_t *tri, *row;  // [n]: the pairs
};

__global__ __launch_bounds__(256) void k_tri_select(const TriSelectArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n)
        return;
    uint32_t tri = a.nTri;
    const uint64_t k = a.keys[i];
    if (key_class(k) == DEME_KEY_CLASS_SM && key_b(k) < a.nTri && key_a(k) < a.nSpheres) {
        const uint32_t o = load_sphere(a.spheres, key_a(k)).owner;
        if (o < a.nOwners && !ghost_of(a.owners[o].family)) {
            const size_t r = (size_t)i * 3;
            const double fx = a.force[r], fy = a.force[r + 1], fz = a.force[r + 2];
            if (fx * fx + fy * fy + fz * fz >= a.thr2)
                tri = key_b(k);
        }
    }
    a.tri[i] = tri, a.row[i] = i;
}

// The inclusive scan of 256 (value, count) entries by run of equal keys; the keys ascend, so an equal key d entries back means one
// run all the way.  Step d adds the entry d back to every entry of its run: a tree of eight levels, the same for every input.  Four
// arrays, not one of records: a wavefront's 8-byte accesses then fall on consecutive banks.
struct TriScanLds {
    double x[256], y[256], z[256];
    uint32_t n[256], tri[256];
};
__device__ inline void tri_seg_scan(TriScanLds& s, uint32_t t, uint32_t tri, double& x, double& y, double& z, uint32_t& n) {
    s.tri[t] = tri, s.x[t] = x, s.y[t] = y, s.z[t] = z, s.n[t] = n;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const bool add = t >= d && s.tri[t - d] == tri;
        double ax = 0., ay = 0., az = 0.;
        uint32_t an = 0;
        if (add)
            ax = s.x[t - d], ay = s.y[t - d], az = s.z[t - d], an = s.n[t - d];
        __syncthreads();
        if (add) {
            x = ax + x, y = ay + y, z = az + z, n = an + n;  // (the earlier rows first)
            s.x[t] = x, s.y[t] = y, s.z[t] = z, s.n[t] = n;
        }
        __syncthreads();
    }
}

// outF: 3 doubles a triangle, outN: one count a triangle, both cleared before; partial: 2 a block
__global__ __launch_bounds__(256) void k_tri_seg_sums(uint32_t n, uint32_t nTri, const uint32_t* __restrict__ tris,
                                                      const uint32_t* __restrict__ rows, const float* __restrict__ force,
                                                      double* __restrict__ outF, uint32_t* __restrict__ outN,
                                                      TriPartial* __restrict__ partial) {
    static_assert(TRI_LOADS_BLOCK_ROWS == 256, "one entry a thread of a block of 256");
    __shared__ TriScanLds s;
    const uint32_t t = threadIdx.x, e = blockIdx.x * TRI_LOADS_BLOCK_ROWS + t;
    if (tris[blockIdx.x * TRI_LOADS_BLOCK_ROWS] >= nTri) {  // behind the counted rows (the block's first entry is one of the list)
        if (t < 2)
            partial[2 * blockIdx.x + t] = TriPartial{0., 0., 0., 0xFFFFFFFFu, 0u};
        return;
    }
    const uint32_t tri = e < n ? tris[e] : 0xFFFFFFFFu;
    double x = 0., y = 0., z = 0.;
    uint32_t cnt = 0;
    if (tri < nTri) {
        const size_t r = (size_t)rows[e] * 3;  // (a row index of k_tri_select: < n)
        x = -(double)force[r], y = -(double)force[r + 1], z = -(double)force[r + 2], cnt = 1;
    }
    tri_seg_scan(s, t, tri, x, y, z, cnt);
    const uint32_t first = s.tri[0], last = s.tri[255];
    const bool runEnd = t == 255 || s.tri[t + 1] != tri;
    if (runEnd && tri == first)
        partial[2 * blockIdx.x] = TriPartial{x, y, z, tri, cnt};
    if (t == 255)  // (one run from end to end: its sum is in the first partial, and this one adds nothing to it)
        partial[2 * blockIdx.x + 1] = last != first ? TriPartial{x, y, z, tri, cnt} : TriPartial{0., 0., 0., tri, 0u};
    if (runEnd && tri != first && tri != last && tri < nTri) {
        outF[3 * (size_t)tri] = x, outF[3 * (size_t)tri + 1] = y, outF[3 * (size_t)tri + 2] = z;
        outN[tri] = cnt;
    }
}

__global__ __launch_bounds__(256) void k_tri_seg_final(uint32_t nPartials, uint32_t nTri, const TriPartial* __restrict__ partial,
                                                       double* __restrict__ outF, uint32_t* __restrict__ outN) {
    __shared__ TriScanLds s;
    __shared__ TriPartial carryLds;
    const uint32_t t = threadIdx.x;
    TriPartial carry{0., 0., 0., 0xFFFFFFFFu, 0u};  // the run the round before ended with: the same in every thread
    for (uint32_t base = 0; base < nPartials; base += 256) {
        TriPartial p{0., 0., 0., 0xFFFFFFFFu, 0u};
        if (base + t < nPartials)
            p = partial[base + t];
        tri_seg_scan(s, t, p.tri, p.x, p.y, p.z, p.n);
        const uint32_t first = s.tri[0];
        if (first >= nTri)  // (the partials ascend: nothing counted from here on)
            break;
        if (p.tri == carry.tri)
            p.x = carry.x + p.x, p.y = carry.y + p.y, p.z = carry.z + p.z, p.n = carry.n + p.n;
        else if (t == 0 && carry.tri < nTri) {  // the carried run ended with its round
            outF[3 * (size_t)carry.tri] = carry.x, outF[3 * (size_t)carry.tri + 1] = carry.y, outF[3 * (size_t)carry.tri + 2] = carry.z;
            outN[carry.tri] = carry.n;
        }
        if (t < 255 && s.tri[t + 1] != p.tri && p.tri < nTri) {
            outF[3 * (size_t)p.tri] = p.x, outF[3 * (size_t)p.tri + 1] = p.y, outF[3 * (size_t)p.tri + 2] = p.z;
            outN[p.tri] = p.n;
        }
        if (t == 255)
            carryLds = p;
        __syncthreads();
        carry = carryLds;
        __syncthreads();  // (the next round writes s and carryLds again)
    }
    if (t == 0 && carry.tri < nTri) {
        outF[3 * (size_t)carry.tri] = carry.x, outF[3 * (size_t)carry.tri + 1] = carry.y, outF[3 * (size_t)carry.tri + 2] = carry.z;
        outN[carry.tri] = carry.n;
    }
}

}  // namespace deme_dev
