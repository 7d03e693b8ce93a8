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
//   k_seg_sums<3> / k_seg_final<3>   the segmented sum of deme_seg_sum.h: the term of a sorted entry is -f of its row, a finished
//                     triangle's sum goes to outF and outN
// The order of every fp64 addition is fixed by the list and the grid (deme_seg_sum.h): two calls on one state give the same bits.
#pragma once
#include "deme_query.h"
#include "deme_seg_sum.h"

namespace deme_dev {

constexpr int TRI_LANES = 3;  // the force on the triangle, xyz

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
            double fx, fy, fz;
            if (row_force_counted(a.force, i, a.thr2, fx, fy, fz))
                tri = key_b(k);
        }
    }
    a.tri[i] = tri, a.row[i] = i;
}

struct TriTerm {  // rows: the sorted row indices
    const uint32_t* rows;
    const float* force;  // record 0: 3 floats a row
    __device__ uint32_t operator()(uint32_t e, double (&v)[TRI_LANES]) const {
        const size_t r = (size_t)rows[e] * 3;  // (a row index of k_tri_select: < n)
        v[0] = -(double)force[r], v[1] = -(double)force[r + 1], v[2] = -(double)force[r + 2];
        return 1u;
    }
};
struct TriOut {  // outF: 3 doubles a triangle, outN: one count a triangle, both cleared before
    double* outF;
    uint32_t* outN;
    __device__ void write(uint32_t tri, const double (&v)[TRI_LANES], uint32_t n) const {
        outF[3 * (size_t)tri] = v[0], outF[3 * (size_t)tri + 1] = v[1], outF[3 * (size_t)tri + 2] = v[2];
        outN[tri] = n;
    }
};

}  // namespace deme_dev
