// deme_tri_wear.h -- contact impulse and sliding work of every mesh triangle, summed over the samples of a run on the device
// (deme_tri_wear_enable / _sample / _read / _reset and their deme_multi_ forms; DEMSolver::EnableMeshWearAccumulation).  The reference
// has no such call.  The statement is in include/deme_hip.h above deme_tri_wear_enable; tests/_tri_wear64.py restates it in numpy.
//
// One sample is the passes of deme_tri_loads.h with another term and another output:
//   k_tri_select      as it is (deme_tri_loads.h): the rows that count are the rows the triangle loads count
//   deme_radix_sort   the (triangle, row) pairs, stably: the rows of a triangle stay in list order
//   k_seg_sums<6, WearTerm, WearOut> / k_seg_final<6, WearOut>   the term of a sorted entry is the six lanes of its row times the
//                     sample's weight; a finished triangle's sum of the sample is ADDED to the triangle's accumulators
// Nothing comes to the host in a sample, and no floating-point atomics are used: the order of every fp64 addition is fixed by the
// list, the grid and the sequence of samples, so two runs of one sequence give the same bits.
#pragma once
#include "deme_tri_loads.h"

namespace deme_dev {

constexpr int WEAR_LANES = 6;  // impulse xyz, normal impulse, sliding work, shear work (and a uint64_t row count: 56 bytes a triangle)

using w3 = v3<double>;  // (deme_mesh.h: vcross, vdot, vadd, vsub, vscale)

struct WearOwner {  // what a row needs of an owner record, as doubles
    double qw;
    w3 u, v, w;  // (qx, qy, qz), the linear velocity, the body-frame angular velocity
};
__device__ inline WearOwner wear_owner(const OwnerRec* __restrict__ owners, uint32_t o) {
    const float4* r = reinterpret_cast<const float4*>(owners + o);
    const float4 q4 = r[1], v4 = r[2], w4 = r[3];  // qw qx qy qz | vx vy vz family | wx wy wz margin (OwnerRec bytes 16-63)
    return {(double)q4.x, {(double)q4.y, (double)q4.z, (double)q4.w}, {(double)v4.x, (double)v4.y, (double)v4.z},
            {(double)w4.x, (double)w4.y, (double)w4.z}};
}
// R(q)v of contact_side_add (deme_contact_inspect.h), the stored quaternion as it stands
__device__ inline w3 wear_rotate(double qw, w3 u, w3 v) {
    const w3 t = vcross(u, v), s = vcross(u, t);
    return {v.x + (2.0 * qw) * t.x + 2.0 * s.x, v.y + (2.0 * qw) * t.y + 2.0 * s.y, v.z + (2.0 * qw) * t.z + 2.0 * s.z};
}
// the velocity of the material point of an owner that sits at the owner-local contact point cp: v + (R w) x (R cp)
__device__ inline w3 wear_point_velocity(const WearOwner& o, const float* __restrict__ cp) {
    const w3 r = wear_rotate(o.qw, o.u, {(double)cp[0], (double)cp[1], (double)cp[2]});
    const w3 w = wear_rotate(o.qw, o.u, o.w), c = vcross(w, r);
    return {o.v.x + c.x, o.v.y + c.y, o.v.z + c.z};
}

// The six lanes of sorted entry e.  Its key is a triangle id, so k_tri_select counted its row: a sphere-mesh row, B < nTri, A <
// nSpheres, A's owner a valid slot.  Every index is checked against its count all the same, as row_owners does; a row whose
// triangle names an owner beyond the table (deme_upload_scene refuses such a scene) adds its impulse and zeros to lanes 3 to 5.
struct WearTerm {
    const uint32_t* rows;  // the sorted row indices
    uint32_t n;            // rows of the list
    const uint64_t* keys;  // the engine's list
    QueryTables t;
    const OwnerRec* owners;
    const float *force, *cpA, *cpB;  // records 0, 2, 3: 3 floats a row
    double weight;
    __device__ uint32_t operator()(uint32_t e, double (&v)[WEAR_LANES]) const {
        const uint32_t i = rows[e];
        if (i >= n)
            return 0u;
        const size_t r = (size_t)i * 3;
        const w3 g{-(double)force[r], -(double)force[r + 1], -(double)force[r + 2]};  // the force ON the triangle
        v[0] = weight * g.x, v[1] = weight * g.y, v[2] = weight * g.z;
        const uint64_t k = keys[i];
        uint32_t oA, oB;
        row_owners(t, k, oA, oB);
        const uint32_t tri = key_b(k);
        if (key_class(k) != DEME_KEY_CLASS_SM || tri >= t.nTri || oA >= t.nOwners || oB >= t.nOwners)
            return 1u;
        const TriRec T = t.tris[tri];
        const WearOwner B = wear_owner(owners, oB);
        const w3 e1{(double)T.n2[0] - (double)T.n1[0], (double)T.n2[1] - (double)T.n1[1], (double)T.n2[2] - (double)T.n1[2]};
        const w3 e2{(double)T.n3[0] - (double)T.n1[0], (double)T.n3[1] - (double)T.n1[1], (double)T.n3[2] - (double)T.n1[2]};
        const w3 N = wear_rotate(B.qw, B.u, vcross(e1, e2));
        const double NN = vdot(N, N);
        if (!(NN > 0.0))  // a degenerate face (or a NaN node) has no normal
            return 1u;
        const double len = sqrt(NN);
        const w3 nh{N.x / len, N.y / len, N.z / len};
        const w3 vA = wear_point_velocity(wear_owner(owners, oA), cpA + r), vB = wear_point_velocity(B, cpB + r);
        const w3 u{vA.x - vB.x, vA.y - vB.y, vA.z - vB.z};
        const double Fn = vdot(g, nh), un = vdot(u, nh);
        const w3 gt{g.x - Fn * nh.x, g.y - Fn * nh.y, g.z - Fn * nh.z};
        const w3 ut{u.x - un * nh.x, u.y - un * nh.y, u.z - un * nh.z};
        const double slide = sqrt(vdot(ut, ut));
        v[3] = weight * fabs(Fn);
        v[4] = weight * (fabs(Fn) * slide);
        v[5] = weight * (sqrt(vdot(gt, gt)) * slide);
        return 1u;
    }
};

// The first Out that accumulates: acc and rows hold the sums of the samples before and are NOT cleared, write adds one sample's sum
// of a triangle to them with a plain load, add and store.  That is safe because seg_block_sums and seg_final_sums call write for a
// key from exactly one thread per launch pair: a run that neither starts with a block's first entry nor ends with its last is
// closed inside that block (one thread, the run's last entry), every other run goes to the partials and is finished by the one
// workgroup of the final pass (thread 0 for a carried run, the run's last partial otherwise) -- never both, since a run closed in a
// block writes no partial.  The keys ascend, so no two runs share a key.  The final pass follows the block pass on one stream, and
// a sample follows the sample before on that stream: the order of the additions onto a triangle is the order of the samples.
struct WearOut {
    double* acc;     // 6 doubles a triangle
    uint64_t* rows;  // one count a triangle
    __device__ void write(uint32_t tri, const double (&v)[WEAR_LANES], uint32_t n) const {
        double* a = acc + WEAR_LANES * (size_t)tri;
#pragma unroll
        for (int j = 0; j < WEAR_LANES; j++)
            a[j] += v[j];
        rows[tri] += n;
    }
};

// deme_tri_wear_read: the asked columns of triangles [first, first + n) packed column by column into one buffer, so that only what
// was asked for crosses to the host, in one copy.  A null column is not asked for.
struct WearGatherArgs {
    uint32_t first, n;
    const double* acc;
    const uint64_t* rows;
    double *impulse, *normalImpulse, *slidingWork, *shearWork;  // [3 n], [n], [n], [n]
    uint64_t* outRows;                                          // [n]
};
__global__ __launch_bounds__(256) void k_tri_wear_gather(const WearGatherArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n)
        return;
    const double* s = a.acc + WEAR_LANES * ((size_t)a.first + i);
    if (a.impulse)
        a.impulse[3 * (size_t)i] = s[0], a.impulse[3 * (size_t)i + 1] = s[1], a.impulse[3 * (size_t)i + 2] = s[2];
    if (a.normalImpulse)
        a.normalImpulse[i] = s[3];
    if (a.slidingWork)
        a.slidingWork[i] = s[4];
    if (a.shearWork)
        a.shearWork[i] = s[5];
    if (a.outRows)
        a.outRows[i] = a.rows[(size_t)a.first + i];
}

}  // namespace deme_dev
