// deme_contact_inspect.h -- bulk numbers of the contact list, summed on the device (deme_inspect_contacts, deme_inspect_contact_counts
// and their deme_multi_ forms; DEMInspector "clump_virial" / "clump_coordination").  The reference has no such inspector.
//
// A row of the current list is COUNTED when its recorded force f (record 0) has (double)fx^2 + (double)fy^2 + (double)fz^2 >=
// (double)thr^2.  A SIDE of a counted row is counted when its owner is an own (non-ghost) clump inside the region; side A carries
// +f and cpA, side B -f and cpB.  A counted side adds r (x) f to the virial, r = R(q) cp with the owner's stored quaternion, all
// in fp64:  R(q)v = v + 2w(u x v) + 2u x (u x v), u = (qx, qy, qz).
//   k_contact_owner_mask   1.0f per owner slot that is an own clump, 0.0f otherwise; the compiled region filter
//                          (deme_region_filter, perSphere == 0, identity 0) then clears the slots outside the region
//   k_contact_sums<false>  one thread per row (and per owner slot, for the clump count): 9 fp64 products and two integers per lane,
//                          reduced by shuffles across the wavefront and through LDS across the block's four; one partial per
//                          block, in block order
//   k_contact_sums_final   one block: the partials strided over its threads, then a fixed tree -- the same bits on every call
//   k_contact_sums<true>   the same row pass counting sides per owner slot with integer atomics
//   k_contact_counts_out   the per-slot counts written in the caller's ids, or added at a slab's global ids
// No floating-point atomics anywhere: the order of every fp64 addition is fixed by the grid.
#pragma once
#include "deme_query.h"

namespace deme_dev {

struct ContactSums {  // DemeContactSums of deme_hip.h, and one block's partial
    double virial[9];
    unsigned long long sides, clumps;
};
static_assert(sizeof(ContactSums) == 88, "ContactSums is 88 bytes");

__global__ __launch_bounds__(256) void k_contact_owner_mask(uint32_t n, const OwnerRec* __restrict__ owners, uint32_t nClumps,
                                                            const uint32_t* __restrict__ o2e, float* __restrict__ mask) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const uint32_t id = o2e ? o2e[i] : i;  // clumps are the caller's first nClumps owners
    mask[i] = (id < nClumps && !ghost_of(owners[i].family)) ? 1.0f : 0.0f;
}

struct ContactSumArgs {
    uint32_t n;            // rows of the list
    uint32_t nSlots;       // owner slots (entries of mask / counts)
    const uint64_t* keys;  // the engine's list
    QueryTables t;
    const OwnerRec* owners;
    const float* mask;  // per owner slot
    const float *force, *cpA, *cpB;  // records 0, 2, 3: 3 floats a row
    double thr2;
    ContactSums* partial;  // [gridDim.x]
    uint32_t* counts;      // per owner slot (PER_OWNER)
};

__device__ inline void contact_side_add(double (&w)[9], const OwnerRec* __restrict__ owners, uint32_t o, const float* __restrict__ cp,
                                        double fx, double fy, double fz) {
    const float4 q4 = reinterpret_cast<const float4*>(owners + o)[1];  // qw, qx, qy, qz (OwnerRec bytes 16-31)
    const double qw = q4.x, ux = q4.y, uy = q4.z, uz = q4.w;
    const double vx = cp[0], vy = cp[1], vz = cp[2];
    const double tx = uy * vz - uz * vy, ty = uz * vx - ux * vz, tz = ux * vy - uy * vx;  // u x v
    const double sx = uy * tz - uz * ty, sy = uz * tx - ux * tz, sz = ux * ty - uy * tx;  // u x (u x v)
    const double rx = vx + (2.0 * qw) * tx + 2.0 * sx;
    const double ry = vy + (2.0 * qw) * ty + 2.0 * sy;
    const double rz = vz + (2.0 * qw) * tz + 2.0 * sz;
    w[0] += rx * fx, w[1] += rx * fy, w[2] += rx * fz;
    w[3] += ry * fx, w[4] += ry * fy, w[5] += ry * fz;
    w[6] += rz * fx, w[7] += rz * fy, w[8] += rz * fz;
}

template <bool PER_OWNER>
__global__ __launch_bounds__(256) void k_contact_sums(const ContactSumArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    double w[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
    uint32_t sides = 0, clumps = 0;
    if (!PER_OWNER && i < a.nSlots)
        clumps = a.mask[i] != 0.0f ? 1u : 0u;
    if (i < a.n) {
        const size_t r = (size_t)i * 3;
        double fx, fy, fz;
        if (row_force_counted(a.force, i, a.thr2, fx, fy, fz)) {
            uint32_t oA, oB;  // owner slots
            row_owners(a.t, a.keys[i], oA, oB);
            if (oA < a.nSlots && a.mask[oA] != 0.0f) {
                sides++;
                if (PER_OWNER)
                    atomicAdd(a.counts + oA, 1u);
                else
                    contact_side_add(w, a.owners, oA, a.cpA + r, fx, fy, fz);
            }
            if (oB < a.nSlots && a.mask[oB] != 0.0f) {
                sides++;
                if (PER_OWNER)
                    atomicAdd(a.counts + oB, 1u);
                else
                    contact_side_add(w, a.owners, oB, a.cpB + r, -fx, -fy, -fz);
            }
        }
    }
    if (PER_OWNER)
        return;
    for (int off = 32; off > 0; off >>= 1) {  // lane 0 of every wavefront ends with its 64 lanes' sums
        for (int j = 0; j < 9; j++)
            w[j] += __shfl_down(w[j], off, 64);
        sides += __shfl_down(sides, off, 64);
        clumps += __shfl_down(clumps, off, 64);
    }
    __shared__ double lw[4][9];
    __shared__ uint32_t ln[4][2];
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) {
        for (int j = 0; j < 9; j++)
            lw[wave][j] = w[j];
        ln[wave][0] = sides, ln[wave][1] = clumps;
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // (a block without a counted side writes zeros: the partials are never cleared)
        ContactSums p;
        for (int j = 0; j < 9; j++)
            p.virial[j] = ((lw[0][j] + lw[1][j]) + lw[2][j]) + lw[3][j];
        p.sides = (unsigned long long)ln[0][0] + ln[1][0] + ln[2][0] + ln[3][0];
        p.clumps = (unsigned long long)ln[0][1] + ln[1][1] + ln[2][1] + ln[3][1];
        a.partial[blockIdx.x] = p;
    }
}

// one block of 256: thread t adds partials t, t + 256, ... in that order, then the 256 sums go down a tree of fixed shape
__global__ __launch_bounds__(256) void k_contact_sums_final(uint32_t nPartials, const ContactSums* __restrict__ partial,
                                                            ContactSums* __restrict__ out) {
    __shared__ double lw[256][9];
    __shared__ unsigned long long ln[256][2];
    const uint32_t t = threadIdx.x;
    double w[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
    unsigned long long sides = 0, clumps = 0;
    for (uint32_t k = t; k < nPartials; k += 256) {
        for (int j = 0; j < 9; j++)
            w[j] += partial[k].virial[j];
        sides += partial[k].sides, clumps += partial[k].clumps;
    }
    for (int j = 0; j < 9; j++)
        lw[t][j] = w[j];
    ln[t][0] = sides, ln[t][1] = clumps;
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
        if (t < s) {
            for (int j = 0; j < 9; j++)
                lw[t][j] += lw[t + s][j];
            ln[t][0] += ln[t + s][0], ln[t][1] += ln[t + s][1];
        }
        __syncthreads();
    }
    if (t == 0) {
        for (int j = 0; j < 9; j++)
            out->virial[j] = lw[0][j];
        out->sides = ln[0][0], out->clumps = ln[0][1];
    }
}

// ownerGid == null: out[caller id of slot i] = counts[i] (every entry of out written once).  Otherwise a slab: the count of an own
// clump is written at its global id (out, nOut entries, was cleared; a clump is an own clump of one slab only).
__global__ __launch_bounds__(256) void k_contact_counts_out(uint32_t n, const uint32_t* __restrict__ counts, const uint32_t* __restrict__ o2e,
                                                            const uint32_t* __restrict__ ownerGid, uint32_t* __restrict__ out, uint32_t nOut) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    uint32_t id = o2e ? o2e[i] : i;
    if (id >= n)
        return;
    if (ownerGid) {
        if (!counts[i])
            return;
        id = ownerGid[id];
    }
    if (id < nOut)
        out[id] = counts[i];
}

}  // namespace deme_dev
