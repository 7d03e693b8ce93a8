// deme_resize.h -- run-time resizing of clumps (deme_change_owner_sizes; the reference's ChangeClumpSizes, dT.cpp:357-405).
//
// A sphere's geometry reaches every kernel through its 16-bit component index (SphereRec::comp) into the table of
// {relx, rely, relz, radius}.  Resizing an owner therefore gives its spheres derived components -- the template entry with each
// of the four values multiplied by the factor in fp32, as the reference's modifyComponents does in place -- and rewrites their
// indices.  The kernels below run only when a resize is requested:
//   k_resize_mark   factor bits scattered onto the caller's owner ids
//   k_resize_keys   one key (comp << 32 | factor bits) per sphere of a marked owner, compacted per wavefront
//   k_resize_uses   how many spheres use each component (the host drops derived entries nobody uses any more)
//   k_resize_apply  every sphere's new index: a marked one through the sorted key -> index table, the others through the remap
// The distinct keys (rocprim sort + run-length encoding) and the new table are built on the host (deme_hip.hip).
#pragma once
#include "deme_device.h"

namespace deme_dev {

__global__ __launch_bounds__(256) void k_resize_mark(uint32_t n, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ factorBits,
                                                     uint32_t* __restrict__ mark) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        mark[ids[i]] = factorBits[i];  // (ids are distinct: the host refuses duplicates)
}

// the factor of sphere slot s's owner (0: not resized); `mark` is indexed by the caller's owner id
__device__ inline uint32_t resize_factor_of(const SphereRec& sr, const uint32_t* __restrict__ o2e, const uint32_t* __restrict__ mark) {
    return mark[o2e ? o2e[sr.owner] : sr.owner];
}

__global__ __launch_bounds__(256) void k_resize_keys(uint32_t nS, const SphereRec* __restrict__ spheres, const uint32_t* __restrict__ o2e,
                                                     const uint32_t* __restrict__ mark, uint64_t* __restrict__ keys, uint32_t* nKeys) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t key = 0;
    bool hit = false;
    if (s < nS) {
        const SphereRec sr = spheres[s];
        const uint32_t f = resize_factor_of(sr, o2e, mark);
        hit = f != 0u;
        key = ((uint64_t)sr.comp << 32) | f;
    }
    // one reservation per wavefront (as k_sweep appends its keys)
    const unsigned long long m = __ballot(hit);
    if (!m)
        return;
    const uint32_t lane = __lane_id();
    const uint32_t leader = (uint32_t)__ffsll((long long)m) - 1u;
    uint32_t base = 0;
    if (lane == leader)
        base = atomicAdd(nKeys, (uint32_t)__popcll(m));
    base = __shfl(base, (int)leader);
    if (hit)
        keys[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = key;
}

__global__ __launch_bounds__(256) void k_resize_uses(uint32_t nS, const SphereRec* __restrict__ spheres, uint32_t* __restrict__ uses) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nS)
        atomicAdd(&uses[spheres[s].comp], 1u);
}

// `geo` (may be null): the per-sphere geometry of the last detection, whose swept radius (radius + that detection's margin) is brought
// up to date at once -- the margin is what the record holds beyond the old radius (`keyOldR`), the owner's own may be newer (an
// asynchronous detection sizes margins on a copy of the owners); the centres follow with the next detection, which a resize forces
__global__ __launch_bounds__(256) void k_resize_apply(uint32_t nS, SphereRec* __restrict__ spheres, const uint32_t* __restrict__ o2e,
                                                      const uint32_t* __restrict__ mark, const uint64_t* __restrict__ keys, uint32_t nKeys,
                                                      const uint32_t* __restrict__ keyIdx, const float* __restrict__ keyOldR,
                                                      const uint32_t* __restrict__ remap, const float4* __restrict__ comp,
                                                      GeoRec* __restrict__ geo) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nS)
        return;
    SphereRec sr = spheres[s];
    const uint32_t f = resize_factor_of(sr, o2e, mark);
    uint32_t nc, lo = 0;
    if (f) {
        const uint64_t key = ((uint64_t)sr.comp << 32) | f;
        uint32_t hi = nKeys;  // keys are sorted and hold this one
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (keys[mid] <= key)
                lo = mid;
            else
                hi = mid;
        }
        nc = keyIdx[lo];
    } else {
        nc = remap[sr.comp];
    }
    if (nc != sr.comp) {
        sr.comp = (uint16_t)nc;
        spheres[s] = sr;
    }
    if (geo && f) {
        const float margin = geo[s].r - keyOldR[lo];
        float r = comp[nc].w;
        r += margin;
        geo[s].r = r;
    }
}

}  // namespace deme_dev
