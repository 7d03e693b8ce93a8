// deme_query.h -- contacts of a few owners, selected on the device (deme_query_owner_contacts; the reference's
// getContactForcesConcerningOwners, algorithms/DEMDynamicMisc.cu:14-100, and DEMSolver::GetOwnerContactClumps).
//
// A script that asks for the force on one plate, or for the neighbours of one clump, needs a few hundred rows of a list of
// millions.  The kernels below run only when such a question is asked:
//   k_query_mark    a mark scattered onto the caller's owner ids
//   k_query_select  one thread per row of the current list: both owners looked up in the tables the force pass uses, translated to
//                   the caller's ids, tested against the marks; the hit rows compacted per wavefront into a scratch buffer, with
//                   the row's four 12-byte records when they are asked for
// A thread writes only below the scratch's capacity while the counter counts every hit: the host reads the count, grows the
// scratch and selects again when it was too small (deme_hip.hip).  The order of the hits is the atomics'; the host sorts them.
#pragma once
#include "deme_device.h"
#include "deme_mesh.h"

namespace deme_dev {

struct __attribute__((aligned(8))) QueryHit {
    uint64_t key;     // the row's key in the caller's ids (order_key_out)
    uint32_t row;     // its index in the engine's list
    uint32_t ownerA;  // caller ids
    uint32_t ownerB;
    uint32_t side;    // 0: A's owner is marked; 1: only B's
};
static_assert(sizeof(QueryHit) == 24, "QueryHit is 24 bytes");

struct QueryTables {  // what a row's owners are looked up in (counts: a row that names something beyond them is never a hit)
    const SphereRec* spheres;
    const TriRec* tris;
    const AnalObj* anal;
    const uint32_t* s2e;  // DevParams::s2e / o2e: null when the engine keeps the caller's numbering
    const uint32_t* o2e;
    uint32_t nSpheres, nTri, nAnal, nOwners;
};

__global__ __launch_bounds__(256) void k_query_mark(uint32_t n, const uint32_t* __restrict__ ids, uint8_t* __restrict__ mark) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        mark[ids[i]] = 1;  // (ids are in range and distinct: the host checks and de-duplicates them)
}

// rec[0..3] (force, torque-only force, cpA, cpB; 3 floats per row of the list) are copied bit for bit into recOut (12 floats per
// hit) when recOut is not null.  cap: rows `hits` (and recOut) hold.
__global__ __launch_bounds__(256) void k_query_select(uint32_t n, const uint64_t* __restrict__ keys, QueryTables t,
                                                      const uint8_t* __restrict__ mark, const float* __restrict__ rec0,
                                                      const float* __restrict__ rec1, const float* __restrict__ rec2,
                                                      const float* __restrict__ rec3, QueryHit* __restrict__ hits,
                                                      float* __restrict__ recOut, uint32_t cap, uint32_t* nHits) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool hit = false;
    QueryHit h{};
    if (i < n) {
        const uint64_t k = keys[i];
        const uint32_t cls = key_class(k), a = key_a(k), b = key_b(k);
        uint32_t oA = 0xFFFFFFFFu, oB = 0xFFFFFFFFu;
        if (a < t.nSpheres)
            oA = load_sphere(t.spheres, a).owner;
        if (cls == DEME_KEY_CLASS_SS) {
            if (b < t.nSpheres)
                oB = load_sphere(t.spheres, b).owner;
        } else if (cls == DEME_KEY_CLASS_SM) {
            if (b < t.nTri)
                oB = t.tris[b].owner;
        } else if (b < t.nAnal) {
            oB = t.anal[b].owner;
        }
        if (oA < t.nOwners && oB < t.nOwners) {
            if (t.o2e)
                oA = t.o2e[oA], oB = t.o2e[oB];
            const bool mA = oA < t.nOwners && mark[oA] != 0, mB = oB < t.nOwners && mark[oB] != 0;
            hit = mA || mB;
            h.key = t.s2e ? make_key(cls, t.s2e[a], cls == DEME_KEY_CLASS_SS ? t.s2e[b] : b) : k;
            h.row = i, h.ownerA = oA, h.ownerB = oB, h.side = mA ? 0u : 1u;
        }
    }
    // one reservation per wavefront (as k_resize_keys and k_sweep append)
    const unsigned long long m = __ballot(hit);
    if (!m)
        return;
    const uint32_t lane = __lane_id();
    const uint32_t leader = (uint32_t)__ffsll((long long)m) - 1u;
    uint32_t base = 0;
    if (lane == leader)
        base = atomicAdd(nHits, (uint32_t)__popcll(m));
    base = __shfl(base, (int)leader);
    const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (!hit || at >= cap)  // the counter has counted the row; the host selects again with room for all of them
        return;
    hits[at] = h;
    if (recOut) {
        float* o = recOut + (size_t)at * 12;
        const size_t r = (size_t)i * 3;
        o[0] = rec0[r], o[1] = rec0[r + 1], o[2] = rec0[r + 2];
        o[3] = rec1[r], o[4] = rec1[r + 1], o[5] = rec1[r + 2];
        o[6] = rec2[r], o[7] = rec2[r + 1], o[8] = rec2[r + 2];
        o[9] = rec3[r], o[10] = rec3[r + 1], o[11] = rec3[r + 2];
    }
}

}  // namespace deme_dev
