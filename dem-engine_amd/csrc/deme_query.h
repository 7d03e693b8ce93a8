// deme_query.h -- contacts of a few owners, selected on the device (deme_query_owner_contacts; the reference's
// getContactForcesConcerningOwners, algorithms/DEMDynamicMisc.cu:14-100, and DEMSolver::GetOwnerContactClumps).
//
// A script that asks for the force on one plate, or for the neighbours of one clump, needs a few hundred rows of a list of
// millions.  The kernels below run only when such a question is asked:
//   k_query_mark    a mark scattered onto the caller's owner ids
//   k_query_select<false>  one thread per row of the current list: both owners looked up in the tables the force pass uses,
//                   translated to the caller's ids, tested against the marks; the hit rows compacted per wavefront into a scratch
//                   buffer, with the row's four 12-byte records when they are asked for
//   k_query_select<true>  the same body for one slab of a decomposed run: global ids from the device books, the merged list's
//                   report-once and flip rules (deme_multi_query_owner_contacts)
//   k_query_owner_state  the 64-byte records of a few owners: a gather by slot, or one slab's share of a question in global ids
//   k_scatter_owner_state  its counterpart: named fields of a few owners' records replaced, by slot or by global id on a slab
// A thread writes only below the scratch's capacity while the counter counts every hit: the host reads the count, grows the
// scratch and selects again when it was too small (deme_hip.hip).  The order of the hits is the atomics'; the host sorts them.
#pragma once
#include "deme_device.h"
#include "deme_mesh.h"
#include "deme_owner_cols.h"

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

// the owner slots of both sides of a row (0xFFFFFFFF: the row names something beyond the tables)
__device__ inline void row_owners(const QueryTables& t, uint64_t k, uint32_t& oA, uint32_t& oB) {
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

// The threshold test of the inspectors: row i's recorded force (record 0, 3 floats a row) as doubles, and whether its squared norm
// reaches thr2 = (double)thr^2.  >=, so a row with a NaN force is never counted.
__device__ inline bool row_force_counted(const float* __restrict__ force, uint32_t i, double thr2, double& fx, double& fy, double& fz) {
    const size_t r = (size_t)i * 3;
    fx = force[r], fy = force[r + 1], fz = force[r + 2];
    return fx * fx + fy * fy + fz * fz >= thr2;
}

__global__ __launch_bounds__(256) void k_query_mark(uint32_t n, const uint32_t* __restrict__ ids, uint8_t* __restrict__ mark) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        mark[ids[i]] = 1;  // (ids are in range and distinct: the host checks and de-duplicates them)
}

// ---- one slab of a decomposed run (deme_multi_query_owner_contacts) -------------------------------------------------------------
// The slab lists its contacts in its own numbering; the question and the answer are in GLOBAL ids.  The books the migration keeps
// on the device translate (SlabGeom::sphereGid / ownerGid, indexed by the slab scene's ids), so no host copy of them is needed.
struct SlabBooksDev {
    const uint32_t* sphereGid;  // the slab scene's sphere id -> global sphere id
    const uint32_t* ownerGid;   // the slab scene's owner id -> global owner id
    uint32_t nOwn;              // the slab's own clumps are its first nOwn owners
    uint32_t nOwnersGlobal;     // entries of the mark array
};

#define DEME_QUERY_FLIPPED 2u  // QueryHit::side bit 1 of a slab's hit: the slab holds the pair the other way round

__host__ __device__ inline uint64_t merged_key(uint64_t cls, uint32_t gA, uint32_t gB) {  // the key of multi_contact_rows
    return ((uint64_t)gA << 34) | (cls << 31) | (uint64_t)gB;
}
__host__ __device__ inline uint32_t merged_key_a(uint64_t k) { return (uint32_t)(k >> 34); }  // (the class sits where key_class reads it)
__host__ __device__ inline uint32_t merged_key_b(uint64_t k) { return (uint32_t)(k & 0x7FFFFFFFull); }

// The compaction of the kernels below: one reservation of the counter per wavefront (as k_resize_keys and k_sweep append); returns
// the slot of this lane's hit, 0xFFFFFFFF for a lane without one.  Every lane of the wavefront calls it.
__device__ inline uint32_t query_append_slot(bool hit, uint32_t* nHits) {
    const unsigned long long m = __ballot(hit);
    if (!m)
        return 0xFFFFFFFFu;
    const uint32_t lane = __lane_id();
    const uint32_t leader = (uint32_t)__ffsll((long long)m) - 1u;
    uint32_t base = 0;
    if (lane == leader)
        base = atomicAdd(nHits, (uint32_t)__popcll(m));
    base = __shfl(base, (int)leader);
    return hit ? base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)) : 0xFFFFFFFFu;
}

// rec[0..3] (force, torque-only force, cpA, cpB; 3 floats per row of the list) are copied into recOut (12 floats per hit) when
// recOut is not null.  cap: rows `hits` (and recOut) hold.
// SLAB false, a single context: a row is a hit when owner A or B (caller ids) is marked; the key is the caller's (order_key_out),
// side 0 or 1, the records bit for bit; bk is not read.
// SLAB true, the rule of multi_contact_rows row by row: a sphere-sphere pair is (smaller, larger) global sphere id; the row is
// reported only by the slab that owns the clump of the (post-swap) sphere A; sphere-mesh and sphere-analytical rows go with sphere
// A's clump.  A reported row is a hit when global owner A or B is marked.  Hits carry the merged key, the global owners, side (bit
// 0, in the merged orientation) and the flipped bit (bit 1); the records of a flipped row as deme_multi_download_contact_records
// gives them: force and torque-only force times -1.0f, cpA and cpB swapped.
template <bool SLAB>
__global__ __launch_bounds__(256) void k_query_select(uint32_t n, const uint64_t* __restrict__ keys, QueryTables t, SlabBooksDev bk,
                                                      const uint8_t* __restrict__ mark, const float* __restrict__ rec0,
                                                      const float* __restrict__ rec1, const float* __restrict__ rec2,
                                                      const float* __restrict__ rec3, QueryHit* __restrict__ hits,
                                                      float* __restrict__ recOut, uint32_t cap, uint32_t* nHits) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool hit = false, flipped = false;
    QueryHit h{};
    if (i < n) {
        const uint64_t k = keys[i];
        const uint32_t cls = key_class(k), a = key_a(k), b = key_b(k);
        uint32_t oA, oB;
        row_owners(t, k, oA, oB);
        if (oA < t.nOwners && oB < t.nOwners) {
            if (t.o2e)  // (a context with ghosts keeps the order it is uploaded in: null on a slab today)
                oA = t.o2e[oA], oB = t.o2e[oB];
            if constexpr (!SLAB) {
                const bool mA = oA < t.nOwners && mark[oA] != 0, mB = oB < t.nOwners && mark[oB] != 0;
                hit = mA || mB;
                h.key = t.s2e ? make_key(cls, t.s2e[a], cls == DEME_KEY_CLASS_SS ? t.s2e[b] : b) : k;
                h.row = i, h.ownerA = oA, h.ownerB = oB, h.side = mA ? 0u : 1u;
            } else {
                uint32_t sA = t.s2e ? t.s2e[a] : a, sB = (t.s2e && cls == DEME_KEY_CLASS_SS) ? t.s2e[b] : b;
                if (oA < t.nOwners && oB < t.nOwners && sA < t.nSpheres && (cls != DEME_KEY_CLASS_SS || sB < t.nSpheres)) {
                    uint32_t gA = bk.sphereGid[sA], gB = cls == DEME_KEY_CLASS_SS ? bk.sphereGid[sB] : sB;
                    if (cls == DEME_KEY_CLASS_SS && gA > gB) {
                        uint32_t x = gA;
                        gA = gB, gB = x;
                        x = oA, oA = oB, oB = x;
                        flipped = true;
                    }
                    if (oA < bk.nOwn) {  // the neighbour that owns that clump reports the pair otherwise
                        const uint32_t goA = bk.ownerGid[oA], goB = bk.ownerGid[oB];
                        const bool mA = goA < bk.nOwnersGlobal && mark[goA] != 0, mB = goB < bk.nOwnersGlobal && mark[goB] != 0;
                        hit = mA || mB;
                        h.key = merged_key(cls, gA, gB);
                        h.row = i, h.ownerA = goA, h.ownerB = goB, h.side = (mA ? 0u : 1u) | (flipped ? DEME_QUERY_FLIPPED : 0u);
                    }
                }
            }
        }
    }
    const uint32_t at = query_append_slot(hit, nHits);
    if (at >= cap)  // (no hit, or the counter has counted the row: the host selects again with room for all of them)
        return;
    hits[at] = h;
    if (recOut) {
        float* o = recOut + (size_t)at * 12;
        const size_t r = (size_t)i * 3;
        const float sgn = flipped ? -1.0f : 1.0f;  // (the recorded force acts on A; a zero changes sign too, as on the host path)
        const float* pa = flipped ? rec3 : rec2;   // (flipped stays false on a single context)
        const float* pb = flipped ? rec2 : rec3;
        for (int j = 0; j < 3; j++) {
            o[j] = SLAB ? sgn * rec0[r + j] : rec0[r + j];
            o[3 + j] = SLAB ? sgn * rec1[r + j] : rec1[r + j];
            o[6 + j] = pa[r + j];
            o[9 + j] = pb[r + j];
        }
    }
}

// ---- pose, velocity and family of a few owners (deme_query_owner_state, deme_multi_query_owner_state) ---------------------------
// A hit is the owner's 64-byte record as it stands, with the word that holds the margin replaced by a tag: the index of the
// question (single context) or the owner's global id (a slab).
__device__ inline void query_state_write(OwnerRec* __restrict__ out, uint32_t at, const OwnerRec* __restrict__ owners, uint32_t slot,
                                         uint32_t tag) {
    OwnerRec r = owners[slot];
    r.margin = __uint_as_float(tag);
    out[at] = r;
}

// bk.ownerGid == null: a gather by slot -- thread i copies owner slots[i] (the host translated the caller's ids) to out[i]; nHits unused.
// Otherwise one thread per owner slot of the slab: the owner's global id looked up, tested against the marks, and taken under the
// rule of the host's slab_reports (deme_decomp.inc) -- own clumps from the slab that owns them, replicated owners (slots from
// nOwnerClumps on) from the first slab of the chain (takeReplicated) --, hits compacted per wavefront as in k_query_select.
__global__ __launch_bounds__(256) void k_query_owner_state(uint32_t n, const OwnerRec* __restrict__ owners, const uint32_t* __restrict__ slots,
                                                           const uint32_t* __restrict__ o2e, SlabBooksDev bk, uint32_t nOwnerClumps, uint32_t takeReplicated,
                                                           const uint8_t* __restrict__ mark, OwnerRec* __restrict__ out, uint32_t cap,
                                                           uint32_t* nHits) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (!bk.ownerGid) {
        if (i < n && i < cap)
            query_state_write(out, i, owners, slots[i], i);
        return;
    }
    bool hit = false;
    uint32_t gid = 0;
    if (i < n) {
        const uint32_t s = o2e ? o2e[i] : i;  // the slab scene's id of this slot
        if (s < n && (s < bk.nOwn || (s >= nOwnerClumps && takeReplicated))) {
            gid = bk.ownerGid[s];
            hit = gid < bk.nOwnersGlobal && mark[gid] != 0;
        }
    }
    const uint32_t at = query_append_slot(hit, nHits);
    if (at < cap)
        query_state_write(out, at, owners, i, gid);
}

// ---- writing pose, velocity and family of a few owners (deme_scatter_owner_state, deme_multi_scatter_owner_state) ------------------
// The host sends one 64-byte record per id with the new values in their fields (the rest of it is not read) and a mask of the
// columns the call gave: DEME_SCATTER_BIT, bit k for pose column k of deme_owner_cols.h.  What a write touches is what k_pack_owners
// touches with dir == 0: margin, inertiaOff and the flag bits of the family word keep their bits.
__device__ inline void scatter_state_write(OwnerRec* __restrict__ owners, uint32_t slot, const OwnerRec* __restrict__ patch, uint32_t row,
                                           uint32_t mask) {
    OwnerRec r = owners[slot];
    const OwnerRec p = patch[row];
#define DEME_COL(abi, T, Rec, f) if (mask & DEME_SCATTER_BIT(abi)) r.f = p.f;
    DEME_OWNER_COLS(DEME_COL, DEME_COL_NONE, DEME_COL_NONE)
#undef DEME_COL
    if (mask & DEME_SCATTER_BIT(familyID)) r.family = (r.family & OWNER_FLAG_BITS) | (p.family & 0xFFu);  // a ghost stays a ghost
    owners[slot] = r;
}

// ownerGid == null: a scatter by slot -- thread i writes patch[i] into owner keys[i] (the host translated the caller's ids; they
// are distinct, so no two threads write one record).  n = nKeys threads.
// Otherwise one thread per owner slot of the slab (n = nOwners): the slot's global id looked up as k_query_owner_state does and
// searched in keys, the asked ids in ascending order with patch in the same order.  Every copy on the slab is written: its own
// clump, a ghost of a neighbour's, a replicated owner (the rule of an upload of the whole state by global id).
__global__ __launch_bounds__(256) void k_scatter_owner_state(uint32_t n, OwnerRec* __restrict__ owners, uint32_t nOwners,
                                                             const uint32_t* __restrict__ keys, uint32_t nKeys,
                                                             const OwnerRec* __restrict__ patch, uint32_t mask,
                                                             const uint32_t* __restrict__ o2e, const uint32_t* __restrict__ ownerGid) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    if (!ownerGid) {
        const uint32_t slot = keys[i];
        if (slot < nOwners)
            scatter_state_write(owners, slot, patch, i, mask);
        return;
    }
    const uint32_t s = o2e ? o2e[i] : i;  // the slab scene's id of this slot
    if (s >= nOwners)
        return;
    const uint32_t gid = ownerGid[s];
    uint32_t lo = 0, hi = nKeys;  // the first key >= gid
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < gid)
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo < nKeys && keys[lo] == gid)
        scatter_state_write(owners, i, patch, lo, mask);
}

}  // namespace deme_dev
