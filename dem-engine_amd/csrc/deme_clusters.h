// deme_clusters.h -- connected components of the contact network, labelled on the device (deme_inspect_clusters and its deme_multi_
// form; DEMClusterInspector): which clumps are joined to which through counted sphere-sphere rows, how large and heavy every
// cluster is and where its centre lies.  The reference has no such call.
//
// The statement is in include/deme_hip.h above deme_inspect_clusters.  Everything per owner lives in the CALLER's id space
// (id = o2e[slot]), so that "the smallest id of a component" means the caller's ids in fast and in exact mode alike.
//   k_cluster_init      one thread per owner slot: parent[id] = id for a vertex, 0xFFFFFFFF otherwise; size[id] = 0
//   k_cluster_link      one thread per row: a lock-free union of the row's two owners, the larger root hooked under the smaller;
//                       the block's count of edges to one integer partial
//   k_cluster_flatten   one thread per owner slot: label[id] = find(id); the counted owners add 1 to size[label] (integer atomics)
//   k_cluster_stats / _final   the summary: integer partials per block in block order, then one block down a fixed tree
//   k_cluster_select    one thread per owner slot: the pair (label, slot) of a counted owner, key nIds for any other; and per id the
//                       flag "a root with a counted owner", whose exclusive scan (k_scan_small) is the rank of the cluster's table row
//   deme_radix_sort     the pairs by label.  Stable: the slots of a cluster stay ascending, the uncounted owners end up behind
//   k_seg_sums<4> / k_seg_final<4>   the segmented sum of deme_seg_sum.h with four fp64 lanes (ClusterTerm: mass, three moments)
//                       and the count; ClusterTableOut writes a finished cluster's row
//   k_cluster_pairs     (a slab of a decomposed run) per local id the pair (global id, global id of its local root)
// No floating-point atomics, and no workgroup waits for another: a thread of k_cluster_link that loses a compare-and-swap goes on
// from the roots it finds next, it never waits for anybody.
#pragma once
#include "deme_query.h"
#include "deme_seg_sum.h"

namespace deme_dev {

constexpr uint32_t CLUSTER_NONE = 0xFFFFFFFFu;
constexpr int CLUSTER_LANES = 4;  // mass, moment xyz

struct ClusterCtl {             // cleared before every call, read back after it
    unsigned long long nRows;   // rows of the cluster table (the total of k_scan_small)
    uint32_t bound;             // a find or a link ran into its bound, or met an id beyond the owners: a defect, never a hang
    uint32_t retries;           // compare-and-swaps of k_cluster_link that lost to another thread
};
static_assert(sizeof(ClusterCtl) == 16, "ClusterCtl is 16 bytes");

struct ClusterStat {  // DemeClusterSummary of deme_hip.h, and one block's partial
    unsigned long long vertices, edges, clusters, singletons, largestSize, largestLabel;
};
static_assert(sizeof(ClusterStat) == 48, "ClusterStat is 48 bytes");

// ---- the forest -----------------------------------------------------------------------------------------------------------------------
// INVARIANT.  parent[x] <= x at all times, and parent[x] only ever decreases: k_cluster_init writes x, a hook writes a root smaller
// than x over x, a halving writes the minimum of what is there and x's grandparent.  So every find walks a strictly decreasing
// chain -- at most nIds steps, no cycle can form -- and a compare-and-swap that fails found parent[hi] != hi: another thread has
// hooked hi meanwhile, the forest has one root fewer, and at most nIds - 1 hooks can ever succeed.  A root is the smallest id of its
// tree (every hook puts the larger root under the smaller), and a link returns only when both ends have one root, so once the
// kernel has ended the trees are the components and their roots the component minima: one pass over the rows, no host iteration.
//
// The eight XCDs have private L2s: every access to parent[] inside k_cluster_link and k_cluster_flatten is an agent-scope atomic --
// relaxed loads (the compiler cannot cache them, and they are served where the atomics are), atomicMin, atomicCAS -- never a plain
// load or store.  A relaxed load may return an older value of a word; that is an earlier parent of x, which is still an ancestor.
__device__ inline uint32_t cluster_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x (a vertex) with path halving: at most nIds + 1 rounds, each one moves x strictly down or returns
__device__ inline uint32_t cluster_find(uint32_t* parent, uint32_t x, uint32_t nIds, ClusterCtl* ctl) {
    for (uint32_t step = 0; step <= nIds; step++) {
        const uint32_t p = cluster_load(parent + x);
        if (p == x)
            return x;
        if (p >= nIds)  // (never: a vertex's parent is a vertex)
            break;
        const uint32_t g = cluster_load(parent + p);
        if (g >= nIds)
            break;
        if (g != p)
            atomicMin(parent + x, g);
        x = g;
    }
    atomicOr(&ctl->bound, 1u);
    return x;
}

__global__ __launch_bounds__(256) void k_cluster_init(uint32_t nSlots, uint32_t nClumps, const OwnerRec* __restrict__ owners,
                                                      const uint32_t* __restrict__ o2e, int ghostsLink, uint32_t* __restrict__ parent,
                                                      uint32_t* __restrict__ size) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nSlots)
        return;
    const uint32_t id = o2e ? o2e[i] : i;  // clumps are the caller's first nClumps owners (k_contact_owner_mask)
    if (id >= nSlots)
        return;
    const bool vertex = id < nClumps && (ghostsLink || !ghost_of(owners[i].family));
    parent[id] = vertex ? id : CLUSTER_NONE;
    size[id] = 0;
}

struct ClusterLinkArgs {
    uint32_t n;            // rows of the list
    uint32_t nSlots;       // owner slots = ids
    const uint64_t* keys;  // the engine's list
    QueryTables t;
    const OwnerRec* owners;
    const uint32_t* o2e;
    const float* force;  // record 0: 3 floats a row
    double thr2;
    uint32_t* parent;           // per id
    const uint32_t* ownerGid;   // a slab: global id per local id (an edge is then counted by the slab that owns its smaller global id)
    uint32_t* edgePartial;      // [gridDim.x]
    ClusterCtl* ctl;
};

// the two vertices (caller ids) and owner slots of row i if the row is an edge
__device__ inline bool cluster_row_edge(const ClusterLinkArgs& a, uint32_t i, uint32_t& ia, uint32_t& ib, uint32_t& oA, uint32_t& oB) {
    double fx, fy, fz;
    const bool counted = row_force_counted(a.force, i, a.thr2, fx, fy, fz);
    const uint64_t k = a.keys[i];
    if (key_class(k) != DEME_KEY_CLASS_SS || !counted)
        return false;
    row_owners(a.t, k, oA, oB);  // owner slots
    if (oA >= a.nSlots || oB >= a.nSlots || oA == oB)
        return false;
    ia = a.o2e ? a.o2e[oA] : oA, ib = a.o2e ? a.o2e[oB] : oB;
    // (parent[id] of a non-vertex is 0xFFFFFFFF from the init to the end: nothing ever hooks or halves it)
    return ia < a.nSlots && ib < a.nSlots && cluster_load(a.parent + ia) != CLUSTER_NONE && cluster_load(a.parent + ib) != CLUSTER_NONE;
}

__global__ __launch_bounds__(256) void k_cluster_link(const ClusterLinkArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t edges = 0, tries = 0;
    uint32_t ia, ib, oA, oB;
    if (i < a.n && cluster_row_edge(a, i, ia, ib, oA, oB)) {
        if (a.ownerGid)
            edges = !ghost_of(a.owners[a.ownerGid[ia] < a.ownerGid[ib] ? oA : oB].family) ? 1u : 0u;
        else
            edges = 1u;
        uint32_t ra = cluster_find(a.parent, ia, a.nSlots, a.ctl), rb = cluster_find(a.parent, ib, a.nSlots, a.ctl);
        while (ra != rb) {
            const uint32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
            if (atomicCAS(a.parent + hi, hi, lo) == hi)
                break;
            if (++tries > a.nSlots) {
                atomicOr(&a.ctl->bound, 1u);
                break;
            }
            ra = cluster_find(a.parent, hi, a.nSlots, a.ctl), rb = cluster_find(a.parent, lo, a.nSlots, a.ctl);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        edges += __shfl_down(edges, off, 64);
        tries += __shfl_down(tries, off, 64);
    }
    __shared__ uint32_t le[4], lt[4];
    if ((threadIdx.x & 63u) == 0)
        le[threadIdx.x >> 6] = edges, lt[threadIdx.x >> 6] = tries;
    __syncthreads();
    if (threadIdx.x == 0) {  // (a block without an edge writes 0: the partials are never cleared)
        a.edgePartial[blockIdx.x] = le[0] + le[1] + le[2] + le[3];
        // the lost compare-and-swaps: one add a block, not one a retry -- millions of adds to one word would cost more than the links
        const uint32_t lost = lt[0] + lt[1] + lt[2] + lt[3];
        if (lost)
            atomicAdd(&a.ctl->retries, lost);
    }
}

__global__ __launch_bounds__(256) void k_cluster_flatten(uint32_t nSlots, const OwnerRec* __restrict__ owners, const uint32_t* __restrict__ o2e,
                                                         uint32_t* parent, uint32_t* __restrict__ label, uint32_t* size, ClusterCtl* ctl) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nSlots)
        return;
    const uint32_t id = o2e ? o2e[i] : i;
    if (id >= nSlots)
        return;
    uint32_t root = CLUSTER_NONE;
    if (cluster_load(parent + id) != CLUSTER_NONE) {
        root = cluster_find(parent, id, nSlots, ctl);
        if (root < nSlots && !ghost_of(owners[i].family))  // a counted owner (a vertex that is a ghost copy links, and is never counted)
            atomicAdd(size + root, 1u);
    }
    label[id] = root;
}

// ---- the summary ----------------------------------------------------------------------------------------------------------------------
__device__ inline void cluster_stat_add(ClusterStat& a, const ClusterStat& b) {
    a.vertices += b.vertices, a.edges += b.edges, a.clusters += b.clusters, a.singletons += b.singletons;
    if (b.largestSize > a.largestSize || (b.largestSize == a.largestSize && b.largestLabel < a.largestLabel))
        a.largestSize = b.largestSize, a.largestLabel = b.largestLabel;
}
// the 256 entries of s down a tree of fixed shape; entry 0 ends with the sum
__device__ inline void cluster_stat_tree(ClusterStat (&s)[256], uint32_t t) {
    __syncthreads();
    for (uint32_t d = 128; d > 0; d >>= 1) {
        if (t < d)
            cluster_stat_add(s[t], s[t + d]);
        __syncthreads();
    }
}

// thread i: id i of the labels and sizes, and the i-th partial of k_cluster_link
__global__ __launch_bounds__(256) void k_cluster_stats(uint32_t nIds, const uint32_t* __restrict__ label, const uint32_t* __restrict__ size,
                                                       uint32_t nEdgePartials, const uint32_t* __restrict__ edgePartial,
                                                       ClusterStat* __restrict__ partial) {
    __shared__ ClusterStat s[256];
    const uint32_t t = threadIdx.x, i = blockIdx.x * blockDim.x + t;
    ClusterStat v{0, 0, 0, 0, 0, CLUSTER_NONE};
    if (i < nIds) {
        const uint32_t l = label[i];
        if (l != CLUSTER_NONE)
            v.vertices = 1;
        if (l == i) {
            const uint32_t n = size[i];
            v.clusters = 1, v.singletons = n == 1 ? 1 : 0, v.largestSize = n, v.largestLabel = i;
        }
    }
    if (i < nEdgePartials)
        v.edges = edgePartial[i];
    s[t] = v;
    cluster_stat_tree(s, t);
    if (t == 0)
        partial[blockIdx.x] = s[0];
}

// one block of 256: thread t adds partials t, t + 256, ... in that order, then the tree
__global__ __launch_bounds__(256) void k_cluster_stats_final(uint32_t nPartials, const ClusterStat* __restrict__ partial,
                                                             ClusterStat* __restrict__ out) {
    __shared__ ClusterStat s[256];
    const uint32_t t = threadIdx.x;
    ClusterStat v{0, 0, 0, 0, 0, CLUSTER_NONE};
    for (uint32_t k = t; k < nPartials; k += 256)
        cluster_stat_add(v, partial[k]);
    s[t] = v;
    cluster_stat_tree(s, t);
    if (t == 0)
        *out = s[0];
}

// ---- the cluster table ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cluster_select(uint32_t nSlots, const OwnerRec* __restrict__ owners, const uint32_t* __restrict__ o2e,
                                                        const uint32_t* __restrict__ label, const uint32_t* __restrict__ size,
                                                        uint32_t* __restrict__ key, uint32_t* __restrict__ slot, uint32_t* __restrict__ rowFlag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nSlots)
        return;
    const uint32_t id = o2e ? o2e[i] : i;
    uint32_t k = nSlots;
    if (id < nSlots) {
        const uint32_t l = label[id];
        if (l < nSlots && !ghost_of(owners[i].family))
            k = l;
        rowFlag[id] = (l == id && size[id] > 0) ? 1u : 0u;  // (o2e is a permutation: every id is written by one thread)
    }
    key[i] = k, slot[i] = i;
}

struct ClusterTableOut {  // nIds entries (times 3) each; rank: the exclusive scan of rowFlag
    const uint32_t* rank;
    uint32_t *label, *size;
    double *mass, *moment;
    __device__ void write(uint32_t l, const double (&v)[CLUSTER_LANES], uint32_t n) const {
        const uint32_t row = rank[l];
        label[row] = l, size[row] = n, mass[row] = v[0];
        for (int j = 0; j < 3; j++)
            moment[3 * (size_t)row + j] = v[1 + j];
    }
};
struct ClusterTerm {  // slots: the sorted owner slots
    DevParams p;
    const uint32_t* slots;
    const OwnerRec* owners;
    const float4* massProps;
    __device__ uint32_t operator()(uint32_t e, double (&v)[CLUSTER_LANES]) const {
        const OwnerRec r = load_owner(owners, slots[e]);  // (a slot of k_cluster_select: < nSlots)
        const d3 P = decode_pos(r.voxelID, r.locX, r.locY, r.locZ, p);
        const double m = (double)massProps[r.inertiaOff].x;
        v[0] = m, v[1] = m * (P.x + (double)p.LBFX), v[2] = m * (P.y + (double)p.LBFY), v[3] = m * (P.z + (double)p.LBFZ);
        return 1u;
    }
};

// ---- a slab of a decomposed run ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cluster_pairs(uint32_t nIds, const uint32_t* __restrict__ label, const uint32_t* __restrict__ ownerGid,
                                                       uint2* __restrict__ pairs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nIds)
        return;
    const uint32_t l = label[i];
    pairs[i] = l < nIds ? make_uint2(ownerGid[i], ownerGid[l]) : make_uint2(CLUSTER_NONE, CLUSTER_NONE);
}

}  // namespace deme_dev
