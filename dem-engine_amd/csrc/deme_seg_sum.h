// deme_seg_sum.h -- the segmented sum of L fp64 lanes and one count by runs of equal keys: the last two passes of the triangle loads
// (deme_tri_loads.h, L = 3), of the fields' owner and contact columns (deme_fields.h, L = 11 and 9) and of the cluster table
// (deme_clusters.h, L = 4); alone on host arrays as deme_seg_sum_f64 (tests/test_seg_sum.py).
//
// The entries come sorted by key, stably (seg_sort of deme_hip.hip): the entries of a key stay in the order their user wrote them
// and the uncounted ones (key nKeys, one past the last key) end up behind every counted one.  The whole list is sorted, so the number
// of counted entries never has to come to the host.
//   k_seg_sums    one workgroup per SEG_BLOCK_ROWS sorted entries: a segmented inclusive scan by key, a tree of fixed shape in LDS
//                 (no thread walks a run alone).  A run that neither starts with the block's first entry nor ends with its last is
//                 closed inside the block and goes straight to the key's output; the block's first and last runs go to two partials
//   k_seg_final   one workgroup: the same scan over the partials in workgroup order, 256 at a time with the open run carried from
//                 one round to the next; it ends at the first round that begins behind the counted entries
// No floating-point atomics anywhere, and no workgroup waits for another inside a kernel: the order of every fp64 addition is fixed
// by the list and the grid, so two calls on one state give the same bits.
#pragma once
#include <stdint.h>

namespace deme_dev {

constexpr unsigned SEG_BLOCK_ROWS = 256;  // sorted entries per workgroup of k_seg_sums, one a thread

// The inclusive scan of 256 entries by run of equal keys; the keys ascend, so an equal key d entries back means one run all the way.
// Step d adds the entry d back to every entry of its run: a tree of eight levels, the same for every input.  An array per lane, not
// an array of records: a wavefront's 8-byte accesses then fall on consecutive banks.  256 * (8 L + 8) bytes: 24.6 KB at L = 11.
template <int L>
struct SegScanLds {
    double v[L][256];
    uint32_t n[256], key[256];
};
template <int L>
struct SegPartial {  // a block's sum over its first or its last run
    double v[L];
    uint32_t key, n;  // (key >= nKeys: the run of the uncounted entries, or an entry past the partials)
};
static_assert(sizeof(SegPartial<3>) == 32, "SegPartial<3> is 32 bytes");

template <int L>
__device__ inline void seg_scan(SegScanLds<L>& s, uint32_t t, uint32_t key, double (&v)[L], uint32_t& n) {
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
__device__ inline SegPartial<L> seg_partial(const double (&v)[L], uint32_t key, uint32_t n) {
    SegPartial<L> p;
#pragma unroll
    for (int j = 0; j < L; j++)
        p.v[j] = v[j];
    p.key = key, p.n = n;
    return p;
}
template <int L>
__device__ inline SegPartial<L> seg_partial_zero(uint32_t key) {
    SegPartial<L> p;
#pragma unroll
    for (int j = 0; j < L; j++)
        p.v[j] = 0.;
    p.key = key, p.n = 0u;
    return p;
}

// One block of the first stage, after its threads have loaded their entry (key 0xFFFFFFFF and zeros past the end of the list).  Out:
// write(key, v, n) stores a finished key; the outputs were cleared before, so a key without a run keeps its zeros.
template <int L, class Out>
__device__ inline void seg_block_sums(SegScanLds<L>& s, uint32_t nKeys, uint32_t key, double (&v)[L], uint32_t cnt, const Out& out,
                                      SegPartial<L>* __restrict__ partial) {
    const uint32_t t = threadIdx.x;
    seg_scan<L>(s, t, key, v, cnt);
    const uint32_t first = s.key[0], last = s.key[255];
    const bool runEnd = t == 255 || s.key[t + 1] != key;
    if (runEnd && key == first)
        partial[2 * blockIdx.x] = seg_partial<L>(v, key, cnt);
    if (t == 255)  // (one run from end to end: its sum is in the first partial, and this one adds nothing to it)
        partial[2 * blockIdx.x + 1] = last != first ? seg_partial<L>(v, key, cnt) : seg_partial_zero<L>(key);
    if (runEnd && key != first && key != last && key < nKeys)
        out.write(key, v, cnt);
}

// the second stage: one workgroup over the partials in workgroup order
template <int L, class Out>
__device__ inline void seg_final_sums(SegScanLds<L>& s, SegPartial<L>& carryLds, uint32_t nPartials, uint32_t nKeys,
                                      const SegPartial<L>* __restrict__ partial, const Out& out) {
    const uint32_t t = threadIdx.x;
    SegPartial<L> carry = seg_partial_zero<L>(0xFFFFFFFFu);  // the run the round before ended with: the same in every thread
    for (uint32_t base = 0; base < nPartials; base += 256) {
        SegPartial<L> p = seg_partial_zero<L>(0xFFFFFFFFu);
        if (base + t < nPartials)
            p = partial[base + t];
        seg_scan<L>(s, t, p.key, p.v, p.n);
        if (s.key[0] >= nKeys)  // (the partials ascend: nothing counted from here on)
            break;
        if (p.key == carry.key) {
#pragma unroll
            for (int j = 0; j < L; j++)
                p.v[j] = carry.v[j] + p.v[j];
            p.n = carry.n + p.n;
        } else if (t == 0 && carry.key < nKeys) {  // the carried run ended with its round
            out.write(carry.key, carry.v, carry.n);
        }
        if (t < 255 && s.key[t + 1] != p.key && p.key < nKeys)
            out.write(p.key, p.v, p.n);
        if (t == 255)
            carryLds = p;
        __syncthreads();
        carry = carryLds;
        __syncthreads();  // (the next round writes s and carryLds again)
    }
    if (t == 0 && carry.key < nKeys)
        out.write(carry.key, carry.v, carry.n);
}

// Term: term(e, v) fills the L lanes of sorted entry e (e < n, its key < nKeys; v comes zeroed) and returns its count, 0 or 1.
// Out: as above.  keys: the sorted keys; partial: 2 a block.  A block behind the counted entries writes two empty partials and
// leaves (the block's first entry is one of the list: the grid is grid_for(n), and n > 0).
template <int L, class Term, class Out>
__global__ __launch_bounds__(256) void k_seg_sums(uint32_t n, uint32_t nKeys, const uint32_t* __restrict__ keys, const Term term,
                                                  const Out out, SegPartial<L>* __restrict__ partial) {
    static_assert(SEG_BLOCK_ROWS == 256, "one entry a thread of a block of 256");
    __shared__ SegScanLds<L> s;
    const uint32_t t = threadIdx.x, e = blockIdx.x * SEG_BLOCK_ROWS + t;
    if (keys[blockIdx.x * SEG_BLOCK_ROWS] >= nKeys) {
        if (t < 2)
            partial[2 * blockIdx.x + t] = seg_partial_zero<L>(0xFFFFFFFFu);
        return;
    }
    const uint32_t key = e < n ? keys[e] : 0xFFFFFFFFu;
    double v[L];
#pragma unroll
    for (int j = 0; j < L; j++)
        v[j] = 0.;
    uint32_t cnt = 0;
    if (key < nKeys)
        cnt = term(e, v);
    seg_block_sums<L>(s, nKeys, key, v, cnt, out, partial);
}

template <int L, class Out>
__global__ __launch_bounds__(256) void k_seg_final(uint32_t nPartials, uint32_t nKeys, const SegPartial<L>* __restrict__ partial,
                                                   const Out out) {
    __shared__ SegScanLds<L> s;
    __shared__ SegPartial<L> carryLds;
    seg_final_sums<L>(s, carryLds, nPartials, nKeys, partial, out);
}

// terms and sums in plain arrays (deme_seg_sum_f64): n x L terms and nKeys x L sums, row-major; every entry counts 1
template <int L>
struct SegArrayTerm {
    const double* terms;
    __device__ uint32_t operator()(uint32_t e, double (&v)[L]) const {
#pragma unroll
        for (int j = 0; j < L; j++)
            v[j] = terms[(size_t)e * L + j];
        return 1u;
    }
};
template <int L>
struct SegArrayOut {
    double* sums;
    uint32_t* counts;
    __device__ void write(uint32_t key, const double (&v)[L], uint32_t n) const {
#pragma unroll
        for (int j = 0; j < L; j++)
            sums[(size_t)key * L + j] = v[j];
        counts[key] = n;
    }
};

}  // namespace deme_dev
