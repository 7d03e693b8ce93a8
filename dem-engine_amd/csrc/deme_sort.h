// deme_sort.h -- a stable least-significant-digit radix sort for the detection's lists (a few hundred thousand to a few million
// entries), built as reduce-then-scan: every pass is three launches on the caller's stream,
//
//   k_count      one workgroup per tile of TILE consecutive keys: the tile's histogram of the pass's digit, written as its column
//                of the table count[digit][tile] -- every entry, zeros included, so the table is never cleared
//   k_scan_rows  one workgroup per digit: the exclusive prefix of its row in place, the row's total beside the table
//   k_scatter    one workgroup per tile: ranks the tile's keys stably by the digit, lays them out by digit in LDS and stores each
//                digit's run at (digits below) + (this digit in the tiles before) + rank
//
// No workgroup waits for another inside a kernel, nothing is accumulated with global atomics and nothing is cleared: the kernels
// cannot hang, and the output is the one a stable sort has -- byte for byte what rocprim::radix_sort_* gives for the same range
// of bits.  Keys travel whole: bits outside [beginBit, endBit) take no part in the order and arrive unchanged.
//
// Order inside a tile (what makes the sort stable): wavefront w owns the tile's keys [w * 64 * KPT, (w + 1) * 64 * KPT), its lane l
// holds the keys l, 64 + l, 128 + l ... of them.  Item by item the lanes with equal digits find each other by ballots; a key's
// rank is the wavefront's count of the digit so far plus the equal lanes below it.  Wavefronts come in order through a prefix of
// their counts.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>
#include <rocprim/block/block_scan.hpp>

namespace deme_sort {

// The tile: 512 threads x 8 keys.  tools/sortbench on MI355X (profiles/r07/sort_shapes.txt), incidences / contact keys / crossing
// records at the flagship's sizes, in us: 256 x 16 184 / 110 / 72, 512 x 8 180 / 112 / 65, 512 x 12 186 / 104 / 76, 512 x 16
// 167 / 115 / 72 -- and at a tenth of the sizes 62 / 56 / 54, 52 / 48 / 46, 60 / 56 / 53, 69 / 65 / 61: a workgroup's time for
// one tile grows with the keys a thread ranks one after the other, and a short list is a single wave of tiles.
#ifndef DEME_SORT_THREADS
#define DEME_SORT_THREADS 512
#endif
#ifndef DEME_SORT_KPT
#define DEME_SORT_KPT 8
#endif
constexpr unsigned THREADS = DEME_SORT_THREADS, WAVE = 64, WAVES = THREADS / WAVE;  // of k_count and k_scatter
constexpr unsigned SCAN_THREADS = 256;                                              // of k_scan_rows
constexpr unsigned RB = 8, RADIX = 1u << RB;         // bits and values of a digit; a range's last pass may be narrower
constexpr unsigned KPT = DEME_SORT_KPT;              // keys per thread
constexpr unsigned TILE = THREADS * KPT;             // keys per workgroup
constexpr unsigned SCAN_IPT = 16;                    // table entries per thread and round of k_scan_rows
constexpr size_t MAX_N = (size_t)1 << 31;            // indices are 32-bit
static_assert(THREADS >= RADIX && THREADS % WAVE == 0, "one thread per digit in the histogram steps");
static_assert(WAVE == 64, "ballots are 64 lanes wide");

using BlockScan = rocprim::block_scan<uint32_t, THREADS>;
using RowScan = rocprim::block_scan<uint32_t, SCAN_THREADS>;

template <typename K>
__device__ inline unsigned digit_of(K k, unsigned shift, unsigned mask) {
    return (unsigned)(k >> shift) & mask;
}

template <typename K>
__global__ __launch_bounds__(THREADS) void k_count(const K* __restrict__ keys, uint32_t n, uint32_t nTiles, unsigned shift, unsigned nbits,
                                                   uint32_t* __restrict__ table) {
    // COPIES counters per digit, side by side, a lane adding to copy (lane % COPIES): equal digits of neighbouring lanes -- the rule in
    // a pass over a list that is nearly in order -- do not meet on one address.  tools/sortbench, profiles/r08/sort_ab.txt: 3 to 7 us
    // a sort ahead of one copy and level with a copy per wavefront; one add per group of equal digits found by ballots is far behind.
    // (The tile's keys are loaded before the first add: eight loads in flight, none waiting behind an atomic.)
    constexpr unsigned COPIES = 4;
    __shared__ uint32_t hist[COPIES * RADIX];
    const unsigned tid = threadIdx.x, tile = blockIdx.x, mask = (1u << nbits) - 1u;
    for (unsigned d = tid; d < COPIES * RADIX; d += THREADS)
        hist[d] = 0;
    __syncthreads();
    const uint32_t base = tile * TILE + tid;
    K k[KPT];
#pragma unroll
    for (unsigned i = 0; i < KPT; i++)
        k[i] = base + i * THREADS < n ? keys[base + i * THREADS] : K(0);
#pragma unroll
    for (unsigned i = 0; i < KPT; i++)
        if (base + i * THREADS < n)
            atomicAdd(&hist[digit_of(k[i], shift, mask) * COPIES + tid % COPIES], 1u);
    __syncthreads();
    if (tid <= mask) {
        uint32_t c = 0;
#pragma unroll
        for (unsigned j = 0; j < COPIES; j++)
            c += hist[tid * COPIES + j];
        table[(size_t)tid * nTiles + tile] = c;
    }
}

// row d of the table becomes its exclusive prefix; totals[d] the row's sum
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_rows(uint32_t* __restrict__ table, uint32_t nTiles, uint32_t* __restrict__ totals) {
    __shared__ typename RowScan::storage_type scanSt;
    uint32_t* row = table + (size_t)blockIdx.x * nTiles;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nTiles; base += SCAN_THREADS * SCAN_IPT) {
        const uint32_t first = base + threadIdx.x * SCAN_IPT;
        uint32_t v[SCAN_IPT], sum = 0;
#pragma unroll
        for (unsigned i = 0; i < SCAN_IPT; i++) {
            v[i] = first + i < nTiles ? row[first + i] : 0u;
            sum += v[i];
        }
        uint32_t excl, total;
        RowScan().exclusive_scan(sum, excl, 0u, total, scanSt);
        __syncthreads();  // (scanSt is used again by the next round)
        uint32_t run = carry + excl;
#pragma unroll
        for (unsigned i = 0; i < SCAN_IPT; i++) {
            if (first + i < nTiles)
                row[first + i] = run;
            run += v[i];
        }
        carry += total;
    }
    if (threadIdx.x == 0)
        totals[blockIdx.x] = carry;
}

template <typename K, bool HAS_V>
__global__ __launch_bounds__(THREADS) void k_scatter(const K* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t n, uint32_t nTiles,
                                                     unsigned shift, unsigned nbits, const uint32_t* __restrict__ table,
                                                     const uint32_t* __restrict__ totals, K* __restrict__ keysOut, uint32_t* __restrict__ valsOut) {
    __shared__ typename BlockScan::storage_type scanSt;
    __shared__ K sKeys[TILE];
    __shared__ uint32_t sVals[HAS_V ? TILE : 1];
    __shared__ uint32_t wcnt[WAVES * RADIX];  // per wavefront and digit: keys so far, then the first slot of its keys in the tile
    __shared__ uint32_t gbase[RADIX];         // per digit: (index in the output) - (slot in the tile)
    const unsigned tid = threadIdx.x, lane = tid % WAVE, w = tid / WAVE, tile = blockIdx.x, mask = (1u << nbits) - 1u;
    const uint32_t tile0 = tile * TILE, nValid = n - tile0 < TILE ? n - tile0 : TILE;
    for (unsigned d = tid; d < WAVES * RADIX; d += THREADS)
        wcnt[d] = 0;
    // a slot past the end of the input holds an all-ones key: the highest digit, and the last of it in input order, so the valid
    // keys take the tile's first nValid slots
    K k[KPT];
    uint32_t v[KPT], rank[KPT];
#pragma unroll
    for (unsigned i = 0; i < KPT; i++) {
        const uint32_t at = w * (WAVE * KPT) + i * WAVE + lane;
        k[i] = at < nValid ? keys[tile0 + at] : ~K(0);
        if (HAS_V)
            v[i] = at < nValid ? vals[tile0 + at] : 0u;
    }
    __syncthreads();
    // (the counters are this wavefront's alone and the LDS executes a wavefront's accesses in program order: every lane reads its
    // digit's count, then the highest lane of each group of equal digits adds the group -- no lane waits for another's result)
    uint32_t* wc = wcnt + w * RADIX;
#pragma unroll
    for (unsigned i = 0; i < KPT; i++) {
        const unsigned d = digit_of(k[i], shift, mask);
        unsigned long long same = ~0ull;  // the lanes whose digit equals this lane's
#pragma unroll
        for (unsigned b = 0; b < RB; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        const uint32_t before = __hip_atomic_load(wc + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        if ((same >> lane) == 1ull)  // (same holds this lane's bit: the highest lane of the group sees nothing above it)
            __hip_atomic_fetch_add(wc + d, (uint32_t)__popcll(same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        rank[i] = before + (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    // thread d: digit d's keys per wavefront -> where each wavefront's run of d starts in the tile, and in the output
    const unsigned dt = tid % RADIX;  // (the threads past the digits hold zeros and write nothing)
    uint32_t pre[WAVES], c = 0;
#pragma unroll
    for (unsigned j = 0; j < WAVES; j++) {
        pre[j] = c;
        c += tid < RADIX ? wcnt[j * RADIX + dt] : 0u;
    }
    uint32_t dstart, dbase;
    BlockScan().exclusive_scan(c, dstart, 0u, scanSt);
    __syncthreads();
    BlockScan().exclusive_scan(tid <= mask ? totals[tid] : 0u, dbase, 0u, scanSt);
    if (tid < RADIX) {
#pragma unroll
        for (unsigned j = 0; j < WAVES; j++)
            wcnt[j * RADIX + dt] = dstart + pre[j];
    }
    if (tid <= mask)
        gbase[tid] = dbase + table[(size_t)tid * nTiles + tile] - dstart;
    __syncthreads();
#pragma unroll
    for (unsigned i = 0; i < KPT; i++) {
        const uint32_t p = wcnt[w * RADIX + digit_of(k[i], shift, mask)] + rank[i];
        sKeys[p] = k[i];
        if (HAS_V)
            sVals[p] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (unsigned i = 0; i < KPT; i++) {
        const uint32_t p = i * THREADS + tid;
        if (p < nValid) {
            const K key = sKeys[p];
            const uint32_t o = gbase[digit_of(key, shift, mask)] + p;
            if (o < n) {  // (always, with a table that k_count and k_scan_rows made of this input)
                keysOut[o] = key;
                if (HAS_V)
                    valsOut[o] = sVals[p];
            }
        }
    }
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline unsigned passes_for(unsigned beginBit, unsigned endBit) { return (endBit - beginBit + RB - 1) / RB; }

// The two-call idiom of the rocprim device algorithms: with tmp == nullptr only `bytes` is set, to the scratch a list of up to
// max(n, cap) entries needs (the count table, and one list's room for the passes in between: the input is left as it is).
// Sorts keysIn (and valsIn) into keysOut (valsOut) by the bits [beginBit, endBit) of the key; n <= MAX_N.
template <typename K, bool HAS_V>
hipError_t radix_sort(void* tmp, size_t& bytes, const K* keysIn, K* keysOut, const uint32_t* valsIn, uint32_t* valsOut, size_t n, size_t cap,
                      unsigned beginBit, unsigned endBit, hipStream_t st) {
    const size_t room = n > cap ? n : cap, tilesRoom = (room + TILE - 1) / TILE;
    const size_t tableB = align256((tilesRoom + 1) * RADIX * 4), keysB = align256(room * sizeof(K)), valsB = HAS_V ? align256(room * 4) : 0;
    if (!tmp) {
        bytes = tableB + keysB + valsB;
        return hipSuccess;
    }
    if (bytes < tableB + keysB + valsB || room > MAX_N || endBit < beginBit || endBit > 8 * sizeof(K))
        return hipErrorInvalidValue;
    if (!n)
        return hipSuccess;
    const unsigned passes = passes_for(beginBit, endBit);
    if (!passes) {
        hipError_t e = hipMemcpyAsync(keysOut, keysIn, n * sizeof(K), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && HAS_V)
            e = hipMemcpyAsync(valsOut, valsIn, n * 4, hipMemcpyDeviceToDevice, st);
        return e;
    }
    uint32_t* table = reinterpret_cast<uint32_t*>(tmp);
    uint32_t* totals = table + tilesRoom * RADIX;
    K* keysAlt = reinterpret_cast<K*>(reinterpret_cast<char*>(tmp) + tableB);
    uint32_t* valsAlt = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(tmp) + tableB + keysB);
    const uint32_t nTiles = (uint32_t)((n + TILE - 1) / TILE);
    const K* kSrc = keysIn;
    const uint32_t* vSrc = valsIn;
    for (unsigned p = 0; p < passes; p++) {
        const unsigned shift = beginBit + p * RB, nbits = endBit - shift < RB ? endBit - shift : RB;
        const bool toOut = (passes - 1 - p) % 2 == 0;  // the last pass lands in the output
        K* kDst = toOut ? keysOut : keysAlt;
        uint32_t* vDst = toOut ? valsOut : valsAlt;
        hipLaunchKernelGGL(k_count<K>, dim3(nTiles), dim3(THREADS), 0, st, kSrc, (uint32_t)n, nTiles, shift, nbits, table);
        hipLaunchKernelGGL(k_scan_rows, dim3(1u << nbits), dim3(SCAN_THREADS), 0, st, table, nTiles, totals);
        hipLaunchKernelGGL((k_scatter<K, HAS_V>), dim3(nTiles), dim3(THREADS), 0, st, kSrc, vSrc, (uint32_t)n, nTiles, shift, nbits, table,
                           totals, kDst, vDst);
        kSrc = kDst, vSrc = vDst;
    }
    return hipGetLastError();
}

}  // namespace deme_sort
