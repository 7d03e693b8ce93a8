// micro-benchmark: the detection's three radix sorts, rocPRIM with the shipped DemeRadixCfg against the project's own sort
// (dem-engine_amd/csrc/deme_sort.h), in one process on one GPU, at the flagship's list sizes and at 1/10 and 1/100 of them.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 [-DDEME_SORT_KPT=8] -o tools/sortbench/sb_own tools/sortbench/sortbench.hip
//   timeout -k 10 300 tools/sortbench/sb_own [repeats] > profiles/r07/sort_ab.txt
// Every repeat times the whole call between two events (rocPRIM's clears included), rocPRIM and own alternating; the table gives
// the best and the median of the repeats and their spread (max - min), and checks that both outputs are byte for byte the same.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "../../dem-engine_amd/csrc/deme_sort.h"

// as in dem-engine_amd/csrc/deme_hip.hip
template <unsigned RB, unsigned IPT = 8>
using DemeRadixCfg = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                                rocprim::radix_sort_onesweep_config<rocprim::kernel_config<1024, IPT>, rocprim::kernel_config<1024, IPT>, RB,
                                                                                    rocprim::block_radix_rank_algorithm::match>,
                                                1024 * 1024>;

static void ck(hipError_t e, const char* what, int line) {
    if (e != hipSuccess) {
        fprintf(stderr, "sortbench.hip:%d: %s: %s\n", line, what, hipGetErrorString(e));
        exit(1);
    }
}
#define CK(x) ck((x), #x, __LINE__)

static bool allIdentical = true;
struct Stat {
    float best, median, spread;
};
static Stat stat_of(std::vector<float> t) {
    std::sort(t.begin(), t.end());
    return {t.front(), t[t.size() / 2], t.back() - t.front()};
}

// uneven digit populations, as the engine's keys have them
static uint32_t bin_id(std::mt19937& g) {  // a cube of 100^3 occupied bins in a grid of 160^3 (22 bits)
    const uint32_t x = g() % 100u, y = g() % 100u, z = g() % 100u;
    return x + 160u * (y + 160u * z);
}
static uint32_t owner_id(std::mt19937& g) {  // 20 bits, the low ids several times as frequent as the high ones
    const uint64_t a = g() & 0xFFFFFu, b = g() & 0xFFFFFu;
    return (uint32_t)((a * b) >> 20);
}
static uint64_t contact_key(std::mt19937& g) {  // A << 33 | class << 31 | B over 3e6 spheres: 24 bits from bit 31
    const uint64_t a = g() % 3000000u, b = g() % 3000000u, cls = (g() % 16u) ? 0u : 1u;
    return a << 33 | cls << 31 | b;
}

template <class Cfg, typename K, bool HAS_V>
static void run_shape(const char* name, size_t n, unsigned b0, unsigned b1, int repeats, K (*draw)(std::mt19937&)) {
    std::vector<K> hk(n);
    std::vector<uint32_t> hv(n);
    std::mt19937 g(7);
    for (size_t i = 0; i < n; i++)
        hk[i] = draw(g), hv[i] = (uint32_t)i;
    K *k0, *kR, *kO;
    uint32_t *v0 = nullptr, *vR = nullptr, *vO = nullptr;
    CK(hipMalloc(&k0, n * sizeof(K))), CK(hipMalloc(&kR, n * sizeof(K))), CK(hipMalloc(&kO, n * sizeof(K)));
    CK(hipMemcpy(k0, hk.data(), n * sizeof(K), hipMemcpyHostToDevice));
    if (HAS_V) {
        CK(hipMalloc(&v0, n * 4)), CK(hipMalloc(&vR, n * 4)), CK(hipMalloc(&vO, n * 4));
        CK(hipMemcpy(v0, hv.data(), n * 4, hipMemcpyHostToDevice));
    }
    auto roc = [&](void* tmp, size_t& bytes) {
        if constexpr (HAS_V)
            return rocprim::radix_sort_pairs<Cfg>(tmp, bytes, k0, kR, v0, vR, n, b0, b1, 0);
        else
            return rocprim::radix_sort_keys<Cfg>(tmp, bytes, k0, kR, n, b0, b1, 0);
    };
    auto own = [&](void* tmp, size_t& bytes) { return deme_sort::radix_sort<K, HAS_V>(tmp, bytes, k0, kO, v0, vO, n, n, b0, b1, 0); };
    size_t needR = 0, needO = 0;
    CK(roc(nullptr, needR)), CK(own(nullptr, needO));
    void *tmpR, *tmpO;
    CK(hipMalloc(&tmpR, needR)), CK(hipMalloc(&tmpO, needO));
    hipEvent_t a, b;
    CK(hipEventCreate(&a)), CK(hipEventCreate(&b));
    std::vector<float> tR, tO;
    for (int it = -2; it < repeats; it++) {  // (two warm-up rounds)
        for (int which = 0; which < 2; which++) {
            float ms;
            CK(hipEventRecord(a, 0));
            CK(which ? own(tmpO, needO) : roc(tmpR, needR));
            CK(hipEventRecord(b, 0));
            CK(hipEventSynchronize(b));
            CK(hipEventElapsedTime(&ms, a, b));
            if (it >= 0)
                (which ? tO : tR).push_back(ms * 1e3f);
        }
    }
    std::vector<K> oR(n), oO(n);
    CK(hipMemcpy(oR.data(), kR, n * sizeof(K), hipMemcpyDeviceToHost)), CK(hipMemcpy(oO.data(), kO, n * sizeof(K), hipMemcpyDeviceToHost));
    bool same = memcmp(oR.data(), oO.data(), n * sizeof(K)) == 0;
    if (HAS_V) {
        std::vector<uint32_t> wR(n), wO(n);
        CK(hipMemcpy(wR.data(), vR, n * 4, hipMemcpyDeviceToHost)), CK(hipMemcpy(wO.data(), vO, n * 4, hipMemcpyDeviceToHost));
        same = same && memcmp(wR.data(), wO.data(), n * 4) == 0;
    }
    allIdentical = allIdentical && same;
    const Stat r = stat_of(tR), o = stat_of(tO);
    printf("%-22s %9zu  [%2u,%2u)  rocprim %7.1f %7.1f %6.1f   own %7.1f %7.1f %6.1f   own/rocprim %.2f  identical %d\n", name, n, b0, b1,
           r.best, r.median, r.spread, o.best, o.median, o.spread, o.best / r.best, (int)same);
    fflush(stdout);
    hipFree(k0), hipFree(kR), hipFree(kO), hipFree(v0), hipFree(vR), hipFree(vO), hipFree(tmpR), hipFree(tmpO);
    hipEventDestroy(a), hipEventDestroy(b);
}

int main(int argc, char** argv) {
    const int repeats = argc > 1 ? atoi(argv[1]) : 9;
    printf("# times in us: best, median, spread (max - min) of %d interleaved repeats; own: tile %u keys (%u threads x %u), %u-bit digits\n",
           repeats, deme_sort::TILE, deme_sort::THREADS, deme_sort::KPT, deme_sort::RB);
    printf("# %-20s %9s  %7s  %31s   %27s\n", "shape", "n", "bits", "rocprim (DemeRadixCfg)", "own");
    for (size_t div : {1, 10, 100}) {
        run_shape<DemeRadixCfg<11, 16>, uint32_t, true>("incidence pairs", 8200000 / div, 0, 22, repeats, bin_id);
        run_shape<DemeRadixCfg<8>, uint64_t, false>("contact keys u64", 4300000 / div, 31, 55, repeats, contact_key);
        run_shape<DemeRadixCfg<10>, uint32_t, true>("crossing-record pairs", 1800000 / div, 0, 20, repeats, owner_id);
    }
    return allIdentical ? 0 : 1;
}
