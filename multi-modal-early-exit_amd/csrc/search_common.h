// Device code shared by the two threshold searches (threshold_search.hip: the accuracy / mean-exit front; threshold_search_cost.hip: the
// accuracy / cost front): the percentile table, the candidate vectors' digits.  SearchVectors, SearchPercentiles and SweepRanks are declared in
// mmee_kernels.h.
#pragma once
#include "mmee_kernels.h"

namespace mmee {

constexpr int kSearchChunkWords = (64 * 1024) / 4;      // the document chunk of sweep_main_kernel: 64 KB of rank records

// numpy's _lerp (lib/_function_base_impl.py), operation by operation: a + (b - a) t, and b - (b - a)(1 - t) where t >= 0.5.  Every product is
// rounded before it is added: a fused multiply-add would change the last bit.
__device__ __forceinline__ double percentile_lerp(double a, double b, double t) {
#pragma clang fp contract(off)
    const double diff = b - a;
    double r = a + diff * t;
    if (t >= 0.5) r = b - diff * (1.0 - t);
    return r;
}

// inline: both searches launch it, each translation unit carries its own copy of the code object
inline __global__ __launch_bounds__(256) void search_table_kernel(const double* __restrict__ sorted, int E1, int N, int P, SearchPercentiles pc, int strict,
                                                                  double* __restrict__ table, unsigned* __restrict__ trank) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= E1 * P) return;
    const int e = i / P, j = i - e * P;
    const double* row = sorted + (size_t)e * N;
    const double t = e < E1 - 1 ? percentile_lerp(row[pc.lo[j]], row[pc.hi[j]], pc.t[j]) : 0.0;      // the final exit's row: 0.0 (generate_thresholds)
    int lo = 0, hi = N;                                              // sweep_thr_kernel's search and its rank word
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (strict ? row[mid] <= t : row[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    table[i] = t;
    trank[i] = t != t ? 0xffffffffu : (unsigned)lo << 8;
}

// splitmix64's finaliser
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// f(e, digit) for e = 0 .. n - 1 in order: the digits of candidate vector v (include/mmee.h MMEE_SEARCH_GRID / _SAMPLED / _MIXTURES)
template <typename F>
__device__ __forceinline__ void search_digits(const SearchVectors& sv, unsigned v, int E1, int P, int n, F&& f) {
    if (sv.source == SEARCH_GRID) {
        unsigned q = v;
        for (int e = 0; e < n; ++e) {
            const unsigned next = q / (unsigned)P;
            f(e, q - next * (unsigned)P);
            q = next;
        }
    } else if (sv.source == SEARCH_SAMPLED) {
        for (int e = 0; e < n; ++e) {
            const unsigned long long z = splitmix64(sv.seed + ((unsigned long long)v * (unsigned)E1 + (unsigned)e + 1ull) * 0x9E3779B97F4A7C15ull);
            f(e, (unsigned)(((z >> 32) * (unsigned long long)P) >> 32));
        }
    } else {
        for (int e = 0; e < n; ++e) {
            const unsigned d = sv.mixtures[(size_t)v * E1 + e];
            f(e, d < (unsigned)P ? d : (unsigned)P - 1u);             // a digit >= P is the caller's error: clamped, nothing is read out of bounds
        }
    }
}

}  // namespace mmee
