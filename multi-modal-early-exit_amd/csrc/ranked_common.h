// Device code shared by the tools that work on dumped (E1, N, K) arrays -- the ranked sweeps (exit_ops.hip), the two threshold searches
// (threshold_search.hip, threshold_search_cost.hip) and the evaluation report (exit_metrics.hip) -- and, for the quota rank, by the forward's
// exit stage (exit_stage.hip).  __device__ __forceinline__ functions only:
// the percentile lerp and the candidate vectors' digits of the searches, and the loops these tools are built from, each written here
// and nowhere else (metrics_curve_kernel excepted, see exit_metrics.hip): ranked_walk, stable_rank_by_counting, quota_rank_by_counting, block1024_scan.
// SearchVectors and SweepRanks are declared in mmee_kernels.h.
#pragma once
#include "mmee_kernels.h"

namespace mmee {

constexpr int kSearchChunkWords = (64 * 1024) / 4;      // the document chunk of ranked_walk: 64 KB of rank records

// numpy's _lerp (lib/_function_base_impl.py), operation by operation: a + (b - a) t, and b - (b - a)(1 - t) where t >= 0.5.  Every product is
// rounded before it is added: a fused multiply-add would change the last bit.
__device__ __forceinline__ double percentile_lerp(double a, double b, double t) {
#pragma clang fp contract(off)
    const double diff = b - a;
    double r = a + diff * t;
    if (t >= 0.5) r = b - diff * (1.0 - t);
    return r;
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

// The ranked walk of a workgroup of 256 threads, one THREAD per threshold vector: the N documents' rank records (rec: rows of E1P words,
// rec[e] = rank << 8 | correct << 6 | e) are streamed through s_rec in chunks of `chunk` documents, and every thread walks every document.
//   exit = first e with rec[e] >= tq(e), else 0 (numpy argmax of an all-False column):  r = rec[0]; for e = E1 - 1 .. 0: r = rec[e] >= tq(e) ? rec[e] : r
// -- two vector instructions per exit, a record read at the same address in every lane (a broadcast) -- and per_document(i, r) receives the
// selected record of document i of the chunk, whose payload bits give (correct, exit).
//   E1C > 0: compile-time exit count, the exit loop unrolled (tq(e) is a register); 0: run-time E1.
//   tq(e)         the thread's rank word of exit e
//   stage(n0, i)  called beside the copy of uint4 i of the chunk that starts at document n0: what else the caller keeps in LDS per chunk
template <int E1C, typename RankWord, typename Stage, typename PerDocument>
__device__ __forceinline__ void ranked_walk(const unsigned* __restrict__ rec, unsigned* s_rec, int E1, int E1P, int N, int chunk, RankWord&& tq,
                                            Stage&& stage, PerDocument&& per_document) {
    for (int n0 = 0; n0 < N; n0 += chunk) {
        const int cnt = N - n0 < chunk ? N - n0 : chunk;
        __syncthreads();
        {
            const uint4* src = reinterpret_cast<const uint4*>(rec + (size_t)n0 * E1P);
            uint4* dst = reinterpret_cast<uint4*>(s_rec);
            const int n16 = cnt * E1P / 4;
            for (int i = threadIdx.x; i < n16; i += 256) {
                dst[i] = src[i];
                stage(n0, i);
            }
        }
        __syncthreads();
        if (E1C > 0) {
#pragma unroll 4
            for (int i = 0; i < cnt; ++i) {
                const unsigned* d = s_rec + i * E1P;                 // the same address in every lane: a broadcast read
                const unsigned d0 = d[0];
                unsigned r = d0;                                     // no exit fires: exit 0
#pragma unroll
                for (int e = E1C - 1; e >= 1; --e) {
                    const unsigned x = d[e];
                    r = x >= tq(e) ? x : r;
                }
                r = d0 >= tq(0) ? d0 : r;                            // exit 0 fires: it is the first
                per_document(i, r);
            }
        } else {
            for (int i = 0; i < cnt; ++i) {
                const unsigned* d = s_rec + i * E1P;
                const unsigned d0 = d[0];
                unsigned r = d0;
                for (int e = E1 - 1; e >= 1; --e) {
                    const unsigned x = d[e];
                    r = x >= tq(e) ? x : r;
                }
                r = d0 >= tq(0) ? d0 : r;
                per_document(i, r);
            }
        }
    }
}

// The stable ascending place of row[n] among row[0 .. N) by counting, for a workgroup of 256 threads with n = 256 blockIdx.x + threadIdx.x:
// (lt, eq_before) = (#{m : row[m] < row[n]}, #{m < n : row[m] == row[n]}), so that lt is the value's rank and lt + eq_before a permutation in
// which equal values keep their order.  The row passes through `tile` (2048 doubles of LDS); a thread with n >= N counts for 0.0 and is ignored.
__device__ __forceinline__ uint2 stable_rank_by_counting(const double* __restrict__ row, int N, int n, double* tile) {
    const double c = n < N ? row[n] : 0.0;
    unsigned lt = 0, eq_before = 0;
    for (int m0 = 0; m0 < N; m0 += 2048) {
        __syncthreads();
        for (int i = threadIdx.x; i < 2048; i += 256) tile[i] = m0 + i < N ? row[m0 + i] : 0.0;
        __syncthreads();
        const int cnt = N - m0 < 2048 ? N - m0 : 2048;
        for (int i = 0; i < cnt; ++i) {
            const double x = tile[i];
            lt += x < c ? 1u : 0u;
            eq_before += (x == c && m0 + i < n) ? 1u : 0u;
        }
    }
    return make_uint2(lt, eq_before);
}

// The quota rank (include/mmee.h, at ee_set_quotas) by the same counting, for a workgroup of 256 threads: how many of the n documents
// (key_at(j), slot_at(j)), j = 0 .. n-1, precede the thread's own (key, slot) -- a larger quota_key, or the same key and a lower slot.  Slots
// are distinct, so over the n documents the result is a permutation of 0 .. n-1.  The documents pass through t_key / t_slot (2048 entries of
// LDS each); a key of 0 ("no document") precedes nobody, and a thread without a document of its own still loads and counts, its result ignored.
// Per pair: two broadcast LDS reads, two 64-bit compares and one 32-bit compare; nothing is added in floating point.
template <typename KeyAt, typename SlotAt>
__device__ __forceinline__ unsigned quota_rank_by_counting(unsigned long long key, int slot, int n, KeyAt&& key_at, SlotAt&& slot_at,
                                                           unsigned long long* t_key, int* t_slot) {
    unsigned before = 0;
    for (int m0 = 0; m0 < n; m0 += 2048) {
        __syncthreads();
        for (int i = threadIdx.x; i < 2048; i += 256) {
            const bool in = m0 + i < n;
            t_key[i] = in ? key_at(m0 + i) : 0ull;
            t_slot[i] = in ? slot_at(m0 + i) : 0;
        }
        __syncthreads();
        const int cnt = n - m0 < 2048 ? n - m0 : 2048;
#pragma unroll 4
        for (int i = 0; i < cnt; ++i) {
            const unsigned long long k = t_key[i];
            const int sl = t_slot[i];
            before += k > key ? 1u : 0u;
            before += (k == key && sl < slot) ? 1u : 0u;
        }
    }
    return before;
}

// A scan over the 1024 threads of a workgroup in thread order, for an associative and commutative `op` on integers (any order of combining
// gives the same bits; floating-point sums do not belong here).  exclusive / inclusive: over the threads before this one / and this one;
// total: over all 1024, the same value in every thread.  `slots`: 16 words of LDS, one per wave.  The barrier between writing and reading the
// slots is inside; a caller that scans chunk after chunk keeps its running carry and a barrier before the slots are written again.
template <typename T>
struct BlockScan {
    T exclusive, inclusive, total;
};

// the cross-wave half: from a thread's prefixes inside its wave and the wave's total (read from lane 63)
template <typename T, typename Op>
__device__ __forceinline__ BlockScan<T> block1024_across_waves(T exclusive, T inclusive, T wave_total, T identity, Op&& op, T* slots) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 63) slots[wave] = wave_total;
    __syncthreads();
    T total = identity;
    for (int k = 0; k < 16; ++k) {
        const T w = slots[k];
        if (k < wave) {
            exclusive = op(w, exclusive);
            inclusive = op(w, inclusive);
        }
        total = op(w, total);
    }
    return {exclusive, inclusive, total};
}

// wave inclusive prefix by shuffles -> cross-wave prefix through the slots
template <typename T, typename Op>
__device__ __forceinline__ BlockScan<T> block1024_scan(T v, T identity, Op&& op, T* slots) {
    const int lane = threadIdx.x & 63;
    T m = v;
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(m, o, 64);
        if (lane >= o) m = op(t, m);
    }
    T below = __shfl_up(m, 1, 64);
    if (lane == 0) below = identity;
    return block1024_across_waves(below, m, m, identity, op, slots);
}

// the sum of a flag (a thread's dense place among the flagged ones): ballot -> popcount inside the wave, no shuffles
__device__ __forceinline__ BlockScan<int> block1024_count(bool flag, int* slots) {
    const unsigned long long ballot = __ballot(flag);
    const int below = __popcll(ballot & ((1ull << (threadIdx.x & 63)) - 1ull));
    return block1024_across_waves(below, below + (flag ? 1 : 0), (int)__popcll(ballot), 0, [](int a, int b) { return a + b; }, slots);
}

}  // namespace mmee
