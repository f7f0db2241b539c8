// The threshold search (ee_threshold_search, include/mmee.h): candidate thresholds from the percentiles of the confidence table, every candidate
// vector scored, and the accuracy / mean-exit Pareto front of the scores -- all on the device.  It replaces what a caller of ee_threshold_sweep
// did on the host (EE/large_scale.py:46-65: per-exit percentiles, random mixtures of them; then an upload of V x E1 doubles, a binary search per
// threshold, a download of V x 2 doubles and a front in numpy).
//
// The ranking pass is the sweeps' own (SweepRanks, exit_ops.hip): rec[n][e] = rank << 8 | correct << 6 | e and every exit's confidences SORTED.
//   search_table_kernel   E1 x P threads: table[e][j] = the j-th of P percentiles of exit e, one lerp of two neighbours of the sorted row, and
//                         trank[e][j] = its rank word by sweep_thr_kernel's rule.  A candidate vector is E1 digits in [0, P): its E1 rank words
//                         are E1 lookups in this E1 x P table -- no threshold is uploaded and none is searched per vector.
//   search_main_kernel    ranked_walk (ranked_common.h: one THREAD per vector, documents as LDS broadcasts, two vector instructions per exit), the
//                         thread's rank words built from its digits -- decoded from the vector's index (grid), hashed (sampled) or loaded
//                         (mixtures) -- through trank in LDS.  Under the POLICY's semantics the last rank word is 0: every document "fires" at
//                         the final exit, which makes it the fallback with no branch in the loop.  One 64-bit atomic max per vector:
//                         bucket[exit_sum] = max(hits << 32 | ~v): the most hits per exit sum, ties to the LOWEST vector index.  Deterministic.
//   search_front_kernel   one workgroup over the buckets in ascending exit sum: a bucket is on the front iff its hits exceed every lower
//                         bucket's (prefix max with a running carry), compacted by its dense place among the kept (block1024_scan and
//                         block1024_count, ranked_common.h).
#include "ranked_common.h"

namespace mmee {

__global__ __launch_bounds__(256) void search_table_kernel(const double* __restrict__ sorted, int E1, int N, int P, SearchPercentiles pc, int strict,
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

void launch_search_table(const double* sorted, int E1, int N, int P, const SearchPercentiles& pc, int strict, double* table, unsigned* trank, hipStream_t s) {
    hipLaunchKernelGGL(search_table_kernel, dim3((E1 * P + 255) / 256), dim3(256), 0, s, sorted, E1, N, P, pc, strict, table, trank);
}

template <int E1C>      // E1C > 0: compile-time exit count (unrolled, rank words in registers); 0: run-time E1 (rank words in the thread's private array)
__global__ __launch_bounds__(256, 2) void search_main_kernel(const unsigned* __restrict__ rec, const unsigned* __restrict__ trank, SearchVectors sv,
                                                             int E1, int E1P, int N, int P, int policy, double* __restrict__ acc,
                                                             double* __restrict__ mean_exit, unsigned long long* __restrict__ buckets) {
    extern __shared__ unsigned s_mem[];                              // CHUNK documents x E1P words, then trank (E1 x P words)
    unsigned* s_rec = s_mem;
    unsigned* s_trank = s_mem + kSearchChunkWords;
    const int chunk = kSearchChunkWords / E1P;
    for (int i = threadIdx.x; i < E1 * P; i += 256) s_trank[i] = trank[i];
    __syncthreads();
    const unsigned long long v = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned vv = v < sv.V ? (unsigned)v : sv.V - 1u;
    const int n_e = E1C > 0 ? E1C : E1;
    unsigned tq[E1C > 0 ? E1C : 64];
    if constexpr (E1C > 0) {
        unsigned dg[E1C];
        search_digits(sv, vv, E1, P, E1C - 1, [&](int e, unsigned d) { dg[e] = d; });
#pragma unroll
        for (int e = 0; e < E1C - 1; ++e) tq[e] = s_trank[e * P + dg[e]];
    } else {
        search_digits(sv, vv, E1, P, E1 - 1, [&](int e, unsigned d) { tq[e] = s_trank[e * P + d]; });
    }
    tq[n_e - 1] = policy ? 0u : s_trank[(n_e - 1) * P];              // POLICY: the final exit takes whoever is left; REFERENCE: the rank of 0.0
    unsigned n_correct = 0, sum_exit = 0;                            // REFERENCE: no exit fires -> exit 0; under POLICY the final exit always fires
    ranked_walk<E1C>(rec, s_rec, E1, E1P, N, chunk, [&](int e) { return tq[e]; }, [](int, int) {}, [&](int, unsigned r) {
        n_correct += (r >> 6) & 1u;
        sum_exit += r & 63u;
    });
    if (v < sv.V) {
        if (acc) acc[v] = (double)n_correct / (double)N;
        if (mean_exit) mean_exit[v] = (double)sum_exit / (double)N;
        atomicMax(&buckets[sum_exit], ((unsigned long long)n_correct << 32) | (unsigned long long)(0xFFFFFFFFu - vv));
    }
}

// One workgroup of 1024 threads walks the buckets in chunks of 1024, ascending exit sum.  A bucket word is 0 (no vector has this exit sum: the
// low half of a written word is 0xFFFFFFFF - v >= 1) or hits << 32 | ~v of its best vector.
//   on the front  <=>  hits > the hits of every LOWER bucket: the exclusive prefix max of the chunk and a running carry;
//   dense place   the exclusive count of the kept and a running carry: ascending exit sum, as emit_leavers_kernel ranks.
// Each kept thread writes its entry and gathers its threshold row from `table` by the vector's digits.
__global__ __launch_bounds__(1024) void search_front_kernel(const unsigned long long* __restrict__ buckets, int n_buckets, SearchVectors sv, int E1,
                                                            int P, const double* __restrict__ table, int cap, int* __restrict__ front_count,
                                                            int* __restrict__ front_exit_sum, int* __restrict__ front_hits,
                                                            unsigned* __restrict__ front_vector, double* __restrict__ front_thr) {
    __shared__ int s_max[16];
    __shared__ int s_cnt[16];
    const auto imax = [](int a, int b) { return a > b ? a : b; };
    const int tid = threadIdx.x;
    int carry_max = -1, carry_cnt = 0;                               // over the chunks so far: the same values in every thread
    for (int base = 0; base < n_buckets; base += 1024) {
        const int i = base + tid;
        const unsigned long long w = i < n_buckets ? buckets[i] : 0ull;
        const int h = w ? (int)(w >> 32) : -1;                       // hits <= N < 2^24
        const BlockScan<int> lower = block1024_scan(h, -1, imax, s_max);
        const bool keep = h > imax(carry_max, lower.exclusive);      // an empty bucket (h = -1) never is
        const BlockScan<int> kept = block1024_count(keep, s_cnt);
        const int pos = carry_cnt + kept.exclusive;
        if (keep && pos < cap) {
            const unsigned v = 0xFFFFFFFFu - (unsigned)(w & 0xFFFFFFFFull);
            front_exit_sum[pos] = i;
            front_hits[pos] = h;
            front_vector[pos] = v;
            double* row = front_thr + (size_t)pos * E1;
            search_digits(sv, v, E1, P, E1 - 1, [&](int e, unsigned d) { row[e] = table[e * P + d]; });
            row[E1 - 1] = table[(E1 - 1) * P];
        }
        carry_max = imax(carry_max, lower.total);
        carry_cnt += kept.total;
        __syncthreads();                                             // s_max and s_cnt are rewritten by the next chunk
    }
    if (tid == 0) front_count[0] = carry_cnt;
}

// false: a workspace allocation failed and nothing was launched
bool launch_threshold_search(const SearchArgs& a, const SearchPercentiles& pc, hipStream_t s) {
    const int E1P = (a.E1 + 3) & ~3, n_buckets = a.N * (a.E1 - 1) + 1, policy = a.semantics == SEARCH_POLICY ? 1 : 0;
    const SweepRanks r(a.conf, a.correct, a.E1, E1P, a.N, nullptr, 0, policy, s);
    if (!r.ok) return false;
    unsigned* trank = nullptr;
    unsigned long long* buckets = nullptr;
    if (hipMallocAsync((void**)&trank, (size_t)a.E1 * a.P * 4, s) != hipSuccess || hipMallocAsync((void**)&buckets, (size_t)n_buckets * 8, s) != hipSuccess) {
        (void)hipGetLastError();
        if (trank) (void)hipFreeAsync(trank, s);
        return false;
    }
    (void)hipMemsetAsync(buckets, 0, (size_t)n_buckets * 8, s);
    launch_search_table(r.sorted, a.E1, a.N, a.P, pc, policy, a.table, trank, s);
    const SearchVectors sv{a.source, a.V, a.seed, a.mixtures};
    const unsigned grid = (unsigned)(((unsigned long long)a.V + 255) / 256);
    const size_t lds = (size_t)kSearchChunkWords * 4 + (size_t)a.E1 * a.P * 4;
    (void)ensure_dynamic_lds<&search_main_kernel<7>>("search_main_kernel", 80 * 1024);
    (void)ensure_dynamic_lds<&search_main_kernel<0>>("search_main_kernel", 80 * 1024);
    if (a.E1 == 7)
        hipLaunchKernelGGL((search_main_kernel<7>), dim3(grid), dim3(256), lds, s, r.rec, trank, sv, a.E1, E1P, a.N, a.P, policy, a.acc, a.mean_exit, buckets);
    else
        hipLaunchKernelGGL((search_main_kernel<0>), dim3(grid), dim3(256), lds, s, r.rec, trank, sv, a.E1, E1P, a.N, a.P, policy, a.acc, a.mean_exit, buckets);
    hipLaunchKernelGGL(search_front_kernel, dim3(1), dim3(1024), 0, s, buckets, n_buckets, sv, a.E1, a.P, a.table, a.N + 1, a.front_count,
                       a.front_exit_sum, a.front_hits, a.front_vector, a.front_thresholds);
    (void)hipFreeAsync(trank, s);
    (void)hipFreeAsync(buckets, s);
    return true;
}

}  // namespace mmee
