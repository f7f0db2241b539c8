// The handle-free tools on dumped (E1, N, K) arrays: the exit policies as one scan kernel, the patience / threshold / rule sweeps, the
// criterion tables (max-softmax, entropy, margin), the temperature fit, and result packing.  (The forward pass's own exit stage: exit_stage.hip.)
//
// What this replaces in the reference:
//   * Policy.max_confidence_global_thresholding_policy / accuracy_calibration_heuristic (EE/policy.py:28-45, 87-104): the nested Python loop
//     "first exit whose float64 max-softmax is strictly above its threshold, else the last" is exit_scan_kernel<SCAN_MSP, RULE_PLAIN>,
//     bit-identical in its integer outputs.
//   * thresh.opt0_2D / large_scale.check_2D_threshold (EE/thresh.py:184-215, EE/large_scale.py:42-84): threshold_sweep.
#include "ranked_common.h"

namespace mmee {

// the float64 max-softmax, entropy and margin of one row (max_softmax_f64, entropy_f64, margin_f64) and the row of a criterion table
// (csf_row_f64) are in mmee_kernels.h: the cascade's deferral test (cascade.hip) calls the same functions

// the criterion a scan event computes from the row itself
template <int EVENT>
__device__ __forceinline__ double row_crit_f64(const double* z, int K) {
    static_assert(EVENT == SCAN_MSP || EVENT == SCAN_ENTROPY || EVENT == SCAN_MARGIN, "events that read the logits row");
    if constexpr (EVENT == SCAN_ENTROPY) return entropy_f64(z, K);
    else if constexpr (EVENT == SCAN_MARGIN) return margin_f64(z, K);
    else return max_softmax_f64(z, K);
}

// argmax of one float64 row, first maximum (as numpy)
__device__ __forceinline__ int argmax_f64(const double* z, int K) {
    double m = z[0];
    int am = 0;
    for (int k = 1; k < K; ++k)
        if (z[k] > m) { m = z[k]; am = k; }
    return am;
}

// ---------------------------------------------------------------------------------------------------------------
// The exit decision on dumped arrays (ee_policy_scan, ee_patience_scan, ee_lte_scan, ee_rule_scan): thread per document, exits in order,
// the first e < E1 - 1 that qualifies, else the final exit E1 - 1, whose own test and patience are never looked at.
//   event      f_e = sign * crit_e > sign * thr[e]   (sign = +1: confidence, strict '>'; -1: entropy / LTE score, strict '<'; negation is exact)
//              crit_e: SCAN_MSP / SCAN_ENTROPY / SCAN_MARGIN the float64 max-softmax / entropy / margin of the row, SCAN_TABLE crit[e][n],
//              SCAN_NONE no event
//   agreement  c_e (PABEE): p_e = argmax_k logits[e][n][k] (first maximum), c_0 = 0, c_e = p_e == p_{e-1} ? c_{e-1} + 1 : 0
//   RULE_PLAIN: f_e;   RULE_STREAK: s_e = f_e ? s_{e-1} + 1 : 0, s_e >= pat[e];   RULE_EITHER: f_e or c_e >= pat[e];   RULE_AGREE: c_e >= pat[e]
// confidence = the event's criterion at the chosen exit; SCAN_NONE: the float64 max-softmax of the chosen row.  The logits are read only where the
// instantiation needs a row (the row events, the agreement, pred, SCAN_NONE's confidence): they may be null otherwise.
// ---------------------------------------------------------------------------------------------------------------
template <int EVENT, int RULE>
__global__ __launch_bounds__(256) void exit_scan_kernel(ScanArgs a) {
    static_assert((EVENT == SCAN_NONE) == (RULE == RULE_AGREE), "without an event only the agreement can decide, and RULE_AGREE looks at no event");
    for (int n = blockIdx.x * 256 + threadIdx.x; n < a.N; n += gridDim.x * 256) {
        const auto row = [&](int e) { return a.logits + ((size_t)e * a.N + n) * a.K; };
        int chosen = a.E1 - 1, prev = -1, run = 0, streak = 0;
        double crit = 0.0;
        for (int e = 0; e < a.E1 - 1; ++e) {
            bool leave = false;
            if constexpr (EVENT != SCAN_NONE) {
                if constexpr (EVENT == SCAN_TABLE) crit = a.crit[(size_t)e * a.N + n];
                else crit = row_crit_f64<EVENT>(row(e), a.K);
                leave = a.sign * crit > a.sign * a.thr[e];
            }
            if constexpr (RULE != RULE_PLAIN) {
                const int pat = a.pat ? a.pat[e] : a.pat_all;
                if constexpr (RULE == RULE_STREAK) {
                    streak = leave ? streak + 1 : 0;
                    leave = streak >= pat;
                } else {
                    const int am = argmax_f64(row(e), a.K);
                    run = (e > 0 && am == prev) ? run + 1 : 0;
                    prev = am;
                    leave = leave || run >= pat;
                }
            }
            if (leave) { chosen = e; break; }
        }
        a.exits[n] = chosen;
        if (a.conf) {
            if constexpr (EVENT == SCAN_TABLE) a.conf[n] = a.crit[(size_t)chosen * a.N + n];
            else if constexpr (EVENT == SCAN_NONE) a.conf[n] = max_softmax_f64(row(chosen), a.K);
            else a.conf[n] = chosen < a.E1 - 1 ? crit : row_crit_f64<EVENT>(row(chosen), a.K);
        }
        if (a.pred) {
            const double* z = row(chosen);
            for (int k = 0; k < a.K; ++k) a.pred[(size_t)n * a.K + k] = z[k];
        }
        if (a.counts) atomicAdd(&a.counts[chosen], 1);
    }
}

// the seven (event, rule) pairs the entry points ask for
void launch_exit_scan(const ScanArgs& a, int event, int rule, hipStream_t s) {
    void (*k)(ScanArgs) = event == SCAN_MSP       ? exit_scan_kernel<SCAN_MSP, RULE_PLAIN>
                          : event == SCAN_ENTROPY ? exit_scan_kernel<SCAN_ENTROPY, RULE_PLAIN>
                          : event == SCAN_MARGIN ? exit_scan_kernel<SCAN_MARGIN, RULE_PLAIN>
                          : event == SCAN_NONE ? exit_scan_kernel<SCAN_NONE, RULE_AGREE>
                          : rule == RULE_PLAIN ? exit_scan_kernel<SCAN_TABLE, RULE_PLAIN>
                          : rule == RULE_STREAK ? exit_scan_kernel<SCAN_TABLE, RULE_STREAK>
                                                : exit_scan_kernel<SCAN_TABLE, RULE_EITHER>;
    hipLaunchKernelGGL(k, dim3(grid_1d(a.N, 256, 4096)), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------------------------------------------
// Patience sweep: V patience values over one dumped (E1, N, K) array.  Thread per document; the run sequence is computed ONCE:
// since c_e grows by exactly one inside a run, the first exit with c_e >= t is the first with c_e == t, so the walk records
// first[c] (c = 1 .. longest run) in LDS as (exit << 1 | correct) and every t is then one lookup (t beyond the longest run: the final
// exit).  Hits, exit sums and the histogram are integers (per-block LDS sums, one 64-bit atomic per block and value): the results do not
// depend on the order of arrival.  E1 <= kPatMaxE1.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kPatMaxE1 = 128;
constexpr int kPatBlock = 128;

__global__ __launch_bounds__(kPatBlock) void patience_sweep_kernel(const double* __restrict__ logits, const long long* __restrict__ refs,
                                                                   int E1, int N, int K, const int* __restrict__ pats, int V,
                                                                   unsigned long long* __restrict__ sums, int* __restrict__ hist) {
    __shared__ unsigned short s_first[(kPatMaxE1 - 1) * kPatBlock];
    __shared__ int s_hist[kPatMaxE1];
    __shared__ unsigned long long s_red[kPatBlock / 64][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x * kPatBlock + tid;
    const bool active = n < N;
    int longest = 0;
    unsigned rec0 = 0, recE = 0;                                     // records of exit 0 (t < 1) and of the final exit
    if (active) {
        const long long ref = refs[n];
        int prev = -1, run = 0;
        for (int e = 0; e < E1; ++e) {
            const int am = argmax_f64(logits + ((size_t)e * N + n) * K, K);
            run = (e > 0 && am == prev) ? run + 1 : 0;
            prev = am;
            const unsigned rec = ((unsigned)e << 1) | (am == ref ? 1u : 0u);
            if (e == 0) rec0 = rec;
            if (e == E1 - 1) recE = rec;
            if (run > longest) { longest = run; s_first[(run - 1) * kPatBlock + tid] = (unsigned short)rec; }
        }
    }
    for (int v = 0; v < V; ++v) {
        const int t = pats[v];
        if (hist) {
            for (int e = tid; e < E1; e += kPatBlock) s_hist[e] = 0;
            __syncthreads();
        }
        unsigned long long hits = 0, exs = 0;
        if (active) {
            const unsigned rec = t < 1 ? rec0 : t <= longest ? (unsigned)s_first[(t - 1) * kPatBlock + tid] : recE;
            hits = rec & 1u;
            exs = rec >> 1;
            if (hist) atomicAdd(&s_hist[rec >> 1], 1);
        }
        for (int o = 32; o > 0; o >>= 1) {
            hits += __shfl_xor(hits, o, 64);
            exs += __shfl_xor(exs, o, 64);
        }
        if (lane == 0) { s_red[wave][0] = hits; s_red[wave][1] = exs; }
        __syncthreads();
        if (tid == 0) {
            unsigned long long h = 0, x = 0;
            for (int w = 0; w < kPatBlock / 64; ++w) { h += s_red[w][0]; x += s_red[w][1]; }
            atomicAdd(&sums[2 * v], h);
            atomicAdd(&sums[2 * v + 1], x);
        }
        if (hist)
            for (int e = tid; e < E1; e += kPatBlock)
                if (s_hist[e]) atomicAdd(&hist[(size_t)v * E1 + e], s_hist[e]);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void patience_sweep_finish_kernel(const unsigned long long* __restrict__ sums, int V, int N,
                                                                    double* __restrict__ acc, double* __restrict__ mean_exit) {
    for (int v = blockIdx.x * 256 + threadIdx.x; v < V; v += gridDim.x * 256) {
        acc[v] = (double)sums[2 * v] / (double)N;
        mean_exit[v] = (double)sums[2 * v + 1] / (double)N;
    }
}

bool launch_patience_sweep(const double* logits, const long long* refs, int E1, int N, int K, const int* pats, int V, double* acc,
                           double* mean_exit, int* hist, hipStream_t s) {
    unsigned long long* sums = nullptr;
    if (hipMallocAsync((void**)&sums, sizeof(unsigned long long) * 2 * V, s) != hipSuccess) return false;
    (void)hipMemsetAsync(sums, 0, sizeof(unsigned long long) * 2 * V, s);
    if (hist) (void)hipMemsetAsync(hist, 0, sizeof(int) * (size_t)V * E1, s);
    hipLaunchKernelGGL(patience_sweep_kernel, dim3((N + kPatBlock - 1) / kPatBlock), dim3(kPatBlock), 0, s, logits, refs, E1, N, K, pats, V,
                       sums, hist);
    hipLaunchKernelGGL(patience_sweep_finish_kernel, dim3(grid_1d(V, 256, 1024)), dim3(256), 0, s, sums, V, N, acc, mean_exit);
    (void)hipFreeAsync(sums, s);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------
// Threshold sweep: one workgroup per threshold vector, documents strided over its 256 threads.
//   exit(v, n) = first e with conf[e][n] >= thr[v][e], else 0 (numpy argmax of an all-False column)
// conf is (E1, N) so consecutive threads read consecutive documents of the same exit row (coalesced).
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void threshold_sweep_kernel(const double* __restrict__ conf, const unsigned char* __restrict__ correct,
                                                              int E1, int N, const double* __restrict__ thr, int V,
                                                              double* __restrict__ acc, double* __restrict__ mean_exit,
                                                              int* __restrict__ hist) {
    __shared__ double s_thr[64];
    __shared__ int s_hist[64];
    __shared__ unsigned long long s_red[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int v = blockIdx.x; v < V; v += gridDim.x) {
        __syncthreads();
        if (tid < E1) { s_thr[tid] = thr[(size_t)v * E1 + tid]; s_hist[tid] = 0; }
        __syncthreads();
        unsigned int n_correct = 0, sum_exit = 0;
        for (int n = tid; n < N; n += 256) {
            int ex = 0;
            for (int e = 0; e < E1; ++e) {
                if (conf[(size_t)e * N + n] >= s_thr[e]) { ex = e; break; }
            }
            n_correct += correct[(size_t)ex * N + n];
            sum_exit += ex;
            if (hist) atomicAdd(&s_hist[ex], 1);
        }
        unsigned long long packed = ((unsigned long long)n_correct << 32) | (unsigned long long)sum_exit;
        for (int o = 32; o > 0; o >>= 1) packed += __shfl_xor(packed, o, 64);
        if (lane == 0) s_red[wave] = packed;
        __syncthreads();
        if (tid == 0) {
            const unsigned long long t = s_red[0] + s_red[1] + s_red[2] + s_red[3];
            acc[v] = (double)(t >> 32) / (double)N;
            mean_exit[v] = (double)(t & 0xffffffffull) / (double)N;
        }
        if (hist && tid < E1) hist[(size_t)v * E1 + tid] = s_hist[tid];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The sweep at the reference's scale (EE/large_scale.py:46-84 with num_mixtures = 1 500 000 threshold vectors, :179-180).  The kernel above
// re-reads the whole (E1, N) float64 table for every vector (2.2 MB x 1.5 M = 3.4 TB of cache traffic) and compares doubles.  Only the
// ORDER of conf[e][n] and thr[v][e] matters, so the comparison is done on integer ranks instead:
//     p[e][n] = #{m : conf[e][m] < conf[e][n]},   t[v][e] = #{m : conf[e][m] < thr[v][e]}      =>      conf[e][n] >= thr[v][e]  <=>  p[e][n] >= t[v][e]
// (>=: every element below thr is below conf, so t <= p; <: conf itself and everything below it is below thr, so t >= p + 1).  Exact for any
// doubles, ties and duplicates included (NaN confidences do not occur: they are softmax maxima).
//   1. sweep_rank_kernel   p by counting (stable_rank_by_counting, ranked_common.h: N^2 / exit, 1.1e10 double compares at 7 x 40 000: ~1 ms)
//                          and, with the tie index from the same pass, the sorted confidences of every exit;
//   2. sweep_thr_kernel    t by binary search in the sorted row;
//   3. sweep_main_kernel   one THREAD per threshold vector (its E1 ranks in registers, its two sums in registers: no reduction across
//                          lanes), the documents streamed through LDS as records  rec[e] = p << 8 | correct << 6 | e: ranked_walk
//                          (ranked_common.h), which hands over the selected record; its payload bits give (correct, exit).  Integer work
//                          per (vector, document): 2 E1 + 4 instructions.
// The table is read once per 256 vectors from L2 (1.3 MB x V / 256).  Needs N < 2^24 and E1 <= 64; the histogram output stays on the kernel above.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sweep_rank_kernel(const double* __restrict__ conf, const unsigned char* __restrict__ correct, int E1, int E1P,
                                                         int N, unsigned* __restrict__ rec, double* __restrict__ sorted) {
    __shared__ double tile[2048];
    const int e = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
    const double* row = conf + (size_t)e * N;
    const uint2 place = stable_rank_by_counting(row, N, n, tile);   // (lt, eq_before), ranked_common.h
    if (n < N) {
        rec[(size_t)n * E1P + e] = (place.x << 8) | ((unsigned)(correct[(size_t)e * N + n] ? 1u : 0u) << 6) | (unsigned)e;
        sorted[(size_t)e * N + place.x + place.y] = row[n];          // equal values take consecutive places in document order
    }
}

// strict != 0 (the rule sweep, conf > thr): t = #{m : conf[e][m] <= thr[v][e]}, so that conf[e][n] > thr[v][e]  <=>  p[e][n] >= t[v][e]
// (>: everything at or below thr is below conf, so t <= p; <=: conf itself and everything below it is at or below thr, so t >= p + 1)
__global__ __launch_bounds__(256) void sweep_thr_kernel(const double* __restrict__ sorted, const double* __restrict__ thr, int E1, int N, long long VE,
                                                        unsigned* __restrict__ T, int strict) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < VE; i += (long long)gridDim.x * 256) {
        const int e = (int)(i % E1);
        const double t = thr[i];
        const double* row = sorted + (size_t)e * N;
        int lo = 0, hi = N;                                          // first index with row[idx] >= t  =  number of confidences below t
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (strict ? row[mid] <= t : row[mid] < t) lo = mid + 1;
            else hi = mid;
        }
        T[i] = t != t ? 0xffffffffu : (unsigned)lo << 8;             // conf >= NaN is false for every document (numpy): a word no record reaches
    }
}

template <int E1C>      // E1C > 0: compile-time exit count (unrolled, ranks in registers); 0: run-time E1 (ranks re-read from the vector's row)
__global__ __launch_bounds__(256, 2) void sweep_main_kernel(const unsigned* __restrict__ rec, const unsigned* __restrict__ T, int E1, int E1P, int N,
                                                            int V, double* __restrict__ acc, double* __restrict__ mean_exit) {
    extern __shared__ unsigned s_rec[];                              // CHUNK documents x E1P words
    const int chunk = (64 * 1024) / (4 * E1P);
    const int v = blockIdx.x * 256 + threadIdx.x;
    const int vv = v < V ? v : V - 1;
    unsigned tq[E1C > 0 ? E1C : 1];
    if (E1C > 0) {
#pragma unroll
        for (int e = 0; e < E1C; ++e) tq[e] = T[(size_t)vv * E1 + e];
    }
    unsigned n_correct = 0, sum_exit = 0;
    const auto rank_word = [&](int e) {
        if constexpr (E1C > 0) return tq[e];
        else return T[(size_t)vv * E1 + e];
    };
    ranked_walk<E1C>(rec, s_rec, E1, E1P, N, chunk, rank_word, [](int, int) {}, [&](int, unsigned r) {
        n_correct += (r >> 6) & 1u;
        sum_exit += r & 63u;
    });
    if (v < V) {
        acc[v] = (double)n_correct / (double)N;
        mean_exit[v] = (double)sum_exit / (double)N;
    }
}

// The ranking step of the ranked sweeps and of the threshold search (SweepRanks, mmee_kernels.h): rec (zeroed, then sweep_rank_kernel), sorted,
// and, with thr, T = the thresholds' ranks (sweep_thr_kernel).
SweepRanks::SweepRanks(const double* conf, const unsigned char* correct, int E1, int E1P, int N, const double* thr, int V, int strict, hipStream_t stream)
    : s(stream) {
    const bool with_T = thr && V > 0;
    ok = hipMallocAsync((void**)&rec, (size_t)N * E1P * 4, s) == hipSuccess && (!with_T || hipMallocAsync((void**)&T, (size_t)V * E1 * 4, s) == hipSuccess) &&
         hipMallocAsync((void**)&sorted, (size_t)E1 * N * 8, s) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); return; }
    (void)hipMemsetAsync(rec, 0, (size_t)N * E1P * 4, s);
    hipLaunchKernelGGL(sweep_rank_kernel, dim3((N + 255) / 256, E1), dim3(256), 0, s, conf, correct, E1, E1P, N, rec, sorted);
    if (!with_T) return;
    const long long VE = (long long)V * E1;
    hipLaunchKernelGGL(sweep_thr_kernel, dim3(grid_1d(VE, 256, 65536)), dim3(256), 0, s, sorted, thr, E1, N, VE, T, strict);
}
SweepRanks::~SweepRanks() {
    if (rec) (void)hipFreeAsync(rec, s);
    if (T) (void)hipFreeAsync(T, s);
    if (sorted) (void)hipFreeAsync(sorted, s);
}

void launch_threshold_sweep(const double* conf, const unsigned char* correct, int E1, int N, const double* thr, int V,
                            double* acc, double* mean_exit, int* hist, hipStream_t s) {
    // ranks: the integer sweep (no histogram, N < 2^24, enough vectors to pay for the O(N^2) ranking pass)
    const bool ranked = !hist && N < (1 << 24) && E1 <= 64 && (long long)V * 8 >= (long long)N;
    if (ranked) {
        const int E1P = (E1 + 3) & ~3;
        const SweepRanks r(conf, correct, E1, E1P, N, thr, V, 0, s);
        if (r.ok) {                                                  // else: the direct kernel needs no workspace
            const int grid = (V + 255) / 256;
            const size_t lds = 64 * 1024;
            (void)ensure_dynamic_lds<&sweep_main_kernel<7>>("sweep_main_kernel", (int)lds);
            (void)ensure_dynamic_lds<&sweep_main_kernel<0>>("sweep_main_kernel", (int)lds);
            if (E1 == 7) hipLaunchKernelGGL((sweep_main_kernel<7>), dim3(grid), dim3(256), lds, s, r.rec, r.T, E1, E1P, N, V, acc, mean_exit);
            else hipLaunchKernelGGL((sweep_main_kernel<0>), dim3(grid), dim3(256), lds, s, r.rec, r.T, E1, E1P, N, V, acc, mean_exit);
            return;
        }
    }
    hipLaunchKernelGGL(threshold_sweep_kernel, dim3(grid_1d(V, 1, 8192)), dim3(256), 0, s, conf, correct, E1, N, thr, V, acc, mean_exit, hist);
}

// ---------------------------------------------------------------------------------------------------------------
// Rule sweep (ee_rule_sweep): V threshold vectors x P patience values over one dumped array, the POLICY's semantics (strict compare, the
// final exit when nothing qualifies), integer sums.  The event is conf > thr (the host negates table and thresholds for '<' criteria).
//   rule_table_kernel   per (e, n): correct = (argmax == reference), agree = PABEE's counter c_e (<= 63: E1 <= 64)
//   rule_sweep_kernel   any E1 <= 64, P <= kRuleMaxP, histogram: one workgroup per threshold vector, documents strided over its threads.
//                       patience_sweep_kernel's trick: a counter that grows by one (the streak s_e; the agreement c_e) reaches t first where
//                       it EQUALS t, so ONE walk records first[c] in LDS and every patience value is a lookup.  EITHER: the walk stops at
//                       the first event; levels never reached take that exit.
//   rule_main_kernel    the reference's search scale (E1 = 7, P <= 8, no histogram), on sweep_main_kernel's integer ranks: one THREAD per
//                       threshold vector, documents as LDS broadcasts, conf > thr as the exact rank compare rec >= T (sweep_thr_kernel,
//                       strict).  Beside its E1 rank words a document brings (rule_aux_kernel) the mask of its correct exits and, per
//                       patience value, its PABEE exit -- both independent of the thresholds.  STREAK: the walk keeps first[c] as 4-bit
//                       entries of one register (entry c at bits 4c, stored as exit ^ E so that an entry never written reads as E); patience
//                       j is one bit-field extract.  EITHER: exit = min(plain exit, PABEE exit j).  Sums per chunk in one packed word.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kRuleMaxP = 128;
constexpr int kRuleFastP = 8;

__global__ __launch_bounds__(256) void rule_table_kernel(const double* __restrict__ logits, const long long* __restrict__ refs, int E1, int N, int K,
                                                         unsigned char* __restrict__ correct, unsigned char* __restrict__ agree) {
    for (int n = blockIdx.x * 256 + threadIdx.x; n < N; n += gridDim.x * 256) {
        const long long ref = refs[n];
        int prev = -1, run = 0;
        for (int e = 0; e < E1; ++e) {
            const int am = argmax_f64(logits + ((size_t)e * N + n) * K, K);
            run = (e > 0 && am == prev) ? run + 1 : 0;
            prev = am;
            correct[(size_t)e * N + n] = am == ref ? 1 : 0;
            agree[(size_t)e * N + n] = (unsigned char)run;
        }
    }
}

__global__ __launch_bounds__(256) void rule_sweep_kernel(const double* __restrict__ conf, const unsigned char* __restrict__ correct,
                                                         const unsigned char* __restrict__ agree, int E1, int N, const double* __restrict__ thr, int V,
                                                         const int* __restrict__ pats, int P, int rule, double* __restrict__ acc,
                                                         double* __restrict__ mean_exit, int* __restrict__ hist) {
    __shared__ double s_thr[64];
    __shared__ unsigned char s_first[63 * 256];                    // [level - 1][thread]: first exit where the counter reached the level
    __shared__ unsigned s_hits[kRuleMaxP], s_exs[kRuleMaxP];
    __shared__ int s_hist[kRuleMaxP * 64];
    const int tid = threadIdx.x, E = E1 - 1;
    for (int v = blockIdx.x; v < V; v += gridDim.x) {
        __syncthreads();
        if (tid < E1) s_thr[tid] = thr[(size_t)v * E1 + tid];
        for (int j = tid; j < P; j += 256) { s_hits[j] = 0; s_exs[j] = 0; }
        if (hist)
            for (int i = tid; i < P * E1; i += 256) s_hist[i] = 0;
        __syncthreads();
        for (int n = tid; n < N; n += 256) {
            int longest = 0, streak = 0, stop = E;                   // stop: the exit of every level the walk never reached
            for (int e = 0; e < E; ++e) {
                const bool f = conf[(size_t)e * N + n] > s_thr[e];
                int c;
                if (rule == RULE_STREAK) c = streak = f ? streak + 1 : 0;
                else c = agree[(size_t)e * N + n];
                if (c > longest) { longest = c; s_first[(c - 1) * 256 + tid] = (unsigned char)e; }
                if (rule == RULE_EITHER && f) { stop = e; break; }
            }
            for (int j = 0; j < P; ++j) {
                const int t = pats[j];
                const int ex = t <= longest ? (int)s_first[(t - 1) * 256 + tid] : stop;
                atomicAdd(&s_hits[j], (unsigned)correct[(size_t)ex * N + n]);
                atomicAdd(&s_exs[j], (unsigned)ex);
                if (hist) atomicAdd(&s_hist[j * E1 + ex], 1);
            }
        }
        __syncthreads();
        for (int j = tid; j < P; j += 256) {
            acc[(size_t)v * P + j] = (double)s_hits[j] / (double)N;
            mean_exit[(size_t)v * P + j] = (double)s_exs[j] / (double)N;
        }
        if (hist)
            for (int i = tid; i < P * E1; i += 256) hist[(size_t)v * P * E1 + i] = s_hist[i];
    }
}

// patience values of the fast kernel, a kernel ARGUMENT (uniform: they live in scalar registers)
struct RulePats {
    int t[kRuleFastP];
    int P;
};

// per document: aux[4 n] = mask of its correct exits, aux[4 n + 1 .. 2] = its PABEE exit for patience j in byte j (first e < E with c_e >= t_j, else E)
__global__ __launch_bounds__(256) void rule_aux_kernel(const unsigned char* __restrict__ correct, const unsigned char* __restrict__ agree, int E1, int N,
                                                       RulePats pt, unsigned* __restrict__ aux) {
    for (int n = blockIdx.x * 256 + threadIdx.x; n < N; n += gridDim.x * 256) {
        unsigned mask = 0, pab[2] = {0, 0};
        for (int e = 0; e < E1; ++e) mask |= (unsigned)(correct[(size_t)e * N + n] ? 1u : 0u) << e;
        for (int j = 0; j < kRuleFastP; ++j) {
            int ex = E1 - 1;
            if (j < pt.P)
                for (int e = 0; e < E1 - 1; ++e)
                    if ((int)agree[(size_t)e * N + n] >= pt.t[j]) { ex = e; break; }
            pab[j >> 2] |= (unsigned)ex << (8 * (j & 3));
        }
        *reinterpret_cast<uint4*>(aux + (size_t)4 * n) = uint4{mask, pab[0], pab[1], 0u};
    }
}

template <int E1C, int RULE>
__global__ __launch_bounds__(256, 2) void rule_main_kernel(const unsigned* __restrict__ rec, const unsigned* __restrict__ aux, const unsigned* __restrict__ T,
                                                           int N, int V, RulePats pt, double* __restrict__ acc, double* __restrict__ mean_exit) {
    static_assert(E1C >= 2 && E1C <= 8, "4-bit entries at bits 4c, c <= E1C - 1 <= 7");
    extern __shared__ unsigned s_rec[];                              // CHUNK documents x (E1P rank words + 4 aux words)
    constexpr int E1P = (E1C + 3) & ~3, E = E1C - 1, RW = E1P + 4;
    constexpr int chunk = (64 * 1024) / (4 * RW);                    // <= 2048 documents: a chunk's packed sums stay below 2^20 / 2^12
    const int v = blockIdx.x * 256 + threadIdx.x;
    const int vv = v < V ? v : V - 1;
    unsigned tq[E1C];
#pragma unroll
    for (int e = 0; e < E1C; ++e) tq[e] = T[(size_t)vv * E1C + e];
    int t4[kRuleFastP];                                              // STREAK: bit position of the entry of patience j; t > E: an entry no walk writes
#pragma unroll
    for (int j = 0; j < kRuleFastP; ++j) t4[j] = 4 * (pt.t[j] < E1C ? pt.t[j] : E1C);
    unsigned n_correct[kRuleFastP], sum_exit[kRuleFastP];
#pragma unroll
    for (int j = 0; j < kRuleFastP; ++j) n_correct[j] = sum_exit[j] = 0;
    for (int n0 = 0; n0 < N; n0 += chunk) {
        const int cnt = N - n0 < chunk ? N - n0 : chunk;
        __syncthreads();
        {
            const uint4* src = reinterpret_cast<const uint4*>(rec + (size_t)n0 * E1P);
            const uint4* asrc = reinterpret_cast<const uint4*>(aux + (size_t)n0 * 4);
            uint4* dst = reinterpret_cast<uint4*>(s_rec);
            for (int i = threadIdx.x; i < cnt * (RW / 4); i += 256) {
                const int d = i / (RW / 4), w = i - d * (RW / 4);
                dst[i] = w < E1P / 4 ? src[d * (E1P / 4) + w] : asrc[d];
            }
        }
        __syncthreads();
        unsigned pk[kRuleFastP];                                     // correct << 20 | exit, summed over the chunk
#pragma unroll
        for (int j = 0; j < kRuleFastP; ++j) pk[j] = 0;
#pragma unroll 2
        for (int i = 0; i < cnt; ++i) {
            const unsigned* d = s_rec + i * RW;                      // the same address in every lane: a broadcast read
            const unsigned cmask = d[E1P];
            if (RULE == RULE_STREAK) {
                unsigned tab = 0;
                int s4 = 0, l4 = 0;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    s4 = d[e] >= tq[e] ? s4 + 4 : 0;
                    const unsigned set = tab | ((unsigned)(e ^ E) << s4);
                    tab = s4 > l4 ? set : tab;
                    l4 = s4 > l4 ? s4 : l4;
                }
#pragma unroll
                for (int j = 0; j < kRuleFastP; ++j)
                    if (j < pt.P) {
                        const unsigned ex = ((tab >> t4[j]) & 7u) ^ (unsigned)E;
                        pk[j] += ex + (((cmask >> ex) & 1u) << 20);
                    }
            } else {
                unsigned r = E;                                      // no event: the final exit
#pragma unroll
                for (int e = E - 1; e >= 0; --e) r = d[e] >= tq[e] ? (unsigned)e : r;
#pragma unroll
                for (int j = 0; j < kRuleFastP; ++j)
                    if (j < pt.P) {
                        const unsigned pab = (d[E1P + 1 + (j >> 2)] >> (8 * (j & 3))) & 255u;
                        const unsigned ex = pab < r ? pab : r;
                        pk[j] += ex + (((cmask >> ex) & 1u) << 20);
                    }
            }
        }
#pragma unroll
        for (int j = 0; j < kRuleFastP; ++j) { n_correct[j] += pk[j] >> 20; sum_exit[j] += pk[j] & 0xfffffu; }
    }
    if (v < V) {
#pragma unroll
        for (int j = 0; j < kRuleFastP; ++j)
            if (j < pt.P) {
                acc[(size_t)v * pt.P + j] = (double)n_correct[j] / (double)N;
                mean_exit[(size_t)v * pt.P + j] = (double)sum_exit[j] / (double)N;
            }
    }
}

// pats_host: the P patience values (the fast kernel takes them by value), pats_dev: the same on the device
bool launch_rule_sweep(const double* conf, const double* logits, const long long* refs, int E1, int N, int K, const double* thr, int V,
                       const int* pats_host, const int* pats_dev, int P, int rule, double* acc, double* mean_exit, int* hist, hipStream_t s) {
    unsigned char *correct = nullptr, *agree = nullptr;
    if (hipMallocAsync((void**)&correct, (size_t)E1 * N, s) != hipSuccess || hipMallocAsync((void**)&agree, (size_t)E1 * N, s) != hipSuccess) {
        (void)hipGetLastError();
        if (correct) (void)hipFreeAsync(correct, s);
        return false;
    }
    const int g0 = grid_1d(N, 256, 4096);
    hipLaunchKernelGGL(rule_table_kernel, dim3(g0), dim3(256), 0, s, logits, refs, E1, N, K, correct, agree);
    // the ranked kernel: the reference's shape, no histogram, enough vectors to pay for the O(N^2) ranking pass (as launch_threshold_sweep)
    bool done = false;
    if (!hist && E1 == 7 && P <= kRuleFastP && N < (1 << 24) && (long long)V * 8 >= (long long)N) {
        constexpr int E1P = 8;
        unsigned* aux = nullptr;
        const SweepRanks r(conf, correct, E1, E1P, N, thr, V, 1, s);
        if (r.ok && hipMallocAsync((void**)&aux, (size_t)N * 16, s) == hipSuccess) {
            RulePats pt{};
            pt.P = P;
            for (int j = 0; j < kRuleFastP; ++j) pt.t[j] = j < P ? pats_host[j] : 1;
            hipLaunchKernelGGL(rule_aux_kernel, dim3(g0), dim3(256), 0, s, correct, agree, E1, N, pt, aux);
            const size_t lds = 64 * 1024;
            const bool ok = ensure_dynamic_lds<&rule_main_kernel<7, RULE_STREAK>>("rule_main_kernel", (int)lds) == hipSuccess &&
                            ensure_dynamic_lds<&rule_main_kernel<7, RULE_EITHER>>("rule_main_kernel", (int)lds) == hipSuccess;
            if (ok) {
                const int grid = (V + 255) / 256;
                if (rule == RULE_STREAK)
                    hipLaunchKernelGGL((rule_main_kernel<7, RULE_STREAK>), dim3(grid), dim3(256), lds, s, r.rec, aux, r.T, N, V, pt, acc, mean_exit);
                else
                    hipLaunchKernelGGL((rule_main_kernel<7, RULE_EITHER>), dim3(grid), dim3(256), lds, s, r.rec, aux, r.T, N, V, pt, acc, mean_exit);
                done = true;
            }
        } else {
            (void)hipGetLastError();                                 // allocation failed: the direct kernel needs no workspace
        }
        if (aux) (void)hipFreeAsync(aux, s);
    }
    if (!done) {
        hipLaunchKernelGGL(rule_sweep_kernel, dim3(grid_1d(V, 1, 8192)), dim3(256), 0, s, conf, correct, agree, E1, N, thr, V, pats_dev, P, rule, acc, mean_exit, hist);
    }
    (void)hipFreeAsync(correct, s);
    (void)hipFreeAsync(agree, s);
    return true;
}

// The criterion table of the sweeps and rule scans (ee_csf_table; ee_msp_table is its CRIT_MAX_CONFIDENCE instantiation):
// table[e][n] = max softmax / entropy / margin (f64) of logits[e][n][:], correct[e][n] = (argmax == reference[n])   (first maximum wins, as numpy)
template <int CRIT>
__global__ __launch_bounds__(256) void csf_table_kernel(const double* __restrict__ logits, const long long* __restrict__ refs,
                                                        int E1, int N, int K, double* __restrict__ conf,
                                                        unsigned char* __restrict__ correct) {
    const size_t total = (size_t)E1 * N;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        int am;
        conf[i] = csf_row_f64(CRIT, logits + i * K, K, am);
        if (correct) correct[i] = refs ? (unsigned char)(refs[i % N] == am) : 0;
    }
}

void launch_csf_table(const double* logits, const long long* refs, int E1, int N, int K, int criterion, double* table, unsigned char* correct,
                      hipStream_t s) {
    void (*k)(const double*, const long long*, int, int, int, double*, unsigned char*) =
        criterion == CRIT_ENTROPY ? csf_table_kernel<CRIT_ENTROPY> : criterion == CRIT_MARGIN ? csf_table_kernel<CRIT_MARGIN>
                                                                                                : csf_table_kernel<CRIT_MAX_CONFIDENCE>;
    hipLaunchKernelGGL(k, dim3(grid_1d((long long)E1 * N, 256, 4096)), dim3(256), 0, s, logits, refs, E1, N, K, table, correct);
}

// The criterion table of MMEE_CRIT_GATE (ee_gate_table): table[e][n] = gate_score_f64 of the raw gate logits head[e][n][0 .. 1], the function
// the decide kernels call, for the E exits that have a gate; row E, the final exit's max-softmax, is csf_table_kernel<CRIT_MAX_CONFIDENCE>'s
__global__ __launch_bounds__(256) void gate_table_kernel(const float* __restrict__ head, size_t total, double* __restrict__ table) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256)
        table[i] = gate_score_f64(head[2 * i], head[2 * i + 1]);
}

void launch_gate_table(const float* head_logits, const double* final_logits, int E, int N, int K, double* table, hipStream_t s) {
    const size_t total = (size_t)E * N;
    if (total) hipLaunchKernelGGL(gate_table_kernel, dim3(grid_1d((long long)total, 256, 4096)), dim3(256), 0, s, head_logits, total, table);
    launch_csf_table(final_logits, nullptr, 1, N, K, CRIT_MAX_CONFIDENCE, table + total, nullptr, s);
}

// The exit ensemble on a dumped array (ee_ensemble_logits; definition in include/mmee.h), by the two device functions of the forward's launch
// (mmee_kernels.h).  Two launches: l[e][n][k] of every row into `out` (also the l table of the ensemble fit, ensemble_fit.hip), then the
// combination in place -- a thread owns one (n, k) column of `out` and walks the exits from the last down, so what it reads below exit m is
// still l.  A NaN row gives NaN l, and fma(0, NaN, a) is NaN: NaN from that exit on, whatever w holds.  Every value rounded through float32,
// as the forward writes it.
__global__ __launch_bounds__(256) void ensemble_logsoftmax_kernel(const double* __restrict__ logits, size_t rows, int K, double* __restrict__ l) {
    const size_t total = rows * (size_t)K;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const size_t r = t / K;
        const double* x = logits + r * K;
        l[t] = ens_logsoftmax_f64([&](int j) { return x[j]; }, K, (int)(t - r * K));
    }
}

__global__ __launch_bounds__(256) void ensemble_combine_kernel(int E1, size_t slab, int K, const double* __restrict__ w, const double* __restrict__ b,
                                                               double* out) {
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < slab; t += (size_t)gridDim.x * 256) {
        const int k = (int)(t % K);
        for (int m = E1 - 1; m >= 0; --m) {
            const double y = ens_combine_f64(w + (size_t)m * E1, b ? b[(size_t)m * K + k] : 0.0, m, [&](int j) { return out[(size_t)j * slab + t]; });
            out[(size_t)m * slab + t] = (double)(float)y;
        }
    }
}

void launch_ensemble_logsoftmax(const double* logits, size_t rows, int K, double* l, hipStream_t s) {
    hipLaunchKernelGGL(ensemble_logsoftmax_kernel, dim3(grid_1d((long long)rows * K, 256, 4096)), dim3(256), 0, s, logits, rows, K, l);
}

void launch_ensemble_logits(const double* logits, int E1, int N, int K, const double* w, const double* b, double* out, hipStream_t s) {
    const size_t slab = (size_t)N * K;
    launch_ensemble_logsoftmax(logits, (size_t)E1 * N, K, out, s);
    hipLaunchKernelGGL(ensemble_combine_kernel, dim3(grid_1d((long long)slab, 256, 4096)), dim3(256), 0, s, E1, slab, K, w, b, out);
}

// ---------------------------------------------------------------------------------------------------------------
// Budgeted exits on a criterion table (ee_quota_scan; definition in include/mmee.h): consecutive groups of G documents, each ranked as one
// forward's stage would be.  exits[n] < 0 marks a document that is still active; nothing is compacted, a document's slot is its index in its
// group, so "the survivors in their order" is the group with the leavers masked out (quota_key 0 = no document).  Per exit below the last:
//   quota_scan_rank_kernel    the forward's counting (quota_rank_by_counting), 256 documents per workgroup, ceil(G / 256) workgroups per group;
//   quota_scan_decide_kernel  one workgroup per group: the active and the fired documents counted (integers), then the decision by the
//                             definition's own expression, rank < q or the event, and the two cut criteria: the documents ranked m - 1 and m
//                             with m the number of leavers.
// The rank launch reads exits, the decide launch writes it: two launches, not one.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void quota_scan_rank_kernel(QuotaScanArgs a, int e, int blocks_per_group) {
    __shared__ unsigned long long t_key[2048];
    __shared__ int t_slot[2048];
    const int g = blockIdx.x / blocks_per_group, lb = blockIdx.x - g * blocks_per_group;
    const long long start = (long long)g * a.G;
    const int ng = (long long)a.N - start < a.G ? (int)(a.N - start) : a.G;
    if (lb * 256 >= ng) return;                                            // the same for every thread of the workgroup
    const double* row = a.table + (size_t)e * a.N + start;
    const int* ex = a.exits + start;
    const double sign = a.sign;
    const int i = lb * 256 + threadIdx.x;
    const bool active = i < ng && ex[i] < 0;
    const unsigned long long key = active ? quota_key(row[i], sign) : 0ull;
    const unsigned r = quota_rank_by_counting(key, i, ng, [&](int j) { return ex[j] < 0 ? quota_key(row[j], sign) : 0ull; }, [](int j) { return j; }, t_key,
                                              t_slot);
    if (active) a.rank[start + i] = (int)r;
}

__global__ __launch_bounds__(256) void quota_scan_decide_kernel(QuotaScanArgs a, int e) {
    __shared__ int s_cnt[2][4];
    const int g = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long start = (long long)g * a.G;
    const int ng = (long long)a.N - start < a.G ? (int)(a.N - start) : a.G;
    const double* row = a.table + (size_t)e * a.N + start;
    int* ex = a.exits + start;
    const int q = a.quotas[e];
    const bool at_least = a.mode == QUOTA_AT_LEAST;
    const double sthr = at_least ? a.sign * a.thr[e] : 0.0;
    int na = 0, nf = 0;
    for (int i = threadIdx.x; i < ng; i += 256) {
        const bool active = ex[i] < 0;
        na += active ? 1 : 0;
        nf += (active && at_least && a.sign * row[i] > sthr) ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) { na += __shfl_xor(na, o, 64); nf += __shfl_xor(nf, o, 64); }
    if (lane == 0) { s_cnt[0][wave] = na; s_cnt[1][wave] = nf; }
    __syncthreads();                                                       // also: every read of exits above is behind us
    na = s_cnt[0][0] + s_cnt[0][1] + s_cnt[0][2] + s_cnt[0][3];
    nf = s_cnt[1][0] + s_cnt[1][1] + s_cnt[1][2] + s_cnt[1][3];
    const int mq = q < na ? q : na;
    const int m = mq > nf ? mq : nf;                                       // the leavers: the top max(q, #fired) (the event is monotone in s)
    double* cut = a.cuts ? a.cuts + ((size_t)g * (a.E1 - 1) + e) * 2 : nullptr;
    for (int i = threadIdx.x; i < ng; i += 256) {
        if (ex[i] >= 0) continue;
        const int r = a.rank[start + i];
        const double c = row[i];
        const bool leave = r < q || (at_least && a.sign * c > sthr);
        if (cut && r == m - 1) cut[0] = c;
        if (cut && r == m) cut[1] = c;
        if (leave) ex[i] = e;
    }
}

__global__ __launch_bounds__(256) void quota_scan_final_kernel(int* __restrict__ exits, int N, int last) {
    for (int n = blockIdx.x * 256 + threadIdx.x; n < N; n += gridDim.x * 256)
        if (exits[n] < 0) exits[n] = last;
}

void launch_quota_scan(const QuotaScanArgs& a, hipStream_t s) {
    const int group = a.G < a.N ? a.G : a.N;
    const int groups = (a.N + a.G - 1) / a.G, bpg = (group + 255) / 256;
    for (int e = 0; e + 1 < a.E1; ++e) {
        hipLaunchKernelGGL(quota_scan_rank_kernel, dim3((unsigned)groups * (unsigned)bpg), dim3(256), 0, s, a, e, bpg);
        hipLaunchKernelGGL(quota_scan_decide_kernel, dim3(groups), dim3(256), 0, s, a, e);
    }
    hipLaunchKernelGGL(quota_scan_final_kernel, dim3(grid_1d(a.N, 256, 4096)), dim3(256), 0, s, a.exits, a.N, a.E1 - 1);
}

// ---------------------------------------------------------------------------------------------------------------
// Per-exit temperature fit: argmin_T mean NLL(softmax(z / T), y)   (TemperatureScaler.set_temperature,
// EE/generic_scaling.py:64-111, L-BFGS-B on sklearn log_loss).  In beta = 1/T the objective
//     f(beta) = mean( logsumexp(beta z) - beta z_y )
// is convex with f' = mean(E_p[z] - z_y) and f'' = mean(Var_p[z]) (p = softmax(beta z)), so a safeguarded Newton
// iteration converges in a handful of steps; one workgroup per exit keeps the whole loop on the device.
// Also returns the quantities calibrate() derives from the scaled logits (EE/eval.py:313-337): NLL, accuracy
// (argmax == label) and mean max-softmax confidence at the fitted temperature.
// ---------------------------------------------------------------------------------------------------------------
__device__ inline void block_sum3(double& a, double& b, double& c, double* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
        c += __shfl_xor(c, o, 64);
    }
    __syncthreads();
    if (lane == 0) { lds[3 * wave] = a; lds[3 * wave + 1] = b; lds[3 * wave + 2] = c; }
    __syncthreads();
    a = b = c = 0.0;
    for (int w = 0; w < nw; ++w) { a += lds[3 * w]; b += lds[3 * w + 1]; c += lds[3 * w + 2]; }
}

__global__ __launch_bounds__(1024) void temperature_fit_kernel(const double* __restrict__ logits, const long long* __restrict__ labels,
                                                               int N, int K, int max_iter, double* __restrict__ T_out,
                                                               double* __restrict__ nll_out, double* __restrict__ acc_out,
                                                               double* __restrict__ conf_out, int* __restrict__ iters_out) {
    __shared__ double red[3 * 16];
    const int e = blockIdx.x;
    const double* L = logits + (size_t)e * N * K;
    double beta = 1.0;                                    // TemperatureScaler starts from T = 1 (generic_scaling.py:42-46)
    int it = 0;
    for (; it < max_iter; ++it) {
        double g = 0.0, h = 0.0, f = 0.0;
        for (int n = threadIdx.x; n < N; n += blockDim.x) {
            const double* z = L + (size_t)n * K;
            double m = z[0];
            for (int k = 1; k < K; ++k) m = fmax(m, z[k]);
            double S = 0.0, A = 0.0, B = 0.0;
            for (int k = 0; k < K; ++k) {
                const double w = exp(beta * (z[k] - m));
                S += w; A += w * z[k]; B += w * z[k] * z[k];
            }
            A /= S; B /= S;
            const double zy = z[labels[n]];
            g += A - zy;
            h += B - A * A;
            f += log(S) + beta * (m - zy);
        }
        block_sum3(g, h, f, red);
        g /= N; h /= N;
        double step = (h > 1e-300) ? g / h : (g > 0 ? 0.5 * beta : -beta);
        double nb = beta - step;
        if (!(nb > 0.0)) nb = 0.5 * beta;                 // stay in beta > 0 (the reference bounds T in (1e-32, inf))
        if (nb > 64.0 * beta) nb = 64.0 * beta;
        const bool done = fabs(nb - beta) <= 1e-13 * beta;
        beta = nb;
        if (done) break;
    }
    // final statistics at the fitted temperature
    double f = 0.0, acc = 0.0, conf = 0.0;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const double* z = L + (size_t)n * K;
        double m = z[0];
        int am = 0;
        for (int k = 1; k < K; ++k)
            if (z[k] > m) { m = z[k]; am = k; }
        double S = 0.0;
        for (int k = 0; k < K; ++k) S += exp(beta * (z[k] - m));
        f += log(S) + beta * (m - z[labels[n]]);
        acc += (am == (int)labels[n]) ? 1.0 : 0.0;
        conf += 1.0 / S;
    }
    block_sum3(f, acc, conf, red);
    if (threadIdx.x == 0) {
        T_out[e] = 1.0 / beta;
        if (nll_out) nll_out[e] = f / N;
        if (acc_out) acc_out[e] = acc / N;
        if (conf_out) conf_out[e] = conf / N;
        if (iters_out) iters_out[e] = it;
    }
}

void launch_temperature_fit(const double* logits, const long long* labels, int E1, int N, int K, int max_iter, double* T_out,
                            double* nll_out, double* acc_out, double* conf_out, int* iters_out, hipStream_t s) {
    hipLaunchKernelGGL(temperature_fit_kernel, dim3(E1), dim3(1024), 0, s, logits, labels, N, K, max_iter, T_out, nll_out,
                       acc_out, conf_out, iters_out);
}

// (logits f32 (n,K), exit_layer i32 (n), confidence f32 (n)) <-> the row of the ONE all-gather of the north star: K + 2 int32 words per document
// (the floats travel as their bit patterns: integer copies and collectives never flush, canonicalise or round them)
__global__ __launch_bounds__(256) void pack_results_kernel(const float* __restrict__ logits, const int* __restrict__ exit_layer,
                                                           const float* __restrict__ conf, int n, int K, int* __restrict__ rows) {
    const long total = (long)n * (K + 2);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int d = (int)(i / (K + 2)), c = (int)(i - (long)d * (K + 2));
        rows[i] = c < K ? __float_as_int(logits[(size_t)d * K + c]) : c == K ? exit_layer[d] : __float_as_int(conf[d]);
    }
}
__global__ __launch_bounds__(256) void unpack_results_kernel(const int* __restrict__ rows, int n, int K, float* __restrict__ logits,
                                                             int* __restrict__ exit_layer, float* __restrict__ conf) {
    const long total = (long)n * (K + 2);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int d = (int)(i / (K + 2)), c = (int)(i - (long)d * (K + 2));
        const int v = rows[i];
        if (c < K) { if (logits) logits[(size_t)d * K + c] = __int_as_float(v); }
        else if (c == K) { if (exit_layer) exit_layer[d] = v; }
        else if (conf) conf[d] = __int_as_float(v);
    }
}
void launch_pack_results(const float* logits, const int* exit_layer, const float* conf, int n, int K, int* rows, hipStream_t s) {
    hipLaunchKernelGGL(pack_results_kernel, dim3(grid_1d((long)n * (K + 2), 256, 4096)), dim3(256), 0, s, logits, exit_layer, conf, n, K, rows);
}
void launch_unpack_results(const int* rows, int n, int K, float* logits, int* exit_layer, float* conf, hipStream_t s) {
    hipLaunchKernelGGL(unpack_results_kernel, dim3(grid_1d((long)n * (K + 2), 256, 4096)), dim3(256), 0, s, rows, n, K, logits, exit_layer, conf);
}

}  // namespace mmee
