// The evaluation report on dumped (E1, N, K) arrays (ee_exit_metrics, include/mmee.h): the seven metrics the reference scores every exit and
// every policy's predictions with (METRICS, EE/eval.py:175-181 / calc_metrics, EE/utils.py:226-237) plus the average confidence, per exit and
// for one operating point, without the array leaving the device.  float64 throughout, as the reference evaluates the float64 store.
//
//   1. metrics_rows_kernel   thread per (row, document): softmax of the (scaled) logits row, conf / correct into an (R, N) table (the operating-
//                            point row gathers through `exits`), confusion[ref][pred] and the exit histogram by INTEGER atomics, and one float64
//                            partial per block for the Brier, NLL and confidence sums (fixed tree inside the block).
//   2. metrics_sort_kernel   every row's (conf, correct) into its stable ascending place by counting (stable_rank_by_counting,
//                            ranked_common.h): place = #{m : c_m < c_n} + #{m < n : c_m == c_n}.  O(N^2) per row.
//   3. metrics_curve_kernel  one workgroup of 1024 threads per row over the sorted row: hits and the equal-mass ECE bins (integer counts in LDS),
//                            then the risk-coverage curve in chunks of 1024 with running carries (the scheme of block1024_scan,
//                            ranked_common.h, written out: through the helper the kernel measured 7.5 % slower, see
//                            profiles/ranked_common_ab.txt), then the means, F1 and the `out` row.
// No floating-point atomic anywhere: every float sum has a fixed order (tree inside a chunk or block, chunks and blocks in order), so the
// output bits are a function of the inputs alone.
#include "ranked_common.h"

namespace mmee {

namespace {

constexpr int kRowsBlock = 256;
constexpr int kRowsMaxBlocks = 256;        // partials per row that metrics_curve_kernel adds in block order

// sum of v over the block's 256 threads in a fixed tree; valid in thread 0.  s: 256 doubles of LDS
__device__ __forceinline__ double block256_sum(double v, double* s) {
    const int tid = threadIdx.x;
    __syncthreads();
    s[tid] = v;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) s[tid] += s[tid + o];
        __syncthreads();
    }
    return s[0];
}

}  // namespace

__global__ __launch_bounds__(kRowsBlock) void metrics_rows_kernel(MetricsArgs a, double* __restrict__ tconf, unsigned char* __restrict__ tcorr,
                                                                   unsigned long long* __restrict__ confusion, double* __restrict__ part) {
    __shared__ double s_red[kRowsBlock];
    const int r = blockIdx.y, N = a.N, K = a.K;
    const bool op = r == a.E1;                                       // the operating-point row
    double sum_brier = 0.0, sum_nll = 0.0, sum_conf = 0.0;
    for (int n = blockIdx.x * kRowsBlock + threadIdx.x; n < N; n += gridDim.x * kRowsBlock) {
        int e = r;
        if (op) {
            const int x = a.exits[n];
            e = x < 0 ? 0 : x >= a.E1 ? a.E1 - 1 : x;                // clamped for the lookup; the histogram counts in-range values only
            if (a.exit_hist && x == e) atomicAdd(&a.exit_hist[e], 1ull);
        }
        double conf;
        bool correct;
        if (a.logits) {
            const double* z = a.logits + ((size_t)e * N + n) * K;
            const bool scale = a.temperatures != nullptr;
            const double T = scale ? a.temperatures[e] : 1.0;
            const auto at = [&](int k) { return scale ? z[k] / T : z[k]; };
            double m = at(0);
            int pred = 0;
            for (int k = 1; k < K; ++k) {
                const double v = at(k);
                if (v > m) { m = v; pred = k; }                      // the FIRST maximum, as np.argmax
            }
            double s = 0.0;
            for (int k = 0; k < K; ++k) s += exp(at(k) - m);
            const long long ref = a.references[n];
            const int refc = ref < 0 ? 0 : ref >= K ? K - 1 : (int)ref;
            double brier = 0.0;
            for (int k = 0; k < K; ++k) {
                const double d = exp(at(k) - m) / s - (k == refc ? 1.0 : 0.0);
                brier += d * d;
            }
            conf = 1.0 / s;                                          // exp(m - m) / s
            correct = (long long)pred == ref;
            sum_brier += brier;
            sum_nll += log(s) - (at(refc) - m);
            atomicAdd(&confusion[((size_t)r * K + refc) * K + pred], 1ull);
        } else {
            conf = a.conf[(size_t)e * N + n];
            correct = a.correct[(size_t)e * N + n] != 0;
        }
        sum_conf += conf;
        tconf[(size_t)r * N + n] = conf;
        tcorr[(size_t)r * N + n] = correct ? 1 : 0;
    }
    double* p = part + ((size_t)r * gridDim.x + blockIdx.x) * 3;
    const double b = block256_sum(sum_brier, s_red), l = block256_sum(sum_nll, s_red), c = block256_sum(sum_conf, s_red);
    if (threadIdx.x == 0) { p[0] = b; p[1] = l; p[2] = c; }
}

__global__ __launch_bounds__(256) void metrics_sort_kernel(const double* __restrict__ tconf, const unsigned char* __restrict__ tcorr, int N,
                                                           double* __restrict__ sconf, unsigned char* __restrict__ scorr) {
    __shared__ double tile[2048];
    const int r = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
    const double* row = tconf + (size_t)r * N;
    const uint2 place = stable_rank_by_counting(row, N, n, tile);   // (lt, eq_before)
    if (n < N) {
        const size_t at = (size_t)r * N + place.x + place.y;         // lt + eq_before < N: a permutation of the row
        sconf[at] = row[n];
        scorr[at] = tcorr[(size_t)r * N + n];
    }
}

// The sorted row c_0 <= ... <= c_{N-1} with k_i = correct.
//   ECE   edges[b] = c[(b N) / n_bins], b < n_bins, edges[n_bins] = 1; bin = #{edges <= c_i} - 1 clipped to [0, n_bins); integer document and hit
//         counts per bin; sum_b (cnt_b / N) |hit_b / cnt_b - edges[b + 1]| in bin order.
//   AURC  E(i) = errors among 0 .. i (integer prefix sum), S_{i+1} = S_0 - E(i).  i <= N - 2 is a POINT when i == 0 or c_i != c_{i-1}; its risk is
//         S_{i+1} / (N - 1 - i), its weight (i - p) / N with p the previous point (-1 before the first): an exclusive prefix max of the word
//         (i + 1) << 32 | E(i), which carries the previous point's risk with it.  Term = (risk_p + risk_i) * 0.5 * weight; the curve's tail
//         (N - 2 - last point documents) repeats the last risk.  Terms are added by a fixed tree per chunk, chunks in order.
__global__ __launch_bounds__(1024) void metrics_curve_kernel(MetricsArgs a, const double* __restrict__ sconf, const unsigned char* __restrict__ scorr,
                                                             const unsigned long long* __restrict__ confusion, const double* __restrict__ part,
                                                             int n_part) {
    __shared__ double s_edges[kMetricsMaxBins + 1];
    __shared__ int s_cnt[kMetricsMaxBins], s_hit[kMetricsMaxBins];
    __shared__ int s_wsum[16];
    __shared__ unsigned long long s_wmax[16];
    __shared__ double s_wterm[16];
    __shared__ double s_f1[1024];
    __shared__ int s_present[1024];
    __shared__ int s_hits;
    const int r = blockIdx.x, N = a.N, K = a.K, nb = a.n_bins;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* c = sconf + (size_t)r * N;
    const unsigned char* k = scorr + (size_t)r * N;

    // ---- hits and the ECE bins ----
    for (int b = tid; b < nb; b += 1024) {
        s_edges[b] = c[(size_t)(((long long)b * N) / nb)];
        s_cnt[b] = 0;
        s_hit[b] = 0;
    }
    if (tid == 0) { s_edges[nb] = 1.0; s_hits = 0; }
    __syncthreads();
    int my_hits = 0;
    for (int i = tid; i < N; i += 1024) {
        const double x = c[i];
        int lo = 0, hi = nb + 1;                                     // the first edge above x = the number of edges at or below it (side="right")
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_edges[mid] <= x) lo = mid + 1;
            else hi = mid;
        }
        const int bin = lo - 1 < 0 ? 0 : lo - 1 > nb - 1 ? nb - 1 : lo - 1;
        const int hit = k[i] ? 1 : 0;
        atomicAdd(&s_cnt[bin], 1);
        if (hit) atomicAdd(&s_hit[bin], 1);
        my_hits += hit;
    }
    for (int o = 32; o >= 1; o >>= 1) my_hits += __shfl_down(my_hits, o, 64);
    if (lane == 0 && my_hits) atomicAdd(&s_hits, my_hits);
    __syncthreads();
    const int hits = s_hits, S0 = N - hits;

    // ---- the risk-coverage curve ----
    const double dN = (double)N;
    int carry_err = 0;                                               // E(base - 1): the same value in every thread
    unsigned long long carry_key = 0;                                // the last point before this chunk, 0: none
    double aurc = 0.0;
    const auto risk_of = [&](unsigned long long key) {               // the risk appended at the point a key stands for; key 0: the curve's first entry
        if (!key) return (double)S0 / dN;
        const int p = (int)(key >> 32) - 1, Ep = (int)(key & 0xffffffffull);
        return (double)(S0 - Ep) / (double)(N - 1 - p);
    };
    for (int base = 0; base < N; base += 1024) {
        const int i = base + tid;
        const bool in = i < N;
        const double ci = in ? c[i] : 0.0;
        int e_incl = in && !k[i] ? 1 : 0;
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(e_incl, o, 64);
            if (lane >= o) e_incl += t;
        }
        if (lane == 63) s_wsum[wave] = e_incl;
        __syncthreads();
        int chunk_err = 0;
        for (int w = 0; w < 16; ++w) {
            if (w < wave) e_incl += s_wsum[w];
            chunk_err += s_wsum[w];
        }
        e_incl += carry_err;                                         // E(i)
        const bool point = i <= N - 2 && (i == 0 || ci != c[i - 1]);
        const unsigned long long key = point ? ((unsigned long long)(i + 1) << 32) | (unsigned)e_incl : 0ull;
        unsigned long long m = key;                                  // inclusive prefix max inside the wave
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long t = __shfl_up(m, o, 64);
            if (lane >= o) m = t > m ? t : m;
        }
        unsigned long long prev = __shfl_up(m, 1, 64);
        if (lane == 0) prev = 0ull;
        if (lane == 63) s_wmax[wave] = m;
        __syncthreads();
        unsigned long long chunk_key = carry_key;
        for (int w = 0; w < 16; ++w) {
            if (w < wave) prev = s_wmax[w] > prev ? s_wmax[w] : prev;
            chunk_key = s_wmax[w] > chunk_key ? s_wmax[w] : chunk_key;
        }
        prev = carry_key > prev ? carry_key : prev;
        double term = 0.0;
        if (point) {
            const int p = (int)(prev >> 32) - 1;                     // -1: no point yet
            term = (risk_of(prev) + risk_of(key)) * 0.5 * ((double)(i - p) / dN);
        }
        for (int o = 32; o >= 1; o >>= 1) term += __shfl_down(term, o, 64);
        if (lane == 0) s_wterm[wave] = term;
        __syncthreads();
        double chunk_term = 0.0;
        for (int w = 0; w < 16; ++w) chunk_term += s_wterm[w];
        aurc += chunk_term;
        carry_err += chunk_err;
        carry_key = chunk_key;
        __syncthreads();                                             // the wave slots are rewritten by the next chunk
    }
    if (carry_key) {                                                 // N >= 2.  The documents behind the last point repeat its risk
        const int t = (N - 2) - ((int)(carry_key >> 32) - 1);
        const double last = risk_of(carry_key);
        if (t > 0) aurc += (last + last) * 0.5 * ((double)t / dN);
    }

    // ---- macro F1 from the confusion counts: classes in order, averaged over those that occur in the references or the predictions ----
    double f1_sum = 0.0;
    int f1_classes = 0;
    if (a.logits) {
        const unsigned long long* cm = confusion + (size_t)r * K * K;
        for (int c0 = 0; c0 < K; c0 += 1024) {
            const int cls = c0 + tid;
            double f = 0.0;
            int present = 0;
            if (cls < K) {
                unsigned long long truth = 0, preds = 0;
                for (int j = 0; j < K; ++j) {
                    truth += cm[(size_t)cls * K + j];
                    preds += cm[(size_t)j * K + cls];
                }
                present = truth + preds > 0 ? 1 : 0;
                if (present) f = (double)(2ull * cm[(size_t)cls * K + cls]) / (double)(truth + preds);      // 2TP / (2TP + FP + FN)
            }
            __syncthreads();
            s_f1[tid] = f;
            s_present[tid] = present;
            __syncthreads();
            if (tid == 0) {
                const int cnt = K - c0 < 1024 ? K - c0 : 1024;
                for (int j = 0; j < cnt; ++j) {
                    if (s_present[j]) { f1_sum += s_f1[j]; ++f1_classes; }
                }
            }
        }
    }

    if (tid == 0) {
        double ece = 0.0;
        for (int b = 0; b < nb; ++b) {
            const double acc = s_cnt[b] > 0 ? (double)s_hit[b] / (double)s_cnt[b] : 0.0;
            ece += ((double)s_cnt[b] / dN) * fabs(acc - s_edges[b + 1]);
        }
        double brier = 0.0, nll = 0.0, conf = 0.0;
        for (int b = 0; b < n_part; ++b) {
            const double* p = part + ((size_t)r * n_part + b) * 3;
            brier += p[0];
            nll += p[1];
            conf += p[2];
        }
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        double* o = a.out + (size_t)r * kMetricCount;
        o[kMetricAccuracy] = (double)hits / dN;
        o[kMetricBrier] = a.logits ? brier / dN : nan;
        o[kMetricNll] = a.logits ? nll / dN : nan;
        o[kMetricF1Micro] = (double)hits / dN;
        o[kMetricF1Macro] = a.logits ? (f1_classes ? f1_sum / (double)f1_classes : 0.0) : nan;
        o[kMetricEce] = ece;
        o[kMetricAurc] = aurc;
        o[kMetricAvgConf] = conf / dN;
    }
}

// false: the workspace allocation failed and nothing was launched
bool launch_exit_metrics(const MetricsArgs& a, hipStream_t s) {
    const int R = a.E1 + (a.exits ? 1 : 0), N = a.N;
    const int n_part = grid_1d(N, kRowsBlock, kRowsMaxBlocks);
    const size_t RN = (size_t)R * N, cm_words = a.logits && !a.confusion ? (size_t)R * a.K * a.K : 0;
    // one allocation: tconf | sconf | part | confusion (when the caller keeps none) | tcorr | scorr
    const size_t o_sconf = RN * 8, o_part = o_sconf + RN * 8, o_cm = o_part + (size_t)R * n_part * 3 * 8, o_tcorr = o_cm + cm_words * 8,
                 o_scorr = o_tcorr + RN, bytes = o_scorr + RN;
    char* ws = nullptr;
    if (hipMallocAsync((void**)&ws, bytes, s) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    double *tconf = reinterpret_cast<double*>(ws), *sconf = reinterpret_cast<double*>(ws + o_sconf), *part = reinterpret_cast<double*>(ws + o_part);
    unsigned char *tcorr = reinterpret_cast<unsigned char*>(ws + o_tcorr), *scorr = reinterpret_cast<unsigned char*>(ws + o_scorr);
    unsigned long long* cm = a.confusion ? a.confusion : reinterpret_cast<unsigned long long*>(ws + o_cm);
    if (a.logits) (void)hipMemsetAsync(cm, 0, (size_t)R * a.K * a.K * 8, s);
    if (a.exit_hist) (void)hipMemsetAsync(a.exit_hist, 0, (size_t)a.E1 * 8, s);
    hipLaunchKernelGGL(metrics_rows_kernel, dim3(n_part, R), dim3(kRowsBlock), 0, s, a, tconf, tcorr, cm, part);
    hipLaunchKernelGGL(metrics_sort_kernel, dim3((N + 255) / 256, R), dim3(256), 0, s, tconf, tcorr, N, sconf, scorr);
    hipLaunchKernelGGL(metrics_curve_kernel, dim3(R), dim3(1024), 0, s, a, sconf, scorr, cm, part, n_part);
    (void)hipFreeAsync(ws, s);
    return true;
}

}  // namespace mmee
