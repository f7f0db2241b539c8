// Risk-controlled exit thresholds (include/mmee.h, "Risk control"): ee_risk_control and ee_binomial_bounds, their kernels and launches.
// Handle-free like the tools of capi_tools.hip; nothing here is reached by a forward.
//   risk_quantise_kernel     float64 (E1,N) loss -> uint32 units of 2^-30, rounded up; raises the error word for a value that is not a loss
//   risk_count_kernel        per threshold vector: loss_sum, exit_sum, cost_sum, exit histogram under the policy's rule.  threshold_sweep_kernel's
//                            shape (exit_ops.hip): a workgroup per vector, documents strided over its 256 threads, coalesced (E1,N) rows -- and,
//                            because a call has few vectors (101 by default, on 256 CUs), gridDim.y workgroups share a vector's documents and
//                            add their integer sums into the zeroed outputs with integer atomics: any order of arrival gives the same bits
//   risk_lgamma_kernel       lg[i] = lgamma(i + 1), i = 0 .. n: the table the next two kernels read
//   risk_cdf_kernel          F[k] = P(Bin(n, alpha) <= k), k = 0 .. n: one workgroup, chunks of 1024 terms, block1024_scan with a running carry
//   risk_select_kernel       one workgroup over the V vectors: p-values, the fixed-sequence prefix / the Bonferroni mask, the certified count,
//                            the certified vector of least cost_sum (ties to the lowest v)
//   binomial_bounds_kernel   one workgroup per query: the two Clopper-Pearson bounds by 64 bisections, each a block sum in a fixed order
// Every sum that decides something is an integer; the floating-point sums (the CDF, the bisections' tails) are taken in an order fixed by the
// thread index alone, so the outputs are a pure function of the inputs.  block1024_scan (ranked_common.h) combines in thread order: a
// floating-point prefix through it is not the sequential sum, but it has the same bits in every run, which is all risk_cdf_kernel needs.
#include <math.h>

#include "capi_internal.h"
#include "ranked_common.h"

using namespace mmee;
using namespace mmee::capi;

namespace {

constexpr unsigned kRiskOne = 1u << 30;                               // a loss of 1 in loss_q's units
constexpr int kRiskMaxN = 1 << 24, kRiskMaxV = 65536, kRiskMaxE1 = 64;

// one term of the binomial distribution: exp(lg[n] - lg[i] - lg[n-i] + i log_t + (n-i) log1m_t), with 0 x (-inf) = 0 (theta = 0 or 1 inside
// a bisection).  Left to right, every product rounded before it is added.
__device__ __forceinline__ double binom_term(const double* __restrict__ lg, int n, int i, double log_t, double log1m_t) {
#pragma clang fp contract(off)
    const double a = i == 0 ? 0.0 : (double)i * log_t;
    const double b = n - i == 0 ? 0.0 : (double)(n - i) * log1m_t;
    return exp(lg[n] - lg[i] - lg[n - i] + a + b);
}

__global__ __launch_bounds__(256) void risk_quantise_kernel(const double* __restrict__ loss, long long total, int binary,
                                                            unsigned* __restrict__ loss_q, int* __restrict__ err) {
    bool bad = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const double v = loss[i];
        const bool ok = v >= 0.0 && v <= 1.0 && !(binary && v != 0.0 && v != 1.0);       // NaN fails both compares
        bad |= !ok;
        const double q = ceil(v * (double)kRiskOne);                  // a power of two: the product is exact, the ceil never understates
        loss_q[i] = !ok ? 0u : q >= (double)kRiskOne ? kRiskOne : (unsigned)q;
    }
    if (bad) atomicOr(err, 1);
}

__global__ __launch_bounds__(256) void risk_count_kernel(const double* __restrict__ conf, double sign, const unsigned* __restrict__ loss_q,
                                                         const unsigned* __restrict__ cost, int E1, int N, const double* __restrict__ thr, int V,
                                                         unsigned long long* __restrict__ loss_sum, long long* __restrict__ exit_sum,
                                                         unsigned long long* __restrict__ cost_sum, int* __restrict__ hist) {
    __shared__ double s_thr[kRiskMaxE1];
    __shared__ int s_hist[kRiskMaxE1];
    __shared__ unsigned long long s_red[4][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int v = blockIdx.x; v < V; v += gridDim.x) {
        __syncthreads();
        if (tid < E1) {
            if (tid < E1 - 1) s_thr[tid] = sign * thr[(size_t)v * E1 + tid];
            s_hist[tid] = 0;
        }
        __syncthreads();
        unsigned long long ls = 0, xs = 0, cs = 0;
        for (long long n = (long long)blockIdx.y * 256 + tid; n < N; n += 256ll * gridDim.y) {
            int ex = E1 - 1;                                          // the final exit is the fall-back; its threshold is not read
            for (int e = 0; e < E1 - 1; ++e) {
                if (sign * conf[(size_t)e * N + (size_t)n] > s_thr[e]) { ex = e; break; }        // strict; a NaN criterion never fires
            }
            ls += loss_q[(size_t)ex * N + (size_t)n];
            xs += (unsigned)ex;
            cs += cost ? cost[(size_t)ex * N + (size_t)n] : (unsigned)ex;
            if (hist) atomicAdd(&s_hist[ex], 1);
        }
        for (int o = 32; o > 0; o >>= 1) {
            ls += __shfl_xor(ls, o, 64);
            xs += __shfl_xor(xs, o, 64);
            cs += __shfl_xor(cs, o, 64);
        }
        if (lane == 0) { s_red[wave][0] = ls; s_red[wave][1] = xs; s_red[wave][2] = cs; }
        __syncthreads();
        if (tid < 3) {                                                // the outputs were zeroed by the launcher; exit_sum stays below 2^30: no sign to mind
            unsigned long long* out = tid == 0 ? loss_sum : tid == 1 ? reinterpret_cast<unsigned long long*>(exit_sum) : cost_sum;
            atomicAdd(&out[v], s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid]);
        }
        if (hist && tid < E1 && s_hist[tid]) atomicAdd(&hist[(size_t)v * E1 + tid], s_hist[tid]);
    }
}

__global__ __launch_bounds__(256) void risk_lgamma_kernel(int n, double* __restrict__ lg) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i <= n; i += (long long)gridDim.x * 256) lg[i] = lgamma((double)i + 1.0);
}

__global__ __launch_bounds__(1024) void risk_cdf_kernel(const double* __restrict__ lg, int n, double alpha, double* __restrict__ F) {
    __shared__ double slots[16];
    const double log_a = log(alpha), log1m_a = log1p(-alpha);
    double carry = 0.0;
    for (int base = 0; base <= n; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const double term = i <= n ? binom_term(lg, n, i, log_a, log1m_a) : 0.0;
        const BlockScan<double> sc = block1024_scan(term, 0.0, [](double a, double b) { return a + b; }, slots);
        const double f = carry + sc.inclusive;
        if (i <= n) F[i] = f < 1.0 ? f : 1.0;
        carry += sc.total;
        __syncthreads();                                              // before the slots are written again
    }
}

// h(a, b) = a log(a / b) + (1 - a) log((1 - a) / (1 - b)), 0 log 0 = 0
__device__ __forceinline__ double risk_kl(double a, double b) {
#pragma clang fp contract(off)
    const double t1 = a > 0.0 ? a * log(a / b) : 0.0;
    const double t2 = 1.0 - a > 0.0 ? (1.0 - a) * log((1.0 - a) / (1.0 - b)) : 0.0;
    return t1 + t2;
}

__global__ __launch_bounds__(1024) void risk_select_kernel(const unsigned long long* __restrict__ loss_sum, const unsigned long long* __restrict__ cost_sum,
                                                           int V, int n, double alpha, double delta, int bound, int method,
                                                           const double* __restrict__ F, double* __restrict__ pvalue,
                                                           unsigned char* __restrict__ certified, int* __restrict__ n_certified,
                                                           int* __restrict__ selected) {
    __shared__ int s_first_fail, s_count, s_selected;
    __shared__ unsigned long long s_min_cost;
    const int tid = threadIdx.x;
    if (tid == 0) { s_first_fail = V; s_count = 0; s_selected = V; s_min_cost = ~0ull; }
    __syncthreads();
    const double level = method == MMEE_RISK_BONFERRONI ? delta / (double)V : delta;
    for (int v = tid; v < V; v += 1024) {
        const unsigned long long ls = loss_sum[v];
        double p;
        if (bound == MMEE_RISK_BINOMIAL) {
            const unsigned long long k = ls >> 30;
            p = F[k < (unsigned long long)n ? (int)k : n];            // loss_q <= 2^30 keeps k <= n; the clamp keeps a bad table in bounds
        } else {
#pragma clang fp contract(off)
            const double r = (double)ls / ((double)n * (double)kRiskOne);
            const double p_h = r < alpha ? exp(-(double)n * risk_kl(r, alpha)) : 1.0;
            const unsigned long long kc = (ls + (kRiskOne - 1u)) >> 30;
            const double eb = 2.718281828459045 * F[kc < (unsigned long long)n ? (int)kc : n];
            const double p_b = eb < 1.0 ? eb : 1.0;
            p = p_h < p_b ? p_h : p_b;
        }
        pvalue[v] = p;
        if (!(p <= level)) atomicMin(&s_first_fail, v);
    }
    __syncthreads();
    const int first_fail = s_first_fail;
    for (int v = tid; v < V; v += 1024) {
        const bool cert = method == MMEE_RISK_BONFERRONI ? pvalue[v] <= level : v < first_fail;      // pvalue[v]: this thread's own store
        certified[v] = cert ? 1 : 0;
        if (cert) {
            atomicAdd(&s_count, 1);
            atomicMin(&s_min_cost, cost_sum[v]);
        }
    }
    __syncthreads();
    const unsigned long long min_cost = s_min_cost;
    for (int v = tid; v < V; v += 1024)
        if (certified[v] && cost_sum[v] == min_cost) atomicMin(&s_selected, v);
    __syncthreads();
    if (tid == 0) {
        *n_certified = s_count;
        *selected = s_selected < V ? s_selected : -1;
    }
}

// F(kk; n, theta) clamped to 1, the same value in all 256 threads: every thread sums its terms i = tid, tid + 256, ... ascending, the 64 lanes
// of a wave fold by xor shuffles, the four waves add in wave order.  Two barriers per call.
__device__ __forceinline__ double bounds_cdf(const double* __restrict__ lg, int n, int kk, double theta, double* s_red) {
    const double log_t = log(theta), log1m_t = log1p(-theta);
    double acc = 0.0;
    for (int i = threadIdx.x; i <= kk; i += 256) acc += binom_term(lg, n, i, log_t, log1m_t);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
    __syncthreads();
    const double f = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
    return f < 1.0 ? f : 1.0;
}

__global__ __launch_bounds__(256) void binomial_bounds_kernel(const int* __restrict__ ns, const int* __restrict__ ks, const double* __restrict__ lg,
                                                              double delta, double* __restrict__ upper, double* __restrict__ lower) {
    __shared__ double s_red[4];
    const int q = blockIdx.x, n = ns[q], k = ks[q];
    double up = 1.0, low = 0.0;
    if (k < n) {                                                      // F(k; n, theta) falls in theta: the root of F = delta
        double lo = 0.0, hi = 1.0;
        for (int it = 0; it < 64; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (bounds_cdf(lg, n, k, mid, s_red) > delta) lo = mid;
            else hi = mid;
        }
        up = 0.5 * (lo + hi);
    }
    if (k > 0) {                                                      // 1 - F(k - 1; n, theta) rises in theta: the root of 1 - F = delta
        double lo = 0.0, hi = 1.0;
        for (int it = 0; it < 64; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (1.0 - bounds_cdf(lg, n, k - 1, mid, s_red) < delta) lo = mid;
            else hi = mid;
        }
        low = 0.5 * (lo + hi);
    }
    if (threadIdx.x == 0) { upper[q] = up; lower[q] = low; }
}

// device memory for the length of one entry point: hipMallocAsync here, hipFreeAsync (in stream order) on every way out of the scope
struct StreamTemp {
    void* p = nullptr;
    hipStream_t s;
    StreamTemp(size_t bytes, hipStream_t stream) : s(stream) {
        if (hipMallocAsync(&p, bytes, s) != hipSuccess) { p = nullptr; (void)hipGetLastError(); }
    }
    StreamTemp(const StreamTemp&) = delete;
    ~StreamTemp() { if (p) (void)hipFreeAsync(p, s); }
};

void launch_lgamma_table(int n, double* lg, hipStream_t s) {
    hipLaunchKernelGGL(risk_lgamma_kernel, dim3(grid_1d((long long)n + 1, 256, 4096)), dim3(256), 0, s, n, lg);
}

}  // namespace

extern "C" {

int ee_risk_control(const double* conf, double sign, const double* loss_f64, const uint32_t* loss_q, const uint32_t* cost, int32_t E1, int32_t N,
                    const double* thr, int32_t V, double alpha, double delta, int32_t bound, int32_t method, uint64_t* loss_sum, int64_t* exit_sum,
                    uint64_t* cost_sum, int32_t* hist, double* pvalue, uint8_t* certified, int32_t* n_certified, int32_t* selected, void* stream) {
    const char* who = "ee_risk_control";
    if (!conf || !thr || !loss_sum || !exit_sum || !cost_sum || !pvalue || !certified || !n_certified || !selected)
        return fail(nullptr, "%s: NULL argument (conf, thr and every output but hist are required; cost and hist may be NULL)", who);
    if ((loss_f64 == nullptr) == (loss_q == nullptr)) return fail(nullptr, "%s: exactly one of loss_f64 and loss_q must be given", who);
    if (E1 < 1 || E1 > kRiskMaxE1) return fail(nullptr, "%s: E1 = %d, need 1 <= E1 <= %d", who, E1, kRiskMaxE1);
    if (N < 1 || N >= kRiskMaxN) return fail(nullptr, "%s: N = %d, need 1 <= N < 2^24", who, N);
    if (V < 1 || V > kRiskMaxV) return fail(nullptr, "%s: V = %d vectors, need 1 <= V <= %d", who, V, kRiskMaxV);
    if (!(alpha > 0.0 && alpha < 1.0)) return fail(nullptr, "%s: alpha = %g, the risk level must lie in (0, 1)", who, alpha);
    if (!(delta > 0.0 && delta < 1.0)) return fail(nullptr, "%s: delta = %g, the failure probability must lie in (0, 1)", who, delta);
    if (sign != 1.0 && sign != -1.0) return fail(nullptr, "%s: sign is +1 or -1", who);
    if (bound != MMEE_RISK_BINOMIAL && bound != MMEE_RISK_HB)
        return fail(nullptr, "%s: bound %d is neither MMEE_RISK_BINOMIAL nor MMEE_RISK_HB", who, bound);
    if (method != MMEE_RISK_FIXED_SEQUENCE && method != MMEE_RISK_BONFERRONI)
        return fail(nullptr, "%s: method %d is neither MMEE_RISK_FIXED_SEQUENCE nor MMEE_RISK_BONFERRONI", who, method);
    if (!have_device(who)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long cells = (long long)E1 * N;
    // workspace: lg [N + 1] doubles | F [N + 1] doubles | loss_q [E1 N] words and the error word (the float64 form only)
    const size_t o_F = sizeof(double) * ((size_t)N + 1), o_q = 2 * o_F, o_err = o_q + (loss_f64 ? sizeof(unsigned) * (size_t)cells : 0);
    const StreamTemp ws(o_err + (loss_f64 ? sizeof(int) : 0), s);
    if (!ws.p) return fail(nullptr, "%s: hipMallocAsync of the workspace failed", who);
    char* base = static_cast<char*>(ws.p);
    double *lg = reinterpret_cast<double*>(base), *F = reinterpret_cast<double*>(base + o_F);
    const unsigned* q = loss_q;
    if (loss_f64) {                                                   // quantise into the workspace and look at the error word before any output is written
        unsigned* qw = reinterpret_cast<unsigned*>(base + o_q);
        int* err_dev = reinterpret_cast<int*>(base + o_err);
        if (hipMemsetAsync(err_dev, 0, sizeof(int), s) != hipSuccess) return fail(nullptr, "%s: memset failed", who);
        hipLaunchKernelGGL(risk_quantise_kernel, dim3(grid_1d(cells, 256, 4096)), dim3(256), 0, s, loss_f64, cells, bound == MMEE_RISK_BINOMIAL ? 1 : 0,
                           qw, err_dev);
        if (launch_status(nullptr, who)) return 1;
        int err = 0;
        if (hipMemcpyAsync(&err, err_dev, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return fail(nullptr, "%s: reading the error word failed: %s", who, hipGetErrorString(hipGetLastError()));
        if (err)
            return fail(nullptr, bound == MMEE_RISK_BINOMIAL ? "%s: a loss is not 0 or 1 (MMEE_RISK_BINOMIAL takes binary tables; MMEE_RISK_HB takes [0, 1]); no output was written"
                                                             : "%s: a loss is not finite or lies outside [0, 1]; no output was written", who);
        q = qw;
    }
    // the sums are added into: zeroed first (behind the loss check, so a refused table leaves them untouched).  Workgroups per vector: enough
    // to put about 1024 on the device when V is small, never more than there are 256-document slices
    if (hipMemsetAsync(loss_sum, 0, sizeof(uint64_t) * (size_t)V, s) != hipSuccess || hipMemsetAsync(exit_sum, 0, sizeof(int64_t) * (size_t)V, s) != hipSuccess ||
        hipMemsetAsync(cost_sum, 0, sizeof(uint64_t) * (size_t)V, s) != hipSuccess ||
        (hist && hipMemsetAsync(hist, 0, sizeof(int32_t) * (size_t)V * E1, s) != hipSuccess))
        return fail(nullptr, "%s: memset failed", who);
    const int per_vector = std::max(1, std::min((1024 + V - 1) / V, (N + 255) / 256));
    hipLaunchKernelGGL(risk_count_kernel, dim3(grid_1d(V, 1, 8192), per_vector), dim3(256), 0, s, conf, sign, q, cost, E1, N, thr, V,
                       reinterpret_cast<unsigned long long*>(loss_sum), reinterpret_cast<long long*>(exit_sum),
                       reinterpret_cast<unsigned long long*>(cost_sum), hist);
    launch_lgamma_table(N, lg, s);
    hipLaunchKernelGGL(risk_cdf_kernel, dim3(1), dim3(1024), 0, s, lg, N, alpha, F);
    hipLaunchKernelGGL(risk_select_kernel, dim3(1), dim3(1024), 0, s, reinterpret_cast<const unsigned long long*>(loss_sum),
                       reinterpret_cast<const unsigned long long*>(cost_sum), V, N, alpha, delta, bound, method, F, pvalue, certified, n_certified,
                       selected);
    return launch_status(nullptr, who);
}

int ee_binomial_bounds(const int32_t* n, const int32_t* k, int32_t Q, double delta, double* upper, double* lower, void* stream) {
    const char* who = "ee_binomial_bounds";
    if (!n || !k || !upper || !lower) return fail(nullptr, "%s: NULL argument (n, k host int32 (Q,); upper, lower dev double (Q,))", who);
    if (Q < 1 || Q > kRiskMaxV) return fail(nullptr, "%s: Q = %d queries, need 1 <= Q <= %d", who, Q, kRiskMaxV);
    if (!(delta > 0.0 && delta < 1.0)) return fail(nullptr, "%s: delta = %g, the failure probability must lie in (0, 1)", who, delta);
    int max_n = 0;
    for (int i = 0; i < Q; ++i) {
        if (n[i] < 1 || n[i] >= kRiskMaxN) return fail(nullptr, "%s: n[%d] = %d, need 1 <= n < 2^24", who, i, n[i]);
        if (k[i] < 0 || k[i] > n[i]) return fail(nullptr, "%s: k[%d] = %d outside [0, n = %d]", who, i, k[i], n[i]);
        max_n = std::max(max_n, n[i]);
    }
    if (!have_device(who)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // workspace: lg [max_n + 1] doubles | n [Q] ints | k [Q] ints
    const size_t o_n = sizeof(double) * ((size_t)max_n + 1), o_k = o_n + sizeof(int) * (size_t)Q;
    const StreamTemp ws(o_k + sizeof(int) * (size_t)Q, s);
    if (!ws.p) return fail(nullptr, "%s: hipMallocAsync of the workspace failed", who);
    char* base = static_cast<char*>(ws.p);
    if (hipMemcpyAsync(base + o_n, n, sizeof(int) * (size_t)Q, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(base + o_k, k, sizeof(int) * (size_t)Q, hipMemcpyHostToDevice, s) != hipSuccess)
        return fail(nullptr, "%s: host-to-device copy of the queries failed", who);
    launch_lgamma_table(max_n, reinterpret_cast<double*>(base), s);
    hipLaunchKernelGGL(binomial_bounds_kernel, dim3(Q), dim3(256), 0, s, reinterpret_cast<const int*>(base + o_n), reinterpret_cast<const int*>(base + o_k),
                       reinterpret_cast<const double*>(base), delta, upper, lower);
    return launch_status(nullptr, who);
}

}  // extern "C"
