// What the device fits share (head_fit.hip: one Linear; mlp_head_fit.hip: dense + tanh + out_proj; lte_fit.hip: the LTE classifier): the
// workspace of a fit, the control words the loss / gradient kernels read to skip a stopped exit, the workgroup sum, and the L-BFGS driver
// (fit_lbfgs.hip: the controller and the finish kernel, one copy, written over a parameter count P) with the point it has an objective evaluate.
#pragma once
#include <functional>
#include <initializer_list>

#include "mmee_kernels.h"

namespace mmee {

constexpr int kFitCtrlThreads = 1024;

// per-exit control words / scalars of the workspace
enum { CI_STOP = 0, CI_EVALS, CI_HALVINGS, CI_COUNT, CI_HEAD, kCtrlInts = 8 };          // CI_STOP: 0 running, else status + 1 (4: bad label)
enum { CD_F = 0, CD_STEP, CD_DG, CD_GNORM, CD_GAMMA, kCtrlDoubles = 8 };

// the sum of v over the workgroup's THREADS threads in a fixed tree order, the same bits in every thread; red: THREADS doubles of LDS
template <int THREADS>
__device__ inline double block_sum(double v, double* red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

// ---- the distilled row step (ee_head_fit_distill, ee_mlp_head_fit_distill; include/mmee.h states the objective) ----------------------------
// A row of K <= 64 classes lies over eight neighbouring lanes: lane `sub` holds class sub + 8 i in slot i.  Both head types call the two
// functions below from every lane of a wave (they shuffle), the one-layer fit from its slab walk, the two-layer fit from its softmax kernel.
constexpr int kRowSlots = 8;

__device__ inline double row8_max(double v) {
    v = fmax(v, __shfl_xor(v, 1));
    v = fmax(v, __shfl_xor(v, 2));
    return fmax(v, __shfl_xor(v, 4));
}
__device__ inline double row8_sum(double v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    return v + __shfl_xor(v, 4);
}

// The teacher's row into registers, each element read once; a row that does not exist reads as zeros.  A logit that is not finite (dump-all
// marks the rows a document never reached with NaN) raises bit 1 of the error word.
__device__ inline void load_teacher_row(const float* trow, bool valid, int sub, int K, float (&tv)[kRowSlots], int* err) {
    bool bad = false;
#pragma unroll
    for (int i = 0; i < kRowSlots; ++i) {
        const int k = sub + 8 * i;
        tv[i] = (valid && k < K) ? trow[k] : 0.f;
        bad |= !__builtin_isfinite(tv[i]);
    }
    if (bad) atomicOr(err, 2);
}

// v: the row's logits z, replaced by N dL/dz = (1 - alpha)(p - onehot(y)) + alpha T (pT - q); returns the row's
// (1 - alpha)(logsumexp(z) - z[y]) + alpha T^2 KL(q || pT), the same bits in the row's eight lanes.  q = softmax(tv / T), p = softmax(z),
// pT = softmax(z / T), all max-shifted; log q and log pT are shifted logits minus the log of their sum, so a q_k that underflows to zero
// contributes exactly zero.  hard = alpha < 1: without it neither y nor p is looked at.  y < 0 (a label out of range, the error word is
// raised) leaves the hard target out.  At T = 1 pT is p and its exponentials are taken once.
__device__ inline double distill_row(double (&v)[kRowSlots], const float (&tv)[kRowSlots], int sub, int K, long long y, bool hard, double alpha,
                                     double T) {
    double m = -INFINITY, tm = -INFINITY;
#pragma unroll
    for (int i = 0; i < kRowSlots; ++i)
        if (sub + 8 * i < K) {
            m = fmax(m, v[i]);
            tm = fmax(tm, (double)tv[i]);
        }
    m = row8_max(m);
    tm = row8_max(tm);
    const bool own = hard && T != 1.0;                       // p needs exponentials of its own
    double eT[kRowSlots], eq[kRowSlots], e1[kRowSlots];
    double sT = 0.0, sq = 0.0, s1 = 0.0, zy = 0.0;
#pragma unroll
    for (int i = 0; i < kRowSlots; ++i) {
        const int k = sub + 8 * i;
        const bool in = k < K;
        if (in && k == (int)y) zy = v[i];
        v[i] = in ? v[i] - m : 0.0;
        eT[i] = in ? exp(v[i] / T) : 0.0;
        eq[i] = in ? exp(((double)tv[i] - tm) / T) : 0.0;
        e1[i] = (own && in) ? exp(v[i]) : eT[i];
        sT += eT[i];
        sq += eq[i];
        s1 += e1[i];
    }
    sT = row8_sum(sT);
    sq = row8_sum(sq);
    s1 = row8_sum(s1);
    zy = row8_sum(zy);
    const double log_sT = log(sT), log_sq = log(sq), inv_sT = 1.0 / sT, inv_sq = 1.0 / sq, inv_s1 = 1.0 / s1;
    const double soft = alpha * T, keep = hard ? 1.0 - alpha : 0.0;
    double kl = 0.0;
#pragma unroll
    for (int i = 0; i < kRowSlots; ++i) {
        const int k = sub + 8 * i;
        if (k < K) {
            const double q = eq[i] * inv_sq;
            const double log_q = ((double)tv[i] - tm) / T - log_sq, log_pT = v[i] / T - log_sT;
            kl = fma(q, log_q - log_pT, kl);
            double d = soft * (eT[i] * inv_sT - q);
            if (hard) d += keep * (e1[i] * inv_s1 - (k == (int)y ? 1.0 : 0.0));
            v[i] = d;
        }
    }
    kl = row8_sum(kl);
    return (hard && y >= 0 ? keep * ((m + log(s1)) - zy) : 0.0) + soft * T * kl;
}

// ---- the gate objective's element (ee_head_fit_gate, ee_mlp_head_fit_gate; include/mmee.h states the objective) ------------------------------
// bce(z, t) = softplus(z) - t z with softplus(z) = max(z, 0) + log1p(exp(-|z|)), which does not overflow; its derivative sigmoid(z) - t from the
// same exponential.  The one-layer fit calls it from its slab walk (gate_row_step), the two-layer fit from its gate row kernel.
__device__ inline double gate_bce(double z, double t, double& dz) {
    const double ez = exp(-fabs(z)), inv = 1.0 / (1.0 + ez);
    dz = (z >= 0.0 ? inv : ez * inv) - t;
    return (fmax(z, 0.0) + log1p(ez)) - t * z;
}

// ---- sample weights (ee_head_fit_weighted, ee_mlp_head_fit_weighted; include/mmee.h states the objective) ------------------------------------
// The weighted fits scale a row's N dL/dz and its loss by scale[e][n] = w[e][n] N / W_e and change nothing behind the row step: every later
// kernel divides by N as before.  launch_row_scale (head_fit.hip) makes the table once per call, one workgroup per exit: W_e in float64 in a
// fixed order (strided partial sums, then the tree of block_sum), error-word bit 2 for a weight that is negative or not finite, bit 3 for
// W_e == 0.  A row whose scale is zero is treated by the row steps as a row that does not exist: zeros are written, no loss is added, and
// neither its label nor its teacher row is read.  Its FEATURES still take part in the gradient pass as 0 * x and must be finite: 0 * NaN is
// not defended against.
void launch_row_scale(const float* weights, int E, int N, double* scale, int* err, hipStream_t s);

// The table lies behind the objective's own scratch (the one-layer fit's chunk partials, the two-layer fit's rows): `scratch_bytes` into the
// tail of a fit's workspace, or into a debug call's buffer
inline double* scale_table(void* tail, size_t scratch_bytes) { return reinterpret_cast<double*>(static_cast<char*>(tail) + scratch_bytes); }

// scale[e][n] of a row, zero for a row that does not exist
__device__ inline double row_scale(const double* scale, int e, int N, long long n) { return n < N ? scale[(size_t)e * N + n] : 0.0; }

// v * sc in the weighted form of a row step, v itself in the unweighted one, whose instruction stream has no multiplication to skip
template <bool WEIGHTED>
__device__ inline double scaled(double v, double sc) {
    if constexpr (WEIGHTED) return v * sc;
    else return v;
}

// The workspace of one fit.  Per exit: control words, scalars, then the parameter-sized vectors; behind them `tail_bytes` of whatever an
// evaluation of the objective needs (the one-layer fit's chunk partials, the two-layer fit's hidden rows).  The error word lives at 0.
struct FitLayout {
    int E, P, M;
    size_t o_ctrl, o_scal, o_ftrial, o_rho, o_vec, o_tail, zero_bytes, bytes;
    size_t vec_stride;               // doubles per exit: (5 + 2 M) * P
    FitLayout(int E_, int P_, int M_, size_t tail_bytes) : E(E_), P(P_), M(M_) {
        auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
        o_ctrl = 256;
        o_scal = al(o_ctrl + sizeof(int) * kCtrlInts * (size_t)E);
        o_ftrial = al(o_scal + sizeof(double) * kCtrlDoubles * (size_t)E);
        o_rho = al(o_ftrial + sizeof(double) * (size_t)E);
        o_vec = al(o_rho + sizeof(double) * (size_t)M * E);
        vec_stride = (size_t)(5 + 2 * M) * P;
        zero_bytes = al(o_vec + sizeof(double) * vec_stride * E);       // everything in front of the tail starts from zero
        o_tail = zero_bytes;
        bytes = o_tail + tail_bytes;
    }
};
enum { V_THETA = 0, V_TRIAL, V_G, V_GTRIAL, V_DIR, V_HIST };            // V_HIST: s[0 .. M), then y[0 .. M)

// Where one evaluation of an objective reads theta and writes L and grad L: the driver's trial point, or a debug call's own buffers.  Host only.
struct FitEvalPoint {
    const double* theta;             // exit e: theta + e * theta_stride
    size_t theta_stride;
    const int* ctrl;                 // per exit kCtrlInts words, or null: every exit runs
    int* err;                        // the error word
    double* loss;                    // exit e: loss[e]
    double* grad;                    // exit e: grad + e * grad_stride
    size_t grad_stride;
    void* tail;                      // the objective's scratch: FitLayout's tail
};

// theta[begin, begin + len) of exit e goes to out32 + e * len and to out64 + e * len, each when given
struct FitOutSeg {
    int begin, len;
    float* out32;
    double* out64;
};
struct FitFinishArgs {
    const char* ws;
    FitLayout lay;
    int n_seg;
    FitOutSeg seg[4];
    double* theta64;                 // (E,P) or null
    double *loss, *grad_norm;        // (E,) or null
    int *evals, *status;             // (E,) or null
};

// The whole fit on stream s: the workspace zeroed, f.theta0 ((lay.E, lay.P), null = 0) as the first trial point, f.max_evals ticks of
// { eval(trial point); controller }, then theta[seg] of every exit to the segments' outputs and f's result pointers.  weights, when not null (the
// weighted head fits' (E,N) table): launch_row_scale once on the zeroed workspace in front of the first tick, to scale_table(tail,
// scratch_bytes), where the objective's own scratch ends.  false: preparing the workspace failed.
bool run_lbfgs_fit(const FitArgs& f, const FitLayout& lay, const std::function<void(const FitEvalPoint&)>& eval,
                   std::initializer_list<FitOutSeg> segs, hipStream_t s, const float* weights, size_t scratch_bytes);

}  // namespace mmee
