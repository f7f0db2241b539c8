// ee_mlp_head_fit (include/mmee.h): two-layer ramp exit heads (dense + tanh + out_proj) fitted on the device from a frozen backbone's CLS rows,
// float64 arithmetic on the float32 features.  The L-BFGS is run_lbfgs_fit (fit_lbfgs.hip), the workspace layout the one-layer fit's
// (head_fit_common.h); this file is the objective: one evaluation of L and grad L at theta = (W1, b1, W2, b2) is seven launches.
//
//   mlp_nt_gemm_kernel<float, tanh>   A = tanh(X W1^T + b1)            (N,H) float64, kept in the workspace          2 N H^2 FLOP
//   mlp_nt_gemm_kernel<double>        Z = A W2^T + b2                  (N,K)
//   mlp_softmax_kernel                D = softmax(Z) - Y in place of Z, the rows' losses, the label check
//                                     (ee_mlp_head_fit_distill: mlp_distill_softmax_kernel in its place, D = N dL/dZ of the mixed objective;
//                                      ee_mlp_head_fit_gate: mlp_gate_kernel, D = (sigmoid(Z) - T) / 2 and the target check)
//   mlp_tn_gemm_kernel<double>        dW2 = D^T A, db2 = D^T 1         written as gradient: / N + l2 theta
//   mlp_dact_kernel                   dA = (D W2) (1 - A^2)            in place of A
//   mlp_tn_gemm_kernel<float>         dW1 = dA^T X, db1 = dA^T 1       written as gradient                           2 N H^2 FLOP
//   mlp_loss_kernel                   L = (sum of the rows' losses) / N + (l2 / 2) ||theta||^2
// ee_mlp_head_fit_weighted: the two softmax kernels are templates over their argument struct, and the weighted structs select (if constexpr)
// the row step that multiplies D and the row's loss by scale[e][n] = w[e][n] N / W_e (launch_row_scale, head_fit_common.h, once per call) and
// skips a row whose scale is zero.  The other six launches are shared, division by N included; the unweighted instantiations are the code
// they were.  ee_mlp_head_fit_gate (two-layer 2-way gate heads, K = 2) puts a third row kernel in the same place: mlp_gate_kernel, the two
// binary cross-entropies of the gate objective against a target in [0, 1] per (exit, row) (gate_bce, head_fit_common.h), with the same
// weighted form (ee_mlp_head_fit_gate_weighted).  launch_eval reads which of the six a call launches off its HeadObjective (mmee_kernels.h);
// run_lbfgs_fit makes the table, behind this file's scratch (scale_table, head_fit_common.h).
//
// Both GEMM kernels are LDS-tiled with BOTH operands staged (64 x 64 output tile, 16 deep, the next tile's global loads in flight behind the
// products) and multiply with v_mfma_f64_16x16x4_f64: four waves of 32 x 32, four accumulators each.  Its C/D map is NOT the f32 one: lane l,
// register r hold row (l >> 4) + 4 r, column l & 15.
//
// Determinism: no atomics on floating-point data.  A workgroup owns its output tile and walks the whole summation index in order (H for the
// NT form, all N rows for the TN form), so every sum has an order that depends on (N, H, K) alone; the exit is the grid's z and nothing
// depends on E.  The price is paid at small H: the TN form has (H / 64)^2 workgroups an exit, each N / 16 steps long.
#include <type_traits>

#include "head_fit_common.h"

namespace mmee {

namespace {

constexpr int kThreads = 256;
constexpr int TM = kMlpHeadFitRows, TN = 64, TK = 16;    // output tile, depth of a staged tile
constexpr int kNtLd = TK + 2;                            // [row][k]: 36 words a row, a half-wave's 16 rows x 2 k fall into 32 distinct bank pairs
constexpr int kTnLd = TM + 16;                           // [k][column]: 160 words a row, two k of a half-wave take the two halves of the banks
constexpr int kSoftRows = 32, kDactRows = 16;
static_assert(TM == 64 && TN == 64 && kThreads == 256, "the staging and wave maps below are written for 64 x 64 tiles and four waves");
using f64x4 = __attribute__((ext_vector_type(4))) double;

struct EvalArgs {
    const float* X;                  // (E,N,H)
    const long long* y;              // (N,)
    const double* theta;             // exit e: theta + e * theta_stride; W1 (H,H), b1 (H,), W2 (K,H), b2 (K,)
    size_t theta_stride;
    const int* ctrl;                 // per exit kCtrlInts words, or null: every exit runs
    int* err;                        // bit 0: a label outside [0,K)
    double *A, *Z, *rowloss;         // (E,N,H) hidden rows then dA; (E,N,K) logits then D; (E,N)
    double* loss;                    // exit e: loss[e * loss_stride]
    size_t loss_stride;
    double* grad;                    // exit e: grad + e * grad_stride, the layout of theta
    size_t grad_stride;
    int N, H, K;
    double l2;
};
// ee_mlp_head_fit_distill: err bit 1 is a teacher logit that is not finite; y is null at alpha = 1
struct DistillEvalArgs : EvalArgs {
    const float* teacher;            // (N,K)
    double alpha, temperature;
};
// ee_mlp_head_fit_weighted: either objective with the row-scale table of launch_row_scale (head_fit_common.h); err bits 2 and 3 are the table's
struct WeightedEvalArgs : EvalArgs {
    const double* scale;             // (E,N): w[e][n] N / W_e
};
struct WeightedDistillEvalArgs : DistillEvalArgs {
    const double* scale;
};
// ee_mlp_head_fit_gate: K == 2 and y null; err bit 0 is a target that is not finite or lies outside [0,1]
struct GateEvalArgs : EvalArgs {
    const double* targets;           // (E,N): c[e][n] = how right classifier(gate input) is at exit e on row n
};
// ee_mlp_head_fit_gate_weighted
struct WeightedGateEvalArgs : GateEvalArgs {
    const double* scale;
};
template <typename Args>
constexpr bool kWeighted = std::is_same_v<Args, WeightedEvalArgs> || std::is_same_v<Args, WeightedDistillEvalArgs> ||
                           std::is_same_v<Args, WeightedGateEvalArgs>;

__device__ inline bool stopped(const int* ctrl, int e) { return ctrl && ctrl[e * kCtrlInts + CI_STOP] != 0; }

// p[0 .. 4) of a row whose column index starts at col, as float64; a column >= lim and a row that does not exist read as zero.
// The float32 source is the feature matrix: lim % 4 == 0 and 16-byte aligned rows, so the four are inside or outside together.
__device__ inline void load4(const float* base, size_t off, int col, int lim, bool row_ok, double (&v)[4]) {
    f32x4 x{0.f, 0.f, 0.f, 0.f};
    if (row_ok && col < lim) x = *reinterpret_cast<const f32x4*>(base + off);
    v[0] = (double)x[0]; v[1] = (double)x[1]; v[2] = (double)x[2]; v[3] = (double)x[3];
}
__device__ inline void load4(const double* base, size_t off, int col, int lim, bool row_ok, double (&v)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (row_ok && col + i < lim) ? base[off + i] : 0.0;
}

__device__ inline f64x4 mfma(double a, double b, f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// ---- C[n][j] = epi(sum_h X[n][h] W[j][h] + b[j]) ------------------------------------------------------------------------------------------------
struct NtArgs {
    const void* X;                   // exit e: rows at X + e * x_stride elements, (N, H) row-major
    size_t x_stride;
    const double* theta;
    size_t theta_stride, oW, ob;     // W (J,H) and b (J,) inside theta
    double* C;                       // exit e: C + e * c_stride, (N, J) row-major
    size_t c_stride;
    const int* ctrl;
    int N, J, H;
};

// grid (ceil(N / TM), ceil(J / TN), E)
template <typename XT, bool TANH>
__global__ __launch_bounds__(kThreads) void mlp_nt_gemm_kernel(NtArgs a) {
    const int e = blockIdx.z, t = threadIdx.x;
    if (stopped(a.ctrl, e)) return;
    __shared__ double As[TM * kNtLd], Bs[TN * kNtLd];
    const int N = a.N, J = a.J, H = a.H, n0 = blockIdx.x * TM, j0 = blockIdx.y * TN;
    const XT* X = static_cast<const XT*>(a.X) + (size_t)e * a.x_stride;
    const double* W = a.theta + (size_t)e * a.theta_stride + a.oW;
    const double* b = a.theta + (size_t)e * a.theta_stride + a.ob;
    const int srow = t >> 2, sq = (t & 3) * 4;                       // staging: row of the tile, first of four k
    const bool x_ok = n0 + srow < N, w_ok = j0 + srow < J;
    const size_t x_off = (size_t)(n0 + srow) * H + sq, w_off = (size_t)(j0 + srow) * H + sq;
    const int lane = t & 63, wv = t >> 6, wm = (wv >> 1) * 32, wn = (wv & 1) * 32, li = lane & 15, lk = lane >> 4;

    f64x4 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f64x4{0.0, 0.0, 0.0, 0.0};

    double pa[4], pb[4];
    load4(X, x_off, sq, H, x_ok, pa);
    load4(W, w_off, sq, H, w_ok, pb);
    for (int k0 = 0; k0 < H; k0 += TK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            As[srow * kNtLd + sq + i] = pa[i];
            Bs[srow * kNtLd + sq + i] = pb[i];
        }
        __syncthreads();
        if (k0 + TK < H) {
            load4(X, x_off + k0 + TK, k0 + TK + sq, H, x_ok, pa);
            load4(W, w_off + k0 + TK, k0 + TK + sq, H, w_ok, pb);
        }
#pragma unroll
        for (int kk = 0; kk < TK; kk += 4) {
            const double a0 = As[(wm + li) * kNtLd + kk + lk], a1 = As[(wm + 16 + li) * kNtLd + kk + lk];
            const double b0 = Bs[(wn + li) * kNtLd + kk + lk], b1 = Bs[(wn + 16 + li) * kNtLd + kk + lk];
            acc[0][0] = mfma(a0, b0, acc[0][0]);
            acc[0][1] = mfma(a0, b1, acc[0][1]);
            acc[1][0] = mfma(a1, b0, acc[1][0]);
            acc[1][1] = mfma(a1, b1, acc[1][1]);
        }
        __syncthreads();
    }

    double* C = a.C + (size_t)e * a.c_stride;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int j = j0 + wn + ni * 16 + li;
            if (j >= J) continue;
            const double bj = b[j];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + wm + mi * 16 + lk + 4 * r;
                if (n >= N) continue;
                const double v = acc[mi][ni][r] + bj;
                C[(size_t)n * J + j] = TANH ? tanh(v) : v;
            }
        }
}

// ---- G[m][c] = (sum_n P[n][m] Q[n][c]) / N + l2 theta,  g[m] = (sum_n P[n][m]) / N + l2 theta -----------------------------------------------
struct TnArgs {
    const double* P;                 // exit e: P + e * p_stride, (N, M) row-major
    size_t p_stride;
    const void* Q;                   // exit e: Q + e * q_stride elements, (N, Cc) row-major
    size_t q_stride;
    const double* theta;
    size_t theta_stride;
    double* grad;
    size_t grad_stride, oW, ob;      // G (M,Cc) and g (M,) inside theta and grad
    const int* ctrl;
    int N, M, Cc;
    double l2;
};

// grid (ceil(M / TM), ceil(Cc / TN), E); the workgroups of the first column tile also sum P's columns
template <typename QT>
__global__ __launch_bounds__(kThreads) void mlp_tn_gemm_kernel(TnArgs a) {
    const int e = blockIdx.z, t = threadIdx.x;
    if (stopped(a.ctrl, e)) return;
    __shared__ double Ps[TK * kTnLd], Qs[TK * kTnLd];
    const int N = a.N, M = a.M, Cc = a.Cc, m0 = blockIdx.x * TM, c0 = blockIdx.y * TN;
    const double* P = a.P + (size_t)e * a.p_stride;
    const QT* Q = static_cast<const QT*>(a.Q) + (size_t)e * a.q_stride;
    const int srow = t >> 4, sq = (t & 15) * 4;                      // staging: row n of the tile, first of four columns
    const int lane = t & 63, wv = t >> 6, wm = (wv >> 1) * 32, wn = (wv & 1) * 32, li = lane & 15, lk = lane >> 4;
    const bool sums = blockIdx.y == 0 && t < TM;

    f64x4 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f64x4{0.0, 0.0, 0.0, 0.0};
    double colsum = 0.0;

    double pa[4], pb[4];
    auto fetch = [&](int n) {
        load4(P, (size_t)n * M + m0 + sq, m0 + sq, M, n < N, pa);
        load4(Q, (size_t)n * Cc + c0 + sq, c0 + sq, Cc, n < N, pb);
    };
    fetch(srow);
    for (int n0 = 0; n0 < N; n0 += TK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            Ps[srow * kTnLd + sq + i] = pa[i];
            Qs[srow * kTnLd + sq + i] = pb[i];
        }
        __syncthreads();
        if (n0 + TK < N) fetch(n0 + TK + srow);
#pragma unroll
        for (int kk = 0; kk < TK; kk += 4) {
            const double a0 = Ps[(kk + lk) * kTnLd + wm + li], a1 = Ps[(kk + lk) * kTnLd + wm + 16 + li];
            const double b0 = Qs[(kk + lk) * kTnLd + wn + li], b1 = Qs[(kk + lk) * kTnLd + wn + 16 + li];
            acc[0][0] = mfma(a0, b0, acc[0][0]);
            acc[0][1] = mfma(a0, b1, acc[0][1]);
            acc[1][0] = mfma(a1, b0, acc[1][0]);
            acc[1][1] = mfma(a1, b1, acc[1][1]);
        }
        if (sums) {
#pragma unroll
            for (int k = 0; k < TK; ++k) colsum += Ps[k * kTnLd + t];
        }
        __syncthreads();
    }

    const double* th = a.theta + (size_t)e * a.theta_stride;
    double* g = a.grad + (size_t)e * a.grad_stride;
    const double dn = (double)N;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int c = c0 + wn + ni * 16 + li;
            if (c >= Cc) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + mi * 16 + lk + 4 * r;
                if (m >= M) continue;
                const size_t i = a.oW + (size_t)m * Cc + c;
                g[i] = acc[mi][ni][r] / dn + a.l2 * th[i];
            }
        }
    if (sums && m0 + t < M) {
        const size_t i = a.ob + m0 + t;
        g[i] = colsum / dn + a.l2 * th[i];
    }
}

// a row whose scale is zero: D = 0 in place of its logits, no loss; Z: the row, sub: the thread's place among the row's eight
__device__ inline void zero_row(double* Z, double* rowloss, int sub, int K) {
    for (int k = sub; k < K; k += 8) Z[k] = 0.0;
    if (sub == 0) *rowloss = 0.0;
}

// ---- max-shifted softmax of the logits, D = P - Y in their place, the rows' losses: eight threads a row, a row's values in registers ------------
// Args: EvalArgs, or WeightedEvalArgs: D and the row's loss times the row's scale, last of all; a row whose scale is zero gets zeros and
// its label is not read (live: the row exists and counts).
// grid (ceil(N / kSoftRows), E)
template <typename Args>
__global__ __launch_bounds__(kThreads) void mlp_softmax_kernel(Args a) {
    const int e = blockIdx.y, t = threadIdx.x, sub = t & 7, K = a.K;
    if (stopped(a.ctrl, e)) return;
    const int row = blockIdx.x * kSoftRows + (t >> 3);
    const bool valid = row < a.N;
    bool live = valid;
    double sc = 1.0;
    if constexpr (kWeighted<Args>) {
        sc = row_scale(a.scale, e, a.N, row);
        live = sc != 0.0;
    }
    double* Z = a.Z + ((size_t)e * a.N + (valid ? row : 0)) * K;
    long long y = live ? a.y[row] : 0;
    if (y < 0 || y >= K) {
        atomicOr(a.err, 1);
        y = -1;
    }
    double v[8];
    double m = -INFINITY;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = sub + 8 * i;
        v[i] = (live && k < K) ? Z[k] : -INFINITY;
        m = fmax(m, v[i]);
    }
    m = fmax(m, __shfl_xor(m, 1));
    m = fmax(m, __shfl_xor(m, 2));
    m = fmax(m, __shfl_xor(m, 4));
    if (!live) m = 0.0;
    double sum = 0.0, zy = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = sub + 8 * i;
        const bool in = live && k < K;
        if (in && k == (int)y) zy = v[i];
        v[i] = in ? exp(v[i] - m) : 0.0;
        sum += v[i];
    }
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    sum += __shfl_xor(sum, 4);
    zy += __shfl_xor(zy, 1);
    zy += __shfl_xor(zy, 2);
    zy += __shfl_xor(zy, 4);
    if (!valid) return;
    if constexpr (kWeighted<Args>) {
        if (!live) {
            zero_row(Z, a.rowloss + (size_t)e * a.N + row, sub, K);
            return;
        }
    }
    const double inv = 1.0 / sum;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = sub + 8 * i;
        if (k < K) Z[k] = scaled<kWeighted<Args>>(v[i] * inv - (k == (int)y ? 1.0 : 0.0), sc);
    }
    if (sub == 0) a.rowloss[(size_t)e * a.N + row] = y >= 0 ? scaled<kWeighted<Args>>((m + log(sum)) - zy, sc) : 0.0;
}

// ---- the distilled counterpart (ee_mlp_head_fit_distill): the mixed row step of distill_row (head_fit_common.h) on the same rows, writing the
// same D in place of Z and the same row losses; the teacher's row comes from global memory, each element read once ----------------------------
// Args: DistillEvalArgs, or WeightedDistillEvalArgs: as for mlp_softmax_kernel; neither the label nor the teacher's row of a row whose scale
// is zero is read.
// grid (ceil(N / kSoftRows), E)
template <typename Args>
__global__ __launch_bounds__(kThreads) void mlp_distill_softmax_kernel(Args a) {
    const int e = blockIdx.y, t = threadIdx.x, sub = t & 7, K = a.K;
    if (stopped(a.ctrl, e)) return;
    const int row = blockIdx.x * kSoftRows + (t >> 3);
    const bool valid = row < a.N, hard = a.alpha < 1.0;
    bool live = valid;
    double sc = 1.0;
    if constexpr (kWeighted<Args>) {
        sc = row_scale(a.scale, e, a.N, row);
        live = sc != 0.0;
    }
    double* Z = a.Z + ((size_t)e * a.N + (valid ? row : 0)) * K;
    long long y = -1;
    if (hard) {
        y = live ? a.y[row] : 0;
        if (y < 0 || y >= K) {
            atomicOr(a.err, 1);
            y = -1;
        }
    }
    float tv[kRowSlots];
    load_teacher_row(a.teacher + (size_t)(valid ? row : 0) * K, live, sub, K, tv, a.err);
    double v[kRowSlots];
#pragma unroll
    for (int i = 0; i < kRowSlots; ++i) v[i] = (live && sub + 8 * i < K) ? Z[sub + 8 * i] : 0.0;
    const double l = distill_row(v, tv, sub, K, y, hard, a.alpha, a.temperature);
    if (!valid) return;
    if constexpr (kWeighted<Args>) {
        if (!live) {
            zero_row(Z, a.rowloss + (size_t)e * a.N + row, sub, K);
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < kRowSlots; ++i)
        if (sub + 8 * i < K) Z[sub + 8 * i] = scaled<kWeighted<Args>>(v[i], sc);
    if (sub == 0) a.rowloss[(size_t)e * a.N + row] = scaled<kWeighted<Args>>(l, sc);
}

// ---- the gate counterpart (ee_mlp_head_fit_gate): the two binary cross-entropies of the gate objective on the row's two logits against the
// target c[e][n]; D = N dL/dz = (sigmoid(z_j) - t_j) / 2 in place of Z with t_1 = c, t_0 = 1 - c, the row's loss (bce(z_1, c) + bce(z_0, 1 - c)) / 2
// -- mlp_loss_kernel divides by N, which makes the objective's 1 / (2N).  The rows keep the softmax kernels' place in the grid, eight lanes a
// row: lane `sub` takes column sub & 1, lanes 0 and 1 write, and the pair's losses meet by one shuffle.  Every lane reads its logit before
// any of the row writes: they are lanes of one wave.
// Args: GateEvalArgs, or WeightedGateEvalArgs: as for mlp_softmax_kernel; the target of a row whose scale is zero is not read.
// grid (ceil(N / kSoftRows), E)
template <typename Args>
__global__ __launch_bounds__(kThreads) void mlp_gate_kernel(Args a) {
    const int e = blockIdx.y, t = threadIdx.x, sub = t & 7, j = sub & 1;
    if (stopped(a.ctrl, e)) return;
    const int row = blockIdx.x * kSoftRows + (t >> 3);
    const bool valid = row < a.N;
    bool live = valid;
    double sc = 1.0;
    if constexpr (kWeighted<Args>) {
        sc = row_scale(a.scale, e, a.N, row);
        live = sc != 0.0;                                    // true for a NaN scale too: the error word is raised then
    }
    double* Z = a.Z + ((size_t)e * a.N + (valid ? row : 0)) * 2;
    double c = live ? a.targets[(size_t)e * a.N + row] : 0.0;
    if (!(c >= 0.0 && c <= 1.0)) {                           // a NaN fails both compares
        atomicOr(a.err, 1);
        c = 0.0;
    }
    double d;
    double l = gate_bce(live ? Z[j] : 0.0, j ? c : 1.0 - c, d);
    l += __shfl_xor(l, 1);
    if (!valid) return;
    if constexpr (kWeighted<Args>) {
        if (!live) {
            zero_row(Z, a.rowloss + (size_t)e * a.N + row, sub, 2);
            return;
        }
    }
    if (sub < 2) Z[j] = scaled<kWeighted<Args>>(0.5 * d, sc);
    if (sub == 0) a.rowloss[(size_t)e * a.N + row] = scaled<kWeighted<Args>>(0.5 * l, sc);
}

// ---- dA = (D W2) (1 - A^2) in place of A: thread = columns t + 256 i of four rows at a time, so a W2 element serves four rows -----------------
// grid (ceil(N / kDactRows), E)
template <int HC>
__global__ __launch_bounds__(kThreads) void mlp_dact_kernel(EvalArgs a) {
    const int e = blockIdx.y, t = threadIdx.x, N = a.N, H = a.H, K = a.K;
    if (stopped(a.ctrl, e)) return;
    const double* W2 = a.theta + (size_t)e * a.theta_stride + (size_t)H * H + H;
    const double* D = a.Z + (size_t)e * N * K;
    double* A = a.A + (size_t)e * N * H;
    for (int rb = 0; rb < kDactRows; rb += 4) {
        const int n0 = blockIdx.x * kDactRows + rb;
        if (n0 >= N) return;
        double s[4][HC];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int i = 0; i < HC; ++i) s[r][i] = 0.0;
        for (int k = 0; k < K; ++k) {
            double d[4], w[HC];
#pragma unroll
            for (int r = 0; r < 4; ++r) d[r] = n0 + r < N ? D[(size_t)(n0 + r) * K + k] : 0.0;
#pragma unroll
            for (int i = 0; i < HC; ++i) {
                const int j = t + kThreads * i;
                w[i] = j < H ? W2[(size_t)k * H + j] : 0.0;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int i = 0; i < HC; ++i) s[r][i] = fma(d[r], w[i], s[r][i]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int i = 0; i < HC; ++i) {
                const int j = t + kThreads * i;
                if (n0 + r < N && j < H) {
                    const size_t at = (size_t)(n0 + r) * H + j;
                    const double av = A[at];
                    A[at] = s[r][i] * fma(-av, av, 1.0);
                }
            }
    }
}

// ---- L = (sum_n loss_n) / N + (l2 / 2) ||theta||^2: one workgroup an exit, strided partial sums, then the fixed tree of block_sum -------------
__global__ __launch_bounds__(kFitCtrlThreads) void mlp_loss_kernel(EvalArgs a) {
    const int e = blockIdx.x, t = threadIdx.x, P = a.H * a.H + a.H + a.K * a.H + a.K;
    if (stopped(a.ctrl, e)) return;
    __shared__ double red[kFitCtrlThreads];
    const double* rl = a.rowloss + (size_t)e * a.N;
    const double* th = a.theta + (size_t)e * a.theta_stride;
    double sum = 0.0, sq = 0.0;
    for (int i = t; i < a.N; i += kFitCtrlThreads) sum += rl[i];
    for (int i = t; i < P; i += kFitCtrlThreads) sq = fma(th[i], th[i], sq);
    sum = block_sum<kFitCtrlThreads>(sum, red);
    sq = block_sum<kFitCtrlThreads>(sq, red);
    if (t == 0) a.loss[(size_t)e * a.loss_stride] = sum / (double)a.N + 0.5 * a.l2 * sq;
}

int ceil_div(int v, int d) { return (v + d - 1) / d; }
size_t params(int H, int K) { return (size_t)H * H + H + (size_t)K * H + K; }
size_t scratch_bytes(int E, int N, int H, int K) { return sizeof(double) * mlp_head_fit_scratch_doubles(E, N, H, K); }

// one evaluation: L and grad L of every running exit; p.tail: mlp_head_fit_scratch_doubles doubles -- hidden rows, logits, the rows' losses;
// what o holds picks the row kernel and its argument struct: gate targets (K == 2) the gate objective, a teacher the distilled one, weights
// the weighted form of any of the three, whose row scales (E,N) lie behind the rows' losses
void launch_eval(const FitEvalPoint& p, const float* X, const HeadObjective& o, int E, int N, int H, int K, double l2, hipStream_t s) {
    EvalArgs a{};
    a.X = X; a.y = o.labels; a.theta = p.theta; a.theta_stride = p.theta_stride; a.ctrl = p.ctrl; a.err = p.err;
    a.A = static_cast<double*>(p.tail); a.Z = a.A + (size_t)E * N * H; a.rowloss = a.Z + (size_t)E * N * K;
    a.loss = p.loss; a.loss_stride = 1; a.grad = p.grad; a.grad_stride = p.grad_stride; a.N = N; a.H = H; a.K = K; a.l2 = l2;
    const size_t HH = (size_t)H * H, oW1 = 0, ob1 = HH, oW2 = HH + H, ob2 = HH + H + (size_t)K * H;
    NtArgs hid{a.X, (size_t)N * H, a.theta, a.theta_stride, oW1, ob1, a.A, (size_t)N * H, a.ctrl, N, H, H};
    hipLaunchKernelGGL((mlp_nt_gemm_kernel<float, true>), dim3(ceil_div(N, TM), ceil_div(H, TN), E), dim3(kThreads), 0, s, hid);
    NtArgs out{a.A, (size_t)N * H, a.theta, a.theta_stride, oW2, ob2, a.Z, (size_t)N * K, a.ctrl, N, K, H};
    hipLaunchKernelGGL((mlp_nt_gemm_kernel<double, false>), dim3(ceil_div(N, TM), ceil_div(K, TN), E), dim3(kThreads), 0, s, out);
    const dim3 sgrid(ceil_div(N, kSoftRows), E);
    const DistillEvalArgs d{a, o.soft.teacher, o.soft.alpha, o.soft.temperature};
    const double* scale = o.weights ? scale_table(p.tail, scratch_bytes(E, N, H, K)) : nullptr;
    const GateEvalArgs g{a, o.gate_targets};
    if (g.targets && scale) hipLaunchKernelGGL(mlp_gate_kernel<WeightedGateEvalArgs>, sgrid, dim3(kThreads), 0, s, WeightedGateEvalArgs{g, scale});
    else if (g.targets) hipLaunchKernelGGL(mlp_gate_kernel<GateEvalArgs>, sgrid, dim3(kThreads), 0, s, g);
    else if (scale && d.teacher)
        hipLaunchKernelGGL(mlp_distill_softmax_kernel<WeightedDistillEvalArgs>, sgrid, dim3(kThreads), 0, s, WeightedDistillEvalArgs{d, scale});
    else if (scale) hipLaunchKernelGGL(mlp_softmax_kernel<WeightedEvalArgs>, sgrid, dim3(kThreads), 0, s, WeightedEvalArgs{a, scale});
    else if (d.teacher) hipLaunchKernelGGL(mlp_distill_softmax_kernel<DistillEvalArgs>, sgrid, dim3(kThreads), 0, s, d);
    else hipLaunchKernelGGL(mlp_softmax_kernel<EvalArgs>, sgrid, dim3(kThreads), 0, s, a);
    TnArgs g2{a.Z, (size_t)N * K, a.A, (size_t)N * H, a.theta, a.theta_stride, a.grad, a.grad_stride, oW2, ob2, a.ctrl, N, K, H, a.l2};
    hipLaunchKernelGGL((mlp_tn_gemm_kernel<double>), dim3(ceil_div(K, TM), ceil_div(H, TN), E), dim3(kThreads), 0, s, g2);
    const dim3 dgrid(ceil_div(N, kDactRows), E);
    switch (ceil_div(H, kThreads)) {
        case 1: hipLaunchKernelGGL((mlp_dact_kernel<1>), dgrid, dim3(kThreads), 0, s, a); break;
        case 2: hipLaunchKernelGGL((mlp_dact_kernel<2>), dgrid, dim3(kThreads), 0, s, a); break;
        case 3: hipLaunchKernelGGL((mlp_dact_kernel<3>), dgrid, dim3(kThreads), 0, s, a); break;
        default: hipLaunchKernelGGL((mlp_dact_kernel<4>), dgrid, dim3(kThreads), 0, s, a); break;
    }
    TnArgs g1{a.A, (size_t)N * H, a.X, (size_t)N * H, a.theta, a.theta_stride, a.grad, a.grad_stride, oW1, ob1, a.ctrl, N, H, H, a.l2};
    hipLaunchKernelGGL((mlp_tn_gemm_kernel<float>), dim3(ceil_div(H, TM), ceil_div(H, TN), E), dim3(kThreads), 0, s, g1);
    hipLaunchKernelGGL(mlp_loss_kernel, dim3(E), dim3(kFitCtrlThreads), 0, s, a);
}

// the weighted fit's row scales (E,N) lie behind the unweighted scratch
FitLayout mlp_layout(int E, int N, int H, int K, int M, bool weighted) {
    return FitLayout(E, (int)params(H, K), M, scratch_bytes(E, N, H, K) + (weighted ? sizeof(double) * (size_t)E * N : 0));
}

}  // namespace

size_t mlp_head_fit_scratch_doubles(int E, int N, int H, int K) { return (size_t)E * N * ((size_t)H + K + 1); }

size_t mlp_head_fit_workspace_bytes(int E, int N, int H, int K, int history, bool weighted) {
    return mlp_layout(E, N, H, K, history, weighted).bytes;
}

void launch_mlp_head_lossgrad(const float* X, const HeadObjective& o, const double* theta, int E, int N, int H, int K, double l2, double* scratch,
                              int* err, double* loss, double* grad, hipStream_t s) {
    if (o.weights) launch_row_scale(o.weights, E, N, scale_table(scratch, scratch_bytes(E, N, H, K)), err, s);
    launch_eval({theta, params(H, K), nullptr, err, loss, grad, params(H, K), scratch}, X, o, E, N, H, K, l2, s);
}

bool launch_mlp_head_fit(const MlpHeadFitArgs& f, hipStream_t s) {
    const int H = f.H, K = f.K, HH = H * H;
    const HeadObjective& o = f.objective;
    return run_lbfgs_fit(f, mlp_layout(f.E, f.N, H, K, f.history, o.weights != nullptr),
                         [&](const FitEvalPoint& p) { launch_eval(p, f.features, o, f.E, f.N, H, K, f.l2, s); },
                         {{0, HH, f.dense_weight, nullptr}, {HH, H, f.dense_bias, nullptr}, {HH + H, K * H, f.weight, nullptr},
                          {HH + H + K * H, K, f.bias, nullptr}}, s, o.weights, scratch_bytes(f.E, f.N, H, K));
}

}  // namespace mmee
