// ee_head_fit (include/mmee.h): one-layer ramp exit heads fitted on the device from a frozen backbone's CLS rows -- L2-regularised softmax
// regression per exit, float64 arithmetic on the float32 features, L-BFGS as a fixed launch list.
//
//   head_fit_lossgrad_kernel    the hot kernel.  Grid (class tile, row chunk, exit).  A workgroup walks the slabs (kHeadFitSlab rows) of its
//                               chunk in order; a slab's rows are staged in LDS once and serve the logits pass (Z = X W^T + b), the max-shifted
//                               softmax (D = P - Y in place of Z) and the gradient pass (D^T X), whose sums stay in registers across the
//                               chunk.  One partial (dW, db, loss) per (exit, chunk) goes to the workspace: no atomics.
//   head_fit_reduce_kernel      sums the chunk partials in chunk order, divides by N, adds the penalty: L and grad L of the trial point.
// ee_head_fit_distill runs the same two kernels: head_fit_lossgrad_kernel is a template over its argument struct, and what the struct selects
// (if constexpr) is the row step between the two passes -- the labelled softmax, or the mixed step against the final classifier's logits
// (distill_row, head_fit_common.h), which reads the teacher's row from global memory: no LDS and no workspace beyond the labelled fit's.
// ee_head_fit_weighted adds sample weights to either objective, again as argument structs of the same kernel: head_fit_row_scale_kernel makes
// scale[e][n] = w[e][n] N / W_e once per call, the weighted row steps multiply a row's N dL/dz and its loss by it and skip a row whose scale is
// zero, and everything behind the row step is shared, division by N included.  The unweighted instantiations are the code they were.
// ee_head_fit_gate (2-way gate heads, K = 2) is one more argument struct of the same kernel: its row step is the two binary cross-entropies of
// the gate objective against a target in [0, 1] per (exit, row) (gate_row_step), everything else -- slabs, logits pass, gradient pass, partials,
// reduce, driver, workspace -- is the labelled fit's at K = 2.
// Which of the five argument structs a call launches is read off its HeadObjective (mmee_kernels.h) in one place, launch_eval.
// This file is the objective; the L-BFGS around it is run_lbfgs_fit (fit_lbfgs.hip), which also makes the weighted fits' row-scale table in
// front of the first tick; the workspace layout, the control words and the table's place (scale_table) are in head_fit_common.h.
//
// Arithmetic form: plain float64 FMAs.  The matrix form (v_mfma_f64_16x16x4_f64) was NOT built, so not measured against it.  Measured for this
// form (profiles/head_fit.txt): 446 GB/s on the feature bytes at N = 40 000, H = 768, K = 16, E = 6 -- latency-bound, not bandwidth-bound; DESIGN.md
// section 7 says where the time goes and why the logits pass is the place to try the matrix form.
//
// Determinism: the chunking is a function of N alone, every sum has a fixed order, and nothing depends on E -- an exit fitted alone gets
// the bits it gets among others.
#include <type_traits>

#include "head_fit_common.h"

namespace mmee {

namespace {

constexpr int S = kHeadFitSlab;
constexpr int kThreads = 256;
constexpr int kLogitTile = 8;            // classes per logits-pass round

__host__ __device__ inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

struct LossGradArgs {
    const float* X;                  // (E,N,H)
    const long long* y;              // (N,)
    const double* theta;             // exit e: theta + e * theta_stride; W (K,H) then b (K,)
    size_t theta_stride;
    const int* ctrl;                 // per exit kCtrlInts words, or null: every exit runs
    int* err;                        // bit 0: a label outside [0,K)
    double* partial;                 // (E, chunks, K*H + K + 1)
    int N, H, K, chunks, slabs_per_chunk;
};
// ee_head_fit_distill: err bit 1 is a teacher logit that is not finite; y is null at alpha = 1
struct DistillLossGradArgs : LossGradArgs {
    const float* teacher;            // (N,K)
    double alpha, temperature;
};
// ee_head_fit_weighted: either objective with the row-scale table of launch_row_scale; err bits 2 and 3 are the table's
struct WeightedLossGradArgs : LossGradArgs {
    const double* scale;             // (E,N): w[e][n] N / W_e
};
struct WeightedDistillLossGradArgs : DistillLossGradArgs {
    const double* scale;
};
// ee_head_fit_gate: K == 2 and y null; err bit 0 is a target that is not finite or lies outside [0,1]
struct GateLossGradArgs : LossGradArgs {
    const double* targets;           // (E,N): c[e][n] = how right classifier(gate input) is at exit e on row n
};
template <typename Args>
constexpr bool kGate = std::is_same_v<Args, GateLossGradArgs>;
template <typename Args>
constexpr bool kDistilled = std::is_base_of_v<DistillLossGradArgs, Args>;
template <typename Args>
constexpr bool kWeighted = std::is_same_v<Args, WeightedLossGradArgs> || std::is_same_v<Args, WeightedDistillLossGradArgs>;

// The mixed row step (distill_row, head_fit_common.h) of the slab walk below: the row's logits and the teacher's row -- float32 from global memory,
// each element read once -- in registers, eight threads a row.  Z [S][Kp] holds the slab's logits and leaves as N dL/dz (zero beyond the slab's
// rows and beyond K); the row's loss goes to `loss` of the first of its eight threads.  Every thread reads its logits before any of the row
// writes: they are lanes of one wave.  The weighted form multiplies the row's N dL/dz and its loss by the row's scale sc (zero for a row
// that does not exist), last of all, and takes a row whose scale is zero for one that does not exist: neither its label nor its teacher row
// is read.
template <typename Args>
__device__ inline void distill_row_step(const Args& a, double* Z, double sc, int n0, int rows, int K, int Kp, double& loss) {
    const int t = threadIdx.x, row = t >> 3, sub = t & 7;
    bool valid = row < rows;
    const bool hard = a.alpha < 1.0;
    if constexpr (kWeighted<Args>) valid = sc != 0.0;        // true for a NaN scale too: the error word is raised then
    long long y = -1;
    if (hard) {
        y = valid ? a.y[n0 + row] : 0;
        if (y < 0 || y >= K) {
            atomicOr(a.err, 1);
            y = -1;
        }
    }
    float tv[kRowSlots];
    load_teacher_row(a.teacher + (size_t)(n0 + row) * K, valid, sub, K, tv, a.err);
    double v[kRowSlots];
#pragma unroll
    for (int i = 0; i < kRowSlots; ++i) v[i] = sub + 8 * i < K ? Z[row * Kp + sub + 8 * i] : 0.0;
    const double l = distill_row(v, tv, sub, K, y, hard, a.alpha, a.temperature);
    if (sub == 0 && valid) loss += scaled<kWeighted<Args>>(l, sc);
#pragma unroll
    for (int i = 0; i < kRowSlots; ++i) {
        const int k = sub + 8 * i;
        if (k < Kp) Z[row * Kp + k] = (valid && k < K) ? scaled<kWeighted<Args>>(v[i], sc) : 0.0;
    }
}

// The gate row step (include/mmee.h, ee_head_fit_gate): the row's loss (bce(z_1, c) + bce(z_0, 1 - c)) / 2 -- the reduce kernel divides by N,
// which makes the objective's 1 / (2N) -- and N dL/dz in place of the two logits, zeros in the padding columns.  Eight threads a row, as in the
// other row steps; each reads both logits before any of the row writes (lanes of one wave, LDS operations in program order).
__device__ inline void gate_row_step(const GateLossGradArgs& a, double* Z, int e, int n0, int rows, int Kp, double& loss) {
    const int t = threadIdx.x, row = t >> 3, sub = t & 7;
    const bool valid = row < rows;
    double c = valid ? a.targets[(size_t)e * a.N + n0 + row] : 0.0;
    if (!(c >= 0.0 && c <= 1.0)) {                           // a NaN fails both compares
        atomicOr(a.err, 1);
        c = 0.0;
    }
    const double z0 = Z[row * Kp], z1 = Z[row * Kp + 1];
    double d0, d1;
    const double l = 0.5 * (gate_bce(z1, c, d1) + gate_bce(z0, 1.0 - c, d0));
    if (sub == 0 && valid) loss += l;
    for (int k = sub; k < Kp; k += 8) Z[row * Kp + k] = (valid && k < 2) ? 0.5 * (k == 0 ? d0 : d1) : 0.0;
}

// KT classes x HC columns (h = t + 256 i) of the gradient per thread; Args: LossGradArgs (labels) or DistillLossGradArgs (soft targets), or
// the Weighted form of either (sample weights)
template <int KT, int HC, typename Args>
__global__ __launch_bounds__(kThreads) void head_fit_lossgrad_kernel(Args a) {
    const int kt = blockIdx.x, c = blockIdx.y, e = blockIdx.z, t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (a.ctrl && a.ctrl[e * kCtrlInts + CI_STOP] != 0) return;
    const int N = a.N, H = a.H, K = a.K, H4 = H >> 2, ld = H + 4, Kp = round_up(K, 16), P = K * H + K;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* Xs = reinterpret_cast<float*>(smem);                                   // [S][ld]
    double* Z = reinterpret_cast<double*>(smem + sizeof(float) * S * ld);         // [S][Kp]: logits, then P - Y
    double* R = Z + S * Kp;                                                        // [4][S][kLogitTile]: the waves' partial logits
    const float* X = a.X + (size_t)e * N * H;
    const double* W = a.theta + (size_t)e * a.theta_stride;
    const double* b = W + (size_t)K * H;
    const int k0 = kt * KT;

    double acc[KT][HC];
#pragma unroll
    for (int j = 0; j < KT; ++j)
#pragma unroll
        for (int i = 0; i < HC; ++i) acc[j][i] = 0.0;
    double gb = 0.0, loss = 0.0;

    const int slab0 = c * a.slabs_per_chunk, n_slabs = (N + S - 1) / S;
    const int slab1 = slab0 + a.slabs_per_chunk < n_slabs ? slab0 + a.slabs_per_chunk : n_slabs;

    // wave w stages rows w, w + 4, ...: S / 4 rows of HC float4 per lane; the weighted form fetches the scale of the row whose row step
    // this thread takes part in (row t >> 3 of the slab; zero beyond N) with them, a gradient pass ahead of its use
    f32x4 pre[S / 4][HC];
    double sc = 1.0;
    auto fetch = [&](int slab) {
        if constexpr (kWeighted<Args>) sc = row_scale(a.scale, e, N, (long long)slab * S + (t >> 3));
#pragma unroll
        for (int r = 0; r < S / 4; ++r) {
            const long long n = (long long)slab * S + w + 4 * r;
#pragma unroll
            for (int i = 0; i < HC; ++i) {
                const int h4 = lane + 64 * i;
                pre[r][i] = (n < N && h4 < H4) ? *reinterpret_cast<const f32x4*>(X + (size_t)n * H + 4 * h4) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    if (slab0 < slab1) fetch(slab0);

    for (int slab = slab0; slab < slab1; ++slab) {
        const int n0 = slab * S, rows = N - n0 < S ? N - n0 : S;
#pragma unroll
        for (int r = 0; r < S / 4; ++r)
#pragma unroll
            for (int i = 0; i < HC; ++i) {
                const int h4 = lane + 64 * i;
                if (h4 < H4) *reinterpret_cast<f32x4*>(Xs + (w + 4 * r) * ld + 4 * h4) = pre[r][i];
            }
        __syncthreads();

        // ---- logits: thread = (row pair rp, rp + 16; column slice sl of 16), kLogitTile classes a round ----
        {
            const int rp = t & 15, sl = t >> 4;
            for (int kc = 0; kc < Kp; kc += kLogitTile) {
                double a0[kLogitTile], a1[kLogitTile];
#pragma unroll
                for (int j = 0; j < kLogitTile; ++j) a0[j] = a1[j] = 0.0;
                if (kc < K) {
                    for (int h = sl; h < H; h += 16) {
                        const double x0 = (double)Xs[rp * ld + h], x1 = (double)Xs[(rp + 16) * ld + h];
#pragma unroll
                        for (int j = 0; j < kLogitTile; ++j) {
                            const double wv = kc + j < K ? W[(size_t)(kc + j) * H + h] : 0.0;
                            a0[j] = fma(wv, x0, a0[j]);
                            a1[j] = fma(wv, x1, a1[j]);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < kLogitTile; ++j) {                  // the wave's four slices: lanes l, l ^ 16, l ^ 32, l ^ 48
                    a0[j] += __shfl_xor(a0[j], 16);
                    a0[j] += __shfl_xor(a0[j], 32);
                    a1[j] += __shfl_xor(a1[j], 16);
                    a1[j] += __shfl_xor(a1[j], 32);
                }
                if (lane < 16) {
#pragma unroll
                    for (int j = 0; j < kLogitTile; ++j) {
                        R[(w * S + rp) * kLogitTile + j] = a0[j];
                        R[(w * S + rp + 16) * kLogitTile + j] = a1[j];
                    }
                }
                __syncthreads();
                {
                    const int row = t >> 3, j = t & 7, k = kc + j;
                    const double z = ((R[(0 * S + row) * kLogitTile + j] + R[(1 * S + row) * kLogitTile + j]) +
                                      (R[(2 * S + row) * kLogitTile + j] + R[(3 * S + row) * kLogitTile + j])) + (k < K ? b[k] : 0.0);
                    Z[row * Kp + k] = z;
                }
                __syncthreads();
            }
        }

        // ---- the row step, the compile-time difference between the two objectives: the row's loss, N dL/dz in place of Z ----
        if constexpr (kDistilled<Args>) distill_row_step(a, Z, sc, n0, rows, K, Kp, loss);
        else if constexpr (kGate<Args>) gate_row_step(a, Z, e, n0, rows, Kp, loss);
        else {
            // max-shifted softmax, loss, D = P - Y: eight threads a row.  The weighted form multiplies D and the loss by the row's scale, last
            // of all; a row whose scale is zero counts as one that does not exist, and its label is not read.
            const int row = t >> 3, sub = t & 7;
            bool valid = row < rows;
            if constexpr (kWeighted<Args>) valid = sc != 0.0;
            long long y = valid ? a.y[n0 + row] : 0;
            if (y < 0 || y >= K) {
                atomicOr(a.err, 1);
                y = -1;
            }
            double m = -INFINITY;
            for (int k = sub; k < K; k += 8) m = fmax(m, Z[row * Kp + k]);
            m = fmax(m, __shfl_xor(m, 1));
            m = fmax(m, __shfl_xor(m, 2));
            m = fmax(m, __shfl_xor(m, 4));
            double sum = 0.0;
            for (int k = sub; k < K; k += 8) sum += exp(Z[row * Kp + k] - m);
            sum += __shfl_xor(sum, 1);
            sum += __shfl_xor(sum, 2);
            sum += __shfl_xor(sum, 4);
            // read before the loop below turns Z into D: the eight threads of a row are lanes of one wave and LDS operations issue in program
            // order, so no sibling has overwritten Z[row][y] yet.  A mapping that spreads a row over waves needs a barrier here.
            const double zy = y >= 0 ? Z[row * Kp + (int)y] : 0.0;
            if (sub == 0 && valid && y >= 0) loss += scaled<kWeighted<Args>>((m + log(sum)) - zy, sc);
            const double inv = 1.0 / sum;
            for (int k = sub; k < Kp; k += 8) {
                const double d = (valid && k < K) ? scaled<kWeighted<Args>>(exp(Z[row * Kp + k] - m) * inv - (k == (int)y ? 1.0 : 0.0), sc) : 0.0;
                Z[row * Kp + k] = d;
            }
        }
        __syncthreads();

        if (slab + 1 < slab1) fetch(slab + 1);               // in flight behind the gradient pass, which reads LDS only

        // ---- gradient: dW[k0 .. k0 + KT) x columns t + 256 i, db ----
#pragma unroll 4                                             // fully unrolled, the <4, 2> and <4, 3> instances spill to scratch
        for (int n = 0; n < S; ++n) {
            double xv[HC];
#pragma unroll
            for (int i = 0; i < HC; ++i) {
                const int h = t + kThreads * i;
                xv[i] = h < H ? (double)Xs[n * ld + h] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < KT; ++j) {
                const double dv = Z[n * Kp + k0 + j];
#pragma unroll
                for (int i = 0; i < HC; ++i) acc[j][i] = fma(dv, xv[i], acc[j][i]);
            }
        }
        if (t < KT)
            for (int n = 0; n < S; ++n) gb += Z[n * Kp + k0 + t];
        __syncthreads();
    }

    double* part = a.partial + ((size_t)e * a.chunks + c) * (size_t)(P + 1);
#pragma unroll
    for (int j = 0; j < KT; ++j)
#pragma unroll
        for (int i = 0; i < HC; ++i) {
            const int k = k0 + j, h = t + kThreads * i;
            if (k < K && h < H) part[(size_t)k * H + h] = acc[j][i];
        }
    if (t < KT && k0 + t < K) part[(size_t)K * H + k0 + t] = gb;
    if (kt == 0) {                                           // every class tile computes the same loss: tile 0 writes it
        if ((t & 7) == 0) R[t >> 3] = loss;
        __syncthreads();
        if (t == 0) {
            double sum = 0.0;
            for (int r = 0; r < S; ++r) sum += R[r];
            part[P] = sum;
        }
    }
}

struct ReduceArgs {
    const double* partial;
    const double* theta;
    size_t theta_stride;
    const int* ctrl;
    double* loss;                    // exit e: loss[e * loss_stride]
    size_t loss_stride;
    double* grad;                    // exit e: grad + e * grad_stride
    size_t grad_stride;
    int N, P, chunks;
    double l2;
};

// grid (ceil(P / 256) + 1, E): the last workgroup of an exit makes the loss, the others 256 gradient entries each
__global__ __launch_bounds__(kThreads) void head_fit_reduce_kernel(ReduceArgs a) {
    const int e = blockIdx.y, t = threadIdx.x, P = a.P;
    if (a.ctrl && a.ctrl[e * kCtrlInts + CI_STOP] != 0) return;
    const double* part = a.partial + (size_t)e * a.chunks * (size_t)(P + 1);
    const double* th = a.theta + (size_t)e * a.theta_stride;
    if (blockIdx.x + 1 < gridDim.x) {
        const int i = blockIdx.x * kThreads + t;
        if (i >= P) return;
        double sum = 0.0;
        for (int c = 0; c < a.chunks; ++c) sum += part[(size_t)c * (P + 1) + i];
        a.grad[(size_t)e * a.grad_stride + i] = sum / (double)a.N + a.l2 * th[i];
        return;
    }
    __shared__ double red[kThreads];
    double sq = 0.0;
    for (int i = t; i < P; i += kThreads) sq = fma(th[i], th[i], sq);
    sq = block_sum<kThreads>(sq, red);
    if (t == 0) {
        double sum = 0.0;
        for (int c = 0; c < a.chunks; ++c) sum += part[(size_t)c * (P + 1) + P];
        a.loss[(size_t)e * a.loss_stride] = sum / (double)a.N + 0.5 * a.l2 * sq;
    }
}

// ---- the weighted fits' row scales: scale[e][n] = w[e][n] N / W_e, W_e = sum_n w[e][n] in float64 -- strided partial sums, then the fixed tree
// of block_sum, as mlp_loss_kernel sums the rows' losses.  Bit 2 of the error word: a weight that is negative or not finite; bit 3: W_e == 0.
// grid (E): one workgroup an exit, once per call
__global__ __launch_bounds__(kFitCtrlThreads) void head_fit_row_scale_kernel(const float* weights, int N, double* scale, int* err) {
    const int e = blockIdx.x, t = threadIdx.x;
    __shared__ double red[kFitCtrlThreads];
    const float* w = weights + (size_t)e * N;
    double sum = 0.0;
    bool bad = false;
    for (int i = t; i < N; i += kFitCtrlThreads) {
        const float v = w[i];
        bad |= !(v >= 0.f) || !__builtin_isfinite(v);
        sum += (double)v;
    }
    if (bad) atomicOr(err, 4);
    sum = block_sum<kFitCtrlThreads>(sum, red);
    if (t == 0 && sum == 0.0) atomicOr(err, 8);
    const double unit = (double)N / sum;
    double* out = scale + (size_t)e * N;
    for (int i = t; i < N; i += kFitCtrlThreads) out[i] = (double)w[i] * unit;
}

// the one-layer fit's workspace: behind the shared part, one partial (dW, db, loss) per (exit, chunk), then the weighted fit's row scales
FitLayout one_layer_layout(int E, int N, int H, int K, int M, bool weighted) {
    return FitLayout(E, K * H + K, M, head_fit_partial_bytes(E, N, H, K) + (weighted ? sizeof(double) * (size_t)E * N : 0));
}

size_t lossgrad_lds_bytes(int H, int K) {
    return sizeof(float) * S * (size_t)(H + 4) + sizeof(double) * S * (size_t)round_up(K, 16) + sizeof(double) * 4 * S * kLogitTile;
}

template <int KT, int HC, typename Args>
void launch_lossgrad_as(const Args& a, int E, hipStream_t s) {
    const size_t lds = lossgrad_lds_bytes(a.H, a.K);
    (void)ensure_dynamic_lds<&head_fit_lossgrad_kernel<KT, HC, Args>>("head_fit_lossgrad_kernel", 160 * 1024);
    hipLaunchKernelGGL((head_fit_lossgrad_kernel<KT, HC, Args>), dim3((a.K + KT - 1) / KT, a.chunks, E), dim3(kThreads), lds, s, a);
}

template <int KT, typename Args>
void launch_lossgrad_k(const Args& a, int E, hipStream_t s) {
    switch ((a.H + kThreads - 1) / kThreads) {
        case 1: launch_lossgrad_as<KT, 1>(a, E, s); break;
        case 2: launch_lossgrad_as<KT, 2>(a, E, s); break;
        case 3: launch_lossgrad_as<KT, 3>(a, E, s); break;
        default: launch_lossgrad_as<KT, 4>(a, E, s); break;
    }
}

template <typename Args>
void launch_lossgrad(const Args& a, int E, hipStream_t s) {
    if (a.K <= 4) launch_lossgrad_k<4>(a, E, s);
    else launch_lossgrad_k<16>(a, E, s);
}

// one evaluation: the partials of every running exit, then their fixed-order sums.  What o holds picks the kernel's argument struct: gate
// targets (K == 2) the gate objective, a teacher the distilled one, weights the weighted form of either, whose row scales lie behind the
// partials in p.tail
void launch_eval(const FitEvalPoint& p, const float* X, const HeadObjective& o, int E, int N, int H, int K, double l2, hipStream_t s) {
    LossGradArgs a{};
    a.X = X; a.y = o.labels; a.theta = p.theta; a.theta_stride = p.theta_stride; a.ctrl = p.ctrl; a.err = p.err;
    a.partial = static_cast<double*>(p.tail); a.N = N; a.H = H; a.K = K;
    const int n_slabs = (a.N + S - 1) / S;
    a.chunks = head_fit_chunks(a.N);
    a.slabs_per_chunk = (n_slabs + a.chunks - 1) / a.chunks;
    const DistillLossGradArgs d{a, o.soft.teacher, o.soft.alpha, o.soft.temperature};
    const double* scale = o.weights ? scale_table(p.tail, head_fit_partial_bytes(E, N, H, K)) : nullptr;
    if (o.gate_targets) launch_lossgrad(GateLossGradArgs{a, o.gate_targets}, E, s);
    else if (scale && d.teacher) launch_lossgrad(WeightedDistillLossGradArgs{d, scale}, E, s);
    else if (scale) launch_lossgrad(WeightedLossGradArgs{a, scale}, E, s);
    else if (d.teacher) launch_lossgrad(d, E, s);
    else launch_lossgrad(a, E, s);
    ReduceArgs r{};
    r.partial = a.partial; r.theta = a.theta; r.theta_stride = a.theta_stride; r.ctrl = a.ctrl; r.loss = p.loss; r.loss_stride = 1;
    r.grad = p.grad; r.grad_stride = p.grad_stride; r.N = a.N; r.P = a.K * a.H + a.K; r.chunks = a.chunks; r.l2 = l2;
    hipLaunchKernelGGL(head_fit_reduce_kernel, dim3((r.P + kThreads - 1) / kThreads + 1, E), dim3(kThreads), 0, s, r);
}

}  // namespace

// A function of N alone, so that an exit's sums do not depend on what else is in the launch: at most kHeadFitMaxChunks chunks of whole slabs,
// none of them empty.
int head_fit_chunks(int N) {
    const int n_slabs = (N + S - 1) / S;
    const int per = (n_slabs + kHeadFitMaxChunks - 1) / kHeadFitMaxChunks;
    return (n_slabs + per - 1) / per;
}

size_t head_fit_workspace_bytes(int E, int N, int H, int K, int history, bool weighted) {
    return one_layer_layout(E, N, H, K, history, weighted).bytes;
}

size_t head_fit_partial_bytes(int E, int N, int H, int K) { return sizeof(double) * (size_t)E * head_fit_chunks(N) * (size_t)(K * H + K + 1); }

void launch_row_scale(const float* weights, int E, int N, double* scale, int* err, hipStream_t s) {
    hipLaunchKernelGGL(head_fit_row_scale_kernel, dim3(E), dim3(kFitCtrlThreads), 0, s, weights, N, scale, err);
}

void launch_head_lossgrad(const float* X, const HeadObjective& o, const double* theta, int E, int N, int H, int K, double l2, double* partial,
                          int* err, double* loss, double* grad, hipStream_t s) {
    const size_t P = (size_t)K * H + K;
    if (o.weights) launch_row_scale(o.weights, E, N, scale_table(partial, head_fit_partial_bytes(E, N, H, K)), err, s);
    launch_eval({theta, P, nullptr, err, loss, grad, P, partial}, X, o, E, N, H, K, l2, s);
}

bool launch_head_fit(const HeadFitArgs& f, hipStream_t s) {
    const int KH = f.K * f.H;
    const HeadObjective& o = f.objective;
    return run_lbfgs_fit(f, one_layer_layout(f.E, f.N, f.H, f.K, f.history, o.weights != nullptr),
                         [&](const FitEvalPoint& p) { launch_eval(p, f.features, o, f.E, f.N, f.H, f.K, f.l2, s); },
                         {{0, KH, f.weight, f.weight64}, {KH, f.K, f.bias, f.bias64}}, s, o.weights, head_fit_partial_bytes(f.E, f.N, f.H, f.K));
}

}  // namespace mmee
