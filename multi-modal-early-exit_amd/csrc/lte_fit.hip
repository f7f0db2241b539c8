// ee_lte_fit (include/mmee.h): the learning-to-exit classifier -- ONE Linear(H, 1) shared by every encoder exit -- fitted on the device from the
// CLS rows a dump-all forward leaves (hidden_cls) and the targets "this exit is wrong here" made from its policy logits.  float64 arithmetic on
// the float32 rows, the L-BFGS of ee_head_fit (run_lbfgs_fit, fit_lbfgs.hip: the same controller and finish kernels, one "exit" of H + 1 parameters).
//
//   lte_fit_lossgrad_kernel  the hot kernel: one pass over the features.  Grid (row chunk, exit), four waves a workgroup, one wave a row.  A wave
//                            loads kRowsPerWave rows at once (lane l holds columns 4l + 256k + j, the order of head_out_lte_kernel), makes their
//                            dot products, the scores, dl/da, and adds dl/da * x to its float64 accumulators from the SAME registers: a row is
//                            read from HBM once per evaluation.  The accumulators live across the units (kLteFitRows rows) of the chunk; at its
//                            end the four waves are added in LDS in wave order and ONE partial (dw, db, loss) per (exit, chunk) is written.
//   lte_fit_reduce_kernel    per parameter: the partials of an exit in chunk order, the exits in ascending order, / N, the penalty.
//   lte_targets_kernel       t = 1 - [argmax(policy logits) == label], first maximum; lte_check_targets_kernel refuses first.
//   lte_scores_kernel        sigmoid(w . x + b) from a float32 (w, b): the expression and order of head_out_lte_kernel.
//
// No floating-point atomics.  The chunking is a function of N alone and every sum has a fixed order: two calls return the same bits.
#include "head_fit_common.h"

namespace mmee {

namespace {

constexpr int R = kLteFitRows;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRowsPerWave = R / kWaves;     // rows a wave has in flight
static_assert(R % kWaves == 0 && (kRowsPerWave & (kRowsPerWave - 1)) == 0, "a unit is a power of two of rows per wave");

struct LossGradArgs {
    const float* X;                  // (E,N,H)
    const double* T;                 // (E,N) targets in [0,1]
    const double* theta;             // w (H,), b
    const int* ctrl;                 // the fit's control words (one "exit"), or null
    int* err;                        // bit 0: a target outside [0,1] or NaN
    double* partial;                 // (E, chunks, H + 2): dw, db, loss
    int N, H, chunks, units_per_chunk;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// lane l's value in every lane (l a constant): two v_readlane, the result is wave-uniform
__device__ __forceinline__ double read_lane(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// NV: float4 column groups per lane (H <= 256 NV); LOSS: kLteLossMse / kLteLossBce
template <int NV, int LOSS>
__global__ __launch_bounds__(kThreads, NV <= 2 ? 4 : 3) void lte_fit_lossgrad_kernel(LossGradArgs a) {
    const int c = blockIdx.x, e = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (a.ctrl && a.ctrl[CI_STOP] != 0) return;
    const int N = a.N, H = a.H, Q = H + 2;
    extern __shared__ __attribute__((aligned(16))) double red[];                  // [kWaves][Q], then the weights
    const float* X = a.X + (size_t)e * N * H;
    const double* T = a.T + (size_t)e * N;

    // The weights live in LDS as float64, not in registers (which the rows in flight and the accumulators need): image [k][j / 2][lane][j % 2],
    // so a lane's 16 bytes lie next to its neighbour's.  A column group past H reads group 0 again with weights of zero: no branch around a
    // load, and its accumulators are never written out.
    double* wl = red + (size_t)kWaves * Q;                                        // [NV][2][64][2]
    int col[NV];
    double acc[NV][4];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int c0 = 4 * lane + 256 * k;
        const bool live = c0 < H;
        col[k] = live ? c0 : 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double v = a.theta[col[k] + j];
            if (w == 0) wl[((2 * k + (j >> 1)) * 64 + lane) * 2 + (j & 1)] = live ? v : 0.0;
            acc[k][j] = 0.0;
        }
    }
    __syncthreads();
    const double b = a.theta[H];
    double gb = 0.0, loss = 0.0;
    bool bad = false;
    const int rr = lane & (kRowsPerWave - 1);

    const int n_units = (N + R - 1) / R, u0 = c * a.units_per_chunk;
    const int u1 = u0 + a.units_per_chunk < n_units ? u0 + a.units_per_chunk : n_units;
    for (int u = u0; u < u1; ++u) {
        asm volatile("" ::: "memory");                         // the weights are read from LDS every unit, not hoisted into registers
        const long long n0 = (long long)u * R + kRowsPerWave * w;
        f32x4 xv[kRowsPerWave][NV];
        // a row past N reads row N - 1 again and contributes dl/da = 0
#pragma unroll
        for (int r = 0; r < kRowsPerWave; ++r) {
            const long long n = n0 + r < N ? n0 + r : N - 1;
            const float* x = X + (size_t)n * H;
#pragma unroll
            for (int k = 0; k < NV; ++k) xv[r][k] = *reinterpret_cast<const f32x4*>(x + col[k]);
        }
        const bool ok = n0 + rr < N;                         // lane l does the scalar work of row l % kRowsPerWave
        const double tg = T[ok ? n0 + rr : N - 1];
        double wd[NV][4];
#pragma unroll
        for (int k = 0; k < NV; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) wd[k][j] = wl[((2 * k + (j >> 1)) * 64 + lane) * 2 + (j & 1)];
        double dot[kRowsPerWave];
#pragma unroll
        for (int r = 0; r < kRowsPerWave; ++r) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < NV; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) s += (double)xv[r][k][j] * wd[k][j];
            dot[r] = s;
        }
#pragma unroll
        for (int r = 0; r < kRowsPerWave; ++r) dot[r] = wave_sum_f64(dot[r]);
        // The rows stay float32 in their registers until the gradient widens them again: without this the compiler keeps the float64 copies of
        // the dot products alive (twice the registers of the rows themselves) and spills.
#pragma unroll
        for (int r = 0; r < kRowsPerWave; ++r)
#pragma unroll
            for (int k = 0; k < NV; ++k) asm volatile("" : "+v"(xv[r][k]));
        double z = dot[0];
#pragma unroll
        for (int r = 1; r < kRowsPerWave; ++r) z = rr == r ? dot[r] : z;
        z += b;
        if (ok && !(tg >= 0.0 && tg <= 1.0)) bad = true;
        const double s = 1.0 / (1.0 + exp(-z));
        double d, l;
        if (LOSS == kLteLossMse) {
            const double q = s - tg;
            l = q * q;
            d = 2.0 * q * s * (1.0 - s);
        } else {
            l = fmax(z, 0.0) + log1p(exp(-fabs(z))) - tg * z;
            d = s - tg;
        }
        d = ok ? d : 0.0;
        l = ok ? l : 0.0;
#pragma unroll
        for (int r = 0; r < kRowsPerWave; ++r) {             // rows in ascending order; lane r holds row r's dl/da and loss
            const double dr = read_lane(d, r);
            loss += read_lane(l, r);
            gb += dr;
#pragma unroll
            for (int k = 0; k < NV; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[k][j] = fma(dr, (double)xv[r][k][j], acc[k][j]);
        }
    }
    if (bad) atomicOr(a.err, 1);

    // the four waves in wave order, one partial a workgroup
    double* mine = red + (size_t)w * Q;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int c0 = 4 * lane + 256 * k;
        if (c0 < H) {
#pragma unroll
            for (int j = 0; j < 4; ++j) mine[c0 + j] = acc[k][j];
        }
    }
    if (lane == 0) {
        mine[H] = gb;
        mine[H + 1] = loss;
    }
    __syncthreads();
    double* part = a.partial + ((size_t)e * a.chunks + c) * (size_t)Q;
    for (int i = t; i < Q; i += kThreads) part[i] = ((red[i] + red[Q + i]) + red[2 * Q + i]) + red[3 * Q + i];
}
static_assert(kWaves == 4, "the workgroup sum above names four waves");

struct ReduceArgs {
    const double* partial;
    const double* theta;
    const int* ctrl;
    double* loss;                    // one double
    double* grad;                    // H + 1 doubles
    int E, N, H, chunks;
    double l2;
};

// grid ceil((H + 2) / 64), 64 G threads: lane = one of 64 entries of (dw, db, loss); wave g sums the chunk partials of the exits g, g + G, ...
// in chunk order; wave 0 then adds the exits in ascending order, divides by N and adds the penalty.
__global__ __launch_bounds__(1024) void lte_fit_reduce_kernel(ReduceArgs a) {
    if (a.ctrl && a.ctrl[CI_STOP] != 0) return;
    __shared__ double S[kLteFitMaxExits][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, G = blockDim.x >> 6;
    const int P = a.H + 1, Q = a.H + 2, i = blockIdx.x * 64 + lane;
    for (int e = g; e < a.E; e += G) {
        double sum = 0.0;
        if (i < Q) {
            const double* p = a.partial + (size_t)e * a.chunks * (size_t)Q + i;
#pragma unroll 8
            for (int c = 0; c < a.chunks; ++c) sum += p[(size_t)c * Q];
        }
        S[e][lane] = sum;
    }
    __syncthreads();
    if (g != 0) return;
    double sum = 0.0;
    for (int e = 0; e < a.E; ++e) sum += S[e][lane];
    if (i < P) a.grad[i] = sum / (double)a.N + a.l2 * a.theta[i];
    if (blockIdx.x == P / 64) {                                                 // the workgroup that holds the loss entry
        double sq = 0.0;
        for (int j = lane; j < P; j += 64) sq = fma(a.theta[j], a.theta[j], sq);
        sq = wave_sum_f64(sq);
        if (i == P) *a.loss = sum / (double)a.N + 0.5 * a.l2 * sq;
    }
}

template <int NV>
void launch_lossgrad_nv(const LossGradArgs& a, int E, int loss, hipStream_t s) {
    const size_t lds = sizeof(double) * (kWaves * (size_t)(a.H + 2) + 256 * NV);   // <= 41 024 bytes: no opt-in
    if (loss == kLteLossMse)
        hipLaunchKernelGGL((lte_fit_lossgrad_kernel<NV, kLteLossMse>), dim3(a.chunks, E), dim3(kThreads), lds, s, a);
    else
        hipLaunchKernelGGL((lte_fit_lossgrad_kernel<NV, kLteLossBce>), dim3(a.chunks, E), dim3(kThreads), lds, s, a);
}

// one evaluation: the partials, then their fixed-order sums
void launch_eval(const FitEvalPoint& p, const float* X, const double* T, int E, int N, int H, int loss, double l2, hipStream_t s) {
    LossGradArgs a{};
    a.X = X; a.T = T; a.theta = p.theta; a.ctrl = p.ctrl; a.err = p.err; a.partial = static_cast<double*>(p.tail); a.N = N; a.H = H;
    const int n_units = (a.N + R - 1) / R;
    a.chunks = lte_fit_chunks(a.N);
    a.units_per_chunk = (n_units + a.chunks - 1) / a.chunks;
    switch ((a.H + 255) / 256) {
        case 1: launch_lossgrad_nv<1>(a, E, loss, s); break;
        case 2: launch_lossgrad_nv<2>(a, E, loss, s); break;
        case 3: launch_lossgrad_nv<3>(a, E, loss, s); break;
        default: launch_lossgrad_nv<4>(a, E, loss, s); break;
    }
    ReduceArgs r{a.partial, a.theta, a.ctrl, p.loss, p.grad, E, a.N, a.H, a.chunks, l2};
    const int G = E < 16 ? E : 16;
    hipLaunchKernelGGL(lte_fit_reduce_kernel, dim3((a.H + 2 + 63) / 64), dim3(64 * G), 0, s, r);
}

FitLayout lte_layout(int E, int N, int H, int M) { return FitLayout(1, H + 1, M, sizeof(double) * lte_fit_partial_doubles(E, N, H)); }

// ---- targets ------------------------------------------------------------------------------------------------------------------------------
// a label outside [0,K) or a NaN logit (a row the document never reached) raises bit 0
__global__ __launch_bounds__(kThreads) void lte_check_targets_kernel(const float* logits, const long long* y, long long EN, int N, int K, int* err) {
    bool bad = false;
    for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < EN; i += (long long)gridDim.x * kThreads) {
        const long long lab = y[i % N];
        if (lab < 0 || lab >= K) bad = true;
        const float* z = logits + (size_t)i * K;
        for (int k = 0; k < K; ++k)
            if (z[k] != z[k]) bad = true;
    }
    if (bad) atomicOr(err, 1);
}

__global__ __launch_bounds__(kThreads) void lte_targets_kernel(const float* logits, const long long* y, long long EN, int N, int K, const int* err,
                                                               double* targets) {
    if (*err != 0) return;                                                       // refused: nothing is written
    for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < EN; i += (long long)gridDim.x * kThreads) {
        const float* z = logits + (size_t)i * K;
        int best = 0;
        float m = z[0];
        for (int k = 1; k < K; ++k)
            if (z[k] > m) {                                                      // strict: the first maximum wins
                m = z[k];
                best = k;
            }
        targets[i] = best == (int)y[i % N] ? 0.0 : 1.0;
    }
}

// ---- scores: the expression and summation order of head_out_lte_kernel (exit_stage.hip) --------------------------------------------------------
__global__ __launch_bounds__(kThreads) void lte_scores_kernel(const float* X, const float* wgt, const float* bias, long long rows, int H, double* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long i = blockIdx.x * (long long)kWaves + wave; i < rows; i += (long long)gridDim.x * kWaves) {
        const float* x = X + (size_t)i * H;
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < kMaxNV; ++k) {
            const int c = 4 * lane + 256 * k;
            if (c < H) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(x + c);
                const f32x4 wv = *reinterpret_cast<const f32x4*>(wgt + c);
#pragma unroll
                for (int j = 0; j < 4; ++j) t += (double)v[j] * (double)wv[j];
            }
        }
        t = wave_sum_f64(t);
        if (lane == 0) out[i] = 1.0 / (1.0 + exp(-(t + (double)bias[0])));
    }
}

}  // namespace

// A function of N alone: at most kLteFitMaxChunks chunks of whole units, none of them empty.
int lte_fit_chunks(int N) {
    const int n_units = (N + R - 1) / R;
    const int per = (n_units + kLteFitMaxChunks - 1) / kLteFitMaxChunks;
    return (n_units + per - 1) / per;
}

size_t lte_fit_partial_doubles(int E, int N, int H) { return (size_t)E * lte_fit_chunks(N) * (size_t)(H + 2); }

size_t lte_fit_workspace_bytes(int E, int N, int H, int history) { return lte_layout(E, N, H, history).bytes; }

void launch_lte_lossgrad(const float* X, const double* T, const double* theta, int E, int N, int H, int loss, double l2, double* partial, int* err,
                         double* loss_out, double* grad, hipStream_t s) {
    launch_eval({theta, 0, nullptr, err, loss_out, grad, 0, partial}, X, T, E, N, H, loss, l2, s);
}

bool launch_lte_fit(const LteFitArgs& f, hipStream_t s) {
    return run_lbfgs_fit(f, lte_layout(f.E, f.N, f.H, f.history),
                         [&](const FitEvalPoint& p) { launch_eval(p, f.features, f.targets, f.E, f.N, f.H, f.loss_kind, f.l2, s); },
                         {{0, f.H, f.weight, nullptr}, {f.H, 1, f.bias, nullptr}}, s, nullptr, 0);
}

void launch_lte_targets(const float* logits, const long long* y, int E, int N, int K, double* targets, int* err, hipStream_t s) {
    const long long EN = (long long)E * N;
    const int grid = grid_1d(EN, kThreads, 4096);
    hipLaunchKernelGGL(lte_check_targets_kernel, dim3(grid), dim3(kThreads), 0, s, logits, y, EN, N, K, err);
    hipLaunchKernelGGL(lte_targets_kernel, dim3(grid), dim3(kThreads), 0, s, logits, y, EN, N, K, err, targets);
}

void launch_lte_scores(const float* X, const float* wgt, const float* bias, int E, int N, int H, double* scores, hipStream_t s) {
    const long long rows = (long long)E * N;
    hipLaunchKernelGGL(lte_scores_kernel, dim3(grid_1d(rows, kWaves, 8192)), dim3(kThreads), 0, s, X, wgt, bias, rows, H, scores);
}

}  // namespace mmee
