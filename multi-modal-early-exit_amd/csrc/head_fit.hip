// ee_head_fit (include/mmee.h): one-layer ramp exit heads fitted on the device from a frozen backbone's CLS rows -- L2-regularised softmax
// regression per exit, float64 arithmetic on the float32 features, L-BFGS as a fixed launch list.
//
//   head_fit_lossgrad_kernel    the hot kernel.  Grid (class tile, row chunk, exit).  A workgroup walks the slabs (kHeadFitSlab rows) of its
//                               chunk in order; a slab's rows are staged in LDS once and serve the logits pass (Z = X W^T + b), the max-shifted
//                               softmax (D = P - Y in place of Z) and the gradient pass (D^T X), whose sums stay in registers across the
//                               chunk.  One partial (dW, db, loss) per (exit, chunk) goes to the workspace: no atomics.
//   head_fit_reduce_kernel      sums the chunk partials in chunk order, divides by N, adds the penalty: L and grad L of the trial point.
//   head_fit_controller_kernel  one workgroup per exit: Armijo test, history update, two-loop recursion, next trial point.
//   head_fit_finish_kernel      copies the result out -- unless the error word is set, in which case no output is touched.
// The controller and the finish kernel are written over a parameter count P and serve the two-layer fit (mlp_head_fit.hip) too, through the
// launchers of head_fit_common.h, which also holds the workspace layout and the control words the two fits share.
//
// Arithmetic form: plain float64 FMAs.  The matrix form (v_mfma_f64_16x16x4_f64) was NOT built, so not measured against it.  Measured for this
// form (profiles/head_fit.txt): 446 GB/s on the feature bytes at N = 40 000, H = 768, K = 16, E = 6 -- latency-bound, not bandwidth-bound; DESIGN.md
// section 7 says where the time goes and why the logits pass is the place to try the matrix form.
//
// Determinism: the chunking is a function of N alone, every sum has a fixed order, an element of a parameter-sized vector is always touched
// by the same thread of the controller, and nothing depends on E -- an exit fitted alone gets the bits it gets among others.
#include "head_fit_common.h"

namespace mmee {

namespace {

constexpr int S = kHeadFitSlab;
constexpr int kThreads = 256;
constexpr int kLogitTile = 8;            // classes per logits-pass round
constexpr int kCtrlThreads = kFitCtrlThreads;
constexpr double kArmijo = 1e-4;
// The Armijo test allows for the rounding of L: below a gradient norm of a few 1e-9 the decrease a good step brings is smaller than the
// resolution of L in float64, and without the allowance no trial point passes any more (measured on the host restatement: 3 of 36 problems
// stall at 1.2e-9 ... 2.4e-9 for 200 evaluations; with 1, 4 or 16 epsilon |L| none does).
constexpr double kArmijoSlack = 8.0 * 2.220446049250313e-16;
constexpr int kMaxHalvings = 30;

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

// KT classes x HC columns (h = t + 256 i) of the gradient per thread
template <int KT, int HC>
__global__ __launch_bounds__(kThreads) void head_fit_lossgrad_kernel(LossGradArgs a) {
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

    // wave w stages rows w, w + 4, ...: S / 4 rows of HC float4 per lane
    f32x4 pre[S / 4][HC];
    auto fetch = [&](int slab) {
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

        // ---- max-shifted softmax, loss, D = P - Y: eight threads a row ----
        {
            const int row = t >> 3, sub = t & 7;
            const bool valid = row < rows;
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
            if (sub == 0 && valid && y >= 0) loss += (m + log(sum)) - zy;
            const double inv = 1.0 / sum;
            for (int k = sub; k < Kp; k += 8) {
                const double d = (valid && k < K) ? exp(Z[row * Kp + k] - m) * inv - (k == (int)y ? 1.0 : 0.0) : 0.0;
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

// the one-layer fit's workspace: behind the shared part, one partial (dW, db, loss) per (exit, chunk)
FitLayout one_layer_layout(int E, int N, int H, int K, int M) {
    return FitLayout(E, K * H + K, M, head_fit_partial_bytes(E, N, H, K));
}

struct CtrlArgs {
    char* ws;
    FitLayout lay;
    double gtol;
    int max_evals;
};

__global__ __launch_bounds__(kCtrlThreads) void head_fit_controller_kernel(CtrlArgs a) {
    const int e = blockIdx.x, t = threadIdx.x, P = a.lay.P, M = a.lay.M;
    __shared__ double red[kCtrlThreads];
    __shared__ double alpha[kHeadFitMaxHistory];
    int* ci = reinterpret_cast<int*>(a.ws + a.lay.o_ctrl) + e * kCtrlInts;
    double* cd = reinterpret_cast<double*>(a.ws + a.lay.o_scal) + e * kCtrlDoubles;
    double* rho = reinterpret_cast<double*>(a.ws + a.lay.o_rho) + (size_t)e * M;
    double* vec = reinterpret_cast<double*>(a.ws + a.lay.o_vec) + (size_t)e * a.lay.vec_stride;
    double *th = vec + (size_t)V_THETA * P, *tr = vec + (size_t)V_TRIAL * P, *g = vec + (size_t)V_G * P, *gt = vec + (size_t)V_GTRIAL * P,
           *d = vec + (size_t)V_DIR * P, *hs = vec + (size_t)V_HIST * P, *hy = hs + (size_t)M * P;
    const int stop_in = ci[CI_STOP], err = *reinterpret_cast<const int*>(a.ws);
    const int evals = ci[CI_EVALS] + 1;
    int halvings = ci[CI_HALVINGS], count = ci[CI_COUNT], head = ci[CI_HEAD];
    const double f = cd[CD_F], dg_in = cd[CD_DG], f_trial = reinterpret_cast<const double*>(a.ws + a.lay.o_ftrial)[e];
    double step = cd[CD_STEP], gamma = cd[CD_GAMMA];
    __syncthreads();                                          // every thread has read the state before thread 0 rewrites it
    if (stop_in != 0) return;
    if (err != 0) {
        if (t == 0) ci[CI_STOP] = 4;
        return;
    }
    const bool first = evals == 1;
    if (!first && !(f_trial <= f + kArmijo * step * dg_in + kArmijoSlack * fabs(f))) {                  // a NaN trial loss halves too
        ++halvings;
        step *= 0.5;
        const int stop = halvings >= kMaxHalvings ? 3 : evals >= a.max_evals ? 2 : 0;
        if (!stop)
            for (int i = t; i < P; i += kCtrlThreads) tr[i] = fma(step, d[i], th[i]);
        if (t == 0) {
            ci[CI_EVALS] = evals; ci[CI_HALVINGS] = halvings; ci[CI_STOP] = stop;
            cd[CD_STEP] = step;
        }
        return;
    }
    // ---- accepted: the pair (s, y), unless s.y <= 0 ----
    if (!first) {
        double sy = 0.0, yy = 0.0;
        for (int i = t; i < P; i += kCtrlThreads) {
            const double s_ = tr[i] - th[i], y_ = gt[i] - g[i];
            sy = fma(s_, y_, sy);
            yy = fma(y_, y_, yy);
        }
        sy = block_sum<kCtrlThreads>(sy, red);
        yy = block_sum<kCtrlThreads>(yy, red);
        if (sy > 0.0) {
            int slot;
            if (count < M) slot = (head + count++) % M;
            else { slot = head; head = (head + 1) % M; }
            for (int i = t; i < P; i += kCtrlThreads) {
                hs[(size_t)slot * P + i] = tr[i] - th[i];
                hy[(size_t)slot * P + i] = gt[i] - g[i];
            }
            if (t == 0) rho[slot] = 1.0 / sy;
            gamma = sy / yy;
        }
    }
    double gg = 0.0;
    for (int i = t; i < P; i += kCtrlThreads) {
        th[i] = tr[i];
        g[i] = gt[i];
        gg = fma(gt[i], gt[i], gg);
    }
    gg = block_sum<kCtrlThreads>(gg, red);
    const double gnorm = sqrt(gg);
    halvings = 0;
    const int stop = gnorm <= a.gtol ? 1 : evals >= a.max_evals ? 2 : 0;
    double dg = 0.0;
    step = 1.0;
    if (!stop) {
        // ---- two-loop recursion: d = -H g ----
        for (int i = t; i < P; i += kCtrlThreads) d[i] = g[i];
        for (int q = count - 1; q >= 0; --q) {                                  // newest pair first
            const int slot = (head + q) % M;
            const double *s_ = hs + (size_t)slot * P, *y_ = hy + (size_t)slot * P;
            double sd = 0.0;
            for (int i = t; i < P; i += kCtrlThreads) sd = fma(s_[i], d[i], sd);
            const double al = rho[slot] * block_sum<kCtrlThreads>(sd, red);
            if (t == 0) alpha[q] = al;
            for (int i = t; i < P; i += kCtrlThreads) d[i] = fma(-al, y_[i], d[i]);
        }
        if (count > 0)
            for (int i = t; i < P; i += kCtrlThreads) d[i] *= gamma;
        for (int q = 0; q < count; ++q) {
            const int slot = (head + q) % M;
            const double *s_ = hs + (size_t)slot * P, *y_ = hy + (size_t)slot * P;
            double yd = 0.0;
            for (int i = t; i < P; i += kCtrlThreads) yd = fma(y_[i], d[i], yd);
            const double beta = rho[slot] * block_sum<kCtrlThreads>(yd, red);       // its barriers publish alpha[]
            const double co = alpha[q] - beta;
            for (int i = t; i < P; i += kCtrlThreads) d[i] = fma(co, s_[i], d[i]);
        }
        for (int i = t; i < P; i += kCtrlThreads) {
            d[i] = -d[i];
            dg = fma(g[i], d[i], dg);
        }
        dg = block_sum<kCtrlThreads>(dg, red);
        if (!(dg < 0.0)) {                                                      // no descent direction: start again from steepest descent
            for (int i = t; i < P; i += kCtrlThreads) d[i] = -g[i];
            dg = -gg;
            count = 0;
            head = 0;
        }
        if (first) step = 1.0 / gnorm;                                          // the very first step; every later one starts at 1
        for (int i = t; i < P; i += kCtrlThreads) tr[i] = fma(step, d[i], th[i]);
    }
    if (t == 0) {
        ci[CI_STOP] = stop; ci[CI_EVALS] = evals; ci[CI_HALVINGS] = halvings; ci[CI_COUNT] = count; ci[CI_HEAD] = head;
        cd[CD_F] = f_trial; cd[CD_STEP] = step; cd[CD_DG] = dg; cd[CD_GNORM] = gnorm; cd[CD_GAMMA] = gamma;
    }
}

// grid (ceil(P / 256), E)
__global__ __launch_bounds__(kThreads) void head_fit_finish_kernel(FitFinishArgs a) {
    if (*reinterpret_cast<const int*>(a.ws) != 0) return;                      // a bad label: the call fails, the outputs stay as they were
    const int e = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x, P = a.lay.P;
    const double* th = reinterpret_cast<const double*>(a.ws + a.lay.o_vec) + (size_t)e * a.lay.vec_stride + (size_t)V_THETA * P;
    if (i < P) {
        for (int q = 0; q < a.n_seg; ++q) {
            const FitOutSeg& sg = a.seg[q];
            if (i < sg.begin || i >= sg.begin + sg.len) continue;
            sg.out32[(size_t)e * sg.len + i - sg.begin] = (float)th[i];
            if (sg.out64) sg.out64[(size_t)e * sg.len + i - sg.begin] = th[i];
        }
        if (a.theta64) a.theta64[(size_t)e * P + i] = th[i];
    }
    if (i == 0) {
        const int* ci = reinterpret_cast<const int*>(a.ws + a.lay.o_ctrl) + e * kCtrlInts;
        const double* cd = reinterpret_cast<const double*>(a.ws + a.lay.o_scal) + e * kCtrlDoubles;
        if (a.loss) a.loss[e] = cd[CD_F];
        if (a.grad_norm) a.grad_norm[e] = cd[CD_GNORM];
        if (a.evals) a.evals[e] = ci[CI_EVALS];
        if (a.status) a.status[e] = ci[CI_STOP] - 1;
    }
}

size_t lossgrad_lds_bytes(int H, int K) {
    return sizeof(float) * S * (size_t)(H + 4) + sizeof(double) * S * (size_t)round_up(K, 16) + sizeof(double) * 4 * S * kLogitTile;
}

template <int KT, int HC>
void launch_lossgrad_as(const LossGradArgs& a, int E, hipStream_t s) {
    const size_t lds = lossgrad_lds_bytes(a.H, a.K);
    (void)ensure_dynamic_lds<&head_fit_lossgrad_kernel<KT, HC>>("head_fit_lossgrad_kernel", 160 * 1024);
    hipLaunchKernelGGL((head_fit_lossgrad_kernel<KT, HC>), dim3((a.K + KT - 1) / KT, a.chunks, E), dim3(kThreads), lds, s, a);
}

template <int KT>
void launch_lossgrad_k(const LossGradArgs& a, int E, hipStream_t s) {
    switch ((a.H + kThreads - 1) / kThreads) {
        case 1: launch_lossgrad_as<KT, 1>(a, E, s); break;
        case 2: launch_lossgrad_as<KT, 2>(a, E, s); break;
        case 3: launch_lossgrad_as<KT, 3>(a, E, s); break;
        default: launch_lossgrad_as<KT, 4>(a, E, s); break;
    }
}

// one evaluation: the partials of every running exit, then their fixed-order sums
void launch_eval(LossGradArgs a, int E, double l2, double* loss, size_t loss_stride, double* grad, size_t grad_stride, hipStream_t s) {
    const int n_slabs = (a.N + S - 1) / S;
    a.chunks = head_fit_chunks(a.N);
    a.slabs_per_chunk = (n_slabs + a.chunks - 1) / a.chunks;
    if (a.K <= 4) launch_lossgrad_k<4>(a, E, s);
    else launch_lossgrad_k<16>(a, E, s);
    ReduceArgs r{};
    r.partial = a.partial; r.theta = a.theta; r.theta_stride = a.theta_stride; r.ctrl = a.ctrl; r.loss = loss; r.loss_stride = loss_stride;
    r.grad = grad; r.grad_stride = grad_stride; r.N = a.N; r.P = a.K * a.H + a.K; r.chunks = a.chunks; r.l2 = l2;
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

size_t head_fit_workspace_bytes(int E, int N, int H, int K, int history) { return one_layer_layout(E, N, H, K, history).bytes; }

size_t head_fit_partial_bytes(int E, int N, int H, int K) { return sizeof(double) * (size_t)E * head_fit_chunks(N) * (size_t)(K * H + K + 1); }

void launch_head_fit_controller(char* ws, const FitLayout& lay, double gtol, int max_evals, hipStream_t s) {
    CtrlArgs c{ws, lay, gtol, max_evals};
    hipLaunchKernelGGL(head_fit_controller_kernel, dim3(lay.E), dim3(kCtrlThreads), 0, s, c);
}

void launch_head_fit_finish(const FitFinishArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(head_fit_finish_kernel, dim3((a.lay.P + kThreads - 1) / kThreads, a.lay.E), dim3(kThreads), 0, s, a);
}

void launch_head_lossgrad(const float* X, const long long* y, const double* theta, int E, int N, int H, int K, double l2, double* partial, int* err,
                          double* loss, double* grad, hipStream_t s) {
    LossGradArgs a{};
    a.X = X; a.y = y; a.theta = theta; a.theta_stride = (size_t)K * H + K; a.ctrl = nullptr; a.err = err; a.partial = partial;
    a.N = N; a.H = H; a.K = K;
    launch_eval(a, E, l2, loss, 1, grad, a.theta_stride, s);
}

bool launch_head_fit(const HeadFitArgs& f, hipStream_t s) {
    const FitLayout lay = one_layer_layout(f.E, f.N, f.H, f.K, f.history);
    char* ws = static_cast<char*>(f.workspace);
    if (hipMemsetAsync(ws, 0, lay.zero_bytes, s) != hipSuccess) return false;           // theta = 0, no history, every exit running
    double* vec = reinterpret_cast<double*>(ws + lay.o_vec);
    const size_t P = lay.P;
    LossGradArgs a{};
    a.X = f.features; a.y = f.labels; a.theta = vec + V_TRIAL * P; a.theta_stride = lay.vec_stride;
    a.ctrl = reinterpret_cast<const int*>(ws + lay.o_ctrl); a.err = reinterpret_cast<int*>(ws);
    a.partial = reinterpret_cast<double*>(ws + lay.o_tail); a.N = f.N; a.H = f.H; a.K = f.K;
    for (int tick = 0; tick < f.max_evals; ++tick) {
        launch_eval(a, f.E, f.l2, reinterpret_cast<double*>(ws + lay.o_ftrial), 1, vec + V_GTRIAL * P, lay.vec_stride, s);
        launch_head_fit_controller(ws, lay, f.gtol, f.max_evals, s);
    }
    const int KH = f.K * f.H;
    FitFinishArgs o{ws, lay, 2, {{0, KH, f.weight, f.weight64}, {KH, f.K, f.bias, f.bias64}, {}, {}}, nullptr, f.loss, f.grad_norm, f.evals, f.status};
    launch_head_fit_finish(o, s);
    return true;
}

}  // namespace mmee
