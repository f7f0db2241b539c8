// ee_ensemble_fit: the weights and biases of the exit ensemble (include/mmee.h, at ee_set_ensemble) from a dumped array, on the device.  Per exit m,
// in float64,
//     L_m(w_m, b_m) = (1/N) sum_n [logsumexp(a_m,n) - a_m,n[y_n]] + (l2/2) (|w_m - e_m|^2 + |b_m|^2),    a_m,n[k] = b_m[k] + sum_{j <= m} w_m[j] l_j,n[k]
// with e_m the unit vector of the plain exit: the penalty pulls toward "no ensemble", and vanishes at the start w_m = e_m, b_m = 0.  Entries j > m
// have zero gradient and stay 0.  This file is the objective; the L-BFGS around it is run_lbfgs_fit (fit_lbfgs.hip).
//
// theta of exit m is [b_m (K), w_m (E1)], the bias first: an exit's parameters then sit at the same places whatever E1 is, the places behind w_m[m]
// hold exact zeros, and so every sum of the controller has the same bits when the exit is fitted in a shorter table.
//
//   ensemble_logsoftmax_kernel (exit_ops.hip)   once per fit: l (E1,N,K) into the workspace, by the forward's own function
//   ensemble_fit_rows_kernel                    one evaluation = one pass over l: a workgroup walks its chunk of documents in tiles it holds in LDS,
//                                               all E1 exits of a document together, so a row l_j is read from memory once; a_m by the
//                                               forward's own ens_combine_f64; one partial (gradient, loss) per chunk and exit
//   ensemble_fit_reduce_kernel                  the chunk partials in chunk order, / N, the penalty
// No floating-point atomics; the chunks are a function of N alone and an accumulator adds its documents in ascending order whatever the tile
// size: the fit is deterministic to the bit, and an exit gets the same bits alone or among others.
#include "head_fit_common.h"

namespace mmee {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxChunks = 512;              // row chunks (= partial gradients) per fit
constexpr int kMinChunkDocs = 8;
constexpr int kMaxTileDocs = 16;
constexpr size_t kLdsDoubles = 7680;         // 60 KB of dynamic LDS: no opt-in

struct RowsArgs {
    const double* l;                 // (E1,N,K)
    const long long* y;              // (N,)
    const double* theta;             // exit m: theta + m * theta_stride, [b (K), w (E1)]
    size_t theta_stride;
    const int* ctrl;
    int* err;
    double* partial;                 // (chunks, E1, Q), Q = K + E1 + 1: the gradient in theta's order, then the loss
    int E1, N, K, chunk_docs, tile_docs;
};

// grid: chunks
__global__ __launch_bounds__(kThreads) void ensemble_fit_rows_kernel(RowsArgs a) {
    extern __shared__ double lds[];
    const int t = threadIdx.x, E1 = a.E1, K = a.K, P = K + E1, Q = P + 1, EK = E1 * K;
    if (a.ctrl) {                                                                // every exit has stopped: nothing reads this evaluation
        bool run = false;
        for (int m = 0; m < E1; ++m) run = run || a.ctrl[m * kCtrlInts + CI_STOP] == 0;
        if (!run) return;
    }
    double* G = lds;                                 // [E1][Q]: pair p is owned by thread p % kThreads
    double* Lt = G + (size_t)E1 * Q;                 // [tile][E1][K]
    double* D = Lt + (size_t)a.tile_docs * EK;       // [tile][E1][K]: a, then dL/da
    double* Lrow = D + (size_t)a.tile_docs * EK;     // [tile][E1]
    for (int p = t; p < E1 * Q; p += kThreads) G[p] = 0.0;
    const int n_begin = blockIdx.x * a.chunk_docs, n_end = min(a.N, n_begin + a.chunk_docs);
    bool bad_label = false, bad_logit = false;
    for (int n0 = n_begin; n0 < n_end; n0 += a.tile_docs) {
        const int td = min(a.tile_docs, n_end - n0);
        for (int i = t; i < td * EK; i += kThreads) {
            const int d = i / EK, r = i - d * EK, j = r / K, k = r - j * K;
            const double v = a.l[((size_t)j * a.N + (n0 + d)) * K + k];
            bad_logit |= !__builtin_isfinite(v);
            Lt[i] = v;
        }
        __syncthreads();
        for (int i = t; i < td * EK; i += kThreads) {
            const int d = i / EK, r = i - d * EK, m = r / K, k = r - m * K;
            const double* th = a.theta + (size_t)m * a.theta_stride;
            const double* lt = Lt + (size_t)d * EK + k;
            D[i] = ens_combine_f64(th + K, th[k], m, [&](int j) { return lt[(size_t)j * K]; });
        }
        __syncthreads();
        for (int i = t; i < td * E1; i += kThreads) {
            const int d = i / E1;
            double* row = D + (size_t)i * K;
            const long long y = a.y[n0 + d];
            const bool ok = y >= 0 && y < K;
            bad_label |= !ok;
            double mx = row[0];
            for (int k = 1; k < K; ++k) mx = fmax(mx, row[k]);
            double s = 0.0;
            for (int k = 0; k < K; ++k) s += exp(row[k] - mx);
            Lrow[i] = ok ? (mx + log(s)) - row[(int)y] : 0.0;
            const double inv = 1.0 / s;
            for (int k = 0; k < K; ++k) row[k] = ok ? exp(row[k] - mx) * inv - (k == (int)y ? 1.0 : 0.0) : 0.0;
        }
        __syncthreads();
        for (int p = t; p < E1 * Q; p += kThreads) {
            const int m = p / Q, q = p - m * Q;
            double acc = G[p];
            if (q < K) {
                for (int d = 0; d < td; ++d) acc += D[((size_t)d * E1 + m) * K + q];
            } else if (q < P) {
                const int j = q - K;
                if (j <= m)
                    for (int d = 0; d < td; ++d) {
                        const double *dr = D + ((size_t)d * E1 + m) * K, *lr = Lt + ((size_t)d * E1 + j) * K;
                        for (int k = 0; k < K; ++k) acc = fma(dr[k], lr[k], acc);
                    }
            } else {
                for (int d = 0; d < td; ++d) acc += Lrow[d * E1 + m];
            }
            G[p] = acc;
        }
        __syncthreads();
    }
    if (bad_label) atomicOr(a.err, 1);
    if (bad_logit) atomicOr(a.err, 2);
    double* part = a.partial + (size_t)blockIdx.x * E1 * Q;
    for (int p = t; p < E1 * Q; p += kThreads) part[p] = G[p];
}

struct ReduceArgs {
    const double* partial;
    const double* theta;
    size_t theta_stride;
    const int* ctrl;
    double* loss;                    // exit m: loss[m]
    double* grad;                    // exit m: grad + m * grad_stride
    size_t grad_stride;
    int E1, N, K, chunks;
    double l2;
};

// grid: E1.  Thread q sums entry q of its exit's partials in chunk order; thread 0 then adds the penalty's part of the loss in theta's order
__global__ __launch_bounds__(kThreads) void ensemble_fit_reduce_kernel(ReduceArgs a) {
    const int m = blockIdx.x, K = a.K, P = K + a.E1, Q = P + 1;
    if (a.ctrl && a.ctrl[m * kCtrlInts + CI_STOP] != 0) return;
    const double* th = a.theta + (size_t)m * a.theta_stride;
    for (int q = threadIdx.x; q < Q; q += kThreads) {
        const double* p = a.partial + (size_t)m * Q + q;
        double sum = 0.0;
#pragma unroll 8
        for (int c = 0; c < a.chunks; ++c) sum += p[(size_t)c * a.E1 * Q];
        if (q < P) {
            const bool free_w = q < K || q - K <= m;                             // the entries above the diagonal stay exact zeros
            a.grad[(size_t)m * a.grad_stride + q] = free_w ? sum / (double)a.N + a.l2 * (th[q] - (q == K + m ? 1.0 : 0.0)) : 0.0;
        } else {
            double sq = 0.0;
            for (int i = 0; i < P; ++i) {
                const double v = th[i] - (i == K + m ? 1.0 : 0.0);
                sq = fma(v, v, sq);
            }
            a.loss[m] = sum / (double)a.N + 0.5 * a.l2 * sq;
        }
    }
}

// theta0 (E1, K + E1) from the caller's start (w0 (E1,E1), b0 (E1,K)), or w = I, b = 0
__global__ __launch_bounds__(kThreads) void ensemble_fit_start_kernel(const double* w0, const double* b0, int E1, int K, double* theta0) {
    const int P = K + E1;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < E1 * P; i += gridDim.x * kThreads) {
        const int m = i / P, q = i - m * P;
        if (q < K) theta0[i] = b0 ? b0[(size_t)m * K + q] : 0.0;
        else theta0[i] = q - K > m ? 0.0 : w0 ? w0[(size_t)m * E1 + (q - K)] : (q - K == m ? 1.0 : 0.0);
    }
}

int chunk_docs(int N) { return std::max(kMinChunkDocs, (N + kMaxChunks - 1) / kMaxChunks); }
int chunks(int N) { return (N + chunk_docs(N) - 1) / chunk_docs(N); }

// the tile a workgroup holds: G, then per document two rows tables and the row losses; 0: not even one document fits
int tile_docs(int E1, int K) {
    const size_t fixed = (size_t)E1 * (K + E1 + 1), per_doc = 2 * (size_t)E1 * K + E1;
    if (fixed + per_doc > kLdsDoubles) return 0;
    return (int)std::min<size_t>(kMaxTileDocs, (kLdsDoubles - fixed) / per_doc);
}

size_t table_doubles(int E1, int N, int K) { return (size_t)E1 * N * K; }
size_t partial_doubles(int E1, int N, int K) { return (size_t)chunks(N) * E1 * (K + E1 + 1); }

FitLayout ensemble_layout(int E1, int N, int K, int M) {
    return FitLayout(E1, K + E1, M, sizeof(double) * (table_doubles(E1, N, K) + partial_doubles(E1, N, K) + (size_t)E1 * (K + E1)));
}

void launch_eval(const FitEvalPoint& p, const long long* y, int E1, int N, int K, double l2, hipStream_t s) {
    double* l = static_cast<double*>(p.tail);
    double* partial = l + table_doubles(E1, N, K);
    const int td = tile_docs(E1, K);
    RowsArgs a{l, y, p.theta, p.theta_stride, p.ctrl, p.err, partial, E1, N, K, chunk_docs(N), td};
    const size_t lds = sizeof(double) * ((size_t)E1 * (K + E1 + 1) + (size_t)td * (2 * (size_t)E1 * K + E1));
    hipLaunchKernelGGL(ensemble_fit_rows_kernel, dim3(chunks(N)), dim3(kThreads), lds, s, a);
    ReduceArgs r{partial, p.theta, p.theta_stride, p.ctrl, p.loss, p.grad, p.grad_stride, E1, N, K, chunks(N), l2};
    hipLaunchKernelGGL(ensemble_fit_reduce_kernel, dim3(E1), dim3(kThreads), 0, s, r);
}

}  // namespace

bool ensemble_fit_supports(int E1, int K) { return tile_docs(E1, K) >= 1; }

size_t ensemble_fit_workspace_bytes(int E1, int N, int K, int history) { return ensemble_layout(E1, N, K, history).bytes; }

bool launch_ensemble_fit(const EnsembleFitArgs& f, hipStream_t s) {
    const int E1 = f.E, N = f.N, K = f.K;
    const FitLayout lay = ensemble_layout(E1, N, K, f.history);
    double* l = reinterpret_cast<double*>(static_cast<char*>(f.workspace) + lay.o_tail);
    double* theta0 = l + table_doubles(E1, N, K) + partial_doubles(E1, N, K);
    launch_ensemble_logsoftmax(f.logits, (size_t)E1 * N, K, l, s);
    hipLaunchKernelGGL(ensemble_fit_start_kernel, dim3(grid_1d((long long)E1 * (K + E1), kThreads, 64)), dim3(kThreads), 0, s, f.w0, f.b0, E1, K, theta0);
    FitArgs g = f;
    g.theta0 = theta0;
    return run_lbfgs_fit(g, lay, [&](const FitEvalPoint& p) { launch_eval(p, f.labels, E1, N, K, f.l2, s); },
                         {{0, K, nullptr, f.b}, {K, E1, nullptr, f.w}}, s, nullptr, 0);
}

}  // namespace mmee
