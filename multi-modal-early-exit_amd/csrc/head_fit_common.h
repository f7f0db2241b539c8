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

// theta[begin, begin + len) of exit e goes to out32 + e * len (and to out64 + e * len when given)
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
// { eval(trial point); controller }, then theta[seg] of every exit to the segments' outputs and f's result pointers.  false: preparing the
// workspace failed.
bool run_lbfgs_fit(const FitArgs& f, const FitLayout& lay, const std::function<void(const FitEvalPoint&)>& eval,
                   std::initializer_list<FitOutSeg> segs, hipStream_t s);

}  // namespace mmee
