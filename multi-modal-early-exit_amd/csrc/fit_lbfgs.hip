// The optimiser of the device fits (ee_head_fit, ee_mlp_head_fit, ee_lte_fit): L-BFGS as a fixed launch list over a workspace (FitLayout,
// head_fit_common.h), written over a parameter count P and knowing nothing of the objective.  An objective (head_fit.hip, mlp_head_fit.hip,
// lte_fit.hip) hands run_lbfgs_fit one callable that evaluates L and grad L at a FitEvalPoint; a tick is that evaluation, then
//   head_fit_controller_kernel  one workgroup per exit: Armijo test, history update, two-loop recursion, next trial point.
// Behind the last tick
//   head_fit_finish_kernel      copies the result out -- unless the error word is set, in which case no output is touched.
//
// Determinism: an element of a parameter-sized vector is always touched by the same thread of the controller, every sum has a fixed order,
// and nothing depends on E -- an exit fitted alone gets the bits it gets among others.
#include <algorithm>

#include "head_fit_common.h"

namespace mmee {

namespace {

constexpr int kThreads = 256;
constexpr int kCtrlThreads = kFitCtrlThreads;
constexpr double kArmijo = 1e-4;
// The Armijo test allows for the rounding of L: below a gradient norm of a few 1e-9 the decrease a good step brings is smaller than the
// resolution of L in float64, and without the allowance no trial point passes any more (measured on the host restatement: 3 of 36 problems
// stall at 1.2e-9 ... 2.4e-9 for 200 evaluations; with 1, 4 or 16 epsilon |L| none does).
constexpr double kArmijoSlack = 8.0 * 2.220446049250313e-16;
constexpr int kMaxHalvings = 30;

struct CtrlArgs {
    char* ws;
    FitLayout lay;
    double gtol;
    int max_evals;
};

// one tick's decision for every exit: reads L(trial) at o_ftrial and grad L(trial) in V_GTRIAL, writes the next trial point into V_TRIAL
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
            if (sg.out32) sg.out32[(size_t)e * sg.len + i - sg.begin] = (float)th[i];      // null: a float64 fit (ee_ensemble_fit)
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

}  // namespace

bool run_lbfgs_fit(const FitArgs& f, const FitLayout& lay, const std::function<void(const FitEvalPoint&)>& eval,
                   std::initializer_list<FitOutSeg> segs, hipStream_t s, const float* weights, size_t scratch_bytes) {
    char* ws = static_cast<char*>(f.workspace);
    if (hipMemsetAsync(ws, 0, lay.zero_bytes, s) != hipSuccess) return false;           // theta = 0, no history, every exit running
    double* vec = reinterpret_cast<double*>(ws + lay.o_vec);
    const size_t P = lay.P;
    // the first trial point is theta0: the controller's first tick accepts it as the start
    for (int e = 0; f.theta0 && e < lay.E; ++e)
        if (hipMemcpyAsync(vec + (size_t)e * lay.vec_stride + V_TRIAL * P, f.theta0 + (size_t)e * P, sizeof(double) * P, hipMemcpyDeviceToDevice,
                           s) != hipSuccess)
            return false;
    const FitEvalPoint p{vec + V_TRIAL * P, lay.vec_stride, reinterpret_cast<const int*>(ws + lay.o_ctrl), reinterpret_cast<int*>(ws),
                         reinterpret_cast<double*>(ws + lay.o_ftrial), vec + V_GTRIAL * P, lay.vec_stride, ws + lay.o_tail};
    const CtrlArgs c{ws, lay, f.gtol, f.max_evals};
    if (weights) launch_row_scale(weights, f.E, f.N, scale_table(p.tail, scratch_bytes), p.err, s);
    for (int tick = 0; tick < f.max_evals; ++tick) {
        eval(p);
        hipLaunchKernelGGL(head_fit_controller_kernel, dim3(lay.E), dim3(kCtrlThreads), 0, s, c);
    }
    FitFinishArgs o{ws, lay, (int)segs.size(), {}, f.theta64, f.loss, f.grad_norm, f.evals, f.status};
    std::copy(segs.begin(), segs.end(), o.seg);
    hipLaunchKernelGGL(head_fit_finish_kernel, dim3((lay.P + kThreads - 1) / kThreads, lay.E), dim3(kThreads), 0, s, o);
    return true;
}

}  // namespace mmee
