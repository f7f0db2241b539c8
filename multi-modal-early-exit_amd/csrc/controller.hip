// Online exit control (the definition is in include/mmee.h, behind the audit's): the two launches a controlled forward adds behind its final
// exit, and the replay of the whole loop on dumped arrays.
//   audit_tally_kernel       what the audit saw in the call: the selected slots (the hash over the call's B slots), and among the shadows of the
//                            final stage -- the documents delivered early that ran on -- how many were delivered with another argmax than the
//                            full model's, in all and per exit.  One workgroup of 1024 threads, chunks of 1024, ballot -> popcount through
//                            block1024_count; the per-exit counts through integer atomics in LDS.  Integer sums only: any order gives the same bits.
//   controller_step_kernel   one thread: the log row of the call, p <- min(V - 1, p - gamma (disagree / sampled - alpha)), the thresholds of
//                            the NEXT call into the vector the decide kernels read at launch time.
//   rolling_control_kernel   the same loop on a criterion table (E1,N) and a 0 / 1 loss table: one workgroup, sequential over the groups of G
//                            consecutive documents that play the calls.
// Small, latency-bound launches in the class of cascade_select_kernel.  The arithmetic of the thresholds and of the step, the exit test and the
// argmax are the shared functions of mmee_kernels.h; controller_advance below is the one copy of "log, step, next thresholds".
#include "ranked_common.h"

namespace mmee {

namespace {

__device__ __forceinline__ long long f64_bits(double x) {
    long long u;
    __builtin_memcpy(&u, &x, sizeof(u));
    return u;
}

// Behind a call's tally, by one thread: the log row (call index, p before and after, the tally, the thresholds the call ran with), the state,
// and thr <- the thresholds of position p_after.  row: controller_log_words(E1) words, or null.  Returns p_after.
__device__ __forceinline__ double controller_advance(const double* path, int V, int E1, double sign, double alpha, double gamma, long long* state,
                                                     const long long* tally, double* thr, long long* row) {
    double p;
    __builtin_memcpy(&p, &state[0], sizeof(p));
    const long long call = state[1], sampled = tally[0], disagree = tally[1];
    const double q = controller_step(p, sampled, disagree, alpha, gamma, V);
    const int nt = controller_tally_words(E1);
    if (row) {
        row[0] = call;
        row[1] = f64_bits(p);
        row[2] = f64_bits(q);
        for (int j = 0; j < nt; ++j) row[3 + j] = tally[j];
        for (int e = 0; e < E1; ++e) row[3 + nt + e] = f64_bits(thr[e]);
    }
    state[0] = f64_bits(q);
    state[1] = call + 1;
    state[2] += sampled != 0 ? 1 : 0;
    state[3] += sampled;
    state[4] += disagree;
    controller_thresholds(path, V, E1, q, sign, thr);
    return q;
}

}  // namespace

__global__ __launch_bounds__(1024) void audit_tally_kernel(AuditTallyArgs a) {
    __shared__ int s_bad[16], s_sel[16];
    __shared__ int s_deliv[kCtlMaxE1], s_agree[kCtlMaxE1];
    const int tid = threadIdx.x;
    const int E = a.E1 - 1;
    if (tid < kCtlMaxE1) { s_deliv[tid] = 0; s_agree[tid] = 0; }
    __syncthreads();
    const int n = a.counts->n_docs;
    long long disagree = 0, sampled = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + tid;
        bool shadow = false, differs = false;
        if (i < n) {
            const int orig = a.doc_orig[i];
            shadow = a.delivered[orig] != 0;
            if (shadow) {
                const float* z = a.pol_logits + (size_t)i * a.K;
                const float* y = a.out_logits + (size_t)orig * a.K;
                const double temp = a.temp;
                const int am_full = row_first_argmax([&](int k) { return (float)((double)z[k] / temp); }, a.K);
                const int am_out = row_first_argmax([&](int k) { return y[k]; }, a.K);
                differs = am_full != am_out;
                const int e = a.out_exit[orig];
                if (e >= 0 && e < E) {                                   // a shadow was delivered below the final exit
                    atomicAdd(&s_deliv[e], 1);
                    if (!differs) atomicAdd(&s_agree[e], 1);
                }
            }
        }
        disagree += block1024_count(shadow && differs, s_bad).total;
        __syncthreads();                                                 // the slots are read: the next chunk may write them
    }
    for (int base = 0; base < a.B; base += 1024) {
        const int slot = base + tid;
        const bool sel = slot < a.B && audit_selected(a.cut, a.seed, (int)((unsigned)slot + (unsigned)a.slot_base));
        sampled += block1024_count(sel, s_sel).total;
        __syncthreads();
    }
    if (tid == 0) { a.tally[0] = sampled; a.tally[1] = disagree; }
    if (tid < E) { a.tally[2 + tid] = s_deliv[tid]; a.tally[2 + E + tid] = s_agree[tid]; }
}

void launch_audit_tally(const AuditTallyArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(audit_tally_kernel, dim3(1), dim3(1024), 0, s, a);
}

__global__ __launch_bounds__(64) void controller_step_kernel(ControllerStepArgs a) {
    if (threadIdx.x != 0) return;
    long long* row = nullptr;
    if (a.log && a.log_cap > 0) row = a.log + (size_t)(a.state[1] % a.log_cap) * controller_log_words(a.E1);
    (void)controller_advance(a.path, a.V, a.E1, a.sign, a.alpha, a.gamma, a.state, a.tally, a.thr, row);
}

void launch_controller_step(const ControllerStepArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(controller_step_kernel, dim3(1), dim3(64), 0, s, a);
}

__global__ __launch_bounds__(1024) void rolling_control_kernel(RollingControlArgs a) {
    __shared__ int s_sel[16], s_bad[16];
    __shared__ int s_deliv[kCtlMaxE1], s_agree[kCtlMaxE1];
    __shared__ double s_thr[kCtlMaxE1];
    __shared__ long long s_state[kCtlStateWords], s_tally[2 + 2 * kCtlMaxE1];
    const int tid = threadIdx.x;
    const int E1 = a.E1, E = E1 - 1;
    if (tid == 0) {
        s_state[0] = f64_bits(a.p0);
        for (int j = 1; j < kCtlStateWords; ++j) s_state[j] = 0;
        controller_thresholds(a.path, a.V, E1, a.p0, a.sign, s_thr);
    }
    const int groups = (a.N + a.G - 1) / a.G;
    for (int g = 0; g < groups; ++g) {
        if (tid < kCtlMaxE1) { s_deliv[tid] = 0; s_agree[tid] = 0; }
        __syncthreads();                                                 // the group's thresholds and zeroed counts are in LDS
        const int n0 = g * a.G;
        const int cnt = a.N - n0 < a.G ? a.N - n0 : a.G;
        const unsigned seed = a.seed + (unsigned)g;
        long long sampled = 0, disagree = 0;
        for (int base = 0; base < cnt; base += 1024) {
            const int slot = base + tid;
            bool sel = false, lost = false;
            if (slot < cnt) {
                const size_t n = (size_t)n0 + slot;
                int exit = E;
                for (int e = E - 1; e >= 0; --e)
                    if (sign_fires(a.sign, a.table[(size_t)e * a.N + n], s_thr[e])) exit = e;
                a.exits[n] = exit;
                sel = audit_selected(a.cut, seed, slot);
                if (sel && exit < E) {
                    lost = a.bad[(size_t)exit * a.N + n] != 0;
                    atomicAdd(&s_deliv[exit], 1);
                    if (!lost) atomicAdd(&s_agree[exit], 1);
                }
            }
            sampled += block1024_count(sel, s_sel).total;
            disagree += block1024_count(lost, s_bad).total;
            __syncthreads();
        }
        if (tid == 0) { s_tally[0] = sampled; s_tally[1] = disagree; }
        if (tid < E) { s_tally[2 + tid] = s_deliv[tid]; s_tally[2 + E + tid] = s_agree[tid]; }
        __syncthreads();
        if (tid == 0)
            (void)controller_advance(a.path, a.V, E1, a.sign, a.alpha, a.gamma, s_state, s_tally, s_thr, a.log + (size_t)g * controller_log_words(E1));
        __syncthreads();
    }
    if (tid == 0 && a.p_out) __builtin_memcpy(a.p_out, &s_state[0], sizeof(double));
}

void launch_rolling_control(const RollingControlArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(rolling_control_kernel, dim3(1), dim3(1024), 0, s, a);
}

}  // namespace mmee
