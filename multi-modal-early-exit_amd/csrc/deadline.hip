// Deadline exits (the definition is in include/mmee.h, behind the controller's): the launches a deadline forward adds.
//   deadline_begin_kernel   the call's first launch, one wave: t0 <- s_memrealtime (the chip-wide 100 MHz counter), "no cut yet", the call's
//                           thresholds (a kernel argument) into the vector its decide launches read, the head of the log row.
//   deadline_check_kernel   one wave in front of every exit's decide launch: the elapsed time into the log row, and -- by deadline_rule of
//                           mmee_kernels.h, once per call at the most -- the always-fires value into thr[exit_index .. E1 - 2], one lane per entry.
// Every lane evaluates the rule on the same words (the clock is a scalar read, wave-uniform), so no lane has to hand a verdict to another;
// lane 0 writes the state and the log.  The host's request word is pinned host memory: it is read with a relaxed system-scope atomic load.
// Latency-bound launches in the class of controller_step_kernel; no decide, layer or row kernel knows about them.
#include "mmee_kernels.h"

namespace mmee {

__global__ __launch_bounds__(64) void deadline_begin_kernel(DeadlineBeginArgs a) {
    const int lane = threadIdx.x;
    if (lane < a.E1) a.thr[lane] = a.thr_in[lane];
    if (a.row && lane < a.E1) a.row[4 + lane] = 0;
    if (lane != 0) return;
    a.state[0] = (long long)__builtin_amdgcn_s_memrealtime();
    a.state[1] = -1;
    a.state[2] = 0;
    if (a.row) { a.row[0] = (long long)a.call; a.row[1] = (long long)a.budget; a.row[2] = -1; a.row[3] = 0; }
}

void launch_deadline_begin(const DeadlineBeginArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(deadline_begin_kernel, dim3(1), dim3(64), 0, s, a);
}

__global__ __launch_bounds__(64) void deadline_check_kernel(DeadlineCheckArgs a) {
    const int lane = threadIdx.x;
    const unsigned long long now = a.now_set ? a.now : __builtin_amdgcn_s_memrealtime();
    const unsigned long long t0 = a.t0_set ? a.t0 : (unsigned long long)a.state[0];
    const int prev_exit = (int)a.state[1], prev_by = (int)a.state[2];
    const unsigned long long word = __hip_atomic_load(a.host_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const DeadlineVerdict v = deadline_rule(t0, now, a.khz, a.budget, a.eta, word, a.call, a.exit_index, a.E1, prev_exit, prev_by);
    __syncthreads();                                                     // every lane has read the state lane 0 rewrites
    const bool cut_now = prev_exit < 0 && v.cut_exit >= 0;
    if (cut_now && lane >= a.exit_index && lane < a.E1 - 1) a.thr[lane] = deadline_always_fires(a.sign);
    if (lane != 0) return;
    if (cut_now) { a.state[1] = v.cut_exit; a.state[2] = v.cut_by; }
    if (a.row) {
        a.row[4 + a.exit_index] = (long long)v.elapsed_ns;
        if (cut_now) { a.row[2] = v.cut_exit; a.row[3] = v.cut_by; }
    }
}

void launch_deadline_check(const DeadlineCheckArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(deadline_check_kernel, dim3(1), dim3(64), 0, s, a);
}

}  // namespace mmee
