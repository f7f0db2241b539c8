// The threshold refinement (ee_threshold_refine, include/mmee.h): S independent chains of steepest-ascent coordinate search on the percentile
// grid of the threshold searches, for J(d) = w hits(d) - cost_sum(d) under a budget on cost_sum, with no host round trip between rounds.  The
// ranking pass and the percentile table are the searches' own (SweepRanks, launch_search_table).
//
// A round scores all (E1 - 1) P single-exit neighbours of a chain's vector in ONE pass of O(E1) work per document.  For a document with base
// exit x0 and next firing exit x1 behind it (E1 - 1 when none), changing the digit of exit e
//   e <  x0   moves the document to e for exactly the digits p whose threshold it beats: a PREFIX [0, k) of p, the table ascends;
//   e == x0   moves it on to x1 for the digits whose threshold it does not beat: the SUFFIX [k, P);
//   e >  x0   changes nothing,
// with k = k[e][n] = #{p : conf[e][n] > table[e][p]}, a property of the document alone: neither the chain nor the round enters.  So
//   refine_prep_kernel    once: kb (E1, N) bytes, kb[e][n] = k | correct << 7, from the rank records and trank -- the strict compare of the values
//                         decides (rec >= trank  <=>  conf > table, exit_ops.hip), duplicated table values and confidences equal to a threshold
//                         included.  Under digit d a document fires at e iff k > d.  Row E1 - 1: k = 0.
//   refine_delta_kernel   per round, grid (document chunks, chains): a thread walks a document's bytes for (x0, x1), adds the base vector's
//                         (hits, exit, cost) and at most x0 + 1 triples (d hits, d exit, d cost) into difference arrays over p -- +D at [e][0] and
//                         -D at [e][k], or +D at [e][k] -- in LDS by integer atomics (the +D at [e][0], one word for the whole wave, summed over
//                         the wave first), and the workgroup adds its non-zero entries to the chain's arrays in the workspace by integer
//                         atomics.  Integers only: exact in any order of arrival.
//   refine_pick_kernel    per round, one workgroup per chain: the arrays to LDS (and zeroed for the next round), thread e scans row e over p --
//                         the running sums ARE the neighbour's differences to the base --, keeps the admissible p of largest gain
//                         w dhits - dcost (lowest p on a tie), thread 0 takes the largest over e (lowest e on a tie), and the chain moves iff the
//                         gain is positive, else retires with status 0.  Round 0 also records the start and retires a start over its budget (2).
//   refine_finish_kernel  the chains' state to the caller's arrays.
// The driver is a fixed list of max_rounds x (delta, pick) launches; the workgroups of a retired chain return at once on its `live` word.  No
// cooperative launch, no barrier across workgroups, no workgroup that waits for another.
#include "ranked_common.h"

namespace mmee {

constexpr int kRefineChunk = 1024;           // documents per workgroup of the delta kernel: four per thread

// a chain's state in the workspace
struct RefineState {
    int *live, *rounds, *status, *hits, *exit_sum, *start_hits;
    unsigned long long *cost_sum, *start_cost_sum;
    unsigned long long* base;                // (S, 3): the base vector's hits, exit sum, cost sum of the round, by atomics
    int *acc_h, *acc_x;                      // (S, M) difference arrays, M = (E1 - 1) (P + 1)
    unsigned long long* acc_c;               // (S, M), two's complement
};

__global__ __launch_bounds__(256) void refine_prep_kernel(const unsigned* __restrict__ rec, const unsigned* __restrict__ trank,
                                                          const unsigned char* __restrict__ correct, int E1, int E1P, int N, int P,
                                                          unsigned char* __restrict__ kb) {
    const int e = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    if (e == E1 - 1) {                                               // the final exit takes whoever is left: no threshold
        kb[(size_t)e * N + n] = correct[(size_t)e * N + n] ? 128u : 0u;
        return;
    }
    const unsigned r = rec[(size_t)n * E1P + e];
    unsigned k = 0;
    for (int p = 0; p < P; ++p) k += trank[e * P + p] <= r ? 1u : 0u;     // the same address in every lane
    kb[(size_t)e * N + n] = (unsigned char)(k | ((r >> 6) & 1u) << 7);
}

__global__ __launch_bounds__(256) void refine_init_kernel(const unsigned char* __restrict__ start, int S, int E1, int P, unsigned char* __restrict__ digits,
                                                          RefineState st) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S * E1) return;
    const int s = i / E1, e = i - s * E1;
    const unsigned d = start[i];
    digits[i] = e == E1 - 1 ? 0 : (unsigned char)(d < (unsigned)P ? d : (unsigned)P - 1u);
    if (e == 0) {
        st.live[s] = 1;
        st.status[s] = 1;                                            // what a chain that never retires ends with
    }
}

// op over the 64 lanes of a wave by DPP, returned wave-uniform: the steps of wave_sum_uniform (mmee_common.h) on integers, for an associative and
// commutative op with identity 0 on the values given (sums; the maximum of non-negative values).  Lanes a step does not write keep op(v, 0).
// Every lane of the wave must be active.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_int_or_zero(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, false);
}
template <typename Op>
__device__ __forceinline__ int wave_reduce_uniform(int v, Op&& op) {
    v = op(v, dpp_int_or_zero<0xB1, 0xf>(v));        // quad_perm [1,0,3,2]
    v = op(v, dpp_int_or_zero<0x4E, 0xf>(v));        // quad_perm [2,3,0,1]
    v = op(v, dpp_int_or_zero<0x141, 0xf>(v));       // row_half_mirror
    v = op(v, dpp_int_or_zero<0x140, 0xf>(v));       // row_mirror
    v = op(v, dpp_int_or_zero<0x142, 0xa>(v));       // row_bcast15 -> rows 1, 3
    v = op(v, dpp_int_or_zero<0x143, 0xc>(v));       // row_bcast31 -> rows 2, 3
    return __builtin_amdgcn_readlane(v, 63);
}

// LDS of the delta and pick kernels: dc (M x 8 bytes) | dh (M x 4) | dx (M x 4) | the kernel's own words
__device__ __forceinline__ void refine_lds(unsigned char* base, int M, unsigned long long*& dc, int*& dh, int*& dx, unsigned long long*& tail) {
    dc = reinterpret_cast<unsigned long long*>(base);
    dh = reinterpret_cast<int*>(base + (size_t)M * 8);
    dx = dh + M;
    tail = reinterpret_cast<unsigned long long*>(base + (size_t)M * 16);
}

__global__ __launch_bounds__(256) void refine_delta_kernel(const unsigned char* __restrict__ kb, const unsigned* __restrict__ cost,
                                                           const unsigned char* __restrict__ digits, int E1, int N, int P, RefineState st) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int s = blockIdx.y;
    if (!st.live[s]) return;                                         // the same word for the whole workgroup
    const int M = (E1 - 1) * (P + 1), P1 = P + 1, last = E1 - 1;
    unsigned long long *dc, *tail;
    int *dh, *dx;
    refine_lds(s_raw, M, dc, dh, dx, tail);
    unsigned long long* s_base = tail;                               // 3 words
    unsigned char* s_dig = reinterpret_cast<unsigned char*>(tail + 3);       // 64 bytes
    for (int i = threadIdx.x; i < M; i += 256) { dc[i] = 0ull; dh[i] = 0; dx[i] = 0; }
    if (threadIdx.x < 3) s_base[threadIdx.x] = 0ull;
    if (threadIdx.x < 64) s_dig[threadIdx.x] = threadIdx.x < last ? digits[(size_t)s * E1 + threadIdx.x] : 0;
    __syncthreads();
    const int n_end = min(N, (int)(blockIdx.x + 1) * kRefineChunk), lane = threadIdx.x & 63;
    unsigned b_hits = 0, b_exit = 0;
    unsigned long long b_cost = 0;
    const auto add = [&](int at, int d_hits, int d_exit, long long d_cost) {
        if (d_hits) atomicAdd(&dh[at], d_hits);
        if (d_exit) atomicAdd(&dx[at], d_exit);
        if (d_cost) atomicAdd(&dc[at], (unsigned long long)d_cost);
    };
    for (int n0 = blockIdx.x * kRefineChunk; n0 < n_end; n0 += 256) {        // the same trips for every thread: the wave sums below need all lanes
        const int n = n0 + threadIdx.x;
        const bool valid = n < n_end;
        int x0 = 0, x1 = last, c0 = 0;                               // no document: nothing below exit 0
        long long k0 = 0;
        if (valid) {
            x0 = last;                                               // the first and the second exit that fire
            for (int e = 0; e < last; ++e) {
                if ((int)(kb[(size_t)e * N + n] & 127u) > (int)s_dig[e]) {
                    if (x0 == last) x0 = e;
                    else { x1 = e; break; }
                }
            }
            c0 = kb[(size_t)x0 * N + n] >> 7;
            k0 = cost ? (long long)cost[(size_t)x0 * N + n] : (long long)x0;
            b_hits += (unsigned)c0;
            b_exit += (unsigned)x0;
            b_cost += (unsigned long long)k0;
            if (x0 < last) {                                         // its own exit lets it go on to x1 for the digits [k, P)
                const int k = (int)(kb[(size_t)x0 * N + n] & 127u), c1 = kb[(size_t)x1 * N + n] >> 7;
                const long long k1 = cost ? (long long)cost[(size_t)x1 * N + n] : (long long)x1;
                add(x0 * P1 + k, c1 - c0, x1 - x0, k1 - k0);
            }
        }
        // An earlier exit e < x0 takes the document for the digits [0, k): -D at [e][k], one atomic per lane at scattered words, and +D at
        // [e][0] -- the SAME word for every lane, so the wave sums its D first (DPP, exact on integers) and lane 0 adds once.  The loop runs to
        // the wave's largest x0 with the other lanes contributing zeros.
        const int x_max = wave_reduce_uniform(x0, [](int a, int b) { return a > b ? a : b; });
        for (int e = 0; e < x_max; ++e) {
            const bool below = valid && e < x0;
            const unsigned b = below ? kb[(size_t)e * N + n] : 0u;
            const int k = (int)(b & 127u);
            const bool on = below && k > 0;
            const int d_hits = on ? (int)(b >> 7) - c0 : 0, d_exit = on ? e - x0 : 0;
            const long long d_cost = on ? (cost ? (long long)cost[(size_t)e * N + n] : (long long)e) - k0 : 0ll;       // |d_cost| < 2^32
            if (on) add(e * P1 + k, -d_hits, -d_exit, -d_cost);      // k <= P: row e has P + 1 entries
            const auto plus = [](int a, int b) { return a + b; };
            const int s_hits = wave_reduce_uniform(d_hits, plus), s_exit = wave_reduce_uniform(d_exit, plus);
            // the cost difference in two pieces whose 64-fold sums fit 32 bits: d_cost = hi 2^16 + lo, 0 <= lo < 2^16, |hi| <= 2^16
            const int s_lo = wave_reduce_uniform((int)(d_cost & 0xFFFF), plus), s_hi = wave_reduce_uniform((int)(d_cost >> 16), plus);
            if (lane == 0) add(e * P1, s_hits, s_exit, (long long)s_hi * 65536 + (long long)s_lo);
        }
    }
    atomicAdd(&s_base[0], (unsigned long long)b_hits);
    atomicAdd(&s_base[1], (unsigned long long)b_exit);
    atomicAdd(&s_base[2], b_cost);
    __syncthreads();
    const size_t row = (size_t)s * M;
    for (int i = threadIdx.x; i < M; i += 256) {
        if (dh[i]) atomicAdd(&st.acc_h[row + i], dh[i]);
        if (dx[i]) atomicAdd(&st.acc_x[row + i], dx[i]);
        if (dc[i]) atomicAdd(&st.acc_c[row + i], dc[i]);
    }
    if (threadIdx.x < 3) atomicAdd(&st.base[(size_t)s * 3 + threadIdx.x], s_base[threadIdx.x]);
}

__global__ __launch_bounds__(256) void refine_pick_kernel(const unsigned long long* __restrict__ hit_value, const unsigned long long* __restrict__ budget,
                                                          unsigned char* __restrict__ digits, int E1, int P, int round, int max_rounds, RefineState st) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int s = blockIdx.x;
    if (!st.live[s]) return;
    const int M = (E1 - 1) * (P + 1), P1 = P + 1, tid = threadIdx.x;
    unsigned long long *dc, *tail;
    int *dh, *dx;
    refine_lds(s_raw, M, dc, dh, dx, tail);
    long long* s_gain = reinterpret_cast<long long*>(tail);          // 64 words each: the best neighbour of every exit
    long long* s_dcost = s_gain + 64;
    int* s_dhits = reinterpret_cast<int*>(s_dcost + 64);
    int* s_dexit = s_dhits + 64;
    int* s_p = s_dexit + 64;
    const size_t row = (size_t)s * M;
    for (int i = tid; i < M; i += 256) {
        dc[i] = st.acc_c[row + i]; dh[i] = st.acc_h[row + i]; dx[i] = st.acc_x[row + i];
        st.acc_c[row + i] = 0ull; st.acc_h[row + i] = 0; st.acc_x[row + i] = 0;          // for the next round
    }
    const unsigned long long base_hits = st.base[(size_t)s * 3], base_exit = st.base[(size_t)s * 3 + 1], base_cost = st.base[(size_t)s * 3 + 2];
    const unsigned long long B = budget ? budget[s] : ~0ull;
    const unsigned long long w64 = hit_value[s];
    const long long w = (long long)(w64 < 0xFFFFFFFFull ? w64 : 0xFFFFFFFFull);
    __syncthreads();                                                 // every thread has read the base
    if (tid < 3) st.base[(size_t)s * 3 + tid] = 0ull;
    if (round == 0) {
        if (tid == 0) {
            st.start_hits[s] = (int)base_hits;
            st.start_cost_sum[s] = base_cost;
            st.hits[s] = (int)base_hits; st.exit_sum[s] = (int)base_exit; st.cost_sum[s] = base_cost;
        }
        if (base_cost > B) {                                         // the start is over its budget: the chain describes it and ends
            if (tid == 0) { st.status[s] = 2; st.live[s] = 0; }
            return;
        }
    }
    if (tid < E1 - 1) {
        long long best = 0, best_c = 0, c = 0;
        int best_h = 0, best_x = 0, best_p = -1, h = 0, x = 0;
        for (int p = 0; p < P; ++p) {
            h += dh[tid * P1 + p]; x += dx[tid * P1 + p]; c += (long long)dc[tid * P1 + p];
            if ((unsigned long long)((long long)base_cost + c) > B) continue;        // not admissible
            const long long gain = w * (long long)h - c;             // |w h| < 2^56, |c| < 2^56
            if (best_p < 0 || gain > best) { best = gain; best_c = c; best_h = h; best_x = x; best_p = p; }
        }
        s_gain[tid] = best; s_dcost[tid] = best_c; s_dhits[tid] = best_h; s_dexit[tid] = best_x; s_p[tid] = best_p;
    }
    __syncthreads();
    if (tid == 0) {
        int be = -1;
        for (int e = 0; e < E1 - 1; ++e)
            if (s_p[e] >= 0 && (be < 0 || s_gain[e] > s_gain[be])) be = e;
        if (be >= 0 && s_gain[be] > 0) {
            digits[(size_t)s * E1 + be] = (unsigned char)s_p[be];
            st.hits[s] = (int)base_hits + s_dhits[be];
            st.exit_sum[s] = (int)base_exit + s_dexit[be];
            st.cost_sum[s] = (unsigned long long)((long long)base_cost + s_dcost[be]);
            st.rounds[s] = round + 1;
            if (round + 1 == max_rounds) st.live[s] = 0;             // status stays 1
        } else {
            st.status[s] = 0;                                        // no admissible single-exit change improves J
            st.live[s] = 0;
        }
    }
}

__global__ __launch_bounds__(256) void refine_finish_kernel(const unsigned char* __restrict__ digits, const double* __restrict__ table, int S, int E1, int P,
                                                            RefineState st, double* __restrict__ thresholds, int* __restrict__ hits,
                                                            int* __restrict__ exit_sum, unsigned long long* __restrict__ cost_sum, int* __restrict__ rounds,
                                                            int* __restrict__ status, int* __restrict__ start_hits,
                                                            unsigned long long* __restrict__ start_cost_sum) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S * E1) return;
    const int s = i / E1, e = i - s * E1;
    if (thresholds) thresholds[i] = e == E1 - 1 ? 0.0 : table[e * P + digits[i]];
    if (e) return;
    if (hits) hits[s] = st.hits[s];
    if (exit_sum) exit_sum[s] = st.exit_sum[s];
    if (cost_sum) cost_sum[s] = st.cost_sum[s];
    if (rounds) rounds[s] = st.rounds[s];
    if (status) status[s] = st.status[s];
    if (start_hits) start_hits[s] = st.start_hits[s];
    if (start_cost_sum) start_cost_sum[s] = st.start_cost_sum[s];
}

// what launch_threshold_refine allocates for its rounds (the ranking pass's own arrays, SweepRanks, come on top while it is enqueued)
size_t threshold_refine_workspace_bytes(int E1, int N, int P, int S) {
    const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t M = (size_t)(E1 - 1) * (P + 1);
    return up((size_t)E1 * P * 8) + up((size_t)E1 * P * 4) + up((size_t)E1 * N) + 6 * up((size_t)S * 4) + 2 * up((size_t)S * 8) + up((size_t)S * 24) +
           2 * up((size_t)S * M * 4) + up((size_t)S * M * 8);
}

// false: a workspace allocation failed and nothing was launched
bool launch_threshold_refine(const RefineArgs& a, const SearchPercentiles& pc, hipStream_t s) {
    const int E1 = a.E1, N = a.N, P = a.P, S = a.S, E1P = (E1 + 3) & ~3;
    const size_t M = (size_t)(E1 - 1) * (P + 1);
    const SweepRanks r(a.conf, a.correct, E1, E1P, N, nullptr, 0, 1, s);
    if (!r.ok) return false;
    char* ws = nullptr;
    const size_t bytes = threshold_refine_workspace_bytes(E1, N, P, S);
    if (hipMallocAsync((void**)&ws, bytes, s) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    size_t o = 0;
    const auto take = [&](size_t b) { char* p = ws + o; o += up(b); return p; };
    double* table_ws = reinterpret_cast<double*>(take((size_t)E1 * P * 8));
    unsigned* trank = reinterpret_cast<unsigned*>(take((size_t)E1 * P * 4));
    unsigned char* kb = reinterpret_cast<unsigned char*>(take((size_t)E1 * N));
    char* state0 = ws + o;                                           // everything from here on starts as zeros
    RefineState st{};
    st.live = reinterpret_cast<int*>(take((size_t)S * 4));
    st.rounds = reinterpret_cast<int*>(take((size_t)S * 4));
    st.status = reinterpret_cast<int*>(take((size_t)S * 4));
    st.hits = reinterpret_cast<int*>(take((size_t)S * 4));
    st.exit_sum = reinterpret_cast<int*>(take((size_t)S * 4));
    st.start_hits = reinterpret_cast<int*>(take((size_t)S * 4));
    st.cost_sum = reinterpret_cast<unsigned long long*>(take((size_t)S * 8));
    st.start_cost_sum = reinterpret_cast<unsigned long long*>(take((size_t)S * 8));
    st.base = reinterpret_cast<unsigned long long*>(take((size_t)S * 24));
    st.acc_h = reinterpret_cast<int*>(take((size_t)S * M * 4));
    st.acc_x = reinterpret_cast<int*>(take((size_t)S * M * 4));
    st.acc_c = reinterpret_cast<unsigned long long*>(take((size_t)S * M * 8));
    (void)hipMemsetAsync(state0, 0, bytes - (size_t)(state0 - ws), s);
    double* table = a.table ? a.table : table_ws;
    launch_search_table(r.sorted, E1, N, P, pc, 1, table, trank, s);
    hipLaunchKernelGGL(refine_prep_kernel, dim3((N + 255) / 256, E1), dim3(256), 0, s, r.rec, trank, a.correct, E1, E1P, N, P, kb);
    const int se_grid = (S * E1 + 255) / 256;
    hipLaunchKernelGGL(refine_init_kernel, dim3(se_grid), dim3(256), 0, s, a.start, S, E1, P, a.digits, st);
    const size_t lds_delta = M * 16 + 24 + 64, lds_pick = M * 16 + 64 * (8 + 8 + 4 + 4 + 4);
    (void)ensure_dynamic_lds<&refine_delta_kernel>("refine_delta_kernel", 72 * 1024);
    (void)ensure_dynamic_lds<&refine_pick_kernel>("refine_pick_kernel", 72 * 1024);
    const dim3 delta_grid((N + kRefineChunk - 1) / kRefineChunk, S);
    for (int round = 0; round < a.max_rounds; ++round) {
        hipLaunchKernelGGL(refine_delta_kernel, delta_grid, dim3(256), lds_delta, s, kb, a.cost, a.digits, E1, N, P, st);
        hipLaunchKernelGGL(refine_pick_kernel, dim3(S), dim3(256), lds_pick, s, a.hit_value, a.budget, a.digits, E1, P, round, a.max_rounds, st);
    }
    hipLaunchKernelGGL(refine_finish_kernel, dim3(se_grid), dim3(256), 0, s, a.digits, table, S, E1, P, st, a.thresholds, a.hits, a.exit_sum, a.cost_sum,
                       a.rounds, a.status, a.start_hits, a.start_cost_sum);
    (void)hipFreeAsync(ws, s);
    return true;
}

}  // namespace mmee
