// The forward pass's exit stage: the exit heads' output projection, the criteria, the on-device exit decision (confidence test -> wavefront
// ballot -> prefix sum -> stream compaction of the document list), row-map expansion, and the CLS / padded hidden-state outputs.
//
// What this replaces in the reference:
//   * LayoutLMv3Exit.out_proj (EE/models/LayoutLMv3.py:92) / classifier.out_proj (HF:821) : head_out_kernel
//   * max_confidence / entropy criteria (EE/models/EE_modules.py:149-160), and the margin   : crit_f32 / crit_f64
//   * Policy.max_confidence_global_thresholding_policy / accuracy_calibration_heuristic (EE/policy.py:28-45, 87-104):
//     the nested Python loop "first exit whose float64 max-softmax is strictly above its threshold, else the last"
//     becomes exit_decide_kernel inside the forward pass: documents that satisfy the test are scattered to the
//     outputs and removed, deeper layers run on the survivors only.  (The same policy on a dumped array: exit_ops.hip.)
// All of it is HBM/latency-bound integer + small-vector work; none of it is shaped into a GEMM.
#include "mmee_kernels.h"
#include "ranked_common.h"

namespace mmee {

// ---------------------------------------------------------------------------------------------------------------
// out[i][c] = <in[row(i)], W[c]> + b[c]; one wave per document
// ---------------------------------------------------------------------------------------------------------------
// LTE (ee_config.use_lte): the same wave also scores its document, u = sigmoid(w . x + b) on the CLS row the exit's head reads (a second row
// source: the head of a 2-layer exit reads its dense layer's output here).  float64 throughout, in a fixed order: lane l adds its columns
// 4l + 256k + j in the order k, j; the lane sums go through one butterfly.  Nothing depends on which documents share the launch.  The
// LTE = false instantiation is the kernel as it was.
template <int WAVES, bool LTE>
__device__ __forceinline__ void head_out_body(const HeadOutArgs& a) {
    const int n = *a.n_docs_ptr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = blockIdx.x * WAVES + wave; i < n; i += gridDim.x * WAVES) {
        const int row = a.gather ? a.gather[i] : i;
        const float* x = a.in + (size_t)row * a.ld;
        f32x4 xv[kMaxNV];
#pragma unroll
        for (int k = 0; k < kMaxNV; ++k) {
            const int c = 4 * lane + 256 * k;
            xv[k] = (c < a.H) ? *reinterpret_cast<const f32x4*>(x + c) : f32x4{0, 0, 0, 0};
        }
        for (int o = 0; o < a.Ko; ++o) {
            const float* w = a.W + (size_t)o * a.H;
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < kMaxNV; ++k) {
                const int c = 4 * lane + 256 * k;
                if (c < a.H) {
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(w + c);
                    s += (xv[k][0] * wv[0] + xv[k][1] * wv[1]) + (xv[k][2] * wv[2] + xv[k][3] * wv[3]);
                }
            }
            s = wave_sum(s);
            if (lane == 0) a.out[(size_t)i * a.Ko + o] = s + a.b[o];
        }
        if constexpr (LTE) {
            const float* lx = a.lte_in + (size_t)(a.lte_gather ? a.lte_gather[i] : i) * a.lte_ld;
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < kMaxNV; ++k) {
                const int c = 4 * lane + 256 * k;
                if (c < a.H) {
                    const f32x4 v = a.lte_split_inv != 0.f ? load_split4(lx, c, a.lte_split_inv) : *reinterpret_cast<const f32x4*>(lx + c);
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(a.lte_w + c);
#pragma unroll
                    for (int j = 0; j < 4; ++j) t += (double)v[j] * (double)wv[j];
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
            if (lane == 0) a.lte_out[i] = 1.0 / (1.0 + exp(-(t + (double)a.lte_b[0])));
        }
    }
}

__global__ __launch_bounds__(256) void head_out_kernel(HeadOutArgs a) { head_out_body<4, false>(a); }
__global__ __launch_bounds__(256) void head_out_lte_kernel(HeadOutArgs a) { head_out_body<4, true>(a); }

void launch_head_out(const HeadOutArgs& a, int max_docs, hipStream_t s) {
    const int grid = grid_1d(max_docs, 4, 1024);
    if (a.lte_out) hipLaunchKernelGGL(head_out_lte_kernel, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(head_out_kernel, dim3(grid), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------------------------------------------
// criteria
// ---------------------------------------------------------------------------------------------------------------
// Margin (MMEE_CRIT_MARGIN; include/mmee.h): top-1 minus top-2 softmax probability, (1 - exp(m2 - m1)) / S with m1 the maximum, m2 the second
// largest value counting multiplicity and S = sum_k exp(x_k - m1) in label order.  m1 and S are the max-softmax's own two passes; m2 comes from a
// third pass that skips ONE label holding m1 (no exp inside it: the decide kernels sit at their register limit in the second pass, and a value
// kept live through it went to scratch).  K = 1: m2 = -inf, exp = 0, margin 1.
// float32, as the model computes exit_states[j][1] (EE/models/EE_modules.py:149-160): the criteria that are functions of a logits row
__device__ inline float crit_row_f32(const float* z, int K, int criterion) {
    if (criterion != CRIT_ENTROPY) {
        float m = z[0];
        for (int k = 1; k < K; ++k) m = fmaxf(m, z[k]);
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += expf(z[k] - m);
        if (criterion != CRIT_MARGIN) return 1.0f / s;
        float m2 = -INFINITY;
        bool seen = false;
        for (int k = 0; k < K; ++k) {
            const bool first = z[k] == m && !seen;
            seen = seen || first;
            m2 = first ? m2 : fmaxf(m2, z[k]);
        }
        return (1.0f - expf(m2 - m)) / s;
    }
    float A = 0.f, B = 0.f;                       // entropy: log(sum e^x) - sum(x e^x)/sum(e^x), no max shift
    for (int k = 0; k < K; ++k) {
        const float e = expf(z[k]);
        A += e;
        B += z[k] * e;
    }
    return logf(A) - B / A;
}

// crit_row_f32, and CRIT_GATE: z is the gate's two logits and the value the float64 gate score rounded once.  The LTE decide kernels call
// crit_row_f32 itself (use_lte and the gate criterion exclude each other: ee_create), and stay the code they were
__device__ inline float crit_f32(const float* z, int K, int criterion) {
    return criterion == CRIT_GATE ? (float)gate_score_f64(z[0], z[1]) : crit_row_f32(z, K, criterion);
}

// float64 on (double)logit / T, as the policy computes it (scipy.special.softmax on the float64 store, EE/policy.py:30-32).  CRIT_GATE: the
// max-softmax, which is what a gate handle reports where there is no gate (the final exit); the gate score itself takes no temperature and
// is gate_score_f64 on the head's logits (exit_decide_body)
__device__ inline double crit_f64(const float* z, int K, double temp, int criterion) {
    if (criterion != CRIT_ENTROPY) {
        double m = (double)z[0] / temp;
        for (int k = 1; k < K; ++k) m = fmax(m, (double)z[k] / temp);
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += exp((double)z[k] / temp - m);
        if (criterion != CRIT_MARGIN) return 1.0 / s;
        double m2 = -INFINITY;
        bool seen = false;
        for (int k = 0; k < K; ++k) {
            const double x = (double)z[k] / temp;
            const bool first = x == m && !seen;
            seen = seen || first;
            m2 = first ? m2 : fmax(m2, x);
        }
        return (1.0 - exp(m2 - m)) / s;
    }
    double A = 0.0, B = 0.0;
    for (int k = 0; k < K; ++k) {
        const double x = (double)z[k] / temp;
        const double e = exp(x);
        A += e;
        B += x * e;
    }
    return log(A) - B / A;
}

// ---------------------------------------------------------------------------------------------------------------
// The exit stage: one workgroup of 1024 threads walks the active documents in chunks of 1024.
//   thread <-> document: criterion (f64), exit test, scatter of leavers to the output arrays;
//   survivors: wave ballot -> popcount prefix -> cross-wave prefix in LDS -> running carry = new dense index,
//   and the same scan over row counts = new dense row offset.
// PATIENCE (PABEE, MMEE_CRIT_PATIENCE): the exit test is "the argmax of the scaled logits has stayed the same for t exits in a row"
// instead of a threshold test.  The criterion written to the outputs is the max-softmax; the run state of document `orig` is
// (p.prev[orig], p.run[orig]), indexed by the original slot so that compaction never moves it, and written unconditionally at
// exit 0, which every document reaches (no reset launch).
// LTE (ee_config.use_lte): the test is "the float64 score head_out_lte_kernel left in a.lte_score is strictly below the threshold"; the score
// is what the outputs carry as the criterion.  Embedding exits have no score (a.lte_score null): 1.0, nobody leaves.
// The max_confidence / entropy / margin kernel is the DECIDE_THRESHOLD instantiation.
// GATE (MMEE_CRIT_GATE; gate strategy, DECIDE_THRESHOLD): below the final exit the criterion is the gate score of a.head_logits (Kh == 2),
// g = gate_score_f64(h0, h1), the test g > thr; what leaves is still the scaled row of a.pol_logits.  The final exit has no gate: the max-softmax.
// RULE (ee_set_exit_rule; THRESHOLD and LTE modes): the mode's test is the EVENT f_e and the rule decides on it.  MMEE_RULE_STREAK: the event
// must have held at t_e exits in a row (s_e = f_e ? s_{e-1} + 1 : 0 in p.run[orig]).  MMEE_RULE_EITHER: the event, or PABEE's counter
// c_e >= t_e ((p.prev[orig], p.run[orig]) exactly as under PATIENCE).  The same state arrays, written unconditionally at exit 0; t_e is the
// launch's own patience (by value, or at p.t_ptr[0]: the host hands every exit its own entry).  RULE_PLAIN compiles to the kernels as they were.
// QUOTA (ee_set_quotas; DECIDE_THRESHOLD with RULE_PLAIN only): the criterion is the one exit_quota_crit_kernel left in q.crit -- the value this
// kernel's own branches below would compute, the gate score under CRIT_GATE -- and the test is on q.rank, the document's place among the stage's
// documents: QUOTA_EXACT rank < q_e, QUOTA_AT_LEAST the threshold test or rank < q_e.  Everything below the `leave` line is shared.  QUOTA_OFF
// compiles to the kernels as they were.
// AUDIT (ee_set_audit; definition in include/mmee.h): a document whose decision is `leave` and that audit_selected picks gets its result as
// always, is marked au.delivered[orig] = 1 and is KEPT; a delivered document decides nothing any more -- it stays until the final exit, writes
// no out_logits / out_exit / out_conf there or anywhere, and still writes its out_all_* / out_head_* rows and its patience / streak state like
// any active document, because everything above the `leave` line runs for it unchanged.  au.delivered is by original slot and is written, not
// read, at exit 0, which every document reaches (no reset launch).  AUDIT = false compiles to the kernels as they were.
// ---------------------------------------------------------------------------------------------------------------
// PABEE's counter: argmax of the scaled logits as they are written out (two f32 logits can round to one scaled value; first maximum wins),
// c_e = the argmax equals the one at the previous exit ? c_{e-1} + 1 : 0, state by original slot
__device__ __forceinline__ int agreement_run(const float* z, int K, double temp, int exit_index, int orig, const PatienceArgs& p) {
    float best = (float)((double)z[0] / temp);
    int am = 0;
    for (int k = 1; k < K; ++k) {
        const float v = (float)((double)z[k] / temp);
        if (v > best) { best = v; am = k; }
    }
    const int run = (exit_index > 0 && p.prev[orig] == am) ? p.run[orig] + 1 : 0;
    p.prev[orig] = am;
    p.run[orig] = run;
    return run;
}

template <int MODE, int RULE = RULE_PLAIN, int QUOTA = QUOTA_OFF, bool AUDIT = false>
__device__ __forceinline__ void exit_decide_body(const DecideArgs& a, const PatienceArgs& p, const QuotaArgs& q = QuotaArgs{}, const AuditArgs& au = AuditArgs{}) {
    constexpr bool PATIENCE = MODE == DECIDE_PATIENCE;
    static_assert(!AUDIT || QUOTA == QUOTA_OFF, "a rank would count the shadows: n_{e+1} would no longer be n_e - q_e");
    static_assert(RULE == RULE_PLAIN || !PATIENCE, "PABEE has no threshold event to build a rule on");
    static_assert(QUOTA == QUOTA_OFF || (MODE == DECIDE_THRESHOLD && RULE == RULE_PLAIN), "a rank is defined for the threshold criteria under the plain rule");
    __shared__ int s_cnt[16], s_rows[16];
    __shared__ unsigned long long s_sq[16];
    __shared__ int s_carry_docs, s_carry_rows;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.counts->n_docs;
    const double thr = a.thr_ptr ? a.thr_ptr[a.exit_index] : a.thr;
    const double temp = a.temp_ptr ? a.temp_ptr[a.exit_index] : a.temp;
    int patience = 0;
    if constexpr (PATIENCE || RULE != RULE_PLAIN) patience = p.t_ptr ? (int)p.t_ptr[0] : p.t;
    int quota = 0;
    if constexpr (QUOTA != QUOTA_OFF) quota = q.q_ptr ? (int)q.q_ptr[0] : q.q;
    if (tid == 0) { s_carry_docs = 0; s_carry_rows = 0; }
    unsigned long long sq = 0;
    __syncthreads();
    for (int base = 0; base < n; base += 1024) {
        const int i = base + tid;
        const bool active = i < n;
        bool keep = false;
        int len = 0, orig = 0;
        if (active) {
            orig = a.doc_orig[i];
            len = a.doc_off[i + 1] - a.doc_off[i];
            const float* z = a.pol_logits + (size_t)i * a.K;
            double crit;
            bool leave;
            if constexpr (QUOTA != QUOTA_OFF) {
                crit = q.crit[i];
                leave = q.rank[i] < quota;
                if constexpr (QUOTA == QUOTA_AT_LEAST) leave = leave || crit_fires(a.criterion, crit, thr);      // strict, as below
            } else if constexpr (PATIENCE) {
                crit = crit_f64(z, a.K, temp, CRIT_MAX_CONFIDENCE);
                leave = agreement_run(z, a.K, temp, a.exit_index, orig, p) >= patience;
            } else if constexpr (MODE == DECIDE_LTE) {
                crit = a.lte_score ? a.lte_score[i] : 1.0;
                leave = a.lte_score && crit < thr;                        // strict, EE/models/LayoutLMv3.py:262
            } else if (a.criterion == CRIT_GATE && !a.is_final && a.head_logits) {
                const float* hz = a.head_logits + (size_t)i * a.Kh;      // the decision reads the two gate logits and nothing else
                crit = gate_score_f64(hz[0], hz[1]);
                leave = crit_fires(CRIT_GATE, crit, thr);                 // strict
            } else {
                crit = crit_f64(z, a.K, temp, a.criterion);
                leave = crit_fires(a.criterion, crit, thr);               // strict, EE/policy.py:33
            }
            if constexpr (RULE == RULE_STREAK) {
                const int streak = leave ? (a.exit_index > 0 ? p.run[orig] : 0) + 1 : 0;
                p.run[orig] = streak;
                leave = streak >= patience;
            } else if constexpr (RULE == RULE_EITHER) {
                const bool agreed = agreement_run(z, a.K, temp, a.exit_index, orig, p) >= patience;
                leave = leave || agreed;
            }
            if (a.no_exit) leave = false;
            if (a.is_final) leave = true;
            if (a.out_all_logits) {
                float* o = a.out_all_logits + ((size_t)a.exit_index * a.B + orig) * a.K;
                for (int k = 0; k < a.K; ++k) o[k] = (float)((double)z[k] / temp);
            }
            if (a.out_all_crit) a.out_all_crit[(size_t)a.exit_index * a.B + orig] = (float)crit;
            if (a.head_logits && a.out_head_logits) {
                const float* hz = a.head_logits + (size_t)i * a.Kh;
                float* o = a.out_head_logits + ((size_t)a.exit_index * a.B + orig) * a.Kh;
                for (int k = 0; k < a.Kh; ++k) o[k] = hz[k];
            }
            if (a.head_logits && a.out_head_crit) {
                const float* hz = a.head_logits + (size_t)i * a.Kh;
                float hc;
                if constexpr (MODE == DECIDE_THRESHOLD) hc = crit_f32(hz, a.Kh, a.criterion);
                else hc = crit_row_f32(hz, a.Kh, PATIENCE ? CRIT_MAX_CONFIDENCE : a.criterion);
                a.out_head_crit[(size_t)a.exit_index * a.B + orig] = hc;
            }
            bool shadow = false;                                          // AUDIT: the document's result is out and it stays in the batch
            if constexpr (AUDIT) {
                const bool was = a.exit_index > 0 && au.delivered[orig] != 0;
                shadow = was || (leave && !a.is_final && audit_selected(au.cut, au.seed, (int)((unsigned)orig + (unsigned)au.slot_base)));
                if (a.exit_index == 0 || shadow != was) au.delivered[orig] = shadow ? 1 : 0;
                leave = leave && !was;                                    // a delivered document writes no result again, the final exit included
            }
            if (leave) {
                if (a.out_logits)
                    for (int k = 0; k < a.K; ++k) a.out_logits[(size_t)orig * a.K + k] = (float)((double)z[k] / temp);
                a.out_exit[orig] = a.exit_index;
                if (a.out_conf) a.out_conf[orig] = (float)crit;
            }
            keep = !leave;
            if constexpr (AUDIT) keep = !a.is_final && (keep || shadow);
        }
        // ---- wavefront ballot + prefix sums ------------------------------------------------------------------
        const unsigned long long ballot = __ballot(keep);
        const int before = __popcll(ballot & ((1ull << lane) - 1ull));       // survivors in lower lanes
        const int klen = keep ? len : 0;
        const int rows_incl = wave_incl_scan(klen, lane);
        if (lane == 63) { s_cnt[wave] = __popcll(ballot); s_rows[wave] = rows_incl; }
        if (keep) sq += (unsigned long long)len * (unsigned long long)len;
        __syncthreads();
        int wdocs = 0, wrows = 0, tdocs = 0, trows = 0;
        for (int w = 0; w < 16; ++w) {
            if (w < wave) { wdocs += s_cnt[w]; wrows += s_rows[w]; }
            tdocs += s_cnt[w];
            trows += s_rows[w];
        }
        const int cd = s_carry_docs, cr = s_carry_rows;
        if (keep) {
            const int k = cd + wdocs + before;
            a.n_doc_orig[k] = orig;
            a.n_doc_off[k] = cr + wrows + rows_incl - len;
            a.n_x_src[k] = a.x_phys[i];
            a.n_meta_src[k] = a.doc_off[i];
        }
        __syncthreads();
        if (tid == 0) { s_carry_docs = cd + tdocs; s_carry_rows = cr + trows; }
        __syncthreads();
    }
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
    if (lane == 0) s_sq[wave] = sq;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < 16; ++w) t += s_sq[w];
        a.n_doc_off[s_carry_docs] = s_carry_rows;
        a.n_counts->n_docs = s_carry_docs;
        a.n_counts->n_rows = s_carry_rows;
        a.n_counts->sum_len_sq = t;
    }
}

__global__ __launch_bounds__(1024) void exit_decide_kernel(DecideArgs a) { exit_decide_body<DECIDE_THRESHOLD>(a, PatienceArgs{}); }
__global__ __launch_bounds__(1024) void exit_decide_patience_kernel(DecideArgs a, PatienceArgs p) { exit_decide_body<DECIDE_PATIENCE>(a, p); }
__global__ __launch_bounds__(1024) void exit_decide_lte_kernel(DecideArgs a) { exit_decide_body<DECIDE_LTE>(a, PatienceArgs{}); }
__global__ __launch_bounds__(1024) void exit_decide_streak_kernel(DecideArgs a, PatienceArgs p) { exit_decide_body<DECIDE_THRESHOLD, RULE_STREAK>(a, p); }
__global__ __launch_bounds__(1024) void exit_decide_either_kernel(DecideArgs a, PatienceArgs p) { exit_decide_body<DECIDE_THRESHOLD, RULE_EITHER>(a, p); }
__global__ __launch_bounds__(1024) void exit_decide_lte_streak_kernel(DecideArgs a, PatienceArgs p) { exit_decide_body<DECIDE_LTE, RULE_STREAK>(a, p); }
__global__ __launch_bounds__(1024) void exit_decide_lte_either_kernel(DecideArgs a, PatienceArgs p) { exit_decide_body<DECIDE_LTE, RULE_EITHER>(a, p); }

__global__ __launch_bounds__(1024) void exit_decide_quota_exact_kernel(DecideArgs a, QuotaArgs q) { exit_decide_body<DECIDE_THRESHOLD, RULE_PLAIN, QUOTA_EXACT>(a, PatienceArgs{}, q); }
__global__ __launch_bounds__(1024) void exit_decide_quota_at_least_kernel(DecideArgs a, QuotaArgs q) { exit_decide_body<DECIDE_THRESHOLD, RULE_PLAIN, QUOTA_AT_LEAST>(a, PatienceArgs{}, q); }

// the AUDIT forms of the seven kernels above: one signature, the stateless ones ignore their PatienceArgs
#define MMEE_DECIDE_AUDIT_KERNEL(name, ...)                                                                  \
    __global__ __launch_bounds__(1024) void name(DecideArgs a, PatienceArgs p, AuditArgs au) {              \
        exit_decide_body<__VA_ARGS__, QUOTA_OFF, true>(a, p, QuotaArgs{}, au);                               \
    }
MMEE_DECIDE_AUDIT_KERNEL(exit_decide_audit_kernel, DECIDE_THRESHOLD, RULE_PLAIN)
MMEE_DECIDE_AUDIT_KERNEL(exit_decide_patience_audit_kernel, DECIDE_PATIENCE, RULE_PLAIN)
MMEE_DECIDE_AUDIT_KERNEL(exit_decide_lte_audit_kernel, DECIDE_LTE, RULE_PLAIN)
MMEE_DECIDE_AUDIT_KERNEL(exit_decide_streak_audit_kernel, DECIDE_THRESHOLD, RULE_STREAK)
MMEE_DECIDE_AUDIT_KERNEL(exit_decide_either_audit_kernel, DECIDE_THRESHOLD, RULE_EITHER)
MMEE_DECIDE_AUDIT_KERNEL(exit_decide_lte_streak_audit_kernel, DECIDE_LTE, RULE_STREAK)
MMEE_DECIDE_AUDIT_KERNEL(exit_decide_lte_either_audit_kernel, DECIDE_LTE, RULE_EITHER)
#undef MMEE_DECIDE_AUDIT_KERNEL

// mode: DECIDE_*, rule: RULE_PLAIN / _STREAK / _EITHER.  The plain threshold and LTE kernels keep no state and take no PatienceArgs (p may be null).
// audit: null launches the kernels as they always were; an audited call (never a dump-all one: the callers see to it) passes its AuditArgs
void launch_decide(const DecideArgs& a, const PatienceArgs* p, int mode, int rule, hipStream_t s, const AuditArgs* audit) {
    using Plain = void (*)(DecideArgs);
    using Stateful = void (*)(DecideArgs, PatienceArgs);
    if (audit) {
        using Audited = void (*)(DecideArgs, PatienceArgs, AuditArgs);
        static const Audited audited[3][3] = {{exit_decide_audit_kernel, exit_decide_streak_audit_kernel, exit_decide_either_audit_kernel},
                                              {exit_decide_patience_audit_kernel, nullptr, nullptr},
                                              {exit_decide_lte_audit_kernel, exit_decide_lte_streak_audit_kernel, exit_decide_lte_either_audit_kernel}};
        hipLaunchKernelGGL(audited[mode][rule], dim3(1), dim3(1024), 0, s, a, p ? *p : PatienceArgs{}, *audit);
        return;
    }
    static const Plain plain[3] = {exit_decide_kernel, nullptr, exit_decide_lte_kernel};
    static const Stateful stateful[3][3] = {{nullptr, exit_decide_streak_kernel, exit_decide_either_kernel},
                                            {exit_decide_patience_kernel, nullptr, nullptr},
                                            {nullptr, exit_decide_lte_streak_kernel, exit_decide_lte_either_kernel}};
    if (plain[mode] && rule == RULE_PLAIN) hipLaunchKernelGGL(plain[mode], dim3(1), dim3(1024), 0, s, a);
    else hipLaunchKernelGGL(stateful[mode][rule], dim3(1), dim3(1024), 0, s, a, *p);
}

// ---------------------------------------------------------------------------------------------------------------
// Budgeted exits (ee_set_quotas; definition in include/mmee.h): the ranking step, two launches between an exit's head (or ensemble launch) and
// its decision.  exit_quota_crit_kernel: one thread per active document, c_i by the expressions of exit_decide_body<DECIDE_THRESHOLD> into the
// stage scratch.  exit_quota_rank_kernel: 256 documents per workgroup, the whole stage tiled through LDS as keys (quota_key) and original
// slots, rank_i by counting (quota_rank_by_counting) -- O(n^2) compares over ceil(n / 256) workgroups, integers only, so the ranks are the same
// bits whatever the grid.  The grid is sized by the call's static document count; a workgroup past the stage's n_docs returns before any barrier.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void exit_quota_crit_kernel(DecideArgs a, QuotaArgs q) {
    const int n = a.counts->n_docs;
    const double temp = a.temp_ptr ? a.temp_ptr[a.exit_index] : a.temp;
    const bool gate = a.criterion == CRIT_GATE && !a.is_final && a.head_logits;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        double crit;
        if (gate) {
            const float* hz = a.head_logits + (size_t)i * a.Kh;
            crit = gate_score_f64(hz[0], hz[1]);
        } else {
            crit = crit_f64(a.pol_logits + (size_t)i * a.K, a.K, temp, a.criterion);
        }
        q.crit[i] = crit;
    }
}

__global__ __launch_bounds__(256) void exit_quota_rank_kernel(DecideArgs a, QuotaArgs q) {
    __shared__ unsigned long long t_key[2048];
    __shared__ int t_slot[2048];
    const int n = a.counts->n_docs;
    if ((int)blockIdx.x * 256 >= n) return;                                // the same for every thread of the workgroup
    const int i = blockIdx.x * 256 + threadIdx.x;
    const double sign = crit_sign(a.criterion);
    const double* crit = q.crit;
    const int* orig = a.doc_orig;
    const unsigned long long key = i < n ? quota_key(crit[i], sign) : 0ull;
    const int slot = i < n ? orig[i] : 0;
    const unsigned r = quota_rank_by_counting(key, slot, n, [&](int j) { return quota_key(crit[j], sign); }, [&](int j) { return orig[j]; }, t_key, t_slot);
    if (i < n) q.rank[i] = (int)r;
}

void launch_exit_quota_crit(const DecideArgs& a, const QuotaArgs& q, int max_docs, hipStream_t s) {
    hipLaunchKernelGGL(exit_quota_crit_kernel, dim3(grid_1d(max_docs, 256, 1024)), dim3(256), 0, s, a, q);
}

void launch_exit_quota_rank(const DecideArgs& a, const QuotaArgs& q, int max_docs, hipStream_t s) {
    hipLaunchKernelGGL(exit_quota_rank_kernel, dim3((max_docs + 255) / 256), dim3(256), 0, s, a, q);
}

void launch_decide_quota(const DecideArgs& a, const QuotaArgs& q, int quota_mode, hipStream_t s) {
    if (quota_mode == QUOTA_EXACT) hipLaunchKernelGGL(exit_decide_quota_exact_kernel, dim3(1), dim3(1024), 0, s, a, q);
    else hipLaunchKernelGGL(exit_decide_quota_at_least_kernel, dim3(1), dim3(1024), 0, s, a, q);
}

// ---------------------------------------------------------------------------------------------------------------
// The exit ensemble (ee_set_ensemble; definition in include/mmee.h): a launch of its own between an exit's head and its decision, because the
// decide kernels sit at their register limit (above).  One thread per (active document, label): it walks its document's K logits for the
// row's maximum and sum itself (K <= 64 values one wave shares through the cache; nothing to reduce across lanes, so the sum is in label
// order), writes l_m[k] to the state row of the document's ORIGINAL slot -- compaction never moves it, and every exit a document reaches
// rewrites its row, so no launch resets it -- and combines the rows 0 .. m-1 that earlier launches left with its own l_m.  Lanes of a
// document read consecutive doubles of every state row.  Latency-bound integer and small-vector work, like decide.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void exit_ensemble_kernel(EnsembleArgs a) {
    const int n = a.counts->n_docs, K = a.K, m = a.exit_index;
    const double temp = a.temp_ptr ? a.temp_ptr[m] : a.temp;
    const double* w_row = a.w + (size_t)m * a.E1;
    const size_t slab = (size_t)a.B * K;                                   // one exit's rows of the state
    const long long total = (long long)n * K;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const int i = (int)(t / K), k = (int)(t - (long long)i * K);
        const float* z = a.pol_logits + (size_t)i * K;
        const size_t slot = (size_t)a.doc_orig[i] * K + k;
        const double l = ens_logsoftmax_f64([&](int j) { return (double)(float)((double)z[j] / temp); }, K, k);
        a.state[(size_t)m * slab + slot] = l;
        const double* st = a.state;
        const double y = ens_combine_f64(w_row, a.b ? a.b[(size_t)m * K + k] : 0.0, m, [&](int j) { return j == m ? l : st[(size_t)j * slab + slot]; });
        a.out[(size_t)i * K + k] = (float)y;
    }
}

void launch_exit_ensemble(const EnsembleArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(exit_ensemble_kernel, dim3(grid_1d((long long)a.B * a.K, 256, 1024)), dim3(256), 0, s, a);
}

// Round 6: the head's output projection and the decision were built as ONE launch (every workgroup writes its documents' logits, fences,
// takes a ticket; the last arrival runs the scan: nobody waits, same bits, 91 GPU tests green) and measured on config 3 (2 x 512 documents, 48 exits per step):
// 52.7 us per exit against 31 + 16 us for the two launches -- the fences and the serial scan behind the last arrival cost what the launch saved.  Removed.

// new dense row r of surviving document k  <-  physical X row n_x_src[k] + t, metadata row n_meta_src[k] + t
__global__ __launch_bounds__(256) void compact_rows_kernel(const StageCounts* n_counts, const int* __restrict__ n_doc_off,
                                                           const int* __restrict__ n_x_src, const int* __restrict__ n_meta_src,
                                                           const RowMeta* __restrict__ meta_old, RowMeta* __restrict__ meta_new,
                                                           int* __restrict__ row_src) {
    const int n = n_counts->n_docs;
    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        const int off = n_doc_off[k], len = n_doc_off[k + 1] - off;
        const int xs = n_x_src[k], ms = n_meta_src[k];
        for (int t = threadIdx.x; t < len; t += 256) {
            row_src[off + t] = xs + t;
            meta_new[off + t] = meta_old[ms + t];
        }
    }
}

void launch_compact_rows(const StageCounts* n_counts, const int* n_doc_off, const int* n_x_src, const int* n_meta_src,
                         const RowMeta* meta_old, RowMeta* meta_new, int* row_src, int max_docs, int num_cus, hipStream_t s) {
    hipLaunchKernelGGL(compact_rows_kernel, dim3(grid_1d(max_docs, 1, num_cus * 8)), dim3(256), 0, s, n_counts, n_doc_off, n_x_src, n_meta_src,
                       meta_old, meta_new, row_src);
}

// out[orig][:] = X[x_phys[i]][:]   (CLS rows, parity/debug output)
// CLS row of every active document -> out[doc_orig ? doc_orig[i] : i].  split_inv != 0: X holds split-f16 rows (1 / scale = split_inv)
__global__ __launch_bounds__(256) void gather_cls_kernel(const float* __restrict__ X, int H, const int* __restrict__ x_phys,
                                                         const int* __restrict__ doc_orig, const int* __restrict__ n_docs_ptr,
                                                         float* __restrict__ out, float split_inv) {
    const int n = *n_docs_ptr;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const float* src = X + (size_t)x_phys[i] * H;
        float* dst = out + (size_t)(doc_orig ? doc_orig[i] : i) * H;
        if (split_inv != 0.f) {
            for (int c = 4 * threadIdx.x; c < H; c += 1024) *reinterpret_cast<f32x4*>(dst + c) = load_split4(src, c, split_inv);
        } else {
            for (int c = threadIdx.x; c < H; c += 256) dst[c] = src[c];
        }
    }
}

// Hidden states in the reference's padded layout (ee_set_hidden_states_out): position p of document d is text token p (packed row
// text_dst[d * T + p], < 0 when the ragged layout dropped it: zeros) or visual row p - T (packed behind the document's ntext[d] text rows).
__global__ __launch_bounds__(256) void rows_to_padded_kernel(const float* __restrict__ X, float split_inv, int H, int B, int T, int Pv,
                                                             const int* __restrict__ text_dst, const int* __restrict__ ntext,
                                                             const int* __restrict__ doc_off, float* __restrict__ out) {
    const int S = T + Pv;
    for (long r = blockIdx.x; r < (long)B * S; r += gridDim.x) {
        const int d = (int)(r / S), p = (int)(r - (long)d * S);
        int row;
        if (p < T) {
            const int t = text_dst[(size_t)d * T + p];
            row = t < 0 ? -1 : doc_off[d] + t;
        } else {
            row = doc_off[d] + (text_dst ? ntext[d] : 0) + (p - T);
        }
        float* dst = out + (size_t)r * H;
        if (row < 0) {
            for (int c = threadIdx.x; c < H; c += 256) dst[c] = 0.f;
        } else if (split_inv != 0.f) {
            const float* src = X + (size_t)row * H;
            for (int c = 4 * threadIdx.x; c < H; c += 1024) *reinterpret_cast<f32x4*>(dst + c) = load_split4(src, c, split_inv);
        } else {
            const float* src = X + (size_t)row * H;
            for (int c = threadIdx.x; c < H; c += 256) dst[c] = src[c];
        }
    }
}
void launch_rows_to_padded(const float* X, float split_inv, int H, int B, int T, int Pv, const int* text_dst, const int* ntext, const int* doc_off,
                           float* out, hipStream_t s) {
    hipLaunchKernelGGL(rows_to_padded_kernel, dim3(grid_1d((long)B * (T + Pv), 1, 4096)), dim3(256), 0, s, X, split_inv, H, B, T, Pv, text_dst, ntext, doc_off, out);
}

void launch_gather_cls(const float* X, int H, const int* x_phys, const int* doc_orig, const int* n_docs_ptr, float* out,
                       int max_docs, hipStream_t s, float split_inv) {
    hipLaunchKernelGGL(gather_cls_kernel, dim3(grid_1d(max_docs, 1, 2048)), dim3(256), 0, s, X, H, x_phys, doc_orig, n_docs_ptr, out, split_inv);
}

}  // namespace mmee
