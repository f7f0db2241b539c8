// Parameter blocks + launchers of the row kernels (prep_embed.hip), the forward pass's exit stage (exit_stage.hip) and the handle-free
// tools on dumped arrays (exit_ops.hip).
#pragma once
#include "mmee_common.h"

namespace mmee {

struct PrepArgs {
    const long long* input_ids;      // (B,T)
    const long long* attention_mask; // (B,T) or null
    const long long* bbox;           // (B,T,4)
    const long long* position_ids;   // (B,T) or null
    const long long* token_type_ids; // (B,T) or null (range check only; the embedding kernel reads them)
    int B, T, Pv, G;
    int pad_id, vocab, max_2d, max_pos, type_vocab;
    int dense_rows;
    // outputs
    int* text_dst;                   // (B,T) row index inside the document, -1 = dropped pad row
    int* emb_pos;                    // (B,T) position id for the position-embedding lookup
    int* ntext;                      // (B)   kept text rows
    int* doc_off;                    // (B+1) stage-0 dense offsets
    int* x_src;                      // (B)   physical offsets (= doc_off at stage 0)
    int* doc_orig;                   // (B)
    RowMeta* meta;
    StageCounts* counts;
    int* err_flag;                   // bit0 token id, bit1 bbox, bit2 position id, bit3 token_type id out of range
};

struct EmbedArgs {
    const long long* input_ids;
    const long long* token_type_ids; // or null
    const long long* bbox;
    const int* emb_pos;
    const int* text_dst;
    const int* ntext;
    const int* doc_off;
    int B, T, Pv, H, cs, ss, max_2d, vocab, type_vocab;
    const float *word, *type, *pos, *xtab, *ytab, *htab, *wtab;
    const float* inputs_embeds;      // (B,T,H) or null: read in place of word[input_ids] (ee_set_inputs_embeds)
    const float *ln1_g, *ln1_b;      // text: embeddings.LayerNorm; visual: layoutlmv3.norm
    float eps1;
    const float *ln2_g, *ln2_b;      // layoutlmv3.LayerNorm
    float eps2;
    const float *cls_token, *pos_embed, *vis_raw;
    float* X;
    void* Xs;                        // when given, the rows are written as split-f16 planes (x split_scale) here and X is not written
    float split_scale;
    int* err_flag;                   // Xs: kErrSplitOverflow
    float* text_part;                // (B, ceil(T/32), H) or null
    float* vis_part;                 // (B, ceil(Pv/32), H) or null
    float* cat_part;                 // (B, cat_chunks, H) or null; text chunks first, then visual chunks
    int cat_chunks;
};

// vision_pool_kernel (vision_first.hip): the visual rows up to layoutlmv3.norm and their partial column sums, nothing stored besides
struct VisionPoolArgs {
    const float *vis_raw, *cls_token, *pos_embed;      // [B][Pv - 1][H], [H], [Pv][H]
    const float *ln_g, *ln_b;                          // layoutlmv3.norm
    float eps;
    int B, Pv, H;
    float* vis_part;                                   // (B, ceil(Pv/32), H)
};

struct HeadOutArgs {
    const float* in;                 // rows of length H
    int ld;
    const int* gather;               // optional: input row of active doc i is in[gather[i]]
    const float* W;                  // [Ko][H]
    const float* b;                  // [Ko]
    int H, Ko;
    const int* n_docs_ptr;
    float* out;                      // [n_docs][Ko]
    // learning-to-exit (ee_config.use_lte): a second row source and one more output, walked by the same wave.  lte_out null: no score
    const float* lte_in;             // CLS rows the exit's head reads: f32 rows, or split-f16 planes when lte_split_inv != 0
    int lte_ld;
    const int* lte_gather;           // optional: the row of active doc i is lte_in[lte_gather[i]]
    float lte_split_inv;             // 1 / plane scale of split rows; 0: f32 rows
    const float* lte_w;              // [H]  encoder.lte_classifier.weight
    const float* lte_b;              // [1]
    double* lte_out;                 // [n_docs] u = sigmoid(w . x + b), float64
};

// thresholds, then temperatures, then the per-exit patience, then the quotas, of one ee_graph_launch: a kernel ARGUMENT of set_thresholds_kernel (no host buffer has to outlive the call)
struct ThrPack {
    double v[4 * (64 + 4)];          // 4 x (MMEE_MAX_ENCODER_EXITS + 3 embedding exits + final): thresholds, temperatures, per-exit patience, quotas
    int n;
};

struct DecideArgs {
    const float* pol_logits;         // [n_docs][K]   logits the policy sees (ramp: head logits; gate: classifier(gate input))
    const float* head_logits;        // [n_docs][Kh]  raw exit-head logits (== pol_logits for ramps); null for the final stage.  CRIT_GATE: the two
                                     // gate logits the decision reads (Kh == 2), and nothing else
    int K, Kh;
    double thr, temp;
    const double* thr_ptr;           // captured-graph forwards (ee_graph_capture): threshold / temperature of exit e at [exit_index] of device
    const double* temp_ptr;          // vectors refreshed in front of every replay; null: the by-value arguments above
    int criterion, is_final, no_exit, exit_index, B;
    const double* lte_score;         // LTE decide kernel: [n_docs] float64 scores of this exit; null (embedding exits): score 1, nobody leaves
    // current stage
    const StageCounts* counts;
    const int* doc_orig;
    const int* doc_off;              // dense offsets (n_docs + 1)
    const int* x_phys;               // physical X offsets of the current stage's documents
    // next stage
    StageCounts* n_counts;
    int* n_doc_orig;
    int* n_doc_off;
    int* n_x_src;
    int* n_meta_src;
    // outputs (original document numbering)
    float* out_logits;               // (B,K)
    int* out_exit;                   // (B)
    float* out_conf;                 // (B)
    float* out_all_logits;           // (E+1,B,K)
    float* out_all_crit;             // (E+1,B)
    float* out_head_logits;          // (E,B,Kh)
    float* out_head_crit;            // (E,B)
};

// patience (MMEE_CRIT_PATIENCE, MMEE_RULE_STREAK, MMEE_RULE_EITHER): the decide kernel's second argument
struct PatienceArgs {
    int t;                           // THIS exit's patience t_e: exit once the argmax has stayed the same (STREAK: the event has held) for t exits in a row
    const double* t_ptr;             // captured-graph forwards: t_e at [0] (the host points it at this exit's entry of the device vector every
                                     // ee_graph_launch refreshes); null: `t`
    int* prev;                       // [max_docs] argmax at the document's previous exit, by original slot
    int* run;                        // [max_docs] run counter c_e (MMEE_RULE_STREAK: the streak s_e), by original slot
};

// result stream (MMEE_FLAG_STREAM_RESULTS; result_stream.hip): the launch behind an exit's decide launch
struct EmitArgs {
    // the stage that reached the exit, and the stage of the documents that stay (n_doc_orig null: the final exit, everybody leaves)
    const StageCounts* counts;
    const int* doc_orig;
    const StageCounts* n_counts;
    const int* n_doc_orig;
    // what the decide launch wrote, by original slot
    const float* out_logits;         // (B,K)
    const int* out_exit;             // (B)
    const float* out_conf;           // (B)
    int K, exit_index;
    int cap;                         // rows the segment buffer holds (max_docs): nothing is stored past it
    int* done;                       // device word: leavers of the exits before this one (read at exit_index > 0, rewritten by every launch)
    int* rows;                       // host-visible [cap][K + 3]: logit bit patterns, exit index, confidence bit pattern, original slot
    int* cum;                        // host-visible [E + 1]: leavers through exit e
};

// ee_config.criterion (include/mmee.h MMEE_CRIT_*; capi_internal.h asserts the values agree)
enum { CRIT_MAX_CONFIDENCE = 0, CRIT_ENTROPY = 1, CRIT_PATIENCE = 2, CRIT_MARGIN = 3, CRIT_GATE = 4 };
// the direction of a threshold criterion: max-softmax, margin and the gate score leave on crit > thr, entropy on crit < thr; strict, so a NaN never fires
// sign_fires is THE test: the decide kernels reach it through crit_fires, the controller's replay (rolling_control_kernel) by the table's sign
__host__ __device__ inline double crit_sign(int criterion) { return criterion == CRIT_ENTROPY ? -1.0 : 1.0; }
__host__ __device__ inline bool sign_fires(double sign, double c, double thr) { return sign < 0.0 ? c < thr : c > thr; }
__host__ __device__ inline bool crit_fires(int criterion, double crit, double thr) { return sign_fires(crit_sign(criterion), crit, thr); }
// The gate score (MMEE_CRIT_GATE; include/mmee.h): the 2-way softmax's probability of column 1 ("correctly gated") of the raw float32 gate
// logits, in float64.  h0 - h1 large: exp overflows to inf and the score is exactly 0; large negative: exactly 1; equal: exactly 0.5.  The one
// copy the decide kernels (exit_stage.hip) and the table kernel of the dumped-array tools (exit_ops.hip) share, so their bits agree.
__device__ inline double gate_score_f64(float h0, float h1) { return 1.0 / (1.0 + exp((double)h0 - (double)h1)); }

// The three confidence scoring functions of a row in float64: the one copy the dumped-array tools (exit_ops.hip: the scans, csf_table_kernel)
// and the cascade's deferral test (cascade.hip) share, so their bits agree.  T: double (a dumped array) or float (a delivered row, widened
// value by value, which is exact).
// float64 max-softmax of one row, as the policy computes it (scipy.special.softmax on the float64 store, EE/policy.py:30-32)
template <typename T>
__device__ __forceinline__ double max_softmax_f64(const T* z, int K) {
    double m = (double)z[0];
    for (int k = 1; k < K; ++k) m = fmax(m, (double)z[k]);
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += exp((double)z[k] - m);
    return 1.0 / s;
}
// float64 entropy of one row, the reference's expression: log A - B / A with A = sum e^z, B = sum z e^z, no max shift (EE/thresh.py:41-45)
template <typename T>
__device__ __forceinline__ double entropy_f64(const T* z, int K) {
    double A = 0.0, B = 0.0;
    for (int k = 0; k < K; ++k) {
        const double x = (double)z[k], e = exp(x);
        A += e;
        B += x * e;
    }
    return log(A) - B / A;
}
// float64 margin of one row (MMEE_CRIT_MARGIN, include/mmee.h): (1 - exp(m2 - m1)) / S, m1 the maximum, m2 the second largest value counting
// multiplicity (the pass that finds the maximum keeps both), S = sum_k exp(z_k - m1) in label order.  >= 0, exactly 0 on a tie, 1 when K = 1
template <typename T>
__device__ __forceinline__ double margin_f64(const T* z, int K) {
    double m1 = (double)z[0], m2 = -INFINITY;
    for (int k = 1; k < K; ++k) {
        const double x = (double)z[k];
        m2 = x > m1 ? m1 : fmax(m2, x);
        m1 = fmax(m1, x);
    }
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += exp((double)z[k] - m1);
    return (1.0 - exp(m2 - m1)) / s;
}
// The row of a criterion table (ee_csf_table): the criterion, and am = the argmax, first maximum (as numpy).  The max-softmax here is
// 1 / sum_k exp(z_k - m) in label order with m that first maximum.
template <typename T>
__device__ __forceinline__ double csf_row_f64(int criterion, const T* z, int K, int& am) {
    double m = (double)z[0];
    am = 0;
    for (int k = 1; k < K; ++k)
        if ((double)z[k] > m) { m = (double)z[k]; am = k; }
    if (criterion == CRIT_ENTROPY) return entropy_f64(z, K);
    if (criterion == CRIT_MARGIN) return margin_f64(z, K);
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += exp((double)z[k] - m);
    return 1.0 / s;
}

// The exit ensemble (include/mmee.h, at ee_set_ensemble): its two functions, the one copy the forward's launch (exit_stage.hip) and the
// dumped-array tool (exit_ops.hip) share, so their bits agree.  Each returns ONE label's value; a thread per (document, label) walks the row
// for M and S itself, in label order, so no value depends on how the threads are grouped.
// l[k] of the row x(0 .. K-1): x is a callable int -> double
template <typename Row>
__device__ inline double ens_logsoftmax_f64(Row x, int K, int k) {
    double m = x(0);
    for (int j = 1; j < K; ++j) m = fmax(m, x(j));
    double s = 0.0;
    for (int j = 0; j < K; ++j) s += exp(x(j) - m);
    return (x(k) - m) - log(s);
}
// a_m[k] = b + sum_{j = 0 .. m} w_row[j] * l(j), fma, j ascending from b: l is a callable int -> double, w_row is row m of w
template <typename Rows>
__device__ inline double ens_combine_f64(const double* w_row, double b, int m, Rows l) {
    double a = b;
#pragma unroll 4
    for (int j = 0; j <= m; ++j) a = fma(w_row[j], l(j), a);
    return a;
}

// the exit ensemble's launch of the forward, between an exit's head and its decision (exit_stage.hip)
struct EnsembleArgs {
    const float* pol_logits;         // [n_docs][K] the head's policy rows of the current stage
    int K, E1, exit_index, B;        // B: the slots of the state (the handle's max_docs)
    double temp;
    const double* temp_ptr;          // captured-graph forwards: the temperature at [exit_index] of the replay's device vector; null: `temp`
    const StageCounts* counts;
    const int* doc_orig;
    const double* w;                 // (E1,E1) on the device
    const double* b;                 // (E1,K) on the device, or null: 0
    double* state;                   // (E1,B,K): l_e of every slot; row exit_index written, rows below it read
    float* out;                      // [n_docs][K] y of the current stage's documents: the policy rows the decision reads
};
void launch_exit_ensemble(const EnsembleArgs& a, hipStream_t s);
// ee_ensemble_logits (exit_ops.hip): the same two functions over a dumped array; out (E1,N,K) holds l between its two launches
void launch_ensemble_logits(const double* logits, int E1, int N, int K, const double* w, const double* b, double* out, hipStream_t s);
void launch_ensemble_logsoftmax(const double* logits, size_t rows, int K, double* l, hipStream_t s);      // its first launch alone: l of every row

// how launch_decide picks its kernel: the exit test (MODE) and the rule built on it (RULE = MMEE_RULE_*; DECIDE_PATIENCE takes RULE_PLAIN only)
enum { DECIDE_THRESHOLD = 0, DECIDE_PATIENCE = 1, DECIDE_LTE = 2 };
enum { RULE_PLAIN = 0, RULE_STREAK = 1, RULE_EITHER = 2, RULE_AGREE = 3 };      // RULE_AGREE: PABEE's counter alone (exit_scan_kernel only)

// Budgeted exits (ee_set_quotas; the definition is in include/mmee.h): the decision compares a document with its batch mates.  Between an
// exit's head (or ensemble launch) and its decision two launches rank the stage: exit_quota_crit_kernel writes the float64 criterion of every
// active document to `crit`, exit_quota_rank_kernel turns the criteria into rank[i] = the number of active documents that precede i.  The
// QUOTA instantiations of the decide kernel read both; the final exit and dump-all calls run the plain kernels and neither launch.
enum { QUOTA_OFF = 0, QUOTA_EXACT = 1, QUOTA_AT_LEAST = 2 };                    // MMEE_QUOTA_* (capi_internal.h asserts the values agree)
struct QuotaArgs {
    int q;                           // THIS exit's quota q_e: the documents of the call that leave here (EXACT), or at least leave here (AT_LEAST)
    const double* q_ptr;             // captured-graph forwards: q_e at [0], as PatienceArgs::t_ptr; null: `q`
    double* crit;                    // [n_docs] stage scratch: c_i, by the stage's document index
    int* rank;                       // [n_docs] stage scratch: rank_i
};
// The order of the ranking as one unsigned compare: s = sign * c, a larger key is a more confident document.  -0.0 and +0.0 share a key
// (s + 0.0); every NaN takes key 1, below every number; 0 is left to "no document" (the dumped-array tool's documents that have left).
__host__ __device__ inline unsigned long long quota_key(double c, double sign) {
    const double s = sign * c + 0.0;
    if (s != s) return 1ull;
    unsigned long long u;
    __builtin_memcpy(&u, &s, sizeof(u));
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
void launch_exit_quota_crit(const DecideArgs& a, const QuotaArgs& q, int max_docs, hipStream_t s);      // the two ranking launches: c_i,
void launch_exit_quota_rank(const DecideArgs& a, const QuotaArgs& q, int max_docs, hipStream_t s);      // then rank_i (max_docs >= n_docs sizes the grids)
void launch_decide_quota(const DecideArgs& a, const QuotaArgs& q, int quota_mode, hipStream_t s);        // QUOTA_EXACT / QUOTA_AT_LEAST; threshold criteria, plain rule

// Audited exits (ee_set_audit; the definition is in include/mmee.h): a hashed, content-blind sample of the call's documents is delivered where
// it leaves and stays in the batch as a shadow until the final exit.  The selection test, the one copy the AUDIT decide kernels, ee_audit_selected
// and (through it) the Python mask share: x = (uint32)slot * 0x9E3779B1 ^ seed through murmur3's fmix32, selected iff x < cut, cut in [0, 2^32].
// (seed 0, slot 0) hashes to 0 and is selected under every cut > 0.
__host__ __device__ inline bool audit_selected(unsigned long long cut, unsigned seed, int slot) {
    unsigned x = (unsigned)slot * 0x9E3779B1u ^ seed;
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return (unsigned long long)x < cut;
}
// the AUDIT decide kernels' third argument
struct AuditArgs {
    int* delivered;                  // [max_docs] by original slot: 1 once the document's result is written; written (not read) at exit_index 0
    unsigned long long cut;          // floor(fraction 2^32 + 0.5) in (0, 2^32]
    unsigned seed;
    int slot_base;                   // the call's slot 0 in the caller's batch (MicroBatchedEngine: the slice's first document)
};
// launch_decide (below) takes it as its last argument: non-null picks the AUDIT form of its seven kernels, at every exit of an audited call, the
// final one included (delivered documents write no result there); null launches the kernels as they were

// Online exit control (ee_set_controller; the definition is in include/mmee.h, behind the audit's): a position p on a path of threshold
// vectors steps against the disagreement the audit observes.  The three functions below are the one copy the forward's two launches, the
// replay tool (ee_rolling_control) and the stand-alone hooks share (controller.hip), so their bits agree; ee_set_controller calls the first
// on the host for the thresholds of the first call.
constexpr int kCtlMaxE1 = 64;                                         // exits a controller takes (the kernels hold a vector per exit in LDS)
constexpr int kCtlStateWords = 5;                                     // the device state: p (float64 bits), calls, steps, sampled_sum, disagree_sum
// the 64-bit words of a log row, and of a tally (sampled, disagree, delivered[E], agree[E]): E = E1 - 1
__host__ __device__ inline int controller_log_words(int E1) { return 5 + 2 * (E1 - 1) + E1; }
__host__ __device__ inline int controller_tally_words(int E1) { return 2 + 2 * (E1 - 1); }
// thr_out[E1] of position p on path (V,E1), V >= 2: below 0 the value that never fires at every exit below the final one; else the lerp between
// rows i = min(floor(p'), V - 2) and i + 1 at t = p' - i, p' = min(p, V - 1), every product rounded before the add.  The final entry is
// path[i]'s (path[0]'s below 0); no forward reads it.
__host__ __device__ inline void controller_thresholds(const double* path, int V, int E1, double p, double sign, double* thr_out) {
#pragma clang fp contract(off)
    if (p < 0.0) {
        for (int e = 0; e < E1 - 1; ++e) thr_out[e] = sign < 0.0 ? -INFINITY : INFINITY;
        thr_out[E1 - 1] = path[E1 - 1];
        return;
    }
    const double top = (double)(V - 1);
    const double q = p < top ? p : top;
    int i = (int)floor(q);
    if (i > V - 2) i = V - 2;
    const double t = q - (double)i;
    const double *a = path + (size_t)i * E1, *b = a + E1;
    for (int e = 0; e < E1 - 1; ++e) {
        const double diff = b[e] - a[e];
        thr_out[e] = a[e] + diff * t;
    }
    thr_out[E1 - 1] = a[E1 - 1];
}
// p after a call that audited `sampled` documents of which `disagree` were delivered early with another answer than the full model's:
// unchanged when nobody was sampled, else min(V - 1, p - gamma (disagree / sampled - alpha)), the product rounded before the subtraction
__host__ __device__ inline double controller_step(double p, long long sampled, long long disagree, double alpha, double gamma, int V) {
#pragma clang fp contract(off)
    if (sampled == 0) return p;
    const double loss = (double)disagree / (double)sampled;
    const double move = gamma * (loss - alpha);
    const double q = p - move;
    const double top = (double)(V - 1);
    return q < top ? q : top;
}
// argmax of the row x(0 .. K-1), x a callable int -> float or double: the lowest index on ties; a row without a maximum (a NaN in it) counts
// as K - 1, exactly like sweep.first_argmax
template <typename Row>
__host__ __device__ inline int row_first_argmax(Row x, int K) {
    auto best = x(0);
    bool nan = best != best;
    int am = 0;
    for (int k = 1; k < K; ++k) {
        const auto v = x(k);
        nan = nan || v != v;
        if (v > best) { best = v; am = k; }
    }
    return nan ? K - 1 : am;
}
// audit_tally_kernel: what the audit saw in one call.  The final stage (counts, doc_orig, the policy rows the final decide launch read and its
// temperature), the delivered marks, the call's results and the audit's selection; tally[controller_tally_words(E1)] is written, not added to
struct AuditTallyArgs {
    const StageCounts* counts;       // the final stage
    const int* doc_orig;
    const float* pol_logits;         // [n_docs][K]: the rows the final decide launch read
    double temp;                     //   and scaled by, (float)((double)z / temp), as it writes them
    int K, B, E1;                    // B: the call's documents (the slots the hash runs over)
    const int* delivered;            // [B] by original slot: the AUDIT decide kernels' marks
    const float* out_logits;         // (B,K)
    const int* out_exit;             // (B)
    unsigned long long cut;
    unsigned seed;
    int slot_base;
    long long* tally;
};
void launch_audit_tally(const AuditTallyArgs& a, hipStream_t s);
// controller_step_kernel: the step behind a tally.  state[kCtlStateWords]; thr[E1] holds the thresholds the call ran with and receives the
// next call's; log: the ring of log_cap rows of controller_log_words(E1) words, or null
struct ControllerStepArgs {
    const double* path;              // (V,E1) on the device
    int V, E1;
    double sign, alpha, gamma;
    long long* state;
    const long long* tally;
    double* thr;
    long long* log;
    int log_cap;
};
void launch_controller_step(const ControllerStepArgs& a, hipStream_t s);
// rolling_control_kernel (ee_rolling_control): the same loop on a dumped criterion table, groups of G consecutive documents as the calls
struct RollingControlArgs {
    const double* table;             // (E1,N)
    const unsigned char* bad;        // (E1,N) 0 / 1: delivering document n at exit e is a loss
    const double* path;              // (V,E1)
    int E1, N, V, G;
    double sign, alpha, gamma, p0;
    unsigned long long cut;
    unsigned seed;
    int* exits;                      // (N)
    long long* log;                  // (ceil(N / G), controller_log_words(E1))
    double* p_out;                   // [1] the position after the last group, or null
};
void launch_rolling_control(const RollingControlArgs& a, hipStream_t s);

// Deadline exits (ee_set_deadline; the definition is in include/mmee.h, behind the controller's): a launch in front of every exit's decide
// launch reads the 100 MHz clock and, once the budget is spent or the host has asked, rewrites the rest of the call's thresholds to the value
// that fires for everybody.  deadline_rule is THE rule: deadline_check_kernel (deadline.hip; the forward and ee_debug_deadline_check launch it)
// and nothing else calls it.
constexpr unsigned long long kDeadlineNone = ~0ull;                   // MMEE_DEADLINE_NONE: stamp, never cut by the clock
constexpr int kDlStateWords = 3;                                      // the device state of the call in flight: t0 (ticks), cut_exit, cut_by
__host__ __device__ inline int deadline_log_words(int E1) { return 4 + E1; }      // call, budget_ns, cut_exit, cut_by, elapsed_ns[E1]
__host__ __device__ inline unsigned long long deadline_sat_add(unsigned long long a, unsigned long long b) {
    const unsigned long long s = a + b;
    return s < a ? ~0ull : s;
}
// ticks of a counter that runs at khz kHz, in ns, rounded down: (d / khz) 10^6 + (d % khz) 10^6 / khz, 2^64 - 1 where that would not fit
__host__ __device__ inline unsigned long long deadline_ticks_to_ns(unsigned long long d, unsigned khz) {
    const unsigned long long q = d / khz, r = d % khz;
    if (q > (~0ull - 999999ull) / 1000000ull) return ~0ull;
    return q * 1000000ull + r * 1000000ull / khz;
}
struct DeadlineVerdict {
    unsigned long long elapsed_ns;   // (now - t0) in ns, the difference taken modulo 2^64
    int cut_exit, cut_by;            // after this check: the exit of the call's cut or -1; 0, 1 (the clock) or 2 (the host)
};
// The check in front of exit `exit_index` of deadline call number `call` (1-based).  A cut is sticky and the final exit cuts nothing: with
// prev_cut_exit >= 0 or exit_index == E1 - 1 the previous pair comes back.  Otherwise the clock cuts when budget != kDeadlineNone and
// sat_add(elapsed, eta) >= budget; else the host does when host_word >= call.
__host__ __device__ inline DeadlineVerdict deadline_rule(unsigned long long t0, unsigned long long now, unsigned khz, unsigned long long budget,
                                                         unsigned long long eta, unsigned long long host_word, unsigned long long call,
                                                         int exit_index, int E1, int prev_cut_exit, int prev_cut_by) {
    DeadlineVerdict v{deadline_ticks_to_ns(now - t0, khz), prev_cut_exit, prev_cut_by};
    if (prev_cut_exit >= 0 || exit_index >= E1 - 1) return v;
    if (budget != kDeadlineNone && deadline_sat_add(v.elapsed_ns, eta) >= budget) { v.cut_exit = exit_index; v.cut_by = 1; }
    else if (host_word >= call) { v.cut_exit = exit_index; v.cut_by = 2; }
    return v;
}
// the threshold that fires for every criterion that is not a NaN: the mirror image of controller_thresholds' never-fires value
__host__ __device__ inline double deadline_always_fires(double sign) { return sign < 0.0 ? INFINITY : -INFINITY; }
// deadline_begin_kernel: the first launch of a deadline call.  t0 <- the clock, no cut yet, thr <- the call's thresholds, the head of the log row
struct DeadlineBeginArgs {
    double thr_in[kCtlMaxE1];        // the call's thresholds, by value
    int E1;
    unsigned long long call, budget;
    long long* state;                // [kDlStateWords]
    double* thr;                     // [E1]: what every decide launch of the call reads
    long long* row;                  // the call's log row (deadline_log_words(E1) words), or null
};
void launch_deadline_begin(const DeadlineBeginArgs& a, hipStream_t s);
// deadline_check_kernel: one workgroup of one wave in front of an exit's decide launch.  now_set / t0_set: the stand-alone hook's injected
// clock (the forward leaves both 0: the kernel reads s_memrealtime and state[0])
struct DeadlineCheckArgs {
    int E1, exit_index;
    unsigned khz;                    // the wall-clock rate the runtime reports
    double sign;
    unsigned long long call, budget, eta;      // eta: eta_ns[exit_index]
    const unsigned long long* host_word;       // pinned, mapped: the latest call number ee_request_cut asked to cut
    long long* state;
    double* thr;
    long long* row;
    int now_set, t0_set;
    unsigned long long now, t0;
};
void launch_deadline_check(const DeadlineCheckArgs& a, hipStream_t s);

// ee_quota_scan (exit_ops.hip): the same decision on a criterion table (E1,N), consecutive groups of G documents ranked independently
struct QuotaScanArgs {
    const double* table;             // (E1,N) on the device
    double sign;
    const int* quotas;               // [E1 - 1] on the device
    const double* thr;               // [E1] on the device (QUOTA_AT_LEAST), or null
    int mode, E1, N, G;
    int* exits;                      // (N)
    double* cuts;                    // (groups, E1 - 1, 2) or null: criterion of the last leaver / of the first stayer, NaN where there is none
    int* rank;                       // (N) scratch
};
void launch_quota_scan(const QuotaScanArgs& a, hipStream_t s);

// exit_scan_kernel<EVENT, RULE>: the exit decision on dumped arrays (ee_policy_scan, ee_patience_scan, ee_lte_scan, ee_rule_scan)
// the event's criterion: float64 max-softmax of the logits row, crit[e][n], no event, float64 entropy / margin of the logits row
enum { SCAN_MSP = 0, SCAN_TABLE = 1, SCAN_NONE = 2, SCAN_ENTROPY = 3, SCAN_MARGIN = 4 };
struct ScanArgs {
    const double* logits;            // (E1,N,K); read for SCAN_MSP / _ENTROPY / _MARGIN, RULE_EITHER, RULE_AGREE and for `pred` only: may be null otherwise
    const double* crit;              // (E1,N) SCAN_TABLE's criterion
    double sign;                     // the event is sign * criterion > sign * thr[e] (+1: '>', -1: '<'; multiplying by +-1 is exact)
    const double* thr;               // [E1] on the device; null for SCAN_NONE
    const int* pat;                  // [E1] per-exit patience on the device, or null: pat_all at every exit
    int pat_all;
    int E1, N, K;
    int* exits;                      // (N)
    double* pred;                    // (N,K) or null: the logits row of the chosen exit
    double* conf;                    // (N) or null: the event's criterion at the chosen exit (SCAN_NONE: the float64 max-softmax of its row)
    int* counts;                     // [E1] or null, zeroed by the caller
};

// X-space CLS probe (xprobe.hip)
struct XProbeArgs {
    const char* xs;                  // split rows of X (LayerNorm output), H * 4 bytes per row, scaled by 1 / xs_inv
    float xs_inv;
    const int* x_phys;               // [n_docs] physical first (CLS) row of every active document
    const int* doc_off;              // [n_docs + 1] dense row offsets (lengths; context rows are written at doc_off[d])
    const int* doc_orig;             // [n_docs] original document id (pair-index slab)
    const StageCounts* counts;
    const float* qc;                 // [n_docs][H] Q of the CLS rows, already divided by sqrt(d)
    const float *wk, *bk, *bv;       // key projection and the biases (rows h * 64 + t of the fused weight), f32
    const float* wv_s;               // value projection as split-f16 rows (the fused Q | K | V weight of ee_finalize), scaled by 1 / wv_inv
    float wv_inv;
    float *u, *s0, *cvec;            // scratch: [max_docs][heads][H], [max_docs][heads][2] (q . b_k, plane scale of u), [max_docs][heads][H]
    int *order, *ticket;             // scratch: [max_docs] documents by falling length, [1] ticket counter of xprobe_attn_kernel
    void* ctx;                       // out: context rows (split planes scaled by ctx_scale), row doc_off[d]
    float ctx_scale;
    const unsigned* pair_idx;
    size_t idx_doc_stride;
    const float *w1, *wx, *wy;       // raw bucket tables [heads][bins]
    int bins1, bins2;
    float inv_sqrt_d;
    int H, heads;
    int* err_flag;
};
bool xprobe_supports(const XProbeArgs& a, int max_len);
void launch_xprobe(const XProbeArgs& a, int max_docs, int max_len, int num_cus, hipStream_t s);

struct ImageDesc {
    long long offset;                // byte offset of the image inside the packed uint8 buffer (HWC, or HW when c == 1)
    int h, w, c, pad;
};

void launch_preprocess_images(const unsigned char* images, const ImageDesc* desc, int B, int R, int KMAX, int max_h, int2* bounds,
                              int* kk, unsigned char* tmp, const float* lut, float* out, unsigned char* out_u8, hipStream_t s);
void launch_collate_pad(const long long* ids, const long long* boxes, const long long* offsets, int B, int T, long long pad_id,
                        long long* out_ids, long long* out_mask, long long* out_bbox, hipStream_t s);
void launch_prep(const PrepArgs& a, hipStream_t s);
// doc_flags[d] = 1 when a key INSIDE document d is masked (any row of it with RowMeta.flags != 0), else 0; d in the numbering of doc_off
void launch_doc_flags(const RowMeta* meta, const int* doc_off, int n_docs, int* doc_flags, hipStream_t s);
void launch_prep_uniform(int B, int Pv, int* doc_off, int* x_src, int* doc_orig, RowMeta* meta, StageCounts* counts, hipStream_t s);
void launch_embed_text(const EmbedArgs& a, hipStream_t s);
void launch_embed_visual(const EmbedArgs& a, hipStream_t s);
void launch_vision_pool(const VisionPoolArgs& a, hipStream_t s);
void launch_copy_survivors(const StageCounts* n_counts, const int* n_doc_orig, int cap, int* survivors, int* count, hipStream_t s);
void launch_pool_finish(const float* part, int chunks, int H, float count, float* pooled, int B, hipStream_t s);
void launch_ln_rows(const float* src, float* dst, const int* row_src, const int* n_rows_ptr, int max_rows, int H,
                    const float* g, const float* b, float eps, int num_cus, hipStream_t s, void* dst_split = nullptr,
                    float split_scale = 1.0f, int* err_flag = nullptr, int pre_parts = 0, size_t pre_stride = 0, const float* pre_bias = nullptr,
                    const void* pre_resid = nullptr, const int* pre_resid_rows = nullptr, float pre_resid_inv = 0.f);
void launch_embed_beit(const float* patch, const float* cls, const float* pos, int B, int Pv, int H, float* X, hipStream_t s);
void launch_patch_mean(const float* X, int H, const int* x_phys, const int* doc_off, const int* n_docs_ptr, float* pooled,
                       int max_docs, hipStream_t s);
void launch_head_out(const HeadOutArgs& a, int max_docs, hipStream_t s);
void launch_decide(const DecideArgs& a, const PatienceArgs* p, int mode, int rule, hipStream_t s,    // p: null where (mode, rule) keeps no state
                   const AuditArgs* audit = nullptr);                                                 // audit: null, or an audited call (not a dump-all one)
void launch_emit_leavers(const EmitArgs& a, hipStream_t s);      // result_stream.hip
void launch_pack_results(const float* logits, const int* exit_layer, const float* conf, int n, int K, int* rows, hipStream_t s);
void launch_unpack_results(const int* rows, int n, int K, float* logits, int* exit_layer, float* conf, hipStream_t s);
void launch_compact_rows(const StageCounts* n_counts, const int* n_doc_off, const int* n_x_src, const int* n_meta_src,
                         const RowMeta* meta_old, RowMeta* meta_new, int* row_src, int max_docs, int num_cus, hipStream_t s);
// out[doc_orig ? doc_orig[i] : i] = CLS row of active document i; split_inv != 0: X holds split-f16 rows scaled by 1 / split_inv
// every row of every document -> out[(d * (T + Pv) + position)][H] (ee_set_hidden_states_out); text_dst null: image-only, Pv rows per document
// attention_maps.hip: side kernels of `output_attentions` / `head_mask` (dump-all, whole layers; never on the hot path)
bool attention_probs_supports(int S);
void launch_attention_probs(const float* qkv, int ld, int split, float qkv_scale, const RowMeta* meta, const int* doc_off, const float* t1,
                            const float* tx, const float* ty, int n1, int c1, int n2, int c2, int H, int heads, int S, int B,
                            const float* head_scale, float* out, hipStream_t s);
void launch_head_scale_ctx(float* ctx, int ld, const int* n_rows_ptr, int max_rows, int H, const float* head_scale, int split, float scale,
                           int num_cus, int* err_flag, hipStream_t s);
void launch_rows_to_padded(const float* X, float split_inv, int H, int B, int T, int Pv, const int* text_dst, const int* ntext, const int* doc_off,
                           float* out, hipStream_t s);
void launch_gather_cls(const float* X, int H, const int* x_phys, const int* doc_orig, const int* n_docs_ptr,
                       float* out, int max_docs, hipStream_t s, float split_inv = 0.f);
void launch_exit_scan(const ScanArgs& a, int event, int rule, hipStream_t s);
// The ranking step of the ranked sweeps and of the threshold search (exit_ops.hip): rec[n][e] = rank << 8 | correct << 6 | e of every document
// (rows of E1P words), sorted (E1, N) = every exit's confidences ascending and, when thr is given, T (V, E1) = the thresholds' rank words.
// ok == false: an allocation failed and nothing was launched.  The workspace is freed in stream order when the object goes out of scope.
struct SweepRanks {
    unsigned *rec = nullptr, *T = nullptr;
    double* sorted = nullptr;
    hipStream_t s;
    bool ok;
    SweepRanks(const double* conf, const unsigned char* correct, int E1, int E1P, int N, const double* thr, int V, int strict, hipStream_t stream);
    SweepRanks(const SweepRanks&) = delete;
    ~SweepRanks();
};
bool launch_rule_sweep(const double* conf, const double* logits, const long long* refs, int E1, int N, int K, const double* thr, int V,
                       const int* pats_host, const int* pats_dev, int P, int rule, double* acc, double* mean_exit, int* hist, hipStream_t s);
bool launch_patience_sweep(const double* logits, const long long* refs, int E1, int N, int K, const int* pats, int V, double* acc,
                           double* mean_exit, int* hist, hipStream_t s);
void launch_threshold_sweep(const double* conf, const unsigned char* correct, int E1, int N, const double* thr, int V,
                            double* acc, double* mean_exit, int* hist, hipStream_t s);
// ee_threshold_search (threshold_search.hip; include/mmee.h MMEE_SEARCH_*, capi_internal.h asserts the values agree)
enum { SEARCH_GRID = 0, SEARCH_SAMPLED = 1, SEARCH_MIXTURES = 2 };
enum { SEARCH_REFERENCE = 0, SEARCH_POLICY = 1 };
// the P percentiles as (lower index, upper index, weight) in the sorted row, from N and P in numpy's index arithmetic: search_table_kernel's ARGUMENT
struct SearchPercentiles {
    int lo[64], hi[64];
    double t[64];
};
// where the candidate vectors' digits come from: a kernel argument of search_main_kernel and search_front_kernel
struct SearchVectors {
    int source;                      // SEARCH_*
    unsigned V;                      // vectors, 1 <= V < 2^32
    unsigned long long seed;         // SEARCH_SAMPLED
    const unsigned char* mixtures;   // SEARCH_MIXTURES: (V,E1) digits
};
struct SearchArgs {
    const double* conf;              // (E1,N)
    const unsigned char* correct;    // (E1,N)
    int E1, N, P, source, semantics;
    unsigned V;
    unsigned long long seed;
    const unsigned char* mixtures;
    double* table;                   // (E1,P)
    double *acc, *mean_exit;         // (V,) or null
    int *front_count, *front_exit_sum, *front_hits;      // [1], [N + 1], [N + 1]
    unsigned* front_vector;          // [N + 1]
    double* front_thresholds;        // (N + 1, E1)
};
bool launch_threshold_search(const SearchArgs& a, const SearchPercentiles& pc, hipStream_t s);
void launch_search_table(const double* sorted, int E1, int N, int P, const SearchPercentiles& pc, int strict, double* table, unsigned* trank, hipStream_t s);
// ee_threshold_search_cost (threshold_search_cost.hip): the same search, the front of (cost_sum down, hits up)
struct SearchCostArgs {
    SearchArgs base;                 // front_exit_sum: the exit sum of each entry's vector
    const unsigned* cost;            // (E1,N): what document n costs when it leaves at exit e
    unsigned long long* cost_sum;    // (V,) or null
    unsigned long long* front_cost_sum;      // [N + 1]
};
bool launch_threshold_search_cost(const SearchCostArgs& a, const SearchPercentiles& pc, hipStream_t s);
// ee_threshold_refine (threshold_refine.hip): S chains of coordinate search on the searches' percentile grid, MMEE_SEARCH_POLICY's exit rule
struct RefineArgs {
    const double* conf;              // (E1,N)
    const unsigned char* correct;    // (E1,N)
    const unsigned* cost;            // (E1,N), or null: cost[e][n] = e
    int E1, N, P, S, max_rounds;
    const unsigned char* start;      // (S,E1) digits
    const unsigned long long* hit_value;     // (S,)
    const unsigned long long* budget;        // (S,) or null: none
    unsigned char* digits;           // (S,E1): the chains' vectors, from the first launch on
    double* thresholds;              // (S,E1) or null
    int *hits, *exit_sum, *rounds, *status, *start_hits;             // (S,) or null
    unsigned long long *cost_sum, *start_cost_sum;                   // (S,) or null
    double* table;                   // (E1,P) or null
};
bool launch_threshold_refine(const RefineArgs& a, const SearchPercentiles& pc, hipStream_t s);
size_t threshold_refine_workspace_bytes(int E1, int N, int P, int S);
// ee_exit_metrics (exit_metrics.hip; include/mmee.h MMEE_METRIC_*, capi_tools.hip asserts the values agree)
enum { kMetricAccuracy = 0, kMetricBrier = 1, kMetricNll = 2, kMetricF1Micro = 3, kMetricF1Macro = 4, kMetricEce = 5, kMetricAurc = 6,
       kMetricAvgConf = 7, kMetricCount = 8 };
constexpr int kMetricsMaxBins = 1024;        // the ECE edges and bin counts of one row live in LDS
constexpr int kMetricsMaxN = 1 << 20;        // the counting sort is O(N^2) per row
struct MetricsArgs {
    const double* logits;            // (E1,N,K), or null: the table form
    const long long* references;     // (N,) with the logits
    const double* conf;              // (E1,N), table form
    const unsigned char* correct;    // (E1,N), table form
    const double* temperatures;      // (E1,) or null
    const int* exits;                // (N,) or null: the operating point, row E1 of the outputs
    int E1, N, K, n_bins;            // n_bins resolved by the caller: 1 .. kMetricsMaxBins
    double* out;                     // (R, kMetricCount), R = E1 + (exits ? 1 : 0)
    unsigned long long* confusion;   // (R,K,K) int64 counts or null (kept in the workspace then)
    unsigned long long* exit_hist;   // (E1,) int64 counts or null
};
bool launch_exit_metrics(const MetricsArgs& a, hipStream_t s);
// criterion: CRIT_MAX_CONFIDENCE, CRIT_ENTROPY or CRIT_MARGIN
void launch_csf_table(const double* logits, const long long* refs, int E1, int N, int K, int criterion, double* table, unsigned char* correct,
                      hipStream_t s);
// ee_gate_table: table (E+1,N); rows 0 .. E-1 = gate_score_f64 of head_logits (E,N,2), row E = the max-softmax of final_logits (N,K) (launch_csf_table's)
void launch_gate_table(const float* head_logits, const double* final_logits, int E, int N, int K, double* table, hipStream_t s);

// Model cascades (cascade.hip; the definition is in include/mmee.h): the three launches of a stage boundary
struct CascadeSelectArgs {
    const float* logits;             // (n,K) the rows the stage delivered, by the stage's document index
    const int* exit_layer;           // (n) the stage's local exit index of every document
    const int* orig;                 // (n) original slot of every document (ascending), or null: the identity (stage 0)
    int n, K, final_exit, criterion; // criterion: CRIT_MAX_CONFIDENCE, CRIT_ENTROPY or CRIT_MARGIN
    double thr;                      // the stage's final threshold entry
    int* next_orig;                  // (n) original slots of the deferred documents, in their order; entries past the count are not written
    int* count;                      // device word: the deferred documents
    double* crit;                    // (n) or null: c of every document
};
void launch_cascade_select(const CascadeSelectArgs& a, hipStream_t s);
constexpr int kCascadeMaxArrays = 8;
struct CascadeGatherArgs {
    const char* src[kCascadeMaxArrays];
    char* dst[kCascadeMaxArrays];
    size_t row_bytes[kCascadeMaxArrays];   // multiples of 4
    int n_arrays;
    const int* slots;                // (cap) source row of destination row j
    const int* count;                // device word: the rows to copy, <= cap
};
void launch_cascade_gather(const CascadeGatherArgs& a, int cap, hipStream_t s);     // cap >= 1 sizes the grid
struct CascadeMergeArgs {
    const float* logits;             // (n,K) a later stage's results, by the stage's document index
    const int* exit_layer;           // (n)
    const float* conf;               // (n)
    const int* slots;                // (n) original slot of every document
    int n, K, exit_offset, stage;
    float* out_logits;               // (B,K) the cascade's outputs, written at the documents' slots only
    int* out_exit;                   // (B)   exit_layer + exit_offset
    float* out_conf;                 // (B)
    int* out_stage;                  // (B)   stage
};
void launch_cascade_merge(const CascadeMergeArgs& a, hipStream_t s);                // n >= 1
void launch_temperature_fit(const double* logits, const long long* labels, int E1, int N, int K, int max_iter, double* T_out,
                            double* nll_out, double* acc_out, double* conf_out, int* iters_out, hipStream_t s);
// ee_head_fit (head_fit.hip): softmax-regression heads per exit, float64 on float32 features; include/mmee.h states the objective
constexpr int kHeadFitSlab = 32;             // rows a workgroup keeps in LDS between the logits and the gradient pass (MMEE_HEAD_FIT_SLAB)
constexpr int kHeadFitMaxChunks = 128;       // row chunks (= partial gradients) per exit
constexpr int kHeadFitMaxH = 1024;           // a slab of kHeadFitSlab float32 rows stays inside the 160 KB of LDS
constexpr int kHeadFitMaxHistory = 32;
// what every device fit carries (fit_lbfgs.hip); P: the parameters of one exit
struct FitArgs {
    const float* features;           // (E,N,H)
    int E, N, H;
    double l2, gtol;
    int max_evals, history;
    void* workspace;                 // the fit's *_workspace_bytes
    const double* theta0;            // the start, or null = 0
    double* theta64;                 // the solution in float64, or null
    double *loss, *grad_norm;        // one per fitted parameter set, or null
    int *evals, *status;             // one per fitted parameter set, or null
};
// the soft targets of the distilled fits (ee_head_fit_distill, ee_mlp_head_fit_distill); teacher null: the hard-label objective
struct DistillTargets {
    const float* teacher = nullptr;  // (N,K) logits of the final classifier, the same for every exit
    double alpha = 0.0;              // weight of the soft term; at 1 the labels are not looked at and may be null
    double temperature = 1.0;
};
// What a head is fitted against.  Host only: an entry point (capi_fit.hip) builds it once from its own arguments and it is handed down
// unchanged to the launch that picks the kernel's argument struct.  Null or default means absent.
struct HeadObjective {
    const long long* labels = nullptr;       // (N,); null: the distilled objective at alpha = 1, the gate objective
    DistillTargets soft;                     // teacher null: no soft term
    const float* weights = nullptr;          // (E,N) sample weights (ee_*_fit_weighted), or null: every row counts once
    const double* gate_targets = nullptr;    // (E,N) in [0,1] (ee_head_fit_gate, ee_mlp_head_fit_gate: K == 2, no labels, no teacher; the two-layer
                                             // fit alone takes weights with them), or null
};
struct HeadFitArgs : FitArgs {       // E parameter sets; theta0 and theta64 null
    HeadObjective objective;
    int K;
    float *weight, *bias;            // (E,K,H), (E,K)
    double *weight64, *bias64;       // the same in float64, or null
};
int head_fit_chunks(int N);
// weighted: the fit carries sample weights, and its workspace the row-scale table (E,N) float64 behind the partials
size_t head_fit_workspace_bytes(int E, int N, int H, int K, int history, bool weighted);
size_t head_fit_partial_bytes(int E, int N, int H, int K);
// false: the memset of the workspace failed.  The error word is the first int of the workspace (bit 0: a label outside [0,K); bit 1: a
// teacher logit that is not finite; bit 2: a sample weight that is negative or not finite; bit 3: an exit whose weights sum to zero; the gate
// objective: bit 0 is a target that is not finite or outside [0,1]).
bool launch_head_fit(const HeadFitArgs& a, hipStream_t s);
// one evaluation at theta (E, K*H + K): loss (E,), grad (E, K*H + K); partial: head_fit_partial_bytes, with weights (E,N) E * N doubles
// more behind them; err: one zeroed int
void launch_head_lossgrad(const float* X, const HeadObjective& o, const double* theta, int E, int N, int H, int K, double l2, double* partial,
                          int* err, double* loss, double* grad, hipStream_t s);
// ee_mlp_head_fit (mlp_head_fit.hip): two-layer heads (dense + tanh + out_proj) per exit; theta = W1 (H,H), b1 (H,), W2 (K,H), b2 (K,)
constexpr int kMlpHeadFitRows = 64;          // the row tile of the GEMM kernels, the largest of the new kernels' tiles (MMEE_MLP_HEAD_FIT_ROWS)
struct MlpHeadFitArgs : FitArgs {    // E parameter sets; theta0 (E,P) required, theta64 (E,P)
    HeadObjective objective;         // gate targets (ee_mlp_head_fit_gate): K == 2, the two-layer gate heads
    int K;
    float *dense_weight, *dense_bias, *weight, *bias;   // (E,H,H), (E,H), (E,K,H), (E,K)
};
size_t mlp_head_fit_workspace_bytes(int E, int N, int H, int K, int history, bool weighted);
size_t mlp_head_fit_scratch_doubles(int E, int N, int H, int K);
// false: preparing the workspace failed.  The error word is the first int of the workspace (bit 0: a label outside [0,K); bit 1: a teacher
// logit that is not finite; bits 2 and 3: the sample weights, as for launch_head_fit; the gate objective: bit 0 is a target that is not finite
// or outside [0,1]).
bool launch_mlp_head_fit(const MlpHeadFitArgs& a, hipStream_t s);
// one evaluation at theta (E,P): loss (E,), grad (E,P); scratch: mlp_head_fit_scratch_doubles doubles, with weights (E,N) E * N doubles
// more behind them; err: one zeroed int
void launch_mlp_head_lossgrad(const float* X, const HeadObjective& o, const double* theta, int E, int N, int H, int K, double l2, double* scratch,
                              int* err, double* loss, double* grad, hipStream_t s);
// ee_lte_fit (lte_fit.hip): the learning-to-exit classifier, one Linear(H, 1) for all encoder exits; theta = w (H,), b
constexpr int kLteFitRows = 16;              // the rows a workgroup treats as a unit: four waves, four rows in flight each (MMEE_LTE_FIT_ROWS)
constexpr int kLteFitMaxChunks = 128;        // row chunks (= partial gradients) per exit
constexpr int kLteFitMaxExits = 64;          // the reduce kernel keeps one sum per exit in LDS
enum { kLteLossMse = 0, kLteLossBce = 1 };   // MMEE_LTE_LOSS_*
struct LteFitArgs : FitArgs {        // one parameter set over E data exits; theta0 and theta64 (H + 1,)
    const double* targets;           // (E,N) in [0,1]
    int loss_kind;
    float *weight, *bias;            // (1,H), (1,)
};
int lte_fit_chunks(int N);
size_t lte_fit_workspace_bytes(int E, int N, int H, int history);
size_t lte_fit_partial_doubles(int E, int N, int H);
// false: preparing the workspace failed.  The error word is the first int of the workspace (bit 0: a target outside [0,1] or NaN).
bool launch_lte_fit(const LteFitArgs& a, hipStream_t s);
// one evaluation at theta (H + 1,): loss_out one double, grad (H + 1,); partial: lte_fit_partial_doubles doubles; err: one zeroed int
void launch_lte_lossgrad(const float* X, const double* T, const double* theta, int E, int N, int H, int loss, double l2, double* partial, int* err,
                         double* loss_out, double* grad, hipStream_t s);
// targets (E,N) = 1 - [argmax(logits (E,N,K)) == y]; err: one zeroed int, bit 0 = a label outside [0,K) or a NaN logit (then nothing is written)
void launch_lte_targets(const float* logits, const long long* y, int E, int N, int K, double* targets, int* err, hipStream_t s);
void launch_lte_scores(const float* X, const float* wgt, const float* bias, int E, int N, int H, double* scores, hipStream_t s);
// ee_ensemble_fit (ensemble_fit.hip): the exit ensemble's w and b per exit from a dumped array; theta of exit m = b_m (K,), w_m (E1,)
struct EnsembleFitArgs : FitArgs {   // E = E1 parameter sets; features null, H 0; theta0 and theta64 null (the start is w0 / b0)
    const double* logits;            // (E1,N,K) un-ensembled scaled rows
    const long long* labels;         // (N,)
    const double *w0, *b0;           // the start (E1,E1), (E1,K); null: w = I, b = 0
    int K;
    double *w, *b;                   // (E1,E1), (E1,K)
};
bool ensemble_fit_supports(int E1, int K);       // a tile of one document fits the 60 KB of LDS the row kernel takes
size_t ensemble_fit_workspace_bytes(int E1, int N, int K, int history);
// false: preparing the workspace failed.  The error word is the first int of the workspace (bit 0: a label outside [0,K); bit 1: a logit
// that is not finite).
bool launch_ensemble_fit(const EnsembleFitArgs& a, hipStream_t s);
void launch_build_value_tables(const float* w1, const float* wx, const float* wy, const unsigned char* lut1,
                               const unsigned char* lut2, int heads, int bins1, int bins2, int n1, int n2, float inv_sqrt_d,
                               float* t1, float* tx, float* ty, hipStream_t s);

}  // namespace mmee
