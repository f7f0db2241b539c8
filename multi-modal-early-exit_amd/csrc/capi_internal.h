// What the translation units of the C-ABI (include/mmee.h) share: the handle, its parameter / weight records, the error helpers every entry
// point returns through, the allocator and the profiling scope.  Private to csrc/capi*.hip:
//   capi.hip          the handle's error ring and allocator, and the loader (ee_create, ee_load_tensor, ee_finalize, ee_destroy)
//   capi_forward.hip  the forward schedule (Forward, ee_forward), its captured-graph form (ee_graph_*), its stage 0 alone (ee_embedding_inputs)
//                     and its pixels-only opening up to exit 0 (ee_forward_vision)
//   capi_query.hip    what reads the last forward back or arms the next one (ee_profile*, ee_stream_next, ee_last_*, ee_suggest_probe_mask, ee_set_*)
//   capi_tools.hip    entry points that never see a handle (clock stamps, policy sweeps, pack / unpack, image feed, the GEMM micro-benchmarks)
//   capi_debug_attention.hip, capi_debug_rows.hip, capi_debug_xprobe.hip, capi_debug_exit.hip, capi_debug_patch.hip, capi_debug_vision.hip   the ee_debug_* hooks of the
//                     attention kernels, of the row kernels, of the X-space CLS probe, of the exit stage, of the patch projection and of the vision pool; what only
//                     they share is in capi_debug.h
//   capi_fit.hip      the device fits, no handle either (ee_head_fit, ee_mlp_head_fit, ee_lte_*, ee_ensemble_fit, ee_debug_*_lossgrad)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mmee.h"
#include "mmee_kernels.h"

static_assert(mmee::CRIT_MAX_CONFIDENCE == MMEE_CRIT_MAX_CONFIDENCE && mmee::CRIT_ENTROPY == MMEE_CRIT_ENTROPY &&
              mmee::CRIT_PATIENCE == MMEE_CRIT_PATIENCE && mmee::CRIT_MARGIN == MMEE_CRIT_MARGIN && mmee::CRIT_GATE == MMEE_CRIT_GATE, "the kernels' criterion codes are the ABI's");
static_assert(mmee::SEARCH_GRID == MMEE_SEARCH_GRID && mmee::SEARCH_SAMPLED == MMEE_SEARCH_SAMPLED && mmee::SEARCH_MIXTURES == MMEE_SEARCH_MIXTURES &&
              mmee::SEARCH_REFERENCE == MMEE_SEARCH_REFERENCE && mmee::SEARCH_POLICY == MMEE_SEARCH_POLICY, "the search's codes are the ABI's");
static_assert(mmee::QUOTA_OFF == MMEE_QUOTA_OFF && mmee::QUOTA_EXACT == MMEE_QUOTA_EXACT && mmee::QUOTA_AT_LEAST == MMEE_QUOTA_AT_LEAST, "the kernels' quota modes are the ABI's");

namespace mmee {
namespace capi {

struct Param {
    float* ptr = nullptr;
    std::vector<int64_t> shape;
    bool loaded = false;
    size_t numel() const {
        size_t n = 1;
        for (auto d : shape) n *= (size_t)d;
        return n;
    }
};

struct LayerW {
    float *qkv_w, *qkv_b, *ao_w, *ao_b, *ao_g, *ao_beta, *f1_w, *f1_b, *f2_w, *f2_b, *f_g, *f_beta;
    float *lam1 = nullptr, *lam2 = nullptr;   // BEiT layer scale (lambda_1 / lambda_2)
    // MMEE_PREC_F32_SPLIT: the four big weights as split-f16 rows (built by ee_finalize) and 1 / weight scale
    float *qkv_s = nullptr, *ao_s = nullptr, *f1_s = nullptr, *f2_s = nullptr;
    float qkv_inv = 1.f, ao_inv = 1.f, f1_inv = 1.f, f2_inv = 1.f;
};
struct HeadW {
    float *dense_w = nullptr, *dense_b = nullptr, *out_w = nullptr, *out_b = nullptr;
    float* dense_s = nullptr;           // split precision: split-f16 rows of dense_w (the head's dense runs on the split GEMM kernel)
    float dense_inv = 1.f;
    int out_dim = 0;
};
// bookkeeping of a forward (ee_last_stage_counts / ee_suggest_probe_mask / ee_last_flops / ee_last_layer_plan read that of the last one)
struct ForwardRecord {
    int last_B = 0, last_T = 0, last_stages = 0;
    uint32_t last_flags = 0;
    bool last_gate_heads = true;                  // gate strategy: were the 2-way gate heads evaluated
    std::vector<int> layer_stage;                 // stage whose rows the layer's attention / attention-out / FFN ran on; -1: none (probe only)
    std::vector<int> layer_qkv_stage;             // stage whose rows the layer's Q|K|V projection ran on
    std::vector<int> layer_probe_stage;           // stage whose CLS rows were probed before the layer's exit decision; -1: no probe
    std::vector<int> layer_xprobe;                // 1: the layer's probe ran in X space
    std::vector<int> exit_stage;                  // stage whose documents reached each exit
    int ks_attn_out = 1, ks_ffn_down = 1;         // MMEE_FLAG_LOW_LATENCY: split-K parts of the layers' attention-output / FFN-down GEMMs (ee_last_k_splits)
};

}  // namespace capi
}  // namespace mmee

struct ee_handle {
    ee_config cfg;
    std::string err;
    int num_cus = 256;
    bool finalized = false;
    std::map<std::string, mmee::capi::Param> params;
    std::vector<std::string> names;
    std::vector<void*> allocs;
    // model pointers
    float *word, *type, *pos, *xtab, *ytab, *htab, *wtab, *emb_g, *emb_b;
    float *patch_w, *patch_b, *cls_token, *pos_embed, *norm_g, *norm_b, *ln_g, *ln_b;
    float *rel1, *relx, *rely;
    std::vector<mmee::capi::LayerW> layers;
    mmee::capi::HeadW emb_heads[3];
    std::vector<mmee::capi::HeadW> enc_heads;
    mmee::capi::HeadW classifier;
    // derived
    float *t1 = nullptr, *tx = nullptr, *ty = nullptr;
    int n1 = 0, c1 = 0, n2 = 0, c2 = 0;
    // workspace
    float *Xs = nullptr, *Ys = nullptr;           // split-f16 copies of X / Y rows (MMEE_PREC_F32_SPLIT)
    float* patch_s = nullptr;                     // split rows of the patch projection weight (when its shape fits the split kernel)
    float patch_inv = 1.f;
    float* absmax_dev = nullptr;
    bool split = false;
    unsigned* pair_idx = nullptr;                 // split mode, LayoutLMv3: one word per (query, key) pair of every document (attention_idx.hip)
    unsigned char *lut1_dev = nullptr, *lut2_dev = nullptr;
    int idx_nb = 0;
    size_t idx_stride = 0;                        // dwords per document slab of pair_idx
    // round 6, 16-bit pair index (attention_idx.hip IDX16): pair_idx holds 2 bytes per pair; the X-space probe reads the 32-bit words of query
    // block 0 from pair_idx0 ([max_docs][idx_nb][1024]); key masks per (document, key tile), "a key inside the document is masked" per document
    bool idx16 = false;
    unsigned* pair_idx0 = nullptr;
    unsigned* keymask = nullptr;
    int* doc_flags = nullptr;
    float* cls_f32 = nullptr;                     // split mode: CLS rows of the active documents rebuilt from the split planes
    // CLS probe (probe-first layers): one row per active document
    float *Yc = nullptr, *Ycs = nullptr, *H1c = nullptr, *Xc = nullptr, *Xcs = nullptr;
    int* xp_order = nullptr;                      // [max_docs + 1]: documents by falling length, ticket counter
    float *Qc = nullptr, *xp_u = nullptr, *xp_s0 = nullptr, *xp_c = nullptr, *xp_part = nullptr;      // X-space probe (xprobe.hip): CLS queries, u, q.b_k, weighted row sums
    float* ll_part = nullptr;                     // MMEE_FLAG_LOW_LATENCY: split-K parts of a layer's residual GEMM (split precision, LayoutLMv3)
    size_t ll_part_floats = 0;                    //   2 * num_cus tiles of 128 x 128 floats, the bound of ee_low_latency_k_splits, whatever H, B, T
    int* iota = nullptr;                          // 0 .. max_docs-1
    float *X, *Y, *QKV, *CTX, *H1, *vis_raw, *text_part, *vis_part, *cat_part, *pooled[3], *hid, *hid2, *head_logits, *pol_logits;
    int *text_dst, *emb_pos, *ntext, *row_src, *err_flag;
    int* queue_heads = nullptr;                   // one work-queue counter per persistent launch of a forward
    int n_queue_heads = 0, next_queue_head = 0;
    mmee::RowMeta* meta[2];
    int *doc_orig, *doc_off, *x_src, *meta_src;   // [(E+3)][max_docs+1]
    mmee::StageCounts* counts;                    // [(E+3)]
    double* thr_dev = nullptr;                    // scratch for ee_policy_scan
    int32_t patience = 0;                         // ee_set_patience (0: not set): the patience of every exit unless patience_vec is set
    std::vector<int32_t> patience_vec;            // ee_set_patience_vector: [E + 1] per-exit patience (empty: the broadcast above)
    int32_t rule = MMEE_RULE_PLAIN;               // ee_set_exit_rule: what the decide launches make of the criterion / LTE event
    bool has_patience() const { return patience >= 1 || !patience_vec.empty(); }
    int32_t patience_at(int e) const { return patience_vec.empty() ? patience : patience_vec[e]; }
    int* pat_state = nullptr;                     // [2][max_docs]: argmax at the previous exit, run counter (by original document slot)
    // learning-to-exit (ee_config.use_lte): encoder.lte_classifier (weight [H], bias [1]) and the float64 scores of the exit being decided
    float *lte_w = nullptr, *lte_b = nullptr;
    double* lte_score = nullptr;                  // [max_docs], by the stage's document index
    // exit ensemble (ee_set_ensemble; include/mmee.h): device copies of w and b, the per-document state and the rows the decision reads instead
    // of the head's.  Allocated by the first ee_set_ensemble; ens_on says whether the forwards launch exit_ensemble_kernel
    bool ens_on = false;
    double *ens_w = nullptr, *ens_b = nullptr;    // (E1,E1), (E1,K): replays of a captured graph read them here
    double* ens_state = nullptr;                  // (E1,max_docs,K): l_e by original document slot (compaction never moves it)
    double* ens_ones = nullptr;                   // [E1] of 1.0: the temperatures a captured decide launch reads behind the ensemble
    float* ens_logits = nullptr;                  // [max_docs][K]: y of the exit being decided, by the stage's document index
    // budgeted exits (ee_set_quotas; include/mmee.h): the mode picks the decide kernel and adds the two ranking launches in front of it
    int32_t quota_mode = MMEE_QUOTA_OFF;
    std::vector<int32_t> quotas;                  // [E]: q_e of every exit below the final one (empty while quotas are off)
    double* quota_crit = nullptr;                 // [max_docs]: c_i of the exit being decided, by the stage's document index
    int* quota_rank = nullptr;                    // [max_docs]: rank_i
    // audited exits (ee_set_audit; include/mmee.h): cut > 0 picks the AUDIT form of the decide kernels in calls that are not dump-all
    uint64_t audit_cut = 0;
    uint32_t audit_seed = 0;
    int32_t audit_slot_base = 0;
    int* audit_delivered = nullptr;               // [max_docs] by original slot, allocated at the first ee_set_audit
    // online exit control (ee_set_controller; include/mmee.h): while ctl_on, every decide launch of a call that is not dump-all reads its
    // threshold at ctl_thr_dev, audits under seed ctl_seed + ctl_calls, and two launches behind the final exit step the position
    bool ctl_on = false;
    int32_t ctl_V = 0, ctl_log_cap = 0;
    double ctl_alpha = 0.0, ctl_gamma = 0.0;
    uint32_t ctl_seed = 0;
    uint64_t ctl_calls = 0;                       // controlled calls enqueued since ee_set_controller (the device state counts them too)
    double* ctl_path = nullptr;                   // (V,E1)
    double* ctl_thr_dev = nullptr;                // [E1]: the thresholds of the NEXT controlled call, rewritten by controller_step_kernel
    long long *ctl_state = nullptr, *ctl_tally = nullptr, *ctl_log = nullptr;      // kCtlStateWords; controller_tally_words; the ring of log rows
    // deadline exits (ee_set_deadline; include/mmee.h): while dl_on, a call that is not dump-all opens with deadline_begin_kernel, every
    // decide launch reads its threshold at dl_thr, and deadline_check_kernel runs in front of each.  budget and eta travel by value
    bool dl_on = false;
    uint64_t dl_budget = 0;
    std::vector<uint64_t> dl_eta;                 // [E1]
    uint32_t dl_khz = 0;                          // the wall-clock rate of the device (hipDeviceAttributeWallClockRate)
    uint64_t dl_calls = 0;                        // deadline calls enqueued on the handle so far (atomic: ee_request_cut reads it from any thread)
    uint64_t dl_log_first = 0;                    // dl_calls when the log was last restarted (ee_set_deadline_log)
    int32_t dl_log_cap = 0;
    uint64_t* dl_word = nullptr;                  // pinned, mapped host word: calls numbered <= *dl_word are cut at their next check
    const unsigned long long* dl_word_dev = nullptr;      // the same word as the check kernel addresses it
    double* dl_thr = nullptr;                     // [E1]
    long long *dl_state = nullptr, *dl_log = nullptr;     // kDlStateWords; the ring of log rows
    // optional per-kernel event timing (ee_profile)
    bool prof_on = false;
    struct ProfRec { int id; hipEvent_t a, b; double flops; };
    std::vector<ProfRec> prof_recs;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_pool;
    size_t prof_used = 0;
    // the workspace is shared by consecutive forwards: a forward enqueued on another stream than the previous one first
    // waits for it (one handle = one forward in flight)
    hipEvent_t fwd_done = nullptr;
    hipStream_t last_stream = nullptr;
    bool has_fwd = false;
    // err_flag of every forward, copied to a pinned host word of its own behind it (a ring: the caller may enqueue several forwards before
    // any has finished).  A later call reports the oldest unreported error of a FINISHED forward without synchronising; a slot is only
    // reused after its forward has been waited for and checked, so no error is ever overwritten unseen.
    struct ErrSlot { hipEvent_t done = nullptr; bool pending = false; };
    static constexpr int kErrSlots = 8;
    ErrSlot errs[kErrSlots];
    int* err_host = nullptr;                      // [kErrSlots] pinned
    unsigned err_seq = 0;                         // forwards enqueued so far
    mmee::capi::ForwardRecord rec;                // bookkeeping of the last forward
    bool mask_on = false;                         // ee_set_probe_mask: the exit-layer schedule is pinned
    const float* next_inputs_embeds = nullptr;    // ee_set_inputs_embeds: read by the next ee_forward, then cleared
    float* next_hidden_out = nullptr;             // ee_set_hidden_states_out: filled by the next ee_forward, then cleared
    const float* next_head_mask = nullptr;        // ee_set_head_mask: (L, heads) factors of the next ee_forward, then cleared
    float* next_attn_out = nullptr;               // ee_set_attentions_out: (L, B, heads, S, S) filled by the next ee_forward, then cleared
    uint64_t probe_mask = 0;
    // captured-graph forms of ee_forward (ee_graph_capture): the launch list of one (inputs, B, T, flags, outputs) configuration as a hipGraphExec;
    // thresholds / temperatures live in a device buffer the decide kernels read, refreshed in front of every replay
    struct GraphRec {
        hipGraphExec_t exec = nullptr;
        double* thr_dev = nullptr;                // [4 * (E + 1)]: thresholds, then temperatures (1.0 when the launch passes none), then the per-exit patience,
                                                  // then the quotas (the final exit's entry unused)
        int n_exits1 = 0;
        bool no_exit = false;
        bool patience = false;                    // captured under MMEE_CRIT_PATIENCE: launches need no thresholds
        int32_t quota_mode = MMEE_QUOTA_OFF;      // the handle's quota mode at capture (MMEE_QUOTA_EXACT: launches need no thresholds)
        mmee::capi::ForwardRecord rec;            // bookkeeping of the captured forward, restored by every launch
    };
    std::vector<GraphRec> graphs;
    // result stream (MMEE_FLAG_STREAM_RESULTS): one pinned, device-mapped buffer of max_docs rows of K + 3 words and E + 1 cumulative counts behind
    // them, allocated at the first flagged forward; the emit launches store into it directly and ee_stream_next hands out its segments
    int32_t* stream_host = nullptr;               // what the host reads
    int32_t* stream_dev = nullptr;                // the same memory as the kernels address it
    int* stream_done = nullptr;                   // device word: the running leaver count of the forward in flight
    std::vector<hipEvent_t> stream_ev;            // [E + 1], timing disabled: recorded behind the emit launch of every exit
    bool stream_armed = false;                    // a flagged forward has been enqueued: its events are recorded
    int stream_next = 0;                          // the next exit ee_stream_next delivers
};

namespace mmee {
namespace capi {

// Defined in capi.hip, once.  h == nullptr: the message goes to the library-wide slot ee_last_error(NULL) reads.
int fail(ee_handle* h, const char* fmt, ...);

#define HIP_OK(h, expr)                                                                                      \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) return mmee::capi::fail(h, "%s failed: %s", #expr, hipGetErrorString(e_));     \
    } while (0)

// What every entry point that launches kernels returns through: a failed dynamic-LDS opt-in of one of ITS launchers (recorded per thread,
// mmee_common.h) with the kernel's name, else the launch error, else 0.
int launch_status(ee_handle* h, const char* who);

// Error flags of forwards that were enqueued earlier and not reported yet, oldest first.  wait = false: only forwards that have finished
// (stops at the first one still running: one handle's forwards finish in order); wait = true: waits for each.  all = false: returns at
// the first forward with flags (the others stay pending); all = true: ORs every pending forward's flags.
int take_errors(ee_handle* h, bool wait, bool all);
int report_errors(ee_handle* h, int err, const char* whose);

// HF relative_position_bucket as a LUT over delta in [-max_delta, max_delta] (capi.hip; ee_finalize and ee_bucket_lut)
void bucket_lut_host(int num_buckets, int max_distance, int max_delta, unsigned char* out);

template <typename T>
int dev_alloc(ee_handle* h, T** p, size_t count) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, count * sizeof(T) + 256);
    if (e != hipSuccess) return fail(h, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
    // the allocator hands back whatever the previous owner left: zero it, so that no kernel can ever act on another handle's stale
    // counters or indices (tools/fuzz_schedules.py found a stale ticket counter this way; a few milliseconds per handle)
    if (hipMemset(q, 0, count * sizeof(T) + 256) != hipSuccess) return fail(h, "hipMemset of a new allocation failed");
    h->allocs.push_back(q);
    *p = reinterpret_cast<T*>(q);
    return 0;
}

// ---- shared by the handle-free entry points (capi_tools.hip, capi_fit.hip, capi_debug_*.hip) ----
// false (and the error message of `who` set) when there is no HIP device
inline bool have_device(const char* who) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev >= 1) return true;
    fail(nullptr, "%s: no HIP device", who);
    return false;
}

// The per-tensor scale of a weight's split-f16 rows (split_weight_rows): 2^e with the e that puts max |w| in
// [2^12, 2^13), capped at 8 (typical |w| ~ 0.02 then sits near 5, its lo plane well inside the f16 normal range); 8 for an all-zero tensor.
inline int split_weight_exponent(float mx) {
    if (!(mx > 0.f)) return 8;
    int ex = 0;
    (void)std::frexp(mx, &ex);            // mx = m * 2^ex, m in [0.5, 1)
    return std::min(8, 13 - ex);
}

// One weight [N][K] as split-f16 rows in `out` with that scale, and 1 / scale in *inv (capi.hip; build_split under ee_finalize,
// ee_debug_xprobe and ee_debug_patch_project).  absmax_dev: one device float of scratch.  Synchronises s.  0, or the refusal in the name of `who`.
int split_weight_rows(ee_handle* h, const char* who, const float* w, int N, int K, float* out, float* absmax_dev, int num_cus, hipStream_t s, float* inv);

// The patch geometries the kernels take (ee_create, ee_debug_patch_project): whole patches, and float4 loads that stay inside one pixel
// row of one patch (P % 4, R % 4) over k-slabs of 32 (C P P % 32).
inline bool patch_geometry_ok(int C, int R, int P) { return C >= 1 && R >= 1 && P >= 1 && R % P == 0 && (C * P * P) % 32 == 0 && P % 4 == 0 && R % 4 == 0; }

// The fields every GEMM of a forward shares (capi_forward.hip; ee_debug_gemm_f32 starts from them too): scale 1, the static priority of the odd
// wave slots, the handle's error word.  A launch sets its own on top.
GemmArgs forward_gemm_args(int* err_flag);

// The patch projection (Conv2d with stride = kernel = a GEMM over flattened patches, HF:75-81): out [B * NP][H] = patches W^T + bias, as
// ee_forward and ee_debug_patch_project launch it (capi_forward.hip).  w_split given: launch_patch_split writes the patches once as split rows
// scaled by kSplitScaleX into split_rows ([B * NP][C P P] words) and the split kernel runs the GEMM; otherwise the f32 kernel gathers the
// patches itself.  prof: the handle whose ee_profile times the split launch, or null.
struct PatchProjection {
    const float* pix;                // [B][C][R][R]
    int B, C, R, P, H;
    const float *w, *bias;           // [H][C P P], [H]
    const float* w_split;            // split-f16 rows of w, or null
    float w_inv;                     //   and 1 / their scale
    float* split_rows;
    float* out;
    int use_dma;                     // GemmArgs::use_dma of the f32 form
    int *tile_counter, *err_flag;
};
void launch_patch_projection(const PatchProjection& p, int num_cus, hipStream_t s, ee_handle* prof);

// Stage 0 of a LayoutLMv3 call, as ee_forward and ee_embedding_inputs run it (capi_forward.hip): the packed layout of the batch, the text
// and visual embeddings into the handle's X / Xs, and the (B, H) means over every position that the embedding-level exits read.
// stage0_prep is launch_prep; stage0_embed is launch_embed_text, the patch projection, launch_embed_visual and one launch_pool_finish per
// mean that is asked for.  The forward builds its attention index between the two.  Both time their launches under the handle's ee_profile.
struct Stage0 {
    const int64_t *input_ids, *attention_mask, *bbox;
    const float* pixel_values;
    const int64_t *token_type_ids, *position_ids;
    const float* inputs_embeds;      // (B, T, H) read in place of the word-embedding rows, or null
    int B, T;
    int dense_rows;                  // MMEE_FLAG_DENSE_ROWS
    int slot;                        // which stage's doc_off / x_src / doc_orig / counts receive the layout (the forward: 0)
    float* pooled[3];                // by MMEE_EXIT_*: where the (B, H) mean goes; null: not computed
    int* patch_tile_counter;         // the patch GEMM's work-queue heads (zeroed), or null: static grid
};
void stage0_prep(ee_handle* h, const Stage0& a, hipStream_t s);
void stage0_embed(ee_handle* h, const Stage0& a, hipStream_t s);

// Device scratch of one entry point (the ee_debug_* hooks, ee_lte_targets): zeroed hipMalloc, freed on every way out of the scope.
struct Scratch {
    std::vector<void*> ptrs;
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    ~Scratch() { for (void* p : ptrs) (void)hipFree(p); }
    template <typename T>
    bool get(T** out, size_t count) {
        void* q = nullptr;
        if (hipMalloc(&q, count * sizeof(T) + 256) != hipSuccess) return false;
        ptrs.push_back(q);
        if (hipMemset(q, 0, count * sizeof(T) + 256) != hipSuccess) return false;
        *out = reinterpret_cast<T*>(q);
        return true;
    }
};

// kernel roles reported by ee_profile_read (their names: kProfNames in capi_query.hip)
enum { P_PREP = 0, P_EMBT, P_GPATCH, P_EMBV, P_GQKV, P_ATTN, P_GAO, P_LN, P_GUP, P_GDOWN, P_HEAD, P_DECIDE, P_COMPACT, P_GCLS, P_PROBE,
       P_PAIRIDX, P_PSPLIT, P_HEADOUT, P_EMIT, P_ENSEMBLE, P_QUOTA, P_CONTROLLER, P_DEADLINE, P_COUNT };

struct ProfScope {
    ee_handle* h;
    hipStream_t s;
    hipEvent_t b = nullptr;
    ProfScope(ee_handle* h_, int id, hipStream_t s_) : h(h_), s(s_) {
        if (!h->prof_on) return;
        if (h->prof_used == h->prof_pool.size()) {
            hipEvent_t a, bb;
            (void)hipEventCreate(&a);
            (void)hipEventCreate(&bb);
            h->prof_pool.push_back({a, bb});
        }
        auto& ev = h->prof_pool[h->prof_used++];
        h->prof_recs.push_back({id, ev.first, ev.second, 0.0});
        b = ev.second;
        (void)hipEventRecord(ev.first, s);
    }
    ~ProfScope() {
        if (b) (void)hipEventRecord(b, s);
    }
};

}  // namespace capi
}  // namespace mmee
