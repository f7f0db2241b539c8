// The forward schedule of libmmee_hip.so: the launch list of one ee_forward call (Forward), ee_forward itself and its captured-graph form
// (ee_graph_capture / ee_graph_launch / ee_graph_destroy).  Host code only enqueues: after an exit stage the number of surviving
// documents/rows lives in device memory and every later kernel sizes itself from it (persistent grid-stride launches), so there is no
// host-side control flow on the exit decision (the reference loops in Python, EE/policy.py:28-45).
#include <cmath>
#include <cstring>
#include <vector>

#include "capi_internal.h"

using namespace mmee;
using namespace mmee::capi;

// the fields every GEMM of the forward shares; a launch sets its own on top
GemmArgs mmee::capi::forward_gemm_args(int* err_flag) {
    GemmArgs g{};
    g.scale = 1.f; g.prio_mode = 1; g.err_flag = err_flag;
    return g;
}

void mmee::capi::launch_patch_projection(const PatchProjection& p, int num_cus, hipStream_t s, ee_handle* prof) {
    const int G = p.R / p.P, M = p.B * G * G;
    GemmArgs pg = forward_gemm_args(p.err_flag);
    pg.bias = p.bias; pg.C = p.out; pg.ldc = p.H; pg.m_static = M; pg.N = p.H;
    pg.K = p.C * p.P * p.P; pg.tile_counter = p.tile_counter;
    if (p.w_split) {
        auto split = [&] { mmee::launch_patch_split(p.pix, p.split_rows, p.B, p.C, p.R, p.P, mmee::kSplitScaleX, num_cus, s, p.err_flag); };
        if (prof) { ProfScope pp(prof, P_PSPLIT, s); split(); }
        else split();
        pg.A = p.split_rows; pg.lda = pg.K; pg.W = p.w_split; pg.alpha = p.w_inv / mmee::kSplitScaleX;
        launch_gemm_split(pg, EPI_BIAS, M, num_cus, s);
        return;
    }
    pg.W = p.w; pg.use_dma = p.use_dma;
    pg.pix = p.pix; pg.C_in = p.C; pg.R = p.R; pg.P = p.P; pg.G = G;
    launch_gemm_f32(pg, EPI_BIAS, AMODE_IM2COL, M, num_cus, s);
}

namespace {

// patch projection of the handle's model -> vis_raw [B * NP][H] (launch_patch_projection).  Split mode: the split patches are staged in H1,
// idle until the first FFN.
void handle_patch_projection(ee_handle* h, const float* pix, int B, int* tile_counter, hipStream_t s) {
    const ee_config& c = h->cfg;
    ProfScope ps(h, P_GPATCH, s);
    PatchProjection p{};
    p.pix = pix; p.B = B; p.C = c.num_channels; p.R = c.input_size; p.P = c.patch_size; p.H = c.hidden_size;
    p.w = h->patch_w; p.bias = h->patch_b; p.out = h->vis_raw;
    if (h->split && h->patch_s) { p.w_split = h->patch_s; p.w_inv = h->patch_inv; p.split_rows = h->H1; }
    p.tile_counter = tile_counter; p.err_flag = h->err_flag;
    launch_patch_projection(p, h->num_cus, s, h);
}

}  // namespace

// ---- LayoutLMv3, stage 0 (Stage0, capi_internal.h), shared by ee_forward and ee_embedding_inputs: the packed layout of the batch ... ----
void mmee::capi::stage0_prep(ee_handle* h, const Stage0& a, hipStream_t s) {
    const ee_config& c = h->cfg;
    const int G = c.input_size / c.patch_size;
    const size_t off = (size_t)a.slot * ((size_t)c.max_docs + 1);
    PrepArgs pa{};
    pa.input_ids = (const long long*)a.input_ids;
    pa.attention_mask = (const long long*)a.attention_mask;
    pa.bbox = (const long long*)a.bbox;
    pa.position_ids = (const long long*)a.position_ids;
    pa.token_type_ids = (const long long*)a.token_type_ids; pa.type_vocab = c.type_vocab_size;
    pa.B = a.B; pa.T = a.T; pa.Pv = G * G + 1; pa.G = G;
    pa.pad_id = c.pad_token_id; pa.vocab = c.vocab_size; pa.max_2d = c.max_2d_position_embeddings; pa.max_pos = c.max_position_embeddings;
    pa.dense_rows = a.dense_rows;
    pa.text_dst = h->text_dst; pa.emb_pos = h->emb_pos; pa.ntext = h->ntext;
    pa.doc_off = h->doc_off + off; pa.x_src = h->x_src + off; pa.doc_orig = h->doc_orig + off;
    pa.meta = h->meta[0]; pa.counts = h->counts + a.slot; pa.err_flag = h->err_flag;
    launch_prep(pa, s);
}

// ... text and visual embeddings, the inputs of the embedding exits
void mmee::capi::stage0_embed(ee_handle* h, const Stage0& a, hipStream_t s) {
    const ee_config& c = h->cfg;
    const int G = c.input_size / c.patch_size, Pv = G * G + 1, H = c.hidden_size, B = a.B, T = a.T;
    const int tch = (T + 31) / 32, vch = (Pv + 31) / 32;
    EmbedArgs ea{};
    ea.input_ids = (const long long*)a.input_ids; ea.token_type_ids = (const long long*)a.token_type_ids; ea.bbox = (const long long*)a.bbox;
    ea.emb_pos = h->emb_pos; ea.text_dst = h->text_dst; ea.ntext = h->ntext; ea.doc_off = h->doc_off + (size_t)a.slot * ((size_t)c.max_docs + 1);
    ea.B = B; ea.T = T; ea.Pv = Pv; ea.H = H; ea.cs = c.coordinate_size; ea.ss = c.shape_size; ea.max_2d = c.max_2d_position_embeddings;
    ea.vocab = c.vocab_size; ea.type_vocab = c.type_vocab_size;
    ea.inputs_embeds = a.inputs_embeds;
    ea.word = h->word; ea.type = h->type; ea.pos = h->pos; ea.xtab = h->xtab; ea.ytab = h->ytab; ea.htab = h->htab; ea.wtab = h->wtab;
    ea.ln1_g = h->emb_g; ea.ln1_b = h->emb_b; ea.eps1 = c.layer_norm_eps;
    ea.ln2_g = h->ln_g; ea.ln2_b = h->ln_b; ea.eps2 = c.layer_norm_eps;
    ea.X = h->X;
    if (h->split) { ea.Xs = h->Xs; ea.split_scale = mmee::kSplitScaleX; ea.err_flag = h->err_flag; }      // split mode: the embeddings exist as split planes only
    ea.text_part = a.pooled[MMEE_EXIT_TEXT_AVG] ? h->text_part : nullptr;
    ea.cat_part = a.pooled[MMEE_EXIT_TEXT_VISUAL_CONCAT] ? h->cat_part : nullptr;
    ea.cat_chunks = tch + vch;
    { ProfScope ps(h, P_EMBT, s); launch_embed_text(ea, s); }

    handle_patch_projection(h, a.pixel_values, B, a.patch_tile_counter, s);

    EmbedArgs va = ea;
    va.ln1_g = h->norm_g; va.ln1_b = h->norm_b; va.eps1 = 1e-6f;        // layoutlmv3.norm = LayerNorm(eps=1e-6), HF:563
    va.cls_token = h->cls_token; va.pos_embed = h->pos_embed; va.vis_raw = h->vis_raw;
    va.vis_part = a.pooled[MMEE_EXIT_VISION_AVG] ? h->vis_part : nullptr;
    {
        ProfScope ps(h, P_EMBV, s);
        launch_embed_visual(va, s);
        if (a.pooled[MMEE_EXIT_VISION_AVG]) launch_pool_finish(h->vis_part, vch, H, (float)Pv, a.pooled[MMEE_EXIT_VISION_AVG], B, s);
        if (a.pooled[MMEE_EXIT_TEXT_AVG]) launch_pool_finish(h->text_part, tch, H, (float)T, a.pooled[MMEE_EXIT_TEXT_AVG], B, s);
        if (a.pooled[MMEE_EXIT_TEXT_VISUAL_CONCAT])
            launch_pool_finish(h->cat_part, tch + vch, H, (float)(T + Pv), a.pooled[MMEE_EXIT_TEXT_VISUAL_CONCAT], B, s);
    }
}

namespace {

__global__ void zero_words_kernel(int* __restrict__ a, int na, int* __restrict__ b, int nb) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < na + nb; i += gridDim.x * blockDim.x) {
        if (i < na) a[i] = 0;
        else b[i - na] = 0;
    }
}

__global__ void set_thresholds_kernel(ThrPack p, double* __restrict__ dst) {
    for (int i = threadIdx.x; i < p.n; i += blockDim.x) dst[i] = p.v[i];
}

// What ee_forward and ee_graph_launch do in FRONT of the launch list: errors of earlier forwards (every finished one is looked at now; the
// slot this forward will use is waited for if need be), and the wait for the previous forward when it ran on another stream.
int forward_pre(ee_handle* h, hipStream_t s) {
    if (!h->fwd_done) HIP_OK(h, hipEventCreateWithFlags(&h->fwd_done, hipEventDisableTiming));
    if (!h->err_host) {
        HIP_OK(h, hipHostMalloc((void**)&h->err_host, sizeof(int) * ee_handle::kErrSlots, hipHostMallocDefault));
        memset(h->err_host, 0, sizeof(int) * ee_handle::kErrSlots);
        for (auto& es : h->errs) HIP_OK(h, hipEventCreateWithFlags(&es.done, hipEventDisableTiming));
    }
    {
        int e = take_errors(h, false, false);
        ee_handle::ErrSlot& mine = h->errs[h->err_seq % ee_handle::kErrSlots];
        if (!e && mine.pending) {
            (void)hipEventSynchronize(mine.done);
            e = take_errors(h, false, false);
        }
        if (e) return report_errors(h, e, "a PREVIOUS forward on this handle");
    }
    if (h->has_fwd && s != h->last_stream) HIP_OK(h, hipStreamWaitEvent(s, h->fwd_done, 0));
    return 0;
}

// ... and BEHIND it: the forward's error word into its own pinned slot, the events later calls wait on.
int forward_post(ee_handle* h, hipStream_t s) {
    const int k = (int)(h->err_seq % ee_handle::kErrSlots);
    HIP_OK(h, hipMemcpyAsync(h->err_host + k, h->err_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_OK(h, hipEventRecord(h->errs[k].done, s));
    h->errs[k].pending = true;
    ++h->err_seq;
    HIP_OK(h, hipEventRecord(h->fwd_done, s));
    h->last_stream = s; h->has_fwd = true;
    return 0;
}

// The arguments of one ee_forward / ee_graph_capture call (include/mmee.h).
struct ForwardArgs {
    const int64_t *input_ids, *attention_mask, *bbox;
    const float* pixel_values;
    const int64_t *token_type_ids, *position_ids;
    int32_t B, T;
    const double *thresholds, *temperatures;
    uint32_t flags;
    float* out_logits;
    int32_t* out_exit;
    float *out_conf, *out_all_logits, *out_all_crit, *out_head_logits, *out_head_crit, *out_hidden_cls;
    void* stream;
};

// The launch list of one forward.  cap == nullptr: the eager call (thresholds / temperatures are kernel arguments).  cap != nullptr: the call
// is being CAPTURED into a graph -- only enqueue operations are issued (no event, no host copy, no profiling), and the decide kernels read
// thresholds and temperatures from cap->thr_dev, so that one captured launch list serves every later threshold vector.
// One object per call: the steps below share the call's constants and move one stage cursor (cur ... cls_ready).
struct Forward {
    ee_handle* const h;
    const ForwardArgs a;
    const ee_handle::GraphRec* const cap;
    const ee_config& c = h->cfg;
    // the one-shot side inputs belong to THIS call whether it succeeds or not (a call that fails validation must not leave them armed)
    float* const hs_out = h->next_hidden_out;                  // (L+1, B, T+Pv, H), ee_set_hidden_states_out
    const float* const embeds_in = h->next_inputs_embeds;      // (B, T, H), ee_set_inputs_embeds
    const float* const head_mask = h->next_head_mask;          // (L, heads), ee_set_head_mask
    float* const attn_out = h->next_attn_out;                  // (L, B, heads, S, S), ee_set_attentions_out
    const hipStream_t s = reinterpret_cast<hipStream_t>(a.stream);
    const bool beit = c.arch == MMEE_ARCH_BEIT, sp = h->split, patience = c.criterion == MMEE_CRIT_PATIENCE;
    const bool no_exit = a.flags & MMEE_FLAG_NO_EXIT, probe_on = !(a.flags & MMEE_FLAG_WHOLE_LAYERS);
    // MMEE_FLAG_ONE_TERM: the layer GEMMs and the attention of a split-precision LayoutLMv3 handle on ONE f16 MFMA term (hi planes only): the
    // "bf16 throughput mode" of SURVEY 8d as a REPORTED deviation (bench.py `lowprec`), never a parity path; probes and heads keep three terms
    // (LayoutLMv3 handles only, as include/mmee.h says: on a BEiT / DiT handle validate() refuses the flag -- ADVICE r04: it used to give an
    // undocumented mix of one-term residual GEMMs and three-term everything else)
    const bool one_term = (a.flags & MMEE_FLAG_ONE_TERM) && sp && !beit;
    // MMEE_FLAG_LOW_LATENCY: the attention-output and FFN-down GEMMs of layer_rest as split-K, S per role from ee_low_latency_k_splits on the
    // call's STATIC row count (run() sets ks_ao / ks_down once the call is valid): the launch list stays a pure function of the call
    const bool low_latency = (a.flags & MMEE_FLAG_LOW_LATENCY) && sp && !beit;
    int ks_ao = 1, ks_down = 1;
    size_t ll_stride = 0;                    // floats between two parts: (rows padded to whole 128-row tiles) x H
    // MMEE_FLAG_STREAM_RESULTS: behind every exit's decide launch, the leavers' rows into the handle's pinned segment buffer and an event (result_stream.hip)
    const bool stream_results = a.flags & MMEE_FLAG_STREAM_RESULTS;
    // audited exits (ee_set_audit): every decide launch of the call is the AUDIT form; a dump-all call ignores the audit, everybody stays anyway
    const bool audit = h->audit_cut != 0 && !no_exit;
    // online exit control (ee_set_controller): every decide launch reads its threshold at h->ctl_thr_dev and audits under the call's own seed;
    // audit_tally_kernel and controller_step_kernel run behind the final exit.  A dump-all call ignores the controller: no step, no seed used
    const bool ctl = h->ctl_on && !no_exit;
    const float* fin_pol = nullptr;          // the rows the final exit's decide launch read, and the temperature it scaled them by
    double fin_temp = 1.0;
    // deadline exits (ee_set_deadline): deadline_begin_kernel opens the call, every decide launch reads its threshold at h->dl_thr and
    // deadline_check_kernel runs in front of each.  A dump-all call ignores the deadline: no launch added, no log row, no call counted
    const bool dl = h->dl_on && !no_exit;
    uint64_t dl_call = 0;                    // this call's number (1-based), set by deadline_begin
    // split precision attention: attention_idx.hip (pair index built once per forward; default) or, with MMEE_ATTN_V=2 or bucket tables
    // beyond 64 bins, attention_pair.hip (clamped Delta tables gathered per layer and head)
    const bool use_idx = sp && attn_variant() == 0 && c.rel_pos_bins <= 64 && c.rel_2d_pos_bins <= 64;
    const bool x_split = sp && !beit;        // LayoutLMv3, split mode: the embeddings and every layer output exist as split planes (Xs) only
    const int B = a.B, T = beit ? 0 : a.T;   // image-only: a document is its 197 visual rows
    const int H = c.hidden_size, I = c.intermediate_size, L = c.num_hidden_layers, K = c.num_labels, E = c.n_embedding_exits + c.n_encoder_exits;
    const int G = c.input_size / c.patch_size, NP = G * G, Pv = NP + 1, cus = h->num_cus;
    const size_t sstride = (size_t)c.max_docs + 1;
    int max_len = 0, max_rows = 0;           // rows of the longest document / of the batch, set once the call is valid
    // the stage cursor: the stage whose documents are active, its row metadata buffer, where its X rows are, the next exits
    int cur = 0, meta_cur = 0, exit_index = 0, next_enc = 0;
    const int* x_phys = nullptr;             // physical X row of every row of stage `cur`
    bool use_row_src = false;                // X rows are read through h->row_src (after a compaction, until a layer rewrites X densely)
    bool cls_ready = false;                  // the last layer was a probe: Xcs / cls_f32 hold the final classifier's input
    bool vision_only = false;                // run_vision: the call ends behind exit 0, nothing is compacted for a layer to read

    // diagnostic library only: MMEE_ATTN_V=2 forces attention_pair.hip (A/B)
    static int attn_variant() { static const int v = mmee::diag_env_int("MMEE_ATTN_V", 0); return v; }

    Forward(ee_handle* h_, const ForwardArgs& a_, const ee_handle::GraphRec* cap_) : h(h_), a(a_), cap(cap_) {
        h->next_hidden_out = nullptr;
        h->next_inputs_embeds = nullptr;
        h->next_head_mask = nullptr;
        h->next_attn_out = nullptr;
    }

    int* S_doc_orig(int st) const { return h->doc_orig + st * sstride; }
    int* S_doc_off(int st) const { return h->doc_off + st * sstride; }
    int* S_x_src(int st) const { return h->x_src + st * sstride; }
    int* S_meta_src(int st) const { return h->meta_src + st * sstride; }

    int validate() const {
        if (!h->finalized) return fail(h, "ee_forward: call ee_finalize after loading the parameters");
        if (!a.pixel_values || !a.out_exit || (!beit && (!a.input_ids || !a.bbox)))
            return fail(h, "ee_forward: pixel_values and out_exit (and input_ids, bbox for LayoutLMv3) are required");
        if (B < 1 || B > c.max_docs) return fail(h, "ee_forward: B=%d outside [1, max_docs=%d]", B, c.max_docs);
        if (!beit && (T < 1 || T > c.max_text_len)) return fail(h, "ee_forward: T=%d outside [1, max_text_len=%d]", T, c.max_text_len);
        if (!a.thresholds && !cap && !patience && !no_exit && h->quota_mode != MMEE_QUOTA_EXACT && !ctl)
            return fail(h, "ee_forward: thresholds required unless MMEE_FLAG_NO_EXIT, MMEE_CRIT_PATIENCE or MMEE_QUOTA_EXACT");
        if (ctl && cap)
            return fail(h, "ee_graph_capture: a controller is set: its seed changes per call and the step reads the call's own results, so controlled "
                           "calls are eager (not built; ee_set_controller(h, NULL, ...) first)");
        if (ctl && a.thresholds)
            return fail(h, "ee_forward: thresholds are given while a controller is set: the controller's position decides them "
                           "(pass NULL, or ee_set_controller(h, NULL, ...) first)");
        if (ctl && !a.out_logits)
            return fail(h, "ee_forward: out_logits is NULL while a controller is set: the loss compares the delivered row with the final exit's");
        if (ctl && stream_results)
            return fail(h, "ee_forward: MMEE_FLAG_STREAM_RESULTS while a controller is set: its audit keeps delivered documents in the stage, which "
                           "emit_leavers cannot tell from the ones that stay (not built; ee_set_controller(h, NULL, ...) first)");
        if (dl && cap)
            return fail(h, "ee_graph_capture: a deadline is set: the call number and the budget travel by value and the begin launch stamps the "
                           "call's own start, so deadline calls are eager (not built; ee_set_deadline(h, MMEE_DEADLINE_OFF, NULL) first)");
        if (dl && (patience || h->rule != MMEE_RULE_PLAIN || c.use_lte || h->quota_mode != MMEE_QUOTA_OFF || h->audit_cut || ctl))
            return fail(h, "ee_forward: a deadline is set together with MMEE_CRIT_PATIENCE, a non-plain exit rule, use_lte, quotas, an audit or a "
                           "controller: a cut must fire at once and for everybody (ee_set_deadline(h, MMEE_DEADLINE_OFF, NULL) first)");
        if (h->quota_mode != MMEE_QUOTA_OFF && (patience || h->rule != MMEE_RULE_PLAIN || c.use_lte))
            return fail(h, "ee_forward: quotas are set, and no rank is defined under MMEE_CRIT_PATIENCE, MMEE_RULE_STREAK / MMEE_RULE_EITHER or use_lte "
                           "(ee_set_quotas(h, NULL, 0, 0) first)");
        if (patience && !h->has_patience() && !no_exit)
            return fail(h, "ee_forward: the patience criterion needs ee_set_patience(h, t) with t >= 1 before the first forward");
        if (h->rule != MMEE_RULE_PLAIN && patience)
            return fail(h, "ee_forward: MMEE_RULE_STREAK / MMEE_RULE_EITHER build on a threshold event, which MMEE_CRIT_PATIENCE does not have");
        if (h->rule != MMEE_RULE_PLAIN && !h->has_patience() && !no_exit)
            return fail(h, "ee_forward: MMEE_RULE_STREAK / MMEE_RULE_EITHER need a patience: ee_set_patience or ee_set_patience_vector before the forward");
        if ((head_mask || attn_out) && (a.flags & (MMEE_FLAG_NO_EXIT | MMEE_FLAG_WHOLE_LAYERS)) != (MMEE_FLAG_NO_EXIT | MMEE_FLAG_WHOLE_LAYERS))
            return fail(h, "ee_forward: head_mask / attention maps exist in dump-all mode with whole layers only (MMEE_FLAG_NO_EXIT | MMEE_FLAG_WHOLE_LAYERS)");
        if ((head_mask || attn_out) && beit) return fail(h, "ee_forward: head_mask / attention maps are built for the LayoutLMv3 layers only");
        if (attn_out && (!(a.flags & MMEE_FLAG_DENSE_ROWS) || !mmee::attention_probs_supports(T + Pv)))
            return fail(h, "ee_forward: attention maps are (B, heads, S, S) in the padded layout: pass MMEE_FLAG_DENSE_ROWS (S <= 1280)");
        if ((a.flags & MMEE_FLAG_ONE_TERM) && (beit || !sp))
            return fail(h, "ee_forward: MMEE_FLAG_ONE_TERM exists for MMEE_PREC_F32_SPLIT LayoutLMv3 handles only");
        if ((a.flags & MMEE_FLAG_LOW_LATENCY) && (beit || !sp))
            return fail(h, "ee_forward: MMEE_FLAG_LOW_LATENCY exists for MMEE_PREC_F32_SPLIT LayoutLMv3 handles only (the split-K residual GEMMs are "
                           "split-precision kernels; %s)", beit ? "this is an MMEE_ARCH_BEIT handle" : "this is an MMEE_PREC_F32 handle");
        if ((a.flags & MMEE_FLAG_LOW_LATENCY) && (a.flags & MMEE_FLAG_ONE_TERM))
            return fail(h, "ee_forward: MMEE_FLAG_LOW_LATENCY together with MMEE_FLAG_ONE_TERM: the split-K parts are three-term GEMMs, the one-term mode "
                           "is a reported deviation; pick one");
        if (hs_out && (a.flags & (MMEE_FLAG_NO_EXIT | MMEE_FLAG_WHOLE_LAYERS)) != (MMEE_FLAG_NO_EXIT | MMEE_FLAG_WHOLE_LAYERS))
            return fail(h, "ee_forward: hidden states are collected in dump-all mode with whole layers only (MMEE_FLAG_NO_EXIT | MMEE_FLAG_WHOLE_LAYERS)");
        if (stream_results && no_exit)
            return fail(h, "ee_forward: MMEE_FLAG_STREAM_RESULTS together with MMEE_FLAG_NO_EXIT: nobody leaves early in dump-all mode, there is nothing to stream");
        if (stream_results && cap)
            return fail(h, "ee_graph_capture: MMEE_FLAG_STREAM_RESULTS belongs to eager calls (the events between the launches are not part of a captured "
                           "launch list)");
        if (audit && stream_results)
            return fail(h, "ee_forward: MMEE_FLAG_STREAM_RESULTS while an audit is set: emit_leavers infers who left from stage membership, and an audited "
                           "document stays in the stage after its result is out (not built; ee_set_audit(h, 0, 0, 0) first)");
        if (stream_results && (!a.out_logits || !a.out_conf))
            return fail(h, "ee_forward: MMEE_FLAG_STREAM_RESULTS needs out_logits and out_conf (a streamed row carries both)");
        if (cap && (hs_out || embeds_in || head_mask || attn_out || h->prof_on))
            return fail(h, "ee_graph_capture: the one-shot side inputs / outputs (inputs_embeds, hidden states, head mask, attention maps) and ee_profile "
                           "belong to eager calls");
        return 0;
    }

    int* next_head() {                    // 8 XCD-local counters x 16 ints (one 64-byte line each); null when they run out: static grid
        if (h->next_queue_head + 128 > h->n_queue_heads) return nullptr;
        int* p = h->queue_heads + h->next_queue_head;
        h->next_queue_head += 128;
        return p;
    }

    GemmArgs gemm_args() const { return forward_gemm_args(h->err_flag); }

    void run_gemm(GemmArgs g, int epi) {
        g.terms = one_term ? 1 : 3;
        if (sp) launch_gemm_split(g, epi, max_rows, cus, s);
        else launch_gemm_f32(g, epi, AMODE_ROWS, max_rows, cus, s);
    }

    // ---- the four layer GEMMs, each described once: everything that depends only on the layer's weights and on the precision -- the weight
    // plane, bias, N, K, the alpha that undoes (weight scale x scale of the input planes), the scale an output written as split planes gets,
    // BEiT's layer scale (lam1 / lam2: null for LayoutLMv3).  split: the split-f16 planes (`sp` for the layer, always for a probe).  The
    // caller adds what differs between launches: rows, buffers, residual, m_ptr, probe / role_tag, k_splits, tile_counter.
    // Q alone: W_q is the first H rows of the fused Q | K | V weight; Q is pre-divided by sqrt(d) (HF:263)
    GemmArgs q_gemm(const LayerW& w, bool split) const {
        GemmArgs g = gemm_args();
        g.W = split ? w.qkv_s : w.qkv_w; g.bias = w.qkv_b; g.N = H; g.K = H; g.alpha = w.qkv_inv / mmee::kSplitScaleX; g.scale_cols = H; g.scale = 0.125f;
        return g;
    }
    GemmArgs qkv_gemm(const LayerW& w, bool split) const {
        GemmArgs g = q_gemm(w, split);
        g.N = 3 * H; g.out_split = split ? 1 : 0; g.out_scale = mmee::kSplitScaleQKV;
        return g;
    }
    GemmArgs attn_out_gemm(const LayerW& w, bool split) const {      // reads the attention context (kSplitScaleCtx)
        GemmArgs g = gemm_args();
        g.W = split ? w.ao_s : w.ao_w; g.bias = w.ao_b; g.N = H; g.K = H; g.alpha = w.ao_inv / mmee::kSplitScaleCtx; g.col_scale = w.lam1;
        return g;
    }
    GemmArgs ffn_up_gemm(const LayerW& w, bool split) const {        // reads a LayerNorm output (kSplitScaleX), writes GELU rows (kSplitScaleH1)
        GemmArgs g = gemm_args();
        g.W = split ? w.f1_s : w.f1_w; g.bias = w.f1_b; g.N = I; g.K = H;
        g.alpha = w.f1_inv / mmee::kSplitScaleX; g.out_split = split ? 1 : 0; g.out_scale = mmee::kSplitScaleH1;
        return g;
    }
    GemmArgs ffn_down_gemm(const LayerW& w, bool split) const {      // reads the GELU rows (kSplitScaleH1)
        GemmArgs g = gemm_args();
        g.W = split ? w.f2_s : w.f2_w; g.bias = w.f2_b; g.N = H; g.K = I; g.alpha = w.f2_inv / mmee::kSplitScaleH1; g.col_scale = w.lam2;
        return g;
    }

    // LayerNorm of the rows src[rows[r]] (rows null: dense) into f32 rows (dst) or split planes scaled by kSplitScaleX (dst_split)
    void ln_rows(const float* src, const int* rows, float* dst, float* dst_split, const float* gamma, const float* beta, const int* n_ptr, int max_n) {
        launch_ln_rows(src, dst, rows, n_ptr, max_n, H, gamma, beta, c.layer_norm_eps, cus, s, dst_split, mmee::kSplitScaleX, h->err_flag);
    }

    // low latency: LayerNorm of the rows completed from the S split-K parts in ll_part (+ bias + residual row resid[resid_rows[r]]; null: dense)
    // into split planes
    void ln_parts(const float* bias, const float* resid, const int* resid_rows, float* dst_split, const float* gamma, const float* beta, int parts,
                  const int* n_ptr) {
        launch_ln_rows(h->ll_part, nullptr, nullptr, n_ptr, max_rows, H, gamma, beta, c.layer_norm_eps, cus, s, dst_split, mmee::kSplitScaleX, h->err_flag,
                       parts, ll_stride, bias, resid, resid_rows, 1.0f / mmee::kSplitScaleX);
    }

    // the layer output X as its readers find it: split planes of Xs (scaled by kSplitScaleX) or f32 rows of X
    const float* x_out() const { return x_split ? h->Xs : h->X; }
    float x_inv() const { return x_split ? 1.0f / mmee::kSplitScaleX : 0.f; }

    void patch_projection() { handle_patch_projection(h, a.pixel_values, B, next_head(), s); }

    // ---- BEiT / DiT: uniform 197-row documents, BeitEmbeddings = patch conv + cls + absolute position embeddings ----
    void embed_beit() {
        { ProfScope ps(h, P_PREP, s); launch_prep_uniform(B, Pv, S_doc_off(0), S_x_src(0), S_doc_orig(0), h->meta[0], h->counts, s); }
        patch_projection();
        { ProfScope ps(h, P_EMBV, s); launch_embed_beit(h->vis_raw, h->cls_token, c.use_abs_pos ? h->pos_embed : nullptr, B, Pv, H, h->X, s); }
    }

    // ---- LayoutLMv3: stage 0 (stage0_prep / stage0_embed above), with the attention index of the call's layers between its two halves ----
    void embed_layoutlmv3() {
        Stage0 st{};
        st.input_ids = a.input_ids; st.attention_mask = a.attention_mask; st.bbox = a.bbox; st.pixel_values = a.pixel_values;
        st.token_type_ids = a.token_type_ids; st.position_ids = a.position_ids; st.inputs_embeds = embeds_in;
        st.B = B; st.T = T; st.dense_rows = (a.flags & MMEE_FLAG_DENSE_ROWS) ? 1 : 0; st.slot = 0;
        for (int i = 0; i < c.n_embedding_exits; ++i) st.pooled[c.embedding_exits[i]] = h->pooled[c.embedding_exits[i]];
        {
            ProfScope ps(h, P_PREP, s);
            stage0_prep(h, st, s);
            // attention_pair.hip skips the key flags in the full key tiles of a document without a masked key inside: one word per document
            if (sp && !use_idx) launch_doc_flags(h->meta[0], S_doc_off(0), B, h->doc_flags, s);
            if (h->pair_idx && use_idx) {    // bucket indices of every (query, key) pair, once per forward: shared by all heads and layers
                ProfScope pi(h, P_PAIRIDX, s);
#ifdef MMEE_DIAG
                if (h->idx16)
                    mmee::launch_pair_index16(h->meta[0], S_doc_off(0), B, h->idx_nb, h->lut1_dev, h->c1, h->n1, h->lut2_dev, h->c2, h->n2, c.rel_pos_bins,
                                              h->pair_idx, h->idx_stride, h->pair_idx0, h->keymask, h->doc_flags, max_len, s);
                else
#endif
                    mmee::launch_pair_index(h->meta[0], S_doc_off(0), B, h->idx_nb, h->lut1_dev, h->c1, h->n1, h->lut2_dev, h->c2, h->n2, c.rel_pos_bins,
                                            h->pair_idx, h->idx_stride, max_len, s);
            }
        }
        st.patch_tile_counter = next_head();
        stage0_embed(h, st, s);
    }

    // Q | K | V projection of every row of the stage, A row r read from A[rows[r]] (rows null: dense)
    void qkv(int l, const float* A, const int* rows) {
        const LayerW& w = h->layers[l];
        GemmArgs g = qkv_gemm(w, sp);
        g.A = A; g.lda = H; g.row_src = rows; g.C = h->QKV; g.ldc = 3 * H; g.m_ptr = &h->counts[cur].n_rows; g.tile_counter = next_head();
        { ProfScope ps(h, P_GQKV, s); run_gemm(g, EPI_BIAS); }
        h->rec.layer_qkv_stage[l] = cur;
    }

    // BEiT (pre-LN): layernorm_before of the stage's rows into CTX, the Q | K | V projection from there
    void beit_qkv(int l, const int* rows) {
        const LayerW& w = h->layers[l];
        { ProfScope ps(h, P_LN, s); ln_rows(h->X, rows, sp ? nullptr : h->CTX, sp ? h->CTX : nullptr, w.ao_g, w.ao_beta, &h->counts[cur].n_rows, max_rows); }
        qkv(l, h->CTX, nullptr);
    }

    // attention over the documents of the stage (Q | K | V in QKV, context into CTX)
    AttnArgs attn_args() {
        AttnArgs at{};
        at.qkv = h->QKV; at.ld = 3 * H; at.ctx = h->CTX; at.ldc = H; at.meta = h->meta[meta_cur]; at.doc_off = S_doc_off(cur);
        at.counts = &h->counts[cur]; at.t1 = h->t1; at.tx = h->tx; at.ty = h->ty; at.n1 = h->n1; at.c1 = h->c1; at.n2 = h->n2; at.c2 = h->c2;
        at.H = H; at.heads = c.num_attention_heads; at.max_len = max_len; at.item_counter = next_head();
        at.ctx_split = sp ? 1 : 0; at.err_flag = h->err_flag; at.ctx_scale = mmee::kSplitScaleCtx; at.qkv_scale = mmee::kSplitScaleQKV;
        at.terms = one_term ? 1 : 3;
        at.pair_idx = (use_idx && !beit) ? h->pair_idx : nullptr;
        at.idx_doc_stride = h->idx_stride; at.idx_nb = h->idx_nb; at.doc_orig = S_doc_orig(cur);
        at.w1 = h->rel1; at.wx = h->relx; at.wy = h->rely; at.bins1 = c.rel_pos_bins; at.bins2 = c.rel_2d_pos_bins;
        at.inv_sqrt_d = 1.0f / std::sqrt((float)(H / c.num_attention_heads));
        at.idx16 = (h->idx16 && at.pair_idx) ? 1 : 0; at.lut1 = h->lut1_dev; at.n_visual = Pv; at.keymask = h->keymask; at.doc_flags = h->doc_flags;
        return at;
    }

    // BEiT has no relative-position bias (at.pair_idx is null, the kernel masks the last key tile's tail), so its split attention takes
    // attention_idx.hip whenever that kernel supports the shape; LayoutLMv3 only when the pair index is built (use_idx)
    void run_attn(const AttnArgs& at) {
        if (sp && (beit || use_idx) && mmee::attention_idx_supports(at)) mmee::launch_attention_idx(at, B, cus, s);
        else if (sp) launch_attention_pair(at, B, cus, c.max_rel_pos, c.max_rel_2d_pos, s);
        else launch_attention_f32(at, B, cus, s);
    }

    // ---- BEiT / DiT layer (BEIT:406-444: pre-LN, layer scale), in the same three pieces as the LayoutLMv3 layer below -----------
    // LN output and attention output take turns in the CTX buffer; the residual stream X / Y stays f32.  The rest of the layer after
    // Q | K | V, on the rows of stage `cur`; x_rows, qkv_off as in layer_rest
    void beit_rest(int l, const int* x_rows, const int* qkv_off) {
        const LayerW& w = h->layers[l];
        const int* rp = &h->counts[cur].n_rows;
        AttnArgs at = attn_args();
        at.qkv_doc_off = qkv_off;
        { ProfScope ps(h, P_ATTN, s); run_attn(at); }
        GemmArgs g = attn_out_gemm(w, sp);        // Y = X + lambda_1 * (ctx Wo^T + bo)
        g.A = h->CTX; g.lda = H; g.C = h->Y; g.ldc = H; g.resid = h->X; g.ldr = H; g.resid_row_src = x_rows; g.m_ptr = rp; g.tile_counter = next_head();
        { ProfScope ps(h, P_GAO, s); run_gemm(g, EPI_RESID); }
        { ProfScope ps(h, P_LN, s); ln_rows(h->Y, nullptr, sp ? nullptr : h->CTX, sp ? h->CTX : nullptr, w.f_g, w.f_beta, rp, max_rows); }
        g = ffn_up_gemm(w, sp);
        g.A = h->CTX; g.lda = H; g.C = h->H1; g.ldc = I; g.m_ptr = rp; g.tile_counter = next_head();
        { ProfScope ps(h, P_GUP, s); run_gemm(g, EPI_GELU); }
        g = ffn_down_gemm(w, sp);      // X = Y + lambda_2 * (h1 W2^T + b2)
        g.A = h->H1; g.lda = I; g.C = h->X; g.ldc = H; g.resid = h->Y; g.ldr = H; g.m_ptr = rp; g.tile_counter = next_head();
        { ProfScope ps(h, P_GDOWN, s); run_gemm(g, EPI_RESID); }
        h->rec.layer_stage[l] = cur;
    }

    // CLS probe of a BEiT layer (split precision): the exit head reads the CLS row of X (f32), which lands in Xc
    void beit_probe(int l) {
        const LayerW& w = h->layers[l];
        ProfScope ps(h, P_PROBE, s);
        const int* nd = &h->counts[cur].n_docs;
        AttnArgs at = attn_args();
        at.q_limit = 32; at.max_len = max_len < 32 ? max_len : 32;
        run_attn(at);
        GemmArgs g = attn_out_gemm(w, true);
        g.A = h->CTX; g.lda = H; g.row_src = S_doc_off(cur); g.C = h->Yc; g.ldc = H;
        g.resid = h->X; g.ldr = H; g.resid_row_src = x_phys; g.probe = 1; g.m_ptr = nd;
        launch_gemm_split(g, EPI_RESID, B, cus, s);
        ln_rows(h->Yc, nullptr, nullptr, h->Ycs, w.f_g, w.f_beta, nd, B);
        g = ffn_up_gemm(w, true);
        g.A = h->Ycs; g.lda = H; g.C = h->H1c; g.ldc = I; g.m_ptr = nd; g.probe = 1;
        launch_gemm_split(g, EPI_GELU, B, cus, s);
        g = ffn_down_gemm(w, true);
        g.A = h->H1c; g.lda = I; g.C = h->Xc; g.ldc = H; g.resid = h->Yc; g.ldr = H; g.probe = 1; g.m_ptr = nd;
        launch_gemm_split(g, EPI_RESID, B, cus, s);
        h->rec.layer_probe_stage[l] = cur;
    }

    // ---- LayoutLMv3 layer (HF:485-512), in three pieces so that an exit layer can decide BEFORE its bulk runs ----------------
    // attention, attention output dense + residual + LayerNorm (HF:299-303), FFN + residual + LayerNorm, on the rows of stage `cur`;
    // x_rows: physical Xs row of every row of the stage (null: dense), qkv_off: where the documents' Q | K | V rows are (null: dense)
    void layer_rest(int l, const int* x_rows, const int* qkv_off) {
        const LayerW& w = h->layers[l];
        const int* rp = &h->counts[cur].n_rows;
        AttnArgs at = attn_args();
        at.qkv_doc_off = qkv_off;
        { ProfScope ps(h, P_ATTN, s); run_attn(at); }
        // side kernels of the reference signature's output_attentions / head_mask (dump-all, whole layers: attention_maps.hip)
        if (attn_out)
            mmee::launch_attention_probs(h->QKV, 3 * H, sp ? 1 : 0, mmee::kSplitScaleQKV, h->meta[meta_cur], S_doc_off(cur), h->t1, h->tx, h->ty, h->n1, h->c1,
                                         h->n2, h->c2, H, c.num_attention_heads, max_len, B, head_mask ? head_mask + (size_t)l * c.num_attention_heads : nullptr,
                                         attn_out + (size_t)l * B * c.num_attention_heads * max_len * max_len, s);
        if (head_mask)
            mmee::launch_head_scale_ctx(h->CTX, H, rp, max_rows, H, head_mask + (size_t)l * c.num_attention_heads, sp ? 1 : 0, mmee::kSplitScaleCtx, cus,
                                        h->err_flag, s);
        GemmArgs g = attn_out_gemm(w, sp);
        g.A = h->CTX; g.lda = H; g.role_tag = 2; g.m_ptr = rp;
        if (ks_ao > 1) {
            // low latency: S parts of alpha * acc into ll_part, no bias; the LayerNorm launch adds the parts in order, the bias, the residual
            // (Xs read through x_rows after a compaction) and writes Ys
            g.bias = nullptr; g.C = h->ll_part; g.ldc = H; g.k_splits = ks_ao; g.split_stride = ll_stride;
            { ProfScope ps(h, P_GAO, s); run_gemm(g, EPI_BIAS); }
            { ProfScope ps(h, P_LN, s); ln_parts(w.ao_b, h->Xs, x_rows, h->Ys, w.ao_g, w.ao_beta, ks_ao, rp); }
        } else {
            g.C = h->Y; g.ldc = H; g.resid = sp ? h->Xs : h->X; g.ldr = H; g.resid_row_src = x_rows;
            g.resid_split_inv = sp ? 1.0f / mmee::kSplitScaleX : 0.f; g.tile_counter = next_head();
            { ProfScope ps(h, P_GAO, s); run_gemm(g, EPI_RESID); }
            // split mode: the LayerNorm output exists only as split planes (22 bits); its readers (next GEMM, residual adds, exit heads) take it from there
            { ProfScope ps(h, P_LN, s); ln_rows(h->Y, nullptr, sp ? nullptr : h->Y, sp ? h->Ys : nullptr, w.ao_g, w.ao_beta, rp, max_rows); }
        }
        g = ffn_up_gemm(w, sp);
        g.A = sp ? h->Ys : h->Y; g.lda = H; g.C = h->H1; g.ldc = I; g.m_ptr = rp; g.tile_counter = next_head();
        { ProfScope ps(h, P_GUP, s); run_gemm(g, EPI_GELU); }
        g = ffn_down_gemm(w, sp);
        g.A = h->H1; g.lda = I; g.role_tag = 3; g.m_ptr = rp;
        if (ks_down > 1) {      // the same with the FFN's bias, the residual Ys (dense: this layer wrote it) and Xs as the output
            g.bias = nullptr; g.C = h->ll_part; g.ldc = H; g.k_splits = ks_down; g.split_stride = ll_stride;
            { ProfScope ps(h, P_GDOWN, s); run_gemm(g, EPI_BIAS); }
            { ProfScope ps(h, P_LN, s); ln_parts(w.f2_b, h->Ys, nullptr, h->Xs, w.f_g, w.f_beta, ks_down, rp); }
        } else {
            g.C = h->X; g.ldc = H; g.resid = sp ? h->Ys : h->Y; g.ldr = H;
            g.resid_split_inv = sp ? 1.0f / mmee::kSplitScaleX : 0.f; g.tile_counter = next_head();
            { ProfScope ps(h, P_GDOWN, s); run_gemm(g, EPI_RESID); }
            { ProfScope ps(h, P_LN, s); ln_rows(h->X, nullptr, sp ? nullptr : h->X, sp ? h->Xs : nullptr, w.f_g, w.f_beta, rp, max_rows); }
        }
        h->rec.layer_stage[l] = cur;
    }

    // CLS probe: the layer's output for the CLS row of every active document, nothing else.  The exit head (and the final classifier)
    // only ever read that row, and a row's arithmetic does not depend on which other rows share its launch, so the value is the one
    // the whole layer would have produced, bit for bit (tests/test_gpu_api.py: early exit == the dump-all row; the dump runs whole layers).
    // fin: the layer's decision is the final classifier's
    void layer_probe(int l, bool fin, bool xspace) {
        const LayerW& w = h->layers[l];
        ProfScope ps(h, P_PROBE, s);
        const int* nd = &h->counts[cur].n_docs;
        if (xspace) {
            // X-space probe (xprobe.hip): Q of the CLS rows (W_q = the first H rows of the fused weight), then the context rows without K | V
            GemmArgs gq = q_gemm(w, true);       // f32 rows into Qc: no output split
            gq.A = h->Xs; gq.lda = H; gq.row_src = x_phys; gq.C = h->Qc; gq.ldc = H; gq.m_ptr = nd; gq.probe = 1;
            launch_gemm_split(gq, EPI_BIAS, B, cus, s);
            mmee::XProbeArgs xa{};
            xa.xs = reinterpret_cast<const char*>(h->Xs); xa.xs_inv = 1.0f / mmee::kSplitScaleX; xa.x_phys = x_phys; xa.doc_off = S_doc_off(cur);
            xa.doc_orig = S_doc_orig(cur); xa.counts = &h->counts[cur]; xa.qc = h->Qc;
            xa.wk = w.qkv_w + (size_t)H * H; xa.bk = w.qkv_b + H; xa.wv_s = w.qkv_s + (size_t)2 * H * H; xa.wv_inv = w.qkv_inv; xa.bv = w.qkv_b + 2 * H;
            xa.u = h->xp_u; xa.s0 = h->xp_s0; xa.cvec = h->xp_c; xa.order = h->xp_order; xa.ticket = h->xp_order + B; xa.ctx = h->CTX; xa.ctx_scale = mmee::kSplitScaleCtx;
            xa.pair_idx = h->idx16 ? h->pair_idx0 : h->pair_idx; xa.idx_doc_stride = h->idx16 ? (size_t)h->idx_nb * 1024 : h->idx_stride; xa.w1 = h->rel1; xa.wx = h->relx; xa.wy = h->rely;
            xa.bins1 = c.rel_pos_bins; xa.bins2 = c.rel_2d_pos_bins; xa.inv_sqrt_d = 1.0f / std::sqrt((float)(H / c.num_attention_heads));
            xa.H = H; xa.heads = c.num_attention_heads; xa.err_flag = h->err_flag;
            mmee::launch_xprobe(xa, B, max_len, cus, s);
            h->rec.layer_xprobe[l] = 1;
        } else {
            AttnArgs at = attn_args();
            at.q_limit = 32; at.max_len = max_len < 32 ? max_len : 32;     // the first 32-query block of every document; row 0 is used
            run_attn(at);
        }
        // the probe GEMMs are a few dozen tiles: static tile assignment (no queue: the pops would cost more than the tiles)
        GemmArgs g = attn_out_gemm(w, true);        // CLS rows only: A = context row doc_off[i], residual = the document's CLS row of Xs
        g.A = h->CTX; g.lda = H; g.row_src = S_doc_off(cur); g.C = h->Yc; g.ldc = H;
        g.resid = h->Xs; g.ldr = H; g.resid_row_src = x_phys; g.resid_split_inv = 1.0f / mmee::kSplitScaleX; g.probe = 1; g.m_ptr = nd;
        launch_gemm_split(g, EPI_RESID, B, cus, s);
        ln_rows(h->Yc, nullptr, nullptr, h->Ycs, w.ao_g, w.ao_beta, nd, B);
        g = ffn_up_gemm(w, true);
        g.A = h->Ycs; g.lda = H; g.C = h->H1c; g.ldc = I; g.m_ptr = nd; g.probe = 1;
        launch_gemm_split(g, EPI_GELU, B, cus, s);
        g = ffn_down_gemm(w, true);
        g.A = h->H1c; g.lda = I; g.probe = 1; g.m_ptr = nd;
        constexpr int kSplitK = 4;
        if (xspace && h->xp_part && (I / 32) % kSplitK == 0) {
            // X space (already a re-association of the whole-layer arithmetic): the 96-stage k-loop of this one-row-per-document GEMM
            // is divided over four workgroups per tile; the LayerNorm kernel adds the four parts in order, the bias and the residual
            g.bias = nullptr; g.C = h->xp_part; g.ldc = H; g.k_splits = kSplitK; g.split_stride = (size_t)B * H;
            launch_gemm_split(g, EPI_BIAS, B, cus, s);
            launch_ln_rows(h->xp_part, nullptr, nullptr, nd, B, H, w.f_g, w.f_beta, c.layer_norm_eps, cus, s, h->Xcs, mmee::kSplitScaleX, h->err_flag,
                           kSplitK, (size_t)B * H, w.f2_b, h->Ycs, nullptr, 1.0f / mmee::kSplitScaleX);
        } else {
            g.C = h->Xc; g.ldc = H; g.resid = h->Ycs; g.ldr = H; g.resid_split_inv = 1.0f / mmee::kSplitScaleX;
            launch_gemm_split(g, EPI_RESID, B, cus, s);
            ln_rows(h->Xc, nullptr, nullptr, h->Xcs, w.f_g, w.f_beta, nd, B);
        }
        // the f32 copy of the CLS rows is read by a head WITHOUT a dense layer on the split kernel only (one-layer heads): the others take Xcs
        const HeadW* hw0 = fin ? &h->classifier : &h->enc_heads[next_enc];
        const bool gate = !fin && c.strategy == MMEE_STRATEGY_GATE;
        const bool dense_ok = hw0->dense_w && hw0->dense_s && (!gate || (h->classifier.dense_w && h->classifier.dense_s));
        if (!dense_ok) launch_gather_cls(h->Xcs, H, h->iota, nullptr, nd, h->cls_f32, B, s, 1.0f / mmee::kSplitScaleX);
        h->rec.layer_probe_stage[l] = cur;
    }

    // in_split / split_rows: the same input rows as split planes (LayerNorm outputs scaled by kSplitScaleX), when they exist: the head's
    // dense then runs on the split GEMM kernel (128 x 128 tiles of the CLS-probe launches) instead of the f32 MFMA kernel
    // lte: the launch of the output projection also leaves the LTE scores of these rows in h->lte_score (head_out_lte_kernel)
    struct LteRows { const float* in; int ld; const int* gather; float split_inv; };
    void run_head(const HeadW& hw, const float* in, int ld, const int* gather, float* hid, float* out, const float* in_split, const int* split_rows,
                  const LteRows* lte = nullptr) {
        const int* n_docs_ptr = &h->counts[cur].n_docs;
        const float* hin = in;
        int hld = ld;
        const int* hg = gather;
        if (hw.dense_w && hw.dense_s && in_split) {
            GemmArgs g = gemm_args();
            g.A = in_split; g.lda = H; g.row_src = split_rows; g.W = hw.dense_s; g.bias = hw.dense_b; g.C = hid; g.ldc = H;
            g.m_ptr = n_docs_ptr; g.N = H; g.K = H; g.probe = 1;
            g.alpha = hw.dense_inv / mmee::kSplitScaleX;
            launch_gemm_split(g, EPI_TANH, B, cus, s);
            hin = hid; hld = H; hg = nullptr;
        } else if (hw.dense_w) {
            GemmArgs g = gemm_args();
            g.A = in; g.lda = ld; g.row_src = gather; g.W = hw.dense_w; g.bias = hw.dense_b; g.C = hid; g.ldc = H;
            // a handful of tiles: static assignment (walking the eight XCD queues would cost more than the tiles)
            g.m_ptr = n_docs_ptr; g.N = H; g.K = H;
            launch_gemm_f32(g, EPI_TANH, AMODE_ROWS, B, cus, s);
            hin = hid; hld = H; hg = nullptr;
        }
        HeadOutArgs ho{};
        ho.in = hin; ho.ld = hld; ho.gather = hg; ho.W = hw.out_w; ho.b = hw.out_b; ho.H = H; ho.Ko = hw.out_dim;
        ho.n_docs_ptr = n_docs_ptr; ho.out = out;
        if (lte) {
            ho.lte_in = lte->in; ho.lte_ld = lte->ld; ho.lte_gather = lte->gather; ho.lte_split_inv = lte->split_inv;
            ho.lte_w = h->lte_w; ho.lte_b = h->lte_b; ho.lte_out = h->lte_score;
        }
        { ProfScope po(h, P_HEADOUT, s); launch_head_out(ho, B, s); }
    }

    // The documents that stay after a decision become stage cur + 1: their rows renumbered densely, X read through the new row map.
    // The only place where the stage cursor advances.
    void compact() {
        ProfScope ps(h, P_COMPACT, s);
        launch_compact_rows(&h->counts[cur + 1], S_doc_off(cur + 1), S_x_src(cur + 1), S_meta_src(cur + 1),
                            h->meta[meta_cur], h->meta[meta_cur ^ 1], h->row_src, B, cus, s);
        meta_cur ^= 1;
        cur += 1;
        x_phys = S_x_src(cur);
        use_row_src = true;
    }

    void x_dense() { x_phys = S_doc_off(cur); use_row_src = false; }      // a layer wrote X densely in the numbering of stage `cur`

    // exit head (or the final classifier), decision, compaction of the documents that stay.  cls_row: `in` is the CLS row leaving a layer
    // (false: the pooled input of an embedding-level exit).  use_lte: the launch that projects the policy logits -- the one head launch every
    // exit has -- also scores the CLS rows, read where the head reads them: the split planes when they exist (the probes leave no f32 copy
    // for 2-layer heads), else the f32 rows.  No launch is added.
    void run_exit(const HeadW* hw, const float* in, int ld, const int* gather, bool is_final, const float* in_split = nullptr,
                  const int* split_rows = nullptr, bool cls_row = true) {
        const float* pol;
        const float* head = nullptr;
        int Kh = K;
        const LteRows lte_rows = in_split ? LteRows{in_split, H, split_rows, 1.0f / mmee::kSplitScaleX} : LteRows{in, ld, gather, 0.f};
        const LteRows* lte = (c.use_lte && cls_row) ? &lte_rows : nullptr;
        {
            ProfScope ps(h, P_HEAD, s);
            if (is_final) {
                run_head(h->classifier, in, ld, gather, h->hid, h->pol_logits, in_split, split_rows, lte);
                pol = h->pol_logits;
            } else if (c.strategy == MMEE_STRATEGY_GATE) {
                // the policy only ever sees classifier(gate input) (EE/utils.py:183-188); the 2-way gate logits (exit_states) are
                // computed when the caller asked for them (the dump of model.forward) or when they decide (MMEE_CRIT_GATE), else not
                const bool want_gate = a.out_head_logits || a.out_head_crit || c.criterion == MMEE_CRIT_GATE;
                if (want_gate) run_head(*hw, in, ld, gather, h->hid, h->head_logits, in_split, split_rows);
                run_head(h->classifier, in, ld, gather, h->hid2, h->pol_logits, in_split, split_rows, lte);  // gated_logits, EE/models/LayoutLMv3.py:768
                pol = h->pol_logits; head = want_gate ? h->head_logits : nullptr; Kh = 2;      // 2-way gate heads, EE/models/LayoutLMv3.py:83
            } else {
                run_head(*hw, in, ld, gather, h->hid, h->head_logits, in_split, split_rows, lte);
                pol = h->head_logits; head = h->head_logits; Kh = K;
            }
        }
        DecideArgs d{};
        d.pol_logits = pol; d.head_logits = head; d.K = K; d.Kh = Kh;
        d.thr = a.thresholds ? a.thresholds[exit_index] : 0.0;
        d.temp = a.temperatures ? a.temperatures[exit_index] : 1.0;
        if (cap) { d.thr_ptr = cap->thr_dev; d.temp_ptr = cap->thr_dev + (E + 1); }      // replays read the vector of THEIR launch
        if (ctl) d.thr_ptr = h->ctl_thr_dev;                                             // the vector the previous call's step left
        if (dl) d.thr_ptr = h->dl_thr;                                                   // the call's own thresholds until a check cuts
        if (h->ens_on) {
            // exit ensemble (ee_set_ensemble): y_m of every active document into a second policy buffer; the decision reads that with temperature 1
            EnsembleArgs en{};
            en.pol_logits = pol; en.K = K; en.E1 = E + 1; en.exit_index = exit_index; en.B = c.max_docs;
            en.temp = d.temp; en.temp_ptr = d.temp_ptr;
            en.counts = &h->counts[cur]; en.doc_orig = S_doc_orig(cur);
            en.w = h->ens_w; en.b = h->ens_b; en.state = h->ens_state; en.out = h->ens_logits;
            { ProfScope ps(h, P_ENSEMBLE, s); launch_exit_ensemble(en, s); }
            d.pol_logits = h->ens_logits; d.temp = 1.0;
            if (cap) d.temp_ptr = h->ens_ones;
        }
        d.criterion = c.criterion; d.is_final = is_final ? 1 : 0; d.no_exit = no_exit ? 1 : 0; d.exit_index = exit_index; d.B = B;
        d.counts = &h->counts[cur]; d.doc_orig = S_doc_orig(cur); d.doc_off = S_doc_off(cur); d.x_phys = x_phys;
        d.n_counts = &h->counts[cur + 1]; d.n_doc_orig = S_doc_orig(cur + 1); d.n_doc_off = S_doc_off(cur + 1);
        d.n_x_src = S_x_src(cur + 1); d.n_meta_src = S_meta_src(cur + 1);
        d.out_logits = a.out_logits; d.out_exit = a.out_exit; d.out_conf = a.out_conf;
        d.out_all_logits = a.out_all_logits; d.out_all_crit = a.out_all_crit;
        d.out_head_logits = a.out_head_logits; d.out_head_crit = a.out_head_crit;
        if (c.use_lte) d.lte_score = lte ? h->lte_score : nullptr;
        PatienceArgs pa{};
        const bool stateful = patience || h->rule != MMEE_RULE_PLAIN;
        if (stateful) {
            pa.t = h->has_patience() ? h->patience_at(exit_index) : 0;                    // not set: a dump-all call, where nobody leaves
            if (cap) pa.t_ptr = cap->thr_dev + 2 * (E + 1) + exit_index;                  // replays read the patience of THEIR launch
            pa.prev = h->pat_state; pa.run = h->pat_state + c.max_docs;
        }
        if (dl) deadline_check();                                                        // right before the decide launch
        if (h->quota_mode != MMEE_QUOTA_OFF && !no_exit && !is_final) {
            // budgeted exits (ee_set_quotas): the stage's criteria and ranks into the scratch, then the QUOTA form of the decide kernel.  The final
            // exit takes everybody and a dump keeps everybody: the plain kernels below, no launch added
            QuotaArgs qa{};
            qa.q = h->quotas[exit_index];
            if (cap) qa.q_ptr = cap->thr_dev + 3 * (E + 1) + exit_index;                  // replays read the quota of THEIR launch
            qa.crit = h->quota_crit; qa.rank = h->quota_rank;
            { ProfScope ps(h, P_QUOTA, s); launch_exit_quota_crit(d, qa, B, s); }
            { ProfScope ps(h, P_QUOTA, s); launch_exit_quota_rank(d, qa, B, s); }
            { ProfScope ps(h, P_DECIDE, s); launch_decide_quota(d, qa, h->quota_mode, s); }
        } else {
            ProfScope ps(h, P_DECIDE, s);
            const AuditArgs au{h->audit_delivered, h->audit_cut, ctl ? (uint32_t)(h->ctl_seed + (uint32_t)h->ctl_calls) : h->audit_seed, h->audit_slot_base};
            launch_decide(d, stateful ? &pa : nullptr, patience ? DECIDE_PATIENCE : c.use_lte ? DECIDE_LTE : DECIDE_THRESHOLD, h->rule, s, audit ? &au : nullptr);
        }
        h->rec.exit_stage[exit_index] = cur;
        if (is_final) { fin_pol = d.pol_logits; fin_temp = d.temp; }
        if (stream_results) emit_leavers(is_final);
        if (!is_final && !vision_only) compact();
        exit_index += 1;
    }

    // result stream: the rows of the documents that left at this exit (those of stage `cur` that are not in stage cur + 1; the final exit: everybody)
    // into the next free rows of the pinned segment buffer, then the event ee_stream_next waits on.  Eager calls only (validate()).
    void emit_leavers(bool is_final) {
        EmitArgs e{};
        e.counts = &h->counts[cur]; e.doc_orig = S_doc_orig(cur);
        if (!is_final) { e.n_counts = &h->counts[cur + 1]; e.n_doc_orig = S_doc_orig(cur + 1); }
        e.out_logits = a.out_logits; e.out_exit = a.out_exit; e.out_conf = a.out_conf;
        e.K = K; e.exit_index = exit_index; e.cap = c.max_docs;
        e.done = h->stream_done; e.rows = h->stream_dev; e.cum = h->stream_dev + (size_t)c.max_docs * (K + 3);
        { ProfScope ps(h, P_EMIT, s); launch_emit_leavers(e, s); }
        (void)hipEventRecord(h->stream_ev[exit_index], s);
    }

    // the segment buffer and the events of the result stream, at the handle's first flagged forward; a later one first waits (on the host) for the
    // last event of the one before, so that no segment is rewritten under a reader, and starts the delivery over
    int stream_begin() {
        if (!h->stream_host) {
            const size_t words = (size_t)c.max_docs * (K + 3) + (size_t)(E + 1);
            HIP_OK(h, hipHostMalloc((void**)&h->stream_host, words * sizeof(int32_t), hipHostMallocMapped));
            memset(h->stream_host, 0, words * sizeof(int32_t));
            void* dev = nullptr;
            HIP_OK(h, hipHostGetDevicePointer(&dev, h->stream_host, 0));
            h->stream_dev = reinterpret_cast<int32_t*>(dev);
        }
        if (!h->stream_done && dev_alloc(h, &h->stream_done, 1)) return 1;
        while ((int)h->stream_ev.size() < E + 1) {
            hipEvent_t ev = nullptr;
            HIP_OK(h, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            h->stream_ev.push_back(ev);
        }
        if (h->stream_armed) HIP_OK(h, hipEventSynchronize(h->stream_ev[E]));
        h->stream_armed = false;                  // until this forward's launch list is complete: every one of its events recorded
        h->stream_next = 0;
        return 0;
    }

    // hidden CLS rows of the active documents into out_hidden_cls[slot] (slot 0: the embeddings, l + 1: the output of layer l);
    // X row of document i: X[rows[i]]
    void gather_hidden(int slot, const float* X, const int* rows, float split_inv) {
        if (a.out_hidden_cls)
            launch_gather_cls(X, H, rows, S_doc_orig(cur), &h->counts[cur].n_docs, a.out_hidden_cls + (size_t)slot * B * H, B, s, split_inv);
    }

    // hidden state entering layer 0 / leaving layer l (EE/models/LayoutLMv3.py:182-183, 284-285): dump-all, so stage 0's numbering holds throughout
    void dump_hidden(int slot) {
        if (!hs_out) return;
        launch_rows_to_padded(x_out(), x_inv(), H, B, T, Pv, beit ? nullptr : h->text_dst, beit ? nullptr : h->ntext, S_doc_off(0),
                              hs_out + (size_t)slot * B * max_len * H, s);
    }

    // A layer that ends in a decision, probe first: the CLS rows of the active documents through the layer alone, the decision on them, the
    // rest of the layer for the documents that stay.  The three schedules differ in where Q | K | V is projected (before the probe, or for the
    // X-space probe after the exit, for the documents that stay only) and in which buffers hold the probed rows (BEiT: f32 rows in Xc;
    // LayoutLMv3: split planes in Xcs, the f32 copy the heads need in cls_f32).
    void probe_first(int l, bool fin, bool xspace) {
        const float* cls = beit ? h->Xc : h->cls_f32;
        const float* cls_split = beit ? nullptr : h->Xcs;
        if (beit) beit_probe(l);
        else layer_probe(l, fin, xspace);
        gather_hidden(l + 1, cls_split ? cls_split : cls, h->iota, cls_split ? 1.0f / mmee::kSplitScaleX : 0.f);
        if (l == L - 1) { cls_ready = true; return; }      // the final classifier below reads the probed rows; the last layer projects nothing
        run_exit(&h->enc_heads[next_enc], cls, H, nullptr, false, cls_split, nullptr);       // compacts: `cur` is now the stage of the documents that stay
        ++next_enc;
        // the rest of the layer for those documents: their rows are gathered through the new row map, as after any exit; their Q | K | V rows
        // are where the previous stage's numbering put them, or projected now
        if (xspace) qkv(l, h->Xs, h->row_src);
        const int* qkv_off = xspace ? nullptr : S_meta_src(cur);
        if (beit) beit_rest(l, h->row_src, qkv_off);
        else layer_rest(l, h->row_src, qkv_off);
        x_dense();
    }

    void layer(int l) {
        const bool exit_here = next_enc < c.n_encoder_exits && c.encoder_exit_layers[next_enc] == l + 1;     // an encoder exit follows layer l
        const bool last = l == L - 1;
        const int* rs = use_row_src ? h->row_src : nullptr;
        // probe first: this layer ends in a decision (an exit head, or the final classifier), split attention kernels, no dump of every layer
        // (the dump keeps every document to the end, so nothing would be saved).  BEiT: the mean-pooled final classifier reads every row of the
        // last layer, so only exit layers before it can be probed
        bool probe = probe_on && sp && !no_exit && (beit ? exit_here && !last : exit_here != last);
        if (probe && !last && !(a.flags & MMEE_FLAG_PROBE_ALWAYS) && h->mask_on) probe = ((h->probe_mask >> l) & 1u) != 0;
        bool xspace = false;
        if (probe && !beit && (a.flags & MMEE_FLAG_XPROBE) && use_idx && h->Qc) {
            mmee::XProbeArgs chk{};
            chk.H = H; chk.heads = c.num_attention_heads; chk.bins1 = c.rel_pos_bins; chk.bins2 = c.rel_2d_pos_bins; chk.pair_idx = h->pair_idx;
            xspace = mmee::xprobe_supports(chk, max_len);
        }
        if (beit) beit_qkv(l, rs);
        else if (!xspace) qkv(l, sp ? h->Xs : h->X, rs);      // the X-space probe decides first and projects afterwards
        if (probe) { probe_first(l, last && !exit_here, xspace); return; }
        if (beit) beit_rest(l, rs, nullptr);
        else layer_rest(l, rs, nullptr);
        x_dense();
        gather_hidden(l + 1, x_out(), x_phys, x_inv());
        dump_hidden(l + 1);
        if (!exit_here) return;
        if (x_split) {
            launch_gather_cls(h->Xs, H, x_phys, nullptr, &h->counts[cur].n_docs, h->cls_f32, B, s, x_inv());
            run_exit(&h->enc_heads[next_enc], h->cls_f32, H, nullptr, false, h->Xs, x_phys);
        } else {
            run_exit(&h->enc_heads[next_enc], h->X, H, x_phys, false);
        }
        ++next_enc;
    }

    // deadline exits: the call's number, its start on the device clock, its thresholds into h->dl_thr, the head of its log row
    long long* deadline_row() const {
        return h->dl_log_cap > 0 ? h->dl_log + (size_t)((dl_call - 1) % (uint64_t)h->dl_log_cap) * deadline_log_words(E + 1) : nullptr;
    }
    void deadline_begin() {
        dl_call = __atomic_add_fetch(&h->dl_calls, 1, __ATOMIC_RELAXED);
        DeadlineBeginArgs b{};
        for (int e = 0; e <= E; ++e) b.thr_in[e] = a.thresholds[e];
        b.E1 = E + 1; b.call = dl_call; b.budget = h->dl_budget; b.state = h->dl_state; b.thr = h->dl_thr; b.row = deadline_row();
        { ProfScope ps(h, P_DEADLINE, s); launch_deadline_begin(b, s); }
    }
    void deadline_check() {
        DeadlineCheckArgs k{};
        k.E1 = E + 1; k.exit_index = exit_index; k.khz = h->dl_khz; k.sign = crit_sign(c.criterion);
        k.call = dl_call; k.budget = h->dl_budget; k.eta = h->dl_eta[exit_index]; k.host_word = h->dl_word_dev;
        k.state = h->dl_state; k.thr = h->dl_thr; k.row = deadline_row();
        { ProfScope ps(h, P_DEADLINE, s); launch_deadline_check(k, s); }
    }

    // online exit control: what the audit saw in this call (the final stage is still `cur`: the final exit compacts nothing), then the step
    // and the thresholds of the next call.  The call's seed is the one its decide launches audited under.
    void control() {
        const int E1 = E + 1;
        AuditTallyArgs t{};
        t.counts = &h->counts[cur]; t.doc_orig = S_doc_orig(cur); t.pol_logits = fin_pol; t.temp = fin_temp; t.K = K; t.B = B; t.E1 = E1;
        t.delivered = h->audit_delivered; t.out_logits = a.out_logits; t.out_exit = a.out_exit;
        t.cut = h->audit_cut; t.seed = (uint32_t)(h->ctl_seed + (uint32_t)h->ctl_calls); t.slot_base = h->audit_slot_base; t.tally = h->ctl_tally;
        { ProfScope ps(h, P_CONTROLLER, s); launch_audit_tally(t, s); }
        ControllerStepArgs st{};
        st.path = h->ctl_path; st.V = h->ctl_V; st.E1 = E1; st.sign = crit_sign(c.criterion); st.alpha = h->ctl_alpha; st.gamma = h->ctl_gamma;
        st.state = h->ctl_state; st.tally = h->ctl_tally; st.thr = h->ctl_thr_dev; st.log = h->ctl_log; st.log_cap = h->ctl_log_cap;
        { ProfScope ps(h, P_CONTROLLER, s); launch_controller_step(st, s); }
        ++h->ctl_calls;
    }

    void final_exit() {
        if (beit) {
            // BeitPooler (BEIT:563-572): LayerNorm(mean of the patch tokens), then the Linear classifier
            launch_patch_mean(h->X, H, x_phys, S_doc_off(cur), &h->counts[cur].n_docs, h->pooled[0], B, s);
            launch_ln_rows(h->pooled[0], h->pooled[0], nullptr, &h->counts[cur].n_docs, B, H, h->ln_g, h->ln_b, c.layer_norm_eps, cus, s);
            run_exit(nullptr, h->pooled[0], H, nullptr, true);
        } else if (sp && L > 0) {
            if (!cls_ready) launch_gather_cls(h->Xs, H, x_phys, nullptr, &h->counts[cur].n_docs, h->cls_f32, B, s, 1.0f / mmee::kSplitScaleX);
            run_exit(nullptr, h->cls_f32, H, nullptr, true, cls_ready ? h->Xcs : h->Xs, cls_ready ? nullptr : x_phys);
        } else {
            run_exit(nullptr, h->X, H, x_phys, true);
        }
    }

    int run() {
        if (const int rc = validate()) return rc;
        max_len = T + Pv;
        max_rows = B * max_len;
        if (low_latency && h->ll_part) {
            ll_stride = (size_t)((max_rows + 127) / 128) * 128 * H;
            ks_ao = ee_low_latency_k_splits(max_rows, H, H, cus);
            ks_down = ee_low_latency_k_splits(max_rows, H, I, cus);
            if ((size_t)ks_ao * ll_stride > h->ll_part_floats) ks_ao = 1;          // (the rule's bound is the buffer's size: never taken)
            if ((size_t)ks_down * ll_stride > h->ll_part_floats) ks_down = 1;
        }
        if (!cap) { const int rc_pre = forward_pre(h, s); if (rc_pre) return rc_pre; }
        if (stream_results) { const int rc_st = stream_begin(); if (rc_st) return rc_st; }
        // (the last refusal, in front of every launch: a deadline call that is refused is not counted and writes no log row)
        if (sp && !use_idx) {          // attention_pair.hip holds Delta tables up to fixed distances: refuse what it cannot hold
            AttnArgs chk{};
            chk.ctx_split = 1; chk.c1 = h->c1; chk.c2 = h->c2; chk.doc_flags = h->doc_flags; chk.doc_orig = S_doc_orig(0);
            if (!mmee::attention_pair_supports(chk, c.max_rel_pos, c.max_rel_2d_pos))
                return fail(h, "ee_forward: the split-precision attention kernels cannot hold this relative-position configuration "
                               "(bins %d / %d, distances %d / %d); use MMEE_PREC_F32", c.rel_pos_bins, c.rel_2d_pos_bins, c.max_rel_pos, c.max_rel_2d_pos);
        }
        if (h->prof_on) { h->prof_recs.clear(); h->prof_used = 0; }
        if (dl) deadline_begin();                                        // the call's first launch: its clock starts here
        // (a kernel, not hipMemsetAsync: the same launch list then serves the eager call and the captured graph -- replays whose memset NODES were
        //  preceded by an eager forward on the handle came back with an unzeroed error word on ROCm 7.2, tools/graph_debug2.py)
        hipLaunchKernelGGL(zero_words_kernel, dim3(32), dim3(256), 0, s, h->err_flag, 4, h->queue_heads, h->n_queue_heads);
        h->next_queue_head = 0;
        if (beit) embed_beit();
        else embed_layoutlmv3();

        ForwardRecord& r = h->rec;
        r.layer_stage.assign(L, -1);
        r.layer_qkv_stage.assign(L, -1);
        r.layer_probe_stage.assign(L, -1);
        r.layer_xprobe.assign(L, 0);
        r.exit_stage.assign(E + 1, 0);
        r.ks_attn_out = ks_ao; r.ks_ffn_down = ks_down;
        x_phys = S_x_src(0);
        for (int i = 0; i < c.n_embedding_exits; ++i) {
            const int kind = c.embedding_exits[i];
            run_exit(&h->emb_heads[kind], h->pooled[kind], H, S_doc_orig(cur), false, nullptr, nullptr, false);
        }
        gather_hidden(0, x_out(), x_phys, x_inv());
        dump_hidden(0);
        // Which exit layers are probed first is part of the CALL, never of timing or history (round 5): every layer that ends
        // in a decision unless ee_set_probe_mask pinned a subset (ee_suggest_probe_mask prices one from a finished forward's stage populations;
        // the caller decides whether to pin it).  The same inputs therefore always run the same launch sequence and return the same bits.
        for (int l = 0; l < L; ++l) layer(l);
        final_exit();
        if (ctl) control();
        if (stream_results) h->stream_armed = true;
        r.last_B = B; r.last_T = T; r.last_stages = E + 1; r.last_flags = a.flags;
        r.last_gate_heads = a.out_head_logits || a.out_head_crit || c.criterion == MMEE_CRIT_GATE;
        if (!cap) { const int rc_post = forward_post(h, s); if (rc_post) return rc_post; }
        return launch_status(h, cap ? "ee_graph_capture" : "ee_forward");
    }

    // ee_forward_vision (include/mmee.h): the forward's opening from the pixels alone, up to and including exit 0; the caller has validated.
    // The layout is the uniform one of an image-only call (Pv rows per document: the decide kernel's bookkeeping reads nothing else of it),
    // in the two stage slots no forward reads back (E + 1, E + 2), so the stage counts of the last forward stay what they were; so do its
    // record and its profile.
    int run_vision(int32_t* survivors, int32_t* count) {
        constexpr int kind = MMEE_EXIT_VISION_AVG;
        const int vch = (Pv + 31) / 32;
        if (const int rc = forward_pre(h, s)) return rc;
        // the error word and the patch GEMM's queue heads, as in front of ee_embedding_inputs
        hipLaunchKernelGGL(zero_words_kernel, dim3(32), dim3(256), 0, s, h->err_flag, 4, h->queue_heads, std::min(h->n_queue_heads, 128));
        const bool prof = h->prof_on;
        h->prof_on = false;
        const ForwardRecord last = h->rec;
        h->rec.exit_stage.assign(E + 1, 0);
        vision_only = true;
        cur = E + 1;
        launch_prep_uniform(B, Pv, S_doc_off(cur), S_x_src(cur), S_doc_orig(cur), h->meta[0], &h->counts[cur], s);
        handle_patch_projection(h, a.pixel_values, B, h->n_queue_heads >= 128 ? h->queue_heads : nullptr, s);
        VisionPoolArgs va{};
        va.vis_raw = h->vis_raw; va.cls_token = h->cls_token; va.pos_embed = h->pos_embed;
        va.ln_g = h->norm_g; va.ln_b = h->norm_b; va.eps = 1e-6f;        // layoutlmv3.norm = LayerNorm(eps=1e-6), HF:563
        va.B = B; va.Pv = Pv; va.H = H; va.vis_part = h->vis_part;
        launch_vision_pool(va, s);
        launch_pool_finish(h->vis_part, vch, H, (float)Pv, h->pooled[kind], B, s);
        x_phys = S_x_src(cur);
        run_exit(&h->emb_heads[kind], h->pooled[kind], H, S_doc_orig(cur), false, nullptr, nullptr, false);
        launch_copy_survivors(&h->counts[cur + 1], S_doc_orig(cur + 1), B, survivors, count, s);
        h->rec = last;
        h->prof_on = prof;
        if (const int rc = forward_post(h, s)) return rc;
        return launch_status(h, "ee_forward_vision");
    }
};

}  // namespace

extern "C" {

int ee_forward(ee_handle* h, const int64_t* input_ids, const int64_t* attention_mask, const int64_t* bbox,
               const float* pixel_values, const int64_t* token_type_ids, const int64_t* position_ids, int32_t B, int32_t T,
               const double* thresholds, const double* temperatures, uint32_t flags, float* out_logits, int32_t* out_exit,
               float* out_conf, float* out_all_logits, float* out_all_crit, float* out_head_logits, float* out_head_crit,
               float* out_hidden_cls, void* stream) {
    if (!h) return 1;
    const ForwardArgs a{input_ids, attention_mask, bbox, pixel_values, token_type_ids, position_ids, B, T, thresholds, temperatures, flags,
                        out_logits, out_exit, out_conf, out_all_logits, out_all_crit, out_head_logits, out_head_crit, out_hidden_cls, stream};
    return Forward(h, a, nullptr).run();
}

// ---- captured-graph form of the forward (round 6) ------------------------------------------------------------------
// The reference evaluates at batch size 1 (EE/configs.py:36; loop EE/utils.py:169-193): ~185 launches per forward, each a few microseconds of
// GPU work.  ee_forward only enqueues, every kernel reads its extent from device memory, and since round 5 the launch list is a pure function of
// the handle's configuration and the call's (B, T, flags, outputs) -- so ONE capture is valid for every later batch in the same buffers.
int ee_graph_capture(ee_handle* h, const int64_t* input_ids, const int64_t* attention_mask, const int64_t* bbox, const float* pixel_values,
                     const int64_t* token_type_ids, const int64_t* position_ids, int32_t B, int32_t T, const double* thresholds,
                     const double* temperatures, uint32_t flags, float* out_logits, int32_t* out_exit, float* out_conf, float* out_all_logits,
                     float* out_all_crit, float* out_head_logits, float* out_head_crit, float* out_hidden_cls, void* stream, int32_t* graph_id) {
    if (!h || !graph_id) return fail(h, "ee_graph_capture: null argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!s) return fail(h, "ee_graph_capture: the legacy null stream cannot be captured; pass a created stream");
    if (flags & MMEE_FLAG_STREAM_RESULTS)          // before the eager warm-up call, which would otherwise run (and stream) first
        return fail(h, "ee_graph_capture: MMEE_FLAG_STREAM_RESULTS belongs to eager calls (the events between the launches are not part of a captured "
                       "launch list)");
    if (h->dl_on)
        return fail(h, "ee_graph_capture: a deadline is set: the call number and the budget travel by value and the begin launch stamps the "
                       "call's own start, so deadline calls are eager (not built; ee_set_deadline(h, MMEE_DEADLINE_OFF, NULL) first)");
    if (h->ctl_on)                                 // before the audit's refusal: a controller implies an audit
        return fail(h, "ee_graph_capture: a controller is set: its seed changes per call and the step reads the call's own results, so controlled "
                       "calls are eager (not built; ee_set_controller(h, NULL, ...) first)");
    if (h->audit_cut)                              // likewise before the warm-up call: the handle's state decides, whatever the flags
        return fail(h, "ee_graph_capture: an audit is set: its seed changes per call and is passed by value, so audited calls are eager "
                       "(not built; ee_set_audit(h, 0, 0, 0) first)");
    const int E1 = h->cfg.n_embedding_exits + h->cfg.n_encoder_exits + 1;
    const ForwardArgs a{input_ids, attention_mask, bbox, pixel_values, token_type_ids, position_ids, B, T, thresholds, temperatures, flags,
                        out_logits, out_exit, out_conf, out_all_logits, out_all_crit, out_head_logits, out_head_crit, out_hidden_cls, stream};
    // (1) the same call, eagerly: it validates the arguments, makes every kernel's one-time set-up (dynamic-LDS opt-ins) happen outside the
    // capture, and leaves its results in the output buffers
    int rc = Forward(h, a, nullptr).run();
    if (rc) return rc;
    HIP_OK(h, hipStreamSynchronize(s));
    {
        const int e = take_errors(h, true, true);
        if (e) return report_errors(h, e, "the warm-up forward of ee_graph_capture");
    }
    ee_handle::GraphRec g;
    g.n_exits1 = E1;
    g.no_exit = (flags & MMEE_FLAG_NO_EXIT) != 0;
    g.patience = h->cfg.criterion == MMEE_CRIT_PATIENCE;
    g.quota_mode = h->quota_mode;
    if (dev_alloc(h, &g.thr_dev, (size_t)4 * E1)) return 1;
    // (2) the launch list again, captured
    hipGraph_t graph = nullptr;
    HIP_OK(h, hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
    rc = Forward(h, a, &g).run();
    const hipError_t ec = hipStreamEndCapture(s, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (ec != hipSuccess || !graph) return fail(h, "ee_graph_capture: hipStreamEndCapture failed: %s", hipGetErrorString(ec));
    const hipError_t ei = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) return fail(h, "ee_graph_capture: hipGraphInstantiate failed: %s", hipGetErrorString(ei));
    g.rec = h->rec;
    h->graphs.push_back(g);
    *graph_id = (int32_t)h->graphs.size() - 1;
    return 0;
}

int ee_graph_launch(ee_handle* h, int32_t graph_id, const double* thresholds, const double* temperatures, void* stream) {
    if (!h) return 1;
    if (graph_id < 0 || graph_id >= (int32_t)h->graphs.size() || !h->graphs[graph_id].exec) return fail(h, "ee_graph_launch: no such graph (%d)", graph_id);
    const ee_handle::GraphRec& g = h->graphs[graph_id];
    if (!thresholds && !g.no_exit && !g.patience && g.quota_mode != MMEE_QUOTA_EXACT)
        return fail(h, "ee_graph_launch: thresholds required (the graph was captured without MMEE_FLAG_NO_EXIT, MMEE_CRIT_PATIENCE or MMEE_QUOTA_EXACT)");
    if (h->prof_on) return fail(h, "ee_graph_launch: ee_profile times eager launches; disarm it first");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int rc_pre = forward_pre(h, s);
    if (rc_pre) return rc_pre;
    ThrPack p{};
    p.n = 4 * g.n_exits1;
    for (int i = 0; i < g.n_exits1; ++i) {
        p.v[i] = thresholds ? thresholds[i] : 0.0;
        p.v[g.n_exits1 + i] = temperatures ? temperatures[i] : 1.0;
        p.v[2 * g.n_exits1 + i] = (double)h->patience_at(i);
        p.v[3 * g.n_exits1 + i] = i < (int)h->quotas.size() ? (double)h->quotas[i] : 0.0;      // the handle's CURRENT quotas (the mode is the capture's)
    }
    hipLaunchKernelGGL(set_thresholds_kernel, dim3(1), dim3(64), 0, s, p, g.thr_dev);
    HIP_OK(h, hipGraphLaunch(g.exec, s));
    h->rec = g.rec;
    const int rc_post = forward_post(h, s);
    if (rc_post) return rc_post;
    return launch_status(h, "ee_graph_launch");
}

// ---- stage 0 alone: the inputs of the embedding-level exit heads without the encoder behind them (include/mmee.h) ------------------------
// Its layout goes to the stage slot no forward reads back (E + 1), so the stage counts of the last forward stay what they were; the packed
// rows land in X / Xs, which every forward rewrites first.
int ee_embedding_inputs(ee_handle* h, const int64_t* input_ids, const int64_t* attention_mask, const int64_t* bbox, const float* pixel_values,
                        const int64_t* token_type_ids, const int64_t* position_ids, int32_t B, int32_t T, float* out_vision, float* out_text,
                        float* out_concat, void* stream) {
    if (!h) return 1;
    const ee_config& c = h->cfg;
    if (c.arch == MMEE_ARCH_BEIT)
        return fail(h, "ee_embedding_inputs: embedding-level exits belong to LayoutLMv3 handles; this is an MMEE_ARCH_BEIT handle");
    if (!h->finalized) return fail(h, "ee_embedding_inputs: call ee_finalize after loading the parameters");
    if (!out_vision && !out_text && !out_concat) return fail(h, "ee_embedding_inputs: out_vision, out_text and out_concat are all NULL: nothing to compute");
    if (!input_ids || !bbox || !pixel_values) return fail(h, "ee_embedding_inputs: input_ids, bbox and pixel_values are required");
    if (B < 1 || B > c.max_docs) return fail(h, "ee_embedding_inputs: B=%d outside [1, max_docs=%d]", B, c.max_docs);
    if (T < 1 || T > c.max_text_len) return fail(h, "ee_embedding_inputs: T=%d outside [1, max_text_len=%d]", T, c.max_text_len);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (const int rc = forward_pre(h, s)) return rc;
    Stage0 st{};
    st.input_ids = input_ids; st.attention_mask = attention_mask; st.bbox = bbox; st.pixel_values = pixel_values;
    st.token_type_ids = token_type_ids; st.position_ids = position_ids;
    st.inputs_embeds = h->next_inputs_embeds;          // one-shot, as in ee_forward: this call consumes it
    h->next_inputs_embeds = nullptr;
    st.B = B; st.T = T; st.slot = c.n_embedding_exits + c.n_encoder_exits + 1;
    st.pooled[MMEE_EXIT_VISION_AVG] = out_vision; st.pooled[MMEE_EXIT_TEXT_AVG] = out_text; st.pooled[MMEE_EXIT_TEXT_VISUAL_CONCAT] = out_concat;
    // the error word and the patch GEMM's queue heads, as in front of a forward (which zeroes all heads again before it hands any out)
    hipLaunchKernelGGL(zero_words_kernel, dim3(32), dim3(256), 0, s, h->err_flag, 4, h->queue_heads, std::min(h->n_queue_heads, 128));
    st.patch_tile_counter = h->n_queue_heads >= 128 ? h->queue_heads : nullptr;
    const bool prof = h->prof_on;                      // ee_profile times forwards: its records stay those of the last one
    h->prof_on = false;
    stage0_prep(h, st, s);
    stage0_embed(h, st, s);
    h->prof_on = prof;
    if (const int rc = forward_post(h, s)) return rc;
    return launch_status(h, "ee_embedding_inputs");
}

// ---- phase 1 of a vision-first call: the forward from the pixels alone, up to exit 0 (include/mmee.h) ------------------------------------
// Towards the handle it behaves as ee_embedding_inputs does: the record, the stage counts and the profile of the last forward stay, and it
// writes only workspace that every forward and graph replay rewrites before reading it.
int ee_forward_vision(ee_handle* h, const float* pixel_values, int32_t B, const double* thresholds, const double* temperatures, uint32_t flags,
                      float* out_logits, int32_t* out_exit, float* out_conf, int32_t* survivors, int32_t* count, void* stream) {
    if (!h) return 1;
    const ee_config& c = h->cfg;
    if (c.arch == MMEE_ARCH_BEIT)
        return fail(h, "ee_forward_vision: embedding-level exits belong to LayoutLMv3 handles; this is an MMEE_ARCH_BEIT handle");
    if (!h->finalized) return fail(h, "ee_forward_vision: call ee_finalize after loading the parameters");
    if (c.n_embedding_exits < 1 || c.embedding_exits[0] != MMEE_EXIT_VISION_AVG)
        return fail(h, "ee_forward_vision: the handle's exit list has no vision_avg exit: there is nothing to decide from the pixels alone");
    if (!pixel_values || !out_exit || !survivors || !count)
        return fail(h, "ee_forward_vision: pixel_values, out_exit, survivors and count are required");
    if (B < 1 || B > c.max_docs) return fail(h, "ee_forward_vision: B=%d outside [1, max_docs=%d]", B, c.max_docs);
    if (flags & (MMEE_FLAG_NO_EXIT | MMEE_FLAG_STREAM_RESULTS | MMEE_FLAG_DENSE_ROWS))
        return fail(h, "ee_forward_vision: MMEE_FLAG_NO_EXIT, MMEE_FLAG_STREAM_RESULTS and MMEE_FLAG_DENSE_ROWS do not go with a vision-first call "
                       "(nobody would leave; the stream's chunks are per call; there are no text rows to keep)");
    if (h->quota_mode != MMEE_QUOTA_OFF)
        return fail(h, "ee_forward_vision: quotas are set: a rank over B documents and a second one over the survivors are not the one-call ranking "
                       "(not built; ee_set_quotas(h, NULL, 0, 0) first)");
    if (h->dl_on)
        return fail(h, "ee_forward_vision: a deadline is set: the budget of a vision-first call would have to span both of its phases "
                       "(not built; ee_set_deadline(h, MMEE_DEADLINE_OFF, NULL) first)");
    if (h->ctl_on)                                 // before the audit's refusal: a controller implies an audit
        return fail(h, "ee_forward_vision: a controller is set: its audit hashes the slot in the call, which phase 2 renumbers "
                       "(not built; ee_set_controller(h, NULL, ...) first)");
    if (h->audit_cut)
        return fail(h, "ee_forward_vision: an audit is set: it hashes the slot in the call, which phase 2 renumbers "
                       "(not built; ee_set_audit(h, 0, 0, 0) first)");
    if (h->next_inputs_embeds || h->next_hidden_out || h->next_head_mask || h->next_attn_out)
        return fail(h, "ee_forward_vision: a one-shot side input / output is armed (inputs_embeds, hidden states, head mask, attention maps): "
                       "they belong to ee_forward, which consumes them");
    const bool patience = c.criterion == MMEE_CRIT_PATIENCE;
    if (!thresholds && !patience) return fail(h, "ee_forward_vision: thresholds required unless MMEE_CRIT_PATIENCE");
    if (patience && !h->has_patience())
        return fail(h, "ee_forward_vision: the patience criterion needs ee_set_patience(h, t) with t >= 1 before the first forward");
    if (h->rule != MMEE_RULE_PLAIN && patience)
        return fail(h, "ee_forward_vision: MMEE_RULE_STREAK / MMEE_RULE_EITHER build on a threshold event, which MMEE_CRIT_PATIENCE does not have");
    if (h->rule != MMEE_RULE_PLAIN && !h->has_patience())
        return fail(h, "ee_forward_vision: MMEE_RULE_STREAK / MMEE_RULE_EITHER need a patience: ee_set_patience or ee_set_patience_vector before the forward");
    // no text, no dump-all outputs; T is read by nothing on this route (the layout is the uniform one of Pv rows per document)
    const ForwardArgs a{nullptr, nullptr, nullptr, pixel_values, nullptr, nullptr, B, 1, thresholds, temperatures, flags,
                        out_logits, out_exit, out_conf, nullptr, nullptr, nullptr, nullptr, nullptr, stream};
    return Forward(h, a, nullptr).run_vision(survivors, count);
}

int ee_graph_destroy(ee_handle* h, int32_t graph_id) {
    if (!h) return 1;
    if (graph_id < 0 || graph_id >= (int32_t)h->graphs.size()) return fail(h, "ee_graph_destroy: no such graph (%d)", graph_id);
    ee_handle::GraphRec& g = h->graphs[graph_id];
    if (g.exec) {
        (void)hipDeviceSynchronize();
        (void)hipGraphExecDestroy(g.exec);
        g.exec = nullptr;
    }
    return 0;
}

}  // extern "C"
