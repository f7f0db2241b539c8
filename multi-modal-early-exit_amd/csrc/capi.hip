// C-ABI of libmmee_hip.so (include/mmee.h): handle, parameter registry, workspace, and the forward pass that chains
// the HIP kernels.  Host code only enqueues: after an exit stage the number of surviving documents/rows lives in
// device memory and every later kernel sizes itself from it (persistent grid-stride launches), so there is no
// host-side control flow on the exit decision (the reference loops in Python, EE/policy.py:28-45).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/mmee.h"
#include "mmee_kernels.h"

using namespace mmee;

namespace {

std::string g_create_error;

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
};

}  // namespace

struct ee_handle {
    ee_config cfg;
    std::string err;
    int num_cus = 256;
    bool finalized = false;
    std::map<std::string, Param> params;
    std::vector<std::string> names;
    std::vector<void*> allocs;
    // model pointers
    float *word, *type, *pos, *xtab, *ytab, *htab, *wtab, *emb_g, *emb_b;
    float *patch_w, *patch_b, *cls_token, *pos_embed, *norm_g, *norm_b, *ln_g, *ln_b;
    float *rel1, *relx, *rely;
    std::vector<LayerW> layers;
    HeadW emb_heads[3];
    std::vector<HeadW> enc_heads;
    HeadW classifier;
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
    int* iota = nullptr;                          // 0 .. max_docs-1
    float *X, *Y, *QKV, *CTX, *H1, *vis_raw, *text_part, *vis_part, *cat_part, *pooled[3], *hid, *hid2, *head_logits, *pol_logits;
    int *text_dst, *emb_pos, *ntext, *row_src, *err_flag;
    int* queue_heads = nullptr;                   // one work-queue counter per persistent launch of a forward
    int n_queue_heads = 0, next_queue_head = 0;
    RowMeta* meta[2];
    int *doc_orig, *doc_off, *x_src, *meta_src;   // [(E+2)][max_docs+1]
    StageCounts* counts;                          // [(E+2)]
    double* thr_dev = nullptr;                    // scratch for ee_policy_scan
    int32_t patience = 0;                         // ee_set_patience (0: not set); read by the decide launches under MMEE_CRIT_PATIENCE
    int* pat_state = nullptr;                     // [2][max_docs]: argmax at the previous exit, run counter (by original document slot)
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
    ForwardRecord rec;                            // bookkeeping of the last forward
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
        double* thr_dev = nullptr;                // [2 * (E + 1) + 1]: thresholds, then temperatures (1.0 when the launch passes none), then the patience
        int n_exits1 = 0;
        bool no_exit = false;
        bool patience = false;                    // captured under MMEE_CRIT_PATIENCE: launches need no thresholds
        ForwardRecord rec;                        // bookkeeping of the captured forward, restored by every launch
    };
    std::vector<GraphRec> graphs;
};

namespace {

int fail(ee_handle* h, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    else g_create_error = buf;
    return 1;
}

#define HIP_OK(h, expr)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return fail(h, "%s failed: %s", #expr, hipGetErrorString(e_));     \
    } while (0)

// What every entry point that launches kernels returns through: a failed dynamic-LDS opt-in of one of ITS launchers (recorded per thread,
// mmee_common.h) with the kernel's name, else the launch error, else 0.
int launch_status(ee_handle* h, const char* who) {
    char lds_msg[192];
    if (mmee::take_lds_error(lds_msg, sizeof(lds_msg))) { (void)hipGetLastError(); return fail(h, "%s: %s", who, lds_msg); }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, "%s: launch failed: %s", who, hipGetErrorString(e));
    return 0;
}

// Error flags of forwards that were enqueued earlier and not reported yet, oldest first.  wait = false: only forwards that have finished
// (stops at the first one still running: one handle's forwards finish in order); wait = true: waits for each.  all = false: returns at
// the first forward with flags (the others stay pending); all = true: ORs every pending forward's flags.
int take_errors(ee_handle* h, bool wait, bool all) {
    if (!h->err_host) return 0;
    int acc = 0;
    for (int i = ee_handle::kErrSlots; i >= 1; --i) {
        if ((unsigned)i > h->err_seq) continue;
        const int k = (int)((h->err_seq - (unsigned)i) % ee_handle::kErrSlots);
        ee_handle::ErrSlot& es = h->errs[k];
        if (!es.pending) continue;
        if (wait) (void)hipEventSynchronize(es.done);
        else if (hipEventQuery(es.done) != hipSuccess) break;
        es.pending = false;
        acc |= h->err_host[k];
        h->err_host[k] = 0;
        if (acc && !all) break;
    }
    return acc;
}

int report_errors(ee_handle* h, int err, const char* whose) {
    if (err & 32)
        return fail(h, "ee_forward: internal error in %s (flags %d): the attention kernel found its dynamic LDS region away from address 0", whose, err);
    if (err & mmee::kErrSplitOverflow)
        return fail(h, "ee_forward: split-precision overflow in %s (flags %d): an activation left the range of the split-f16 planes (|LayerNorm out|, "
                       "|Q/sqrt(d)|, |K|, |V|, |GELU out|, |pixel_values| <= 3750, |attention context| <= 937) and was clamped, so its results are WRONG; "
                       "run this checkpoint with precision \"fp32\"", whose, err);
    if (err)
        return fail(h, "ee_forward: input out of range in %s (flags %d: 1 = token id, 2 = bbox outside [0, max_2d), 4 = position id, 8 = token_type id); "
                       "its results are invalid", whose, err);
    return 0;
}

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

int add_param(ee_handle* h, const std::string& name, float** slot, std::vector<int64_t> shape, float* into = nullptr) {
    Param p;
    p.shape = shape;
    if (into) p.ptr = into;
    else if (dev_alloc(h, &p.ptr, p.numel())) return 1;
    if (slot) *slot = p.ptr;
    h->params[name] = p;
    h->names.push_back(name);
    return 0;
}

int add_head(ee_handle* h, const std::string& name, HeadW* hw, int H, int out_dim, bool two) {
    hw->out_dim = out_dim;
    if (two) {
        if (add_param(h, name + ".dense.weight", &hw->dense_w, {H, H})) return 1;
        if (add_param(h, name + ".dense.bias", &hw->dense_b, {H})) return 1;
    }
    if (add_param(h, name + ".out_proj.weight", &hw->out_w, {out_dim, H})) return 1;
    if (add_param(h, name + ".out_proj.bias", &hw->out_b, {out_dim})) return 1;
    return 0;
}

// HF relative_position_bucket (HF:392-413) as a LUT over delta in [-max_delta, max_delta].  torch evaluates the log
// branch in float32 and truncates; the only integers whose float32 value sits on a bucket edge are the exact edges
// max_exact * 2^(k/ratio), where float32 lands on the integer itself — floor(t + 1e-6) in double reproduces that
// (pinned against the HF-generated LUT in tests/golden/bucket_lut.npz).
void bucket_lut_host(int num_buckets, int max_distance, int max_delta, unsigned char* out) {
    const int nb = num_buckets / 2, me = nb / 2;
    for (int d = -max_delta; d <= max_delta; ++d) {
        int ret = d > 0 ? nb : 0;
        const int n = d < 0 ? -d : d;
        int v;
        if (n < me) v = n;
        else {
            const double t = std::log((double)n / me) / std::log((double)max_distance / me) * (nb - me);
            v = me + (int)std::floor(t + 1e-6);
            if (v > nb - 1) v = nb - 1;
        }
        out[d + max_delta] = (unsigned char)(ret + v);
    }
}

// kernel roles reported by ee_profile_read; the HIP symbol each role launches is in the second column
const char* const kProfNames[] = {
    "prep|doc_prep_kernel+doc_scan_kernel+row_meta_kernel",
    "embed_text|embed_text_kernel",
    "gemm_patch|patch_split_kernel+gemm_split_kernel<.., 0, false> (f32: gemm_f32_kernel<0,1>)",
    "embed_visual|embed_visual_kernel+pool_finish_kernel",
    "gemm_qkv|gemm_f32_kernel<0,0>",
    "attention|attention_f32_kernel",
    "gemm_attn_out|gemm_f32_kernel<2,0>",
    "layernorm|ln_rows_kernel",
    "gemm_ffn_up|gemm_f32_kernel<1,0>",
    "gemm_ffn_down|gemm_f32_kernel<2,0>",
    "exit_head|gemm_f32_kernel<3,0>+head_out_kernel",
    "exit_decide|exit_decide_kernel (patience: exit_decide_patience_kernel)",
    "compact|compact_rows_kernel",
    "gather_cls|gather_cls_kernel",
    "cls_probe|attention_idx_kernel+gemm_split_kernel<.., 1>+ln_rows_kernel+gather_cls_kernel (CLS rows of an exit layer, before its decision)",
    // nested roles: each is timed INSIDE the role named in brackets (so a sum over roles must leave them out)
    "pair_index|pair_index_kernel [inside prep]",
    "patch_split|patch_split_kernel [inside gemm_patch]",
    "head_out|head_out_kernel [inside exit_head]",
};
enum { P_PREP = 0, P_EMBT, P_GPATCH, P_EMBV, P_GQKV, P_ATTN, P_GAO, P_LN, P_GUP, P_GDOWN, P_HEAD, P_DECIDE, P_COMPACT, P_GCLS, P_PROBE,
       P_PAIRIDX, P_PSPLIT, P_HEADOUT, P_COUNT };

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

}  // namespace

extern "C" {

int ee_profile(ee_handle* h, int32_t enable) {
    if (!h) return 1;
    h->prof_on = enable != 0;
    h->prof_recs.clear();
    h->prof_used = 0;
    return 0;
}

int ee_profile_read(ee_handle* h, int32_t idx, char* name_out, int32_t name_cap, double* total_ms, int32_t* launches) {
    if (!h) return 1;
    if (idx < 0 || idx >= P_COUNT) return 2;
    (void)hipDeviceSynchronize();
    double ms = 0.0;
    int n = 0;
    for (auto& r : h->prof_recs)
        if (r.id == idx) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) { ms += t; ++n; }
        }
    if (name_out && name_cap > 0) {
        strncpy(name_out, kProfNames[idx], name_cap - 1);
        name_out[name_cap - 1] = 0;
    }
    if (total_ms) *total_ms = ms;
    if (launches) *launches = n;
    return 0;
}

int ee_bucket_lut(int32_t num_buckets, int32_t max_distance, int32_t max_delta, uint8_t* out_host) {
    if (!out_host || num_buckets < 4 || num_buckets > 256 || max_delta < 0) return 1;
    bucket_lut_host(num_buckets, max_distance, max_delta, out_host);
    return 0;
}

const char* ee_last_error(const ee_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int ee_create(const ee_config* c, ee_handle** out) {
    if (!c || !out) return fail(nullptr, "ee_create: null argument");
    if (c->abi_version != MMEE_ABI_VERSION) return fail(nullptr, "ee_create: abi_version %d != %d", c->abi_version, MMEE_ABI_VERSION);
    const int H = c->hidden_size, I = c->intermediate_size, L = c->num_hidden_layers, K = c->num_labels;
    if (H % 128 || I % 128 || H > 1024) return fail(nullptr, "hidden_size/intermediate_size must be multiples of 128, hidden_size <= 1024");
    if (H % c->num_attention_heads || H / c->num_attention_heads != 64) return fail(nullptr, "head dim must be 64");
    const bool beit = c->arch == MMEE_ARCH_BEIT;
    if (c->arch != MMEE_ARCH_LAYOUTLMV3 && !beit) return fail(nullptr, "unknown arch %d", c->arch);
    if (!beit && 4 * c->coordinate_size + 2 * c->shape_size != H) return fail(nullptr, "4*coordinate_size + 2*shape_size != hidden_size");
    if (beit && c->n_embedding_exits) return fail(nullptr, "the BEiT / DiT variant has encoder-layer exits only");
    if (beit && !c->use_mean_pooling) return fail(nullptr, "BEiT / DiT: only use_mean_pooling = 1 is built");
    if (c->input_size % c->patch_size || (c->num_channels * c->patch_size * c->patch_size) % 32 || c->patch_size % 4 || c->input_size % 4)
        return fail(nullptr, "unsupported patch geometry");
    if (K < 1 || K > 64) return fail(nullptr, "num_labels must be in [1,64]");
    if (c->n_embedding_exits < 0 || c->n_embedding_exits > 3 || c->n_encoder_exits < 0 || c->n_encoder_exits > MMEE_MAX_ENCODER_EXITS)
        return fail(nullptr, "bad exit counts");
    for (int i = 0; i < c->n_encoder_exits; ++i) {
        const int l = c->encoder_exit_layers[i];
        if (l < 1 || l > L || (i && l <= c->encoder_exit_layers[i - 1])) return fail(nullptr, "encoder_exit_layers must be ascending in [1,L]");
    }
    if (c->max_docs < 1 || c->max_text_len < (beit ? 0 : 1) || c->max_text_len > 1024) return fail(nullptr, "max_docs >= 1, 1 <= max_text_len <= 1024");
    if (c->precision != MMEE_PREC_F32 && c->precision != MMEE_PREC_F32_SPLIT)
        return fail(nullptr, "precision %d not built (MMEE_PREC_F32 and MMEE_PREC_F32_SPLIT are; bf16 cannot meet the 1e-4 logit tolerance)", c->precision);
    if (c->precision == MMEE_PREC_F32_SPLIT &&
        !(mmee::gemm_split_supports(3 * H, H) && mmee::gemm_split_supports(H, H) && mmee::gemm_split_supports(I, H) && mmee::gemm_split_supports(H, I)))
        return fail(nullptr, "MMEE_PREC_F32_SPLIT needs hidden_size and intermediate_size to be multiples of 256 (got %d, %d)", H, I);
    {   // the split GEMM addresses a gathered A row by a 32-bit byte offset from the tile's first source row
        const double x_bytes = (double)c->max_docs * (double)(c->max_text_len + (c->input_size / c->patch_size) * (c->input_size / c->patch_size) + 1) * H * 4.0;
        if (c->precision == MMEE_PREC_F32_SPLIT && x_bytes >= 4294967296.0)
            return fail(nullptr, "MMEE_PREC_F32_SPLIT: max_docs * rows per document * hidden_size * 4 must stay below 4 GiB (got %.2f GiB); "
                                 "use a smaller max_docs per handle", x_bytes / 1073741824.0);
    }
    if (c->precision == MMEE_PREC_F32_SPLIT && !beit && !(c->rel_pos_bins <= 64 && c->rel_2d_pos_bins <= 64) &&
        !(c->max_rel_pos <= 128 && c->max_rel_2d_pos <= 256))
        return fail(nullptr, "MMEE_PREC_F32_SPLIT: the split-precision attention kernels hold bucket tables of <= 64 bins (attention_idx) or "
                             "distances <= 128 / 256 (attention_pair); got bins %d / %d, distances %d / %d: use MMEE_PREC_F32",
                    c->rel_pos_bins, c->rel_2d_pos_bins, c->max_rel_pos, c->max_rel_2d_pos);
    if (c->precision == MMEE_PREC_F32_SPLIT && (c->num_attention_heads < 1 || c->rel_pos_bins < 2 || c->rel_2d_pos_bins < 2) && !beit)
        return fail(nullptr, "bad relative-position configuration");
    if (c->exit_head_num_layers != 1 && c->exit_head_num_layers != 2) return fail(nullptr, "exit_head_num_layers must be 1 or 2");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, "no HIP device: libmmee_hip needs an MI355X (there is no CPU fallback)");

    ee_handle* h = new ee_handle();
    h->cfg = *c;
    h->split = c->precision == MMEE_PREC_F32_SPLIT;
    hipDeviceProp_t prop;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) h->num_cus = prop.multiProcessorCount;

    // ---- parameter registry (HF names) ------------------------------------------------------------------------
    const int NP = (c->input_size / c->patch_size) * (c->input_size / c->patch_size);
    const bool two = c->exit_head_num_layers == 2;
    const int out_dim = c->strategy == MMEE_STRATEGY_RAMP ? K : 2;     // EE/models/LayoutLMv3.py:83
    int rc = 0;
    h->layers.resize(L);
    h->enc_heads.resize(c->n_encoder_exits);
    if (beit) {
        // BEiT / DiT (transformers 4.x parameter names, as in the DiT checkpoints the reference's "dit" branch loads,
        // EE/configs.py:429-449).  Exit heads are this build's extrapolation: the reference has none.
        const std::string p = "beit.";
        rc |= add_param(h, p + "embeddings.cls_token", &h->cls_token, {1, 1, H});
        if (c->use_abs_pos) rc |= add_param(h, p + "embeddings.position_embeddings", &h->pos_embed, {1, NP + 1, H});
        rc |= add_param(h, p + "embeddings.patch_embeddings.projection.weight", &h->patch_w, {H, c->num_channels, c->patch_size, c->patch_size});
        rc |= add_param(h, p + "embeddings.patch_embeddings.projection.bias", &h->patch_b, {H});
        for (int l = 0; l < L && !rc; ++l) {
            LayerW& w = h->layers[l];
            const std::string q = p + "encoder.layer." + std::to_string(l) + ".";
            rc |= dev_alloc(h, &w.qkv_w, (size_t)3 * H * H);
            rc |= dev_alloc(h, &w.qkv_b, (size_t)3 * H);
            if (rc) break;
            if (hipMemset(w.qkv_b, 0, sizeof(float) * 3 * H) != hipSuccess) { rc = fail(h, "hipMemset failed"); break; }   // key has no bias
            const char* nm[3] = {"query", "key", "value"};
            for (int t = 0; t < 3; ++t) {
                rc |= add_param(h, q + "attention.attention." + nm[t] + ".weight", nullptr, {H, H}, w.qkv_w + (size_t)t * H * H);
                if (t != 1) rc |= add_param(h, q + "attention.attention." + nm[t] + ".bias", nullptr, {H}, w.qkv_b + (size_t)t * H);
            }
            rc |= add_param(h, q + "attention.output.dense.weight", &w.ao_w, {H, H});
            rc |= add_param(h, q + "attention.output.dense.bias", &w.ao_b, {H});
            rc |= add_param(h, q + "layernorm_before.weight", &w.ao_g, {H});
            rc |= add_param(h, q + "layernorm_before.bias", &w.ao_beta, {H});
            rc |= add_param(h, q + "intermediate.dense.weight", &w.f1_w, {I, H});
            rc |= add_param(h, q + "intermediate.dense.bias", &w.f1_b, {I});
            rc |= add_param(h, q + "output.dense.weight", &w.f2_w, {H, I});
            rc |= add_param(h, q + "output.dense.bias", &w.f2_b, {H});
            rc |= add_param(h, q + "layernorm_after.weight", &w.f_g, {H});
            rc |= add_param(h, q + "layernorm_after.bias", &w.f_beta, {H});
            if (c->layer_scale) {
                rc |= add_param(h, q + "lambda_1", &w.lam1, {H});
                rc |= add_param(h, q + "lambda_2", &w.lam2, {H});
            }
        }
        if (c->use_mean_pooling) {
            rc |= add_param(h, p + "pooler.layernorm.weight", &h->ln_g, {H});
            rc |= add_param(h, p + "pooler.layernorm.bias", &h->ln_b, {H});
        } else {
            rc |= add_param(h, p + "layernorm.weight", &h->ln_g, {H});
            rc |= add_param(h, p + "layernorm.bias", &h->ln_b, {H});
        }
        for (int k = 0; k < c->n_encoder_exits && !rc; ++k)
            rc |= add_head(h, p + "encoder.early_exits." + std::to_string(k), &h->enc_heads[k], H, out_dim, two);
        h->classifier.out_dim = K;                                     // BeitForImageClassification.classifier = Linear(H, K)
        rc |= add_param(h, "classifier.weight", &h->classifier.out_w, {K, H});
        rc |= add_param(h, "classifier.bias", &h->classifier.out_b, {K});
    } else {
    const std::string p = "layoutlmv3.";
    rc |= add_param(h, p + "embeddings.word_embeddings.weight", &h->word, {c->vocab_size, H});
    rc |= add_param(h, p + "embeddings.token_type_embeddings.weight", &h->type, {c->type_vocab_size, H});
    rc |= add_param(h, p + "embeddings.position_embeddings.weight", &h->pos, {c->max_position_embeddings, H});
    rc |= add_param(h, p + "embeddings.x_position_embeddings.weight", &h->xtab, {c->max_2d_position_embeddings, c->coordinate_size});
    rc |= add_param(h, p + "embeddings.y_position_embeddings.weight", &h->ytab, {c->max_2d_position_embeddings, c->coordinate_size});
    rc |= add_param(h, p + "embeddings.h_position_embeddings.weight", &h->htab, {c->max_2d_position_embeddings, c->shape_size});
    rc |= add_param(h, p + "embeddings.w_position_embeddings.weight", &h->wtab, {c->max_2d_position_embeddings, c->shape_size});
    rc |= add_param(h, p + "embeddings.LayerNorm.weight", &h->emb_g, {H});
    rc |= add_param(h, p + "embeddings.LayerNorm.bias", &h->emb_b, {H});
    rc |= add_param(h, p + "patch_embed.proj.weight", &h->patch_w, {H, c->num_channels, c->patch_size, c->patch_size});
    rc |= add_param(h, p + "patch_embed.proj.bias", &h->patch_b, {H});
    rc |= add_param(h, p + "cls_token", &h->cls_token, {1, 1, H});
    rc |= add_param(h, p + "pos_embed", &h->pos_embed, {1, NP + 1, H});
    rc |= add_param(h, p + "norm.weight", &h->norm_g, {H});
    rc |= add_param(h, p + "norm.bias", &h->norm_b, {H});
    rc |= add_param(h, p + "LayerNorm.weight", &h->ln_g, {H});
    rc |= add_param(h, p + "LayerNorm.bias", &h->ln_b, {H});
    rc |= add_param(h, p + "encoder.rel_pos_bias.weight", &h->rel1, {c->num_attention_heads, c->rel_pos_bins});
    rc |= add_param(h, p + "encoder.rel_pos_x_bias.weight", &h->relx, {c->num_attention_heads, c->rel_2d_pos_bins});
    rc |= add_param(h, p + "encoder.rel_pos_y_bias.weight", &h->rely, {c->num_attention_heads, c->rel_2d_pos_bins});
    for (int l = 0; l < L && !rc; ++l) {
        LayerW& w = h->layers[l];
        const std::string q = p + "encoder.layer." + std::to_string(l) + ".";
        rc |= dev_alloc(h, &w.qkv_w, (size_t)3 * H * H);
        rc |= dev_alloc(h, &w.qkv_b, (size_t)3 * H);
        if (rc) break;
        const char* nm[3] = {"query", "key", "value"};
        for (int t = 0; t < 3; ++t) {           // fused [3H][H] weight: Q rows, K rows, V rows
            rc |= add_param(h, q + "attention.self." + nm[t] + ".weight", nullptr, {H, H}, w.qkv_w + (size_t)t * H * H);
            rc |= add_param(h, q + "attention.self." + nm[t] + ".bias", nullptr, {H}, w.qkv_b + (size_t)t * H);
        }
        rc |= add_param(h, q + "attention.output.dense.weight", &w.ao_w, {H, H});
        rc |= add_param(h, q + "attention.output.dense.bias", &w.ao_b, {H});
        rc |= add_param(h, q + "attention.output.LayerNorm.weight", &w.ao_g, {H});
        rc |= add_param(h, q + "attention.output.LayerNorm.bias", &w.ao_beta, {H});
        rc |= add_param(h, q + "intermediate.dense.weight", &w.f1_w, {I, H});
        rc |= add_param(h, q + "intermediate.dense.bias", &w.f1_b, {I});
        rc |= add_param(h, q + "output.dense.weight", &w.f2_w, {H, I});
        rc |= add_param(h, q + "output.dense.bias", &w.f2_b, {H});
        rc |= add_param(h, q + "output.LayerNorm.weight", &w.f_g, {H});
        rc |= add_param(h, q + "output.LayerNorm.bias", &w.f_beta, {H});
    }
    const char* emb_nm[3] = {"vision_exit_embeddings", "text_exit_embeddings", "concat_exit_embeddings"};
    for (int i = 0; i < c->n_embedding_exits && !rc; ++i) {
        const int kind = c->embedding_exits[i];
        if (kind < 0 || kind > 2) { rc = fail(nullptr, "bad embedding exit kind"); break; }
        rc |= add_head(h, p + emb_nm[kind], &h->emb_heads[kind], H, out_dim, two);
    }
    for (int k = 0; k < c->n_encoder_exits && !rc; ++k)
        rc |= add_head(h, p + "encoder.early_exits." + std::to_string(k), &h->enc_heads[k], H, out_dim, two);
    rc |= add_head(h, "classifier", &h->classifier, H, K, true);       // HF:799-823, always dense + out_proj
    }

    // ---- workspace --------------------------------------------------------------------------------------------
    const size_t Bm = c->max_docs, Tm = c->max_text_len, Pv = NP + 1;
    const size_t rows = Bm * (Tm + Pv);
    const int E = c->n_embedding_exits + c->n_encoder_exits;
    const size_t tch = (Tm + 31) / 32, vch = (Pv + 31) / 32;
    if (!rc) {
        rc |= dev_alloc(h, &h->X, rows * H);
        rc |= dev_alloc(h, &h->Y, rows * H);
        rc |= dev_alloc(h, &h->QKV, rows * 3 * H);
        rc |= dev_alloc(h, &h->CTX, rows * H);
        rc |= dev_alloc(h, &h->H1, rows * I);
        if (h->split) {
            rc |= dev_alloc(h, &h->Xs, rows * H);
            rc |= dev_alloc(h, &h->Ys, rows * H);
            rc |= dev_alloc(h, &h->absmax_dev, 4);
            rc |= dev_alloc(h, &h->cls_f32, Bm * H);
            {
                rc |= dev_alloc(h, &h->Yc, Bm * H);
                rc |= dev_alloc(h, &h->Ycs, Bm * H);
                rc |= dev_alloc(h, &h->H1c, Bm * I);
                rc |= dev_alloc(h, &h->Xc, Bm * H);
                rc |= dev_alloc(h, &h->Xcs, Bm * H);
                rc |= dev_alloc(h, &h->iota, Bm);
                if (!beit) {
                    rc |= dev_alloc(h, &h->Qc, Bm * H);
                    rc |= dev_alloc(h, &h->xp_u, Bm * (size_t)c->num_attention_heads * H);
                    rc |= dev_alloc(h, &h->xp_s0, Bm * (size_t)c->num_attention_heads * 2);
                    rc |= dev_alloc(h, &h->xp_order, Bm + 1);
                    rc |= dev_alloc(h, &h->xp_c, Bm * (size_t)c->num_attention_heads * H);
                    rc |= dev_alloc(h, &h->xp_part, 4 * Bm * H);      // split-K parts of the probe's FFN-down rows
                }
                if (!rc) {
                    std::vector<int> io(Bm);
                    for (size_t i = 0; i < Bm; ++i) io[i] = (int)i;
                    if (hipMemcpy(h->iota, io.data(), sizeof(int) * Bm, hipMemcpyHostToDevice) != hipSuccess) rc = fail(h, "hipMemcpy failed");
                }
            }
            if (!beit) {
                h->idx_nb = (int)((Tm + Pv + 31) / 32);
                const int maxpos = (int)std::max(Tm, Pv);
                // Round 6: the 16-bit pair index + delta table (attention_idx.hip, IDX16) is bit-identical to the word index and its lookups are 13 %
                // cheaper, but the 4 KB delta table it refills per work item costs more than that returns (9.27 against 9.15 ms per forward of 256
                // documents): measured, not shipped.  MMEE_ATTN_IDX=16 selects it in the DIAGNOSTIC library (A/B, tests of the form).
                static const int idx_env = mmee::diag_env_int("MMEE_ATTN_IDX", 32);
                h->idx16 = idx_env == 16 && mmee::attention_idx16_fits(c->rel_pos_bins, c->rel_2d_pos_bins, 2 * maxpos - 1);
                h->idx_stride = (size_t)h->idx_nb * h->idx_nb * (h->idx16 ? 512 : 1024);
                rc |= dev_alloc(h, &h->pair_idx, Bm * h->idx_stride);
                if (h->idx16) {
                    rc |= dev_alloc(h, &h->pair_idx0, Bm * (size_t)h->idx_nb * 1024);
                    rc |= dev_alloc(h, &h->keymask, Bm * (size_t)h->idx_nb);
                    rc |= dev_alloc(h, &h->doc_flags, Bm);
                }
            }
        }
        rc |= dev_alloc(h, &h->vis_raw, Bm * NP * H);
        rc |= dev_alloc(h, &h->text_part, Bm * tch * H);
        rc |= dev_alloc(h, &h->vis_part, Bm * vch * H);
        rc |= dev_alloc(h, &h->cat_part, Bm * (tch + vch) * H);
        for (int k = 0; k < 3; ++k) rc |= dev_alloc(h, &h->pooled[k], Bm * H);
        rc |= dev_alloc(h, &h->hid, Bm * H);
        rc |= dev_alloc(h, &h->hid2, Bm * H);
        rc |= dev_alloc(h, &h->head_logits, Bm * 64);
        rc |= dev_alloc(h, &h->pol_logits, Bm * 64);
        rc |= dev_alloc(h, &h->text_dst, Bm * Tm + 1);
        rc |= dev_alloc(h, &h->emb_pos, Bm * Tm + 1);
        rc |= dev_alloc(h, &h->ntext, Bm);
        rc |= dev_alloc(h, &h->row_src, rows);
        rc |= dev_alloc(h, &h->err_flag, 4);
        h->n_queue_heads = 128 * (12 * L + 4 * (E + 1) + 16);     // 8 XCD-local heads per launch, one 64-byte line each
        rc |= dev_alloc(h, &h->queue_heads, (size_t)h->n_queue_heads);
        rc |= dev_alloc(h, &h->meta[0], rows);
        rc |= dev_alloc(h, &h->meta[1], rows);
        const size_t st = (size_t)(E + 2) * (Bm + 1);
        rc |= dev_alloc(h, &h->doc_orig, st);
        rc |= dev_alloc(h, &h->doc_off, st);
        rc |= dev_alloc(h, &h->x_src, st);
        rc |= dev_alloc(h, &h->meta_src, st);
        rc |= dev_alloc(h, &h->counts, (size_t)(E + 2));
        rc |= dev_alloc(h, &h->thr_dev, 256);
        rc |= dev_alloc(h, &h->pat_state, 2 * Bm);
    }
    if (rc) {
        g_create_error = h->err.empty() ? g_create_error : h->err;
        for (void* q : h->allocs) (void)hipFree(q);
        delete h;
        return 1;
    }
    *out = h;
    return 0;
}

int ee_destroy(ee_handle* h) {
    if (!h) return 0;
    (void)hipDeviceSynchronize();
    for (auto& ev : h->prof_pool) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    for (auto& g : h->graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (h->fwd_done) (void)hipEventDestroy(h->fwd_done);
    if (h->err_host) (void)hipHostFree(h->err_host);
    for (auto& es : h->errs) if (es.done) (void)hipEventDestroy(es.done);
    for (void* q : h->allocs) (void)hipFree(q);
    delete h;
    return 0;
}

int32_t ee_num_expected_tensors(const ee_handle* h) { return h ? (int32_t)h->names.size() : 0; }
const char* ee_expected_tensor_name(const ee_handle* h, int32_t i) {
    if (!h || i < 0 || i >= (int32_t)h->names.size()) return nullptr;
    return h->names[i].c_str();
}

static inline float half_to_float(uint16_t v) {
    const uint32_t s = (v >> 15) & 1, e = (v >> 10) & 31, m = v & 1023;
    uint32_t u;
    if (e == 0) {
        if (m == 0) u = s << 31;
        else {
            int ee = -1;
            uint32_t mm = m;
            do { ++ee; mm <<= 1; } while (!(mm & 1024));
            u = (s << 31) | ((uint32_t)(127 - 15 - ee) << 23) | ((mm & 1023) << 13);
        }
    } else if (e == 31) u = (s << 31) | 0x7f800000u | (m << 13);
    else u = (s << 31) | ((e + 112) << 23) | (m << 13);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int ee_load_tensor(ee_handle* h, const char* name, const void* data, const int64_t* shape, int32_t ndim, int32_t dtype,
                   int32_t is_device) {
    if (!h || !name || !data || !shape) return fail(h, "ee_load_tensor: null argument");
    auto it = h->params.find(name);
    if (it == h->params.end()) return fail(h, "ee_load_tensor: unknown parameter '%s'", name);
    Param& p = it->second;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
    bool same = (size_t)ndim == p.shape.size();
    for (int i = 0; same && i < ndim; ++i) same = shape[i] == p.shape[i];
    if (!same) {
        std::string want, got;
        for (auto d : p.shape) want += std::to_string(d) + ",";
        for (int i = 0; i < ndim; ++i) got += std::to_string(shape[i]) + ",";
        return fail(h, "ee_load_tensor: '%s' has shape (%s) but the config expects (%s)", name, got.c_str(), want.c_str());
    }
    if (dtype == MMEE_DT_F32) {
        HIP_OK(h, hipMemcpy(p.ptr, data, n * sizeof(float), is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    } else if ((dtype == MMEE_DT_F16 || dtype == MMEE_DT_BF16) && !is_device) {
        std::vector<float> tmp(n);
        const uint16_t* s = static_cast<const uint16_t*>(data);
        for (size_t i = 0; i < n; ++i) {
            if (dtype == MMEE_DT_BF16) {
                const uint32_t u = (uint32_t)s[i] << 16;
                memcpy(&tmp[i], &u, 4);
            } else tmp[i] = half_to_float(s[i]);
        }
        HIP_OK(h, hipMemcpy(p.ptr, tmp.data(), n * sizeof(float), hipMemcpyHostToDevice));
    } else {
        return fail(h, "ee_load_tensor: dtype %d (device=%d) not supported; pass f32, or f16/bf16 from host memory", dtype, is_device);
    }
    p.loaded = true;
    h->finalized = false;
    return 0;
}

int ee_finalize(ee_handle* h) {
    if (!h) return 1;
    std::string missing;
    int nmiss = 0;
    for (auto& n : h->names)
        if (!h->params[n].loaded) {
            if (nmiss < 8) missing += n + " ";
            ++nmiss;
        }
    if (nmiss) return fail(h, "ee_finalize: %d parameter(s) not loaded: %s%s", nmiss, missing.c_str(), nmiss > 8 ? "..." : "");
    const ee_config& c = h->cfg;
    if (h->split) {
        // split-f16 rows of the four big weights of every layer; per-tensor power-of-two scale that puts max|w| in
        // [2^12, 2^13) (capped at 2^8: typical |w| ~ 0.02 then sits near 5, its lo plane well inside the f16 normal range)
        const int H = c.hidden_size, I = c.intermediate_size;
        auto build = [&](const float* w, int N, int K, float** out, float* inv) -> int {
            if (!*out && dev_alloc(h, out, (size_t)N * K)) return 1;
            mmee::launch_absmax(w, (size_t)N * K, h->absmax_dev, nullptr);
            float mx = 0.f;
            HIP_OK(h, hipMemcpy(&mx, h->absmax_dev, sizeof(float), hipMemcpyDeviceToHost));
            if (!(mx < 3.0e38f)) return fail(h, "ee_finalize: a weight tensor holds inf/nan");
            int e = 8;
            if (mx > 0.f) {
                int ex = 0;
                (void)std::frexp(mx, &ex);            // mx = m * 2^ex, m in [0.5, 1)
                e = std::min(8, 13 - ex);
            }
            const float scale = std::ldexp(1.0f, e);
            *inv = std::ldexp(1.0f, -e);
            mmee::launch_split_rows(w, *out, nullptr, N, N, K, scale, h->num_cus, nullptr);
            return 0;
        };
        for (auto& w : h->layers) {
            if (build(w.qkv_w, 3 * H, H, &w.qkv_s, &w.qkv_inv)) return 1;
            if (build(w.ao_w, H, H, &w.ao_s, &w.ao_inv)) return 1;
            if (build(w.f1_w, I, H, &w.f1_s, &w.f1_inv)) return 1;
            if (build(w.f2_w, H, I, &w.f2_s, &w.f2_inv)) return 1;
        }
        // the dense layer of every exit head and of the classifier (EE/models/LayoutLMv3.py:86-93, HF:799-823): H x H, on CLS rows
        if (mmee::gemm_split_supports(H, H) && c.arch != MMEE_ARCH_BEIT) {
            auto head = [&](HeadW& hw) -> int { return hw.dense_w ? build(hw.dense_w, H, H, &hw.dense_s, &hw.dense_inv) : 0; };
            for (auto& hw : h->enc_heads) if (head(hw)) return 1;
            if (head(h->classifier)) return 1;
        }
        const int Kp = c.num_channels * c.patch_size * c.patch_size;
        const size_t NPp = (size_t)(c.input_size / c.patch_size) * (c.input_size / c.patch_size);
        const bool fits = NPp * Kp <= ((size_t)c.max_text_len + NPp + 1) * I;      // the split patches are staged in H1
        if (mmee::gemm_split_supports(H, Kp) && c.patch_size % 4 == 0 && fits && build(h->patch_w, H, Kp, &h->patch_s, &h->patch_inv)) return 1;
        HIP_OK(h, hipDeviceSynchronize());
    }
    if (c.arch == MMEE_ARCH_BEIT) {      // absolute position embeddings only: the attention kernel gets one-entry zero tables
        h->c1 = h->c2 = 0;
        h->n1 = h->n2 = 4;
        if (!h->t1) {
            if (dev_alloc(h, &h->t1, (size_t)c.num_attention_heads * 4)) return 1;
            if (dev_alloc(h, &h->tx, (size_t)c.num_attention_heads * 4)) return 1;
            if (dev_alloc(h, &h->ty, (size_t)c.num_attention_heads * 4)) return 1;
        }
        HIP_OK(h, hipMemset(h->t1, 0, sizeof(float) * c.num_attention_heads * 4));
        HIP_OK(h, hipMemset(h->tx, 0, sizeof(float) * c.num_attention_heads * 4));
        HIP_OK(h, hipMemset(h->ty, 0, sizeof(float) * c.num_attention_heads * 4));
        HIP_OK(h, hipDeviceSynchronize());
        h->finalized = true;
        return 0;
    }
    const int NP = (c.input_size / c.patch_size) * (c.input_size / c.patch_size);
    const int maxpos = std::max(c.max_text_len, NP + 1);
    h->c1 = maxpos - 1;
    h->n1 = 2 * maxpos - 1;
    h->c2 = c.max_2d_position_embeddings - 1;
    h->n2 = 2 * c.max_2d_position_embeddings - 1;
    if (!h->t1) {
        if (dev_alloc(h, &h->t1, (size_t)c.num_attention_heads * h->n1)) return 1;
        if (dev_alloc(h, &h->tx, (size_t)c.num_attention_heads * h->n2)) return 1;
        if (dev_alloc(h, &h->ty, (size_t)c.num_attention_heads * h->n2)) return 1;
    }
    std::vector<unsigned char> l1(h->n1), l2(h->n2);
    bucket_lut_host(c.rel_pos_bins, c.max_rel_pos, h->c1, l1.data());
    bucket_lut_host(c.rel_2d_pos_bins, c.max_rel_2d_pos, h->c2, l2.data());
    if (!h->lut1_dev) {
        if (dev_alloc(h, &h->lut1_dev, (size_t)h->n1 + 4)) return 1;      // + 4: pair_index_kernel stages them as whole words
        if (dev_alloc(h, &h->lut2_dev, (size_t)h->n2 + 4)) return 1;
    }
    unsigned char *d1 = h->lut1_dev, *d2 = h->lut2_dev;      // kept: the per-forward pair index is built from them
    HIP_OK(h, hipMemcpy(d1, l1.data(), h->n1, hipMemcpyHostToDevice));
    HIP_OK(h, hipMemcpy(d2, l2.data(), h->n2, hipMemcpyHostToDevice));
    launch_build_value_tables(h->rel1, h->relx, h->rely, d1, d2, c.num_attention_heads, c.rel_pos_bins, c.rel_2d_pos_bins,
                              h->n1, h->n2, 1.0f / std::sqrt((float)(c.hidden_size / c.num_attention_heads)), h->t1, h->tx,
                              h->ty, nullptr);
    HIP_OK(h, hipDeviceSynchronize());
    h->finalized = true;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
}  // extern "C"

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
        if (!a.thresholds && !cap && !patience && !no_exit)
            return fail(h, "ee_forward: thresholds required unless MMEE_FLAG_NO_EXIT or MMEE_CRIT_PATIENCE");
        if (patience && h->patience < 1 && !no_exit)
            return fail(h, "ee_forward: the patience criterion needs ee_set_patience(h, t) with t >= 1 before the first forward");
        if ((head_mask || attn_out) && (a.flags & (MMEE_FLAG_NO_EXIT | MMEE_FLAG_WHOLE_LAYERS)) != (MMEE_FLAG_NO_EXIT | MMEE_FLAG_WHOLE_LAYERS))
            return fail(h, "ee_forward: head_mask / attention maps exist in dump-all mode with whole layers only (MMEE_FLAG_NO_EXIT | MMEE_FLAG_WHOLE_LAYERS)");
        if ((head_mask || attn_out) && beit) return fail(h, "ee_forward: head_mask / attention maps are built for the LayoutLMv3 layers only");
        if (attn_out && (!(a.flags & MMEE_FLAG_DENSE_ROWS) || !mmee::attention_probs_supports(T + Pv)))
            return fail(h, "ee_forward: attention maps are (B, heads, S, S) in the padded layout: pass MMEE_FLAG_DENSE_ROWS (S <= 1280)");
        if ((a.flags & MMEE_FLAG_ONE_TERM) && (beit || !sp))
            return fail(h, "ee_forward: MMEE_FLAG_ONE_TERM exists for MMEE_PREC_F32_SPLIT LayoutLMv3 handles only");
        if (hs_out && (a.flags & (MMEE_FLAG_NO_EXIT | MMEE_FLAG_WHOLE_LAYERS)) != (MMEE_FLAG_NO_EXIT | MMEE_FLAG_WHOLE_LAYERS))
            return fail(h, "ee_forward: hidden states are collected in dump-all mode with whole layers only (MMEE_FLAG_NO_EXIT | MMEE_FLAG_WHOLE_LAYERS)");
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

    // the fields every GEMM of the forward shares; a launch sets its own on top
    GemmArgs gemm_args() const {
        GemmArgs g{};
        g.scale = 1.f; g.prio_mode = 1; g.err_flag = h->err_flag;
        return g;
    }

    void run_gemm(GemmArgs g, int epi) {
        g.terms = one_term ? 1 : 3;
        if (sp) launch_gemm_split(g, epi, max_rows, cus, s);
        else launch_gemm_f32(g, epi, AMODE_ROWS, max_rows, cus, s);
    }

    // the layer output X as its readers find it: split planes of Xs (scaled by kSplitScaleX) or f32 rows of X
    const float* x_out() const { return x_split ? h->Xs : h->X; }
    float x_inv() const { return x_split ? 1.0f / mmee::kSplitScaleX : 0.f; }

    // patch projection (Conv2d with stride = kernel = a GEMM over flattened patches, HF:75-81) -> vis_raw [B * NP][H].  Split mode:
    // the patches are written once as split rows (into H1, idle until the first FFN) and the split kernel runs the GEMM; otherwise
    // the f32 kernel gathers the patches itself.
    void patch_projection() {
        ProfScope ps(h, P_GPATCH, s);
        GemmArgs pg = gemm_args();
        pg.bias = h->patch_b; pg.C = h->vis_raw; pg.ldc = H; pg.m_static = B * NP; pg.N = H;
        pg.K = c.num_channels * c.patch_size * c.patch_size; pg.tile_counter = next_head();
        if (sp && h->patch_s) {
            { ProfScope pp(h, P_PSPLIT, s); mmee::launch_patch_split(a.pixel_values, h->H1, B, c.num_channels, c.input_size, c.patch_size, mmee::kSplitScaleX, cus, s, h->err_flag); }
            pg.A = h->H1; pg.lda = pg.K; pg.W = h->patch_s; pg.alpha = h->patch_inv / mmee::kSplitScaleX;
            launch_gemm_split(pg, EPI_BIAS, B * NP, cus, s);
            return;
        }
        pg.W = h->patch_w;
        pg.pix = a.pixel_values; pg.C_in = c.num_channels; pg.R = c.input_size; pg.P = c.patch_size; pg.G = G;
        launch_gemm_f32(pg, EPI_BIAS, AMODE_IM2COL, B * NP, cus, s);
    }

    // ---- BEiT / DiT: uniform 197-row documents, BeitEmbeddings = patch conv + cls + absolute position embeddings ----
    void embed_beit() {
        { ProfScope ps(h, P_PREP, s); launch_prep_uniform(B, Pv, S_doc_off(0), S_x_src(0), S_doc_orig(0), h->meta[0], h->counts, s); }
        patch_projection();
        { ProfScope ps(h, P_EMBV, s); launch_embed_beit(h->vis_raw, h->cls_token, c.use_abs_pos ? h->pos_embed : nullptr, B, Pv, H, h->X, s); }
    }

    // ---- LayoutLMv3: packed layout of stage 0, text and visual embeddings, the inputs of the embedding exits ----
    void embed_layoutlmv3() {
        PrepArgs pa{};
        pa.input_ids = (const long long*)a.input_ids;
        pa.attention_mask = (const long long*)a.attention_mask;
        pa.bbox = (const long long*)a.bbox;
        pa.position_ids = (const long long*)a.position_ids;
        pa.token_type_ids = (const long long*)a.token_type_ids; pa.type_vocab = c.type_vocab_size;
        pa.B = B; pa.T = T; pa.Pv = Pv; pa.G = G;
        pa.pad_id = c.pad_token_id; pa.vocab = c.vocab_size; pa.max_2d = c.max_2d_position_embeddings; pa.max_pos = c.max_position_embeddings;
        pa.dense_rows = (a.flags & MMEE_FLAG_DENSE_ROWS) ? 1 : 0;
        pa.text_dst = h->text_dst; pa.emb_pos = h->emb_pos; pa.ntext = h->ntext;
        pa.doc_off = S_doc_off(0); pa.x_src = S_x_src(0); pa.doc_orig = S_doc_orig(0);
        pa.meta = h->meta[0]; pa.counts = h->counts; pa.err_flag = h->err_flag;
        {
            ProfScope ps(h, P_PREP, s);
            launch_prep(pa, s);
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

        bool need[3] = {false, false, false};
        for (int i = 0; i < c.n_embedding_exits; ++i) need[c.embedding_exits[i]] = true;
        const int tch = (T + 31) / 32, vch = (Pv + 31) / 32;
        EmbedArgs ea{};
        ea.input_ids = pa.input_ids; ea.token_type_ids = (const long long*)a.token_type_ids; ea.bbox = pa.bbox;
        ea.emb_pos = h->emb_pos; ea.text_dst = h->text_dst; ea.ntext = h->ntext; ea.doc_off = S_doc_off(0);
        ea.B = B; ea.T = T; ea.Pv = Pv; ea.H = H; ea.cs = c.coordinate_size; ea.ss = c.shape_size; ea.max_2d = c.max_2d_position_embeddings;
        ea.vocab = c.vocab_size; ea.type_vocab = c.type_vocab_size;
        ea.inputs_embeds = embeds_in;
        ea.word = h->word; ea.type = h->type; ea.pos = h->pos; ea.xtab = h->xtab; ea.ytab = h->ytab; ea.htab = h->htab; ea.wtab = h->wtab;
        ea.ln1_g = h->emb_g; ea.ln1_b = h->emb_b; ea.eps1 = c.layer_norm_eps;
        ea.ln2_g = h->ln_g; ea.ln2_b = h->ln_b; ea.eps2 = c.layer_norm_eps;
        ea.X = h->X;
        if (sp) { ea.Xs = h->Xs; ea.split_scale = mmee::kSplitScaleX; ea.err_flag = h->err_flag; }      // split mode: the embeddings exist as split planes only
        ea.text_part = need[MMEE_EXIT_TEXT_AVG] ? h->text_part : nullptr;
        ea.cat_part = need[MMEE_EXIT_TEXT_VISUAL_CONCAT] ? h->cat_part : nullptr;
        ea.cat_chunks = tch + vch;
        { ProfScope ps(h, P_EMBT, s); launch_embed_text(ea, s); }

        patch_projection();

        EmbedArgs va = ea;
        va.ln1_g = h->norm_g; va.ln1_b = h->norm_b; va.eps1 = 1e-6f;        // layoutlmv3.norm = LayerNorm(eps=1e-6), HF:563
        va.cls_token = h->cls_token; va.pos_embed = h->pos_embed; va.vis_raw = h->vis_raw;
        va.vis_part = need[MMEE_EXIT_VISION_AVG] ? h->vis_part : nullptr;
        {
            ProfScope ps(h, P_EMBV, s);
            launch_embed_visual(va, s);
            if (need[MMEE_EXIT_VISION_AVG]) launch_pool_finish(h->vis_part, vch, H, (float)Pv, h->pooled[0], B, s);
            if (need[MMEE_EXIT_TEXT_AVG]) launch_pool_finish(h->text_part, tch, H, (float)T, h->pooled[1], B, s);
            if (need[MMEE_EXIT_TEXT_VISUAL_CONCAT]) launch_pool_finish(h->cat_part, tch + vch, H, (float)(T + Pv), h->pooled[2], B, s);
        }
    }

    // Q | K | V projection of every row of the stage, A row r read from A[rows[r]] (rows null: dense), Q pre-divided by sqrt(d) (HF:263)
    void qkv(int l, const float* A, const int* rows) {
        const LayerW& w = h->layers[l];
        GemmArgs g = gemm_args();
        g.A = A; g.lda = H; g.row_src = rows; g.W = sp ? w.qkv_s : w.qkv_w; g.bias = w.qkv_b; g.C = h->QKV; g.ldc = 3 * H;
        g.alpha = w.qkv_inv / mmee::kSplitScaleX; g.out_split = sp ? 1 : 0; g.out_scale = mmee::kSplitScaleQKV;
        g.m_ptr = &h->counts[cur].n_rows; g.N = 3 * H; g.K = H; g.scale_cols = H; g.scale = 0.125f; g.tile_counter = next_head();
        { ProfScope ps(h, P_GQKV, s); run_gemm(g, EPI_BIAS); }
        h->rec.layer_qkv_stage[l] = cur;
    }

    // BEiT (pre-LN): layernorm_before of the stage's rows into CTX, the Q | K | V projection from there
    void beit_qkv(int l, const int* rows) {
        const LayerW& w = h->layers[l];
        { ProfScope ps(h, P_LN, s); launch_ln_rows(h->X, sp ? nullptr : h->CTX, rows, &h->counts[cur].n_rows, max_rows, H, w.ao_g, w.ao_beta, c.layer_norm_eps, cus, s, sp ? h->CTX : nullptr, mmee::kSplitScaleX, h->err_flag); }
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
        else if (sp) launch_attention_pair(at, B, cus, c.max_rel_pos, c.max_rel_2d_pos, (a.flags & MMEE_FLAG_DENSE_ROWS) ? 1 : 0, s);
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
        GemmArgs g = gemm_args();        // Y = X + lambda_1 * (ctx Wo^T + bo)
        g.A = h->CTX; g.lda = H; g.W = sp ? w.ao_s : w.ao_w; g.bias = w.ao_b; g.C = h->Y; g.ldc = H; g.resid = h->X; g.ldr = H; g.resid_row_src = x_rows;
        g.alpha = w.ao_inv / mmee::kSplitScaleCtx; g.col_scale = w.lam1; g.m_ptr = rp; g.N = H; g.K = H; g.tile_counter = next_head();
        { ProfScope ps(h, P_GAO, s); run_gemm(g, EPI_RESID); }
        { ProfScope ps(h, P_LN, s); launch_ln_rows(h->Y, sp ? nullptr : h->CTX, nullptr, rp, max_rows, H, w.f_g, w.f_beta, c.layer_norm_eps, cus, s, sp ? h->CTX : nullptr, mmee::kSplitScaleX, h->err_flag); }
        g = gemm_args();
        g.A = h->CTX; g.lda = H; g.W = sp ? w.f1_s : w.f1_w; g.bias = w.f1_b; g.C = h->H1; g.ldc = I; g.m_ptr = rp; g.N = I; g.K = H;
        g.alpha = w.f1_inv / mmee::kSplitScaleX; g.out_split = sp ? 1 : 0; g.out_scale = mmee::kSplitScaleH1; g.tile_counter = next_head();
        { ProfScope ps(h, P_GUP, s); run_gemm(g, EPI_GELU); }
        g = gemm_args();      // X = Y + lambda_2 * (h1 W2^T + b2)
        g.A = h->H1; g.lda = I; g.W = sp ? w.f2_s : w.f2_w; g.bias = w.f2_b; g.C = h->X; g.ldc = H; g.resid = h->Y; g.ldr = H; g.col_scale = w.lam2;
        g.alpha = w.f2_inv / mmee::kSplitScaleH1; g.m_ptr = rp; g.N = H; g.K = I; g.tile_counter = next_head();
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
        GemmArgs g = gemm_args();
        g.A = h->CTX; g.lda = H; g.row_src = S_doc_off(cur); g.W = w.ao_s; g.bias = w.ao_b; g.C = h->Yc; g.ldc = H;
        g.resid = h->X; g.ldr = H; g.resid_row_src = x_phys; g.col_scale = w.lam1;
        g.alpha = w.ao_inv / mmee::kSplitScaleCtx; g.probe = 1; g.m_ptr = nd; g.N = H; g.K = H;
        launch_gemm_split(g, EPI_RESID, B, cus, s);
        launch_ln_rows(h->Yc, nullptr, nullptr, nd, B, H, w.f_g, w.f_beta, c.layer_norm_eps, cus, s, h->Ycs, mmee::kSplitScaleX, h->err_flag);
        g = gemm_args();
        g.A = h->Ycs; g.lda = H; g.W = w.f1_s; g.bias = w.f1_b; g.C = h->H1c; g.ldc = I; g.m_ptr = nd; g.N = I; g.K = H;
        g.alpha = w.f1_inv / mmee::kSplitScaleX; g.out_split = 1; g.out_scale = mmee::kSplitScaleH1; g.probe = 1;
        launch_gemm_split(g, EPI_GELU, B, cus, s);
        g = gemm_args();
        g.A = h->H1c; g.lda = I; g.W = w.f2_s; g.bias = w.f2_b; g.C = h->Xc; g.ldc = H; g.resid = h->Yc; g.ldr = H; g.col_scale = w.lam2;
        g.alpha = w.f2_inv / mmee::kSplitScaleH1; g.probe = 1; g.m_ptr = nd; g.N = H; g.K = I;
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
        GemmArgs g = gemm_args();
        g.A = h->CTX; g.lda = H; g.W = sp ? w.ao_s : w.ao_w; g.bias = w.ao_b; g.C = h->Y; g.ldc = H; g.resid = sp ? h->Xs : h->X; g.ldr = H; g.resid_row_src = x_rows;
        g.resid_split_inv = sp ? 1.0f / mmee::kSplitScaleX : 0.f;
        g.alpha = w.ao_inv / mmee::kSplitScaleCtx; g.role_tag = 2; g.m_ptr = rp; g.N = H; g.K = H; g.tile_counter = next_head();
        { ProfScope ps(h, P_GAO, s); run_gemm(g, EPI_RESID); }
        // split mode: the LayerNorm output exists only as split planes (22 bits); its readers (next GEMM, residual adds, exit heads) take it from there
        { ProfScope ps(h, P_LN, s); launch_ln_rows(h->Y, sp ? nullptr : h->Y, nullptr, rp, max_rows, H, w.ao_g, w.ao_beta, c.layer_norm_eps, cus, s, sp ? h->Ys : nullptr, mmee::kSplitScaleX, h->err_flag); }
        g = gemm_args();
        g.A = sp ? h->Ys : h->Y; g.lda = H; g.W = sp ? w.f1_s : w.f1_w; g.bias = w.f1_b; g.C = h->H1; g.ldc = I; g.m_ptr = rp; g.N = I; g.K = H; g.tile_counter = next_head();
        g.alpha = w.f1_inv / mmee::kSplitScaleX; g.out_split = sp ? 1 : 0; g.out_scale = mmee::kSplitScaleH1;
        { ProfScope ps(h, P_GUP, s); run_gemm(g, EPI_GELU); }
        g = gemm_args();
        g.A = h->H1; g.lda = I; g.W = sp ? w.f2_s : w.f2_w; g.bias = w.f2_b; g.C = h->X; g.ldc = H; g.resid = sp ? h->Ys : h->Y; g.ldr = H;
        g.resid_split_inv = sp ? 1.0f / mmee::kSplitScaleX : 0.f;
        g.alpha = w.f2_inv / mmee::kSplitScaleH1; g.role_tag = 3; g.m_ptr = rp; g.N = H; g.K = I; g.tile_counter = next_head();
        { ProfScope ps(h, P_GDOWN, s); run_gemm(g, EPI_RESID); }
        { ProfScope ps(h, P_LN, s); launch_ln_rows(h->X, sp ? nullptr : h->X, nullptr, rp, max_rows, H, w.f_g, w.f_beta, c.layer_norm_eps, cus, s, sp ? h->Xs : nullptr, mmee::kSplitScaleX, h->err_flag); }
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
            GemmArgs gq = gemm_args();
            gq.A = h->Xs; gq.lda = H; gq.row_src = x_phys; gq.W = w.qkv_s; gq.bias = w.qkv_b; gq.C = h->Qc; gq.ldc = H;
            gq.alpha = w.qkv_inv / mmee::kSplitScaleX; gq.m_ptr = nd; gq.N = H; gq.K = H; gq.scale_cols = H; gq.scale = 0.125f; gq.probe = 1;
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
        GemmArgs g = gemm_args();        // CLS rows only: A = context row doc_off[i], residual = the document's CLS row of Xs
        g.A = h->CTX; g.lda = H; g.row_src = S_doc_off(cur); g.W = w.ao_s; g.bias = w.ao_b; g.C = h->Yc; g.ldc = H;
        g.resid = h->Xs; g.ldr = H; g.resid_row_src = x_phys; g.resid_split_inv = 1.0f / mmee::kSplitScaleX;
        g.alpha = w.ao_inv / mmee::kSplitScaleCtx; g.probe = 1; g.m_ptr = nd; g.N = H; g.K = H;
        launch_gemm_split(g, EPI_RESID, B, cus, s);
        launch_ln_rows(h->Yc, nullptr, nullptr, nd, B, H, w.ao_g, w.ao_beta, c.layer_norm_eps, cus, s, h->Ycs, mmee::kSplitScaleX, h->err_flag);
        g = gemm_args();
        g.A = h->Ycs; g.lda = H; g.W = w.f1_s; g.bias = w.f1_b; g.C = h->H1c; g.ldc = I; g.m_ptr = nd; g.N = I; g.K = H;
        g.alpha = w.f1_inv / mmee::kSplitScaleX; g.out_split = 1; g.out_scale = mmee::kSplitScaleH1; g.probe = 1;
        launch_gemm_split(g, EPI_GELU, B, cus, s);
        g = gemm_args();
        constexpr int kSplitK = 4;
        if (xspace && h->xp_part && (I / 32) % kSplitK == 0) {
            // X space (already a re-association of the whole-layer arithmetic): the 96-stage k-loop of this one-row-per-document GEMM
            // is divided over four workgroups per tile; the LayerNorm kernel adds the four parts in order, the bias and the residual
            g.A = h->H1c; g.lda = I; g.W = w.f2_s; g.C = h->xp_part; g.ldc = H; g.k_splits = kSplitK; g.split_stride = (size_t)B * H;
            g.alpha = w.f2_inv / mmee::kSplitScaleH1; g.probe = 1; g.m_ptr = nd; g.N = H; g.K = I;
            launch_gemm_split(g, EPI_BIAS, B, cus, s);
            launch_ln_rows(h->xp_part, nullptr, nullptr, nd, B, H, w.f_g, w.f_beta, c.layer_norm_eps, cus, s, h->Xcs, mmee::kSplitScaleX, h->err_flag,
                           kSplitK, (size_t)B * H, w.f2_b, h->Ycs, 1.0f / mmee::kSplitScaleX);
        } else {
            g.A = h->H1c; g.lda = I; g.W = w.f2_s; g.bias = w.f2_b; g.C = h->Xc; g.ldc = H; g.resid = h->Ycs; g.ldr = H;
            g.resid_split_inv = 1.0f / mmee::kSplitScaleX; g.alpha = w.f2_inv / mmee::kSplitScaleH1; g.probe = 1; g.m_ptr = nd; g.N = H; g.K = I;
            launch_gemm_split(g, EPI_RESID, B, cus, s);
            launch_ln_rows(h->Xc, nullptr, nullptr, nd, B, H, w.f_g, w.f_beta, c.layer_norm_eps, cus, s, h->Xcs, mmee::kSplitScaleX, h->err_flag);
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
    void run_head(const HeadW& hw, const float* in, int ld, const int* gather, float* hid, float* out, const float* in_split, const int* split_rows) {
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

    // exit head (or the final classifier), decision, compaction of the documents that stay
    void run_exit(const HeadW* hw, const float* in, int ld, const int* gather, bool is_final, const float* in_split = nullptr,
                  const int* split_rows = nullptr) {
        const float* pol;
        const float* head = nullptr;
        int Kh = K;
        {
            ProfScope ps(h, P_HEAD, s);
            if (is_final) {
                run_head(h->classifier, in, ld, gather, h->hid, h->pol_logits, in_split, split_rows);
                pol = h->pol_logits;
            } else if (c.strategy == MMEE_STRATEGY_GATE) {
                // the policy only ever sees classifier(gate input) (EE/utils.py:183-188); the 2-way gate logits (exit_states) are
                // computed when the caller asked for them (the dump of model.forward), not in the fast path
                const bool want_gate = a.out_head_logits || a.out_head_crit;
                if (want_gate) run_head(*hw, in, ld, gather, h->hid, h->head_logits, in_split, split_rows);
                run_head(h->classifier, in, ld, gather, h->hid2, h->pol_logits, in_split, split_rows);  // gated_logits, EE/models/LayoutLMv3.py:768
                pol = h->pol_logits; head = want_gate ? h->head_logits : nullptr; Kh = 2;      // 2-way gate heads, EE/models/LayoutLMv3.py:83
            } else {
                run_head(*hw, in, ld, gather, h->hid, h->head_logits, in_split, split_rows);
                pol = h->head_logits; head = h->head_logits; Kh = K;
            }
        }
        DecideArgs d{};
        d.pol_logits = pol; d.head_logits = head; d.K = K; d.Kh = Kh;
        d.thr = a.thresholds ? a.thresholds[exit_index] : 0.0;
        d.temp = a.temperatures ? a.temperatures[exit_index] : 1.0;
        if (cap) { d.thr_ptr = cap->thr_dev; d.temp_ptr = cap->thr_dev + (E + 1); }      // replays read the vector of THEIR launch
        d.criterion = c.criterion; d.is_final = is_final ? 1 : 0; d.no_exit = no_exit ? 1 : 0; d.exit_index = exit_index; d.B = B;
        d.counts = &h->counts[cur]; d.doc_orig = S_doc_orig(cur); d.doc_off = S_doc_off(cur); d.x_phys = x_phys;
        d.n_counts = &h->counts[cur + 1]; d.n_doc_orig = S_doc_orig(cur + 1); d.n_doc_off = S_doc_off(cur + 1);
        d.n_x_src = S_x_src(cur + 1); d.n_meta_src = S_meta_src(cur + 1);
        d.out_logits = a.out_logits; d.out_exit = a.out_exit; d.out_conf = a.out_conf;
        d.out_all_logits = a.out_all_logits; d.out_all_crit = a.out_all_crit;
        d.out_head_logits = a.out_head_logits; d.out_head_crit = a.out_head_crit;
        if (patience) {
            PatienceArgs pa{};
            pa.t = h->patience;
            if (cap) pa.t_ptr = cap->thr_dev + 2 * (E + 1);                               // replays read the patience of THEIR launch
            pa.prev = h->pat_state; pa.run = h->pat_state + c.max_docs;
            ProfScope ps(h, P_DECIDE, s);
            launch_decide_patience(d, pa, s);
        } else {
            ProfScope ps(h, P_DECIDE, s);
            launch_decide(d, s);
        }
        h->rec.exit_stage[exit_index] = cur;
        if (!is_final) compact();
        exit_index += 1;
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
        if (!cap) { const int rc_pre = forward_pre(h, s); if (rc_pre) return rc_pre; }
        // (a kernel, not hipMemsetAsync: the same launch list then serves the eager call and the captured graph -- replays whose memset NODES were
        //  preceded by an eager forward on the handle came back with an unzeroed error word on ROCm 7.2, tools/graph_debug2.py)
        hipLaunchKernelGGL(zero_words_kernel, dim3(32), dim3(256), 0, s, h->err_flag, 4, h->queue_heads, h->n_queue_heads);
        h->next_queue_head = 0;
        if (h->prof_on) { h->prof_recs.clear(); h->prof_used = 0; }
        if (sp && !use_idx) {          // attention_pair.hip holds Delta tables up to fixed distances: refuse what it cannot hold
            AttnArgs chk{};
            chk.ctx_split = 1; chk.c1 = h->c1; chk.c2 = h->c2;
            if (!mmee::attention_pair_supports(chk, c.max_rel_pos, c.max_rel_2d_pos))
                return fail(h, "ee_forward: the split-precision attention kernels cannot hold this relative-position configuration "
                               "(bins %d / %d, distances %d / %d); use MMEE_PREC_F32", c.rel_pos_bins, c.rel_2d_pos_bins, c.max_rel_pos, c.max_rel_2d_pos);
        }
        if (beit) embed_beit();
        else embed_layoutlmv3();

        ForwardRecord& r = h->rec;
        r.layer_stage.assign(L, -1);
        r.layer_qkv_stage.assign(L, -1);
        r.layer_probe_stage.assign(L, -1);
        r.layer_xprobe.assign(L, 0);
        r.exit_stage.assign(E + 1, 0);
        x_phys = S_x_src(0);
        for (int i = 0; i < c.n_embedding_exits; ++i) {
            const int kind = c.embedding_exits[i];
            run_exit(&h->emb_heads[kind], h->pooled[kind], H, S_doc_orig(cur), false);
        }
        gather_hidden(0, x_out(), x_phys, x_inv());
        dump_hidden(0);
        // Which exit layers are probed first is part of the CALL, never of timing or history (round 5): every layer that ends
        // in a decision unless ee_set_probe_mask pinned a subset (ee_suggest_probe_mask prices one from a finished forward's stage populations;
        // the caller decides whether to pin it).  The same inputs therefore always run the same launch sequence and return the same bits.
        for (int l = 0; l < L; ++l) layer(l);
        final_exit();
        r.last_B = B; r.last_T = T; r.last_stages = E + 1; r.last_flags = a.flags;
        r.last_gate_heads = a.out_head_logits || a.out_head_crit;
        if (!cap) { const int rc_post = forward_post(h, s); if (rc_post) return rc_post; }
        return launch_status(h, cap ? "ee_graph_capture" : "ee_forward");
    }
};

// Synchronises the stream, then copies the first n StageCounts (of the last forward) to the host.
int read_stage_counts(ee_handle* h, void* stream, int n, std::vector<StageCounts>& sc) {
    HIP_OK(h, hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    sc.resize(n);
    HIP_OK(h, hipMemcpy(sc.data(), h->counts, sizeof(StageCounts) * n, hipMemcpyDeviceToHost));
    return 0;
}

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
    if (dev_alloc(h, &g.thr_dev, (size_t)2 * E1 + 1)) return 1;
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
    if (!thresholds && !g.no_exit && !g.patience)
        return fail(h, "ee_graph_launch: thresholds required (the graph was captured without MMEE_FLAG_NO_EXIT or MMEE_CRIT_PATIENCE)");
    if (h->prof_on) return fail(h, "ee_graph_launch: ee_profile times eager launches; disarm it first");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int rc_pre = forward_pre(h, s);
    if (rc_pre) return rc_pre;
    ThrPack p{};
    p.n = 2 * g.n_exits1 + 1;
    for (int i = 0; i < g.n_exits1; ++i) {
        p.v[i] = thresholds ? thresholds[i] : 0.0;
        p.v[g.n_exits1 + i] = temperatures ? temperatures[i] : 1.0;
    }
    p.v[2 * g.n_exits1] = (double)h->patience;
    hipLaunchKernelGGL(set_thresholds_kernel, dim3(1), dim3(64), 0, s, p, g.thr_dev);
    HIP_OK(h, hipGraphLaunch(g.exec, s));
    h->rec = g.rec;
    const int rc_post = forward_post(h, s);
    if (rc_post) return rc_post;
    return launch_status(h, "ee_graph_launch");
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

int ee_last_stage_counts(ee_handle* h, int32_t* docs_out, int32_t* rows_out, int32_t cap, int32_t* n_stages_out, void* stream) {
    if (!h || !h->rec.last_stages) return fail(h, "ee_last_stage_counts: no forward has run");
    const ForwardRecord& r = h->rec;
    std::vector<StageCounts> sc;
    if (read_stage_counts(h, stream, r.last_stages, sc)) return 1;
    const int err = take_errors(h, true, true);       // every forward enqueued so far has finished: all of their flags are reported here
    if (n_stages_out) *n_stages_out = r.last_stages;
    for (int i = 0; i < r.last_stages && i < cap; ++i) {
        if (docs_out) docs_out[i] = sc[r.exit_stage[i]].n_docs;
        if (rows_out) rows_out[i] = sc[r.exit_stage[i]].n_rows;
    }
    return report_errors(h, err, "a forward since the last check");
}

int ee_set_inputs_embeds(ee_handle* h, const float* embeds) {
    if (!h) return 1;
    if (embeds && h->cfg.arch == MMEE_ARCH_BEIT) return fail(h, "ee_set_inputs_embeds: an image-only model has no text embeddings");
    h->next_inputs_embeds = embeds;
    return 0;
}

int ee_set_hidden_states_out(ee_handle* h, float* out) {
    if (!h) return 1;
    h->next_hidden_out = out;
    return 0;
}

int ee_set_head_mask(ee_handle* h, const float* mask) {
    if (!h) return 1;
    h->next_head_mask = mask;
    return 0;
}

int ee_set_attentions_out(ee_handle* h, float* out) {
    if (!h) return 1;
    h->next_attn_out = out;
    return 0;
}

int ee_set_criterion(ee_handle* h, int32_t criterion) {
    if (!h) return 1;
    if (criterion != MMEE_CRIT_MAX_CONFIDENCE && criterion != MMEE_CRIT_ENTROPY && criterion != MMEE_CRIT_PATIENCE)
        return fail(h, "ee_set_criterion: unknown criterion %d", criterion);
    h->cfg.criterion = criterion;      // read by the decide kernel's arguments of every later ee_forward
    return 0;
}

int ee_set_patience(ee_handle* h, int32_t t) {
    if (!h) return 1;
    if (t < 1) return fail(h, "ee_set_patience: t=%d, the patience must be >= 1", t);
    h->patience = t;                   // eager forwards pass it by value; ee_graph_launch writes it to the graph's device vector
    return 0;
}

int ee_set_probe_mask(ee_handle* h, int32_t enabled, uint64_t mask) {
    if (!h) return 1;
    h->mask_on = enabled != 0;
    h->probe_mask = mask;
    return 0;
}

// The cost model that used to pick the schedule inside ee_forward from "whichever earlier forward had finished" (rounds 2-4), as an explicit,
// deterministic query: which exit layers are worth probing first, judged from the stage populations of the LAST forward on this handle.  A
// probe pays when the rows it saves (attention, attention-out, FFN -- and under MMEE_FLAG_XPROBE the Q | K | V projection -- of the documents
// that leave) cost more than the probe itself (a pass over every K | V row, or every LayerNorm row in X space, for the CLS queries + three
// latency-bound GEMMs on one row per document).  Rates as measured on MI355X.
int ee_suggest_probe_mask(ee_handle* h, uint32_t flags, uint64_t* mask_out, void* stream) {
    if (!h || !mask_out) return fail(h, "ee_suggest_probe_mask: null argument");
    const ForwardRecord& r = h->rec;
    if (!r.last_stages) return fail(h, "ee_suggest_probe_mask: no forward has run");
    if (r.last_flags & MMEE_FLAG_NO_EXIT) return fail(h, "ee_suggest_probe_mask: the last forward was a dump (nobody left): run a thresholded forward first");
    std::vector<StageCounts> sc;
    if (read_stage_counts(h, stream, r.last_stages + 1, sc)) return 1;
    const ee_config& c = h->cfg;
    const bool beit = c.arch == MMEE_ARCH_BEIT;
    const double H = c.hidden_size, I = c.intermediate_size;
    const int L = c.num_hidden_layers;
    uint64_t mask = 0;
    bool xs = false;
    if (h->split && !beit && (flags & MMEE_FLAG_XPROBE) && h->Qc && h->pair_idx && c.rel_pos_bins <= 64 && c.rel_2d_pos_bins <= 64) {
        mmee::XProbeArgs chk{};
        chk.H = c.hidden_size; chk.heads = c.num_attention_heads; chk.bins1 = c.rel_pos_bins; chk.bins2 = c.rel_2d_pos_bins; chk.pair_idx = h->pair_idx;
        const int G = c.input_size / c.patch_size;
        xs = mmee::xprobe_supports(chk, r.last_T + G * G + 1);
    }
    for (int k = 0; k < c.n_encoder_exits && h->split; ++k) {
        const int l = c.encoder_exit_layers[k] - 1;
        if (l == L - 1) continue;                     // the last layer: always the probe alone (LayoutLMv3) / always whole (BEiT mean pooling)
        const int st = c.n_embedding_exits + k;      // stage whose documents reach this decision
        if (st + 1 > r.last_stages) break;
        const double rows = sc[st].n_rows, leave = (double)sc[st].n_rows - (double)sc[st + 1].n_rows;
        if (rows <= 0) { mask |= 1ull << l; continue; }
        const double len = (double)sc[st].sum_len_sq / rows;      // mean keys per query
        const double t_row = 2.0 * (H * H + 2.0 * H * I + (xs ? 3.0 * H * H : 0.0)) / 380e12 + 4.0 * len * H / 200e12;
        const double cost = ((2.0 * H + I) / 32.0) * 0.9e-6 + (xs ? 180e-6 + rows * 4.0 * H / 4.5e12 : 100e-6 + rows * 8.0 * H / 3.6e12);
        if (leave * t_row > 1.1 * cost) mask |= 1ull << l;
    }
    *mask_out = mask;
    return 0;
}

// Shader-clock stamps (bench.py: docs_per_sec_per_ghz).  s_memtime counts shader clocks, s_memrealtime a constant 100 MHz.  The shader-clock
// counters of different CUs are NOT aligned with each other (measured, round 5: pairing a stamp taken on one CU with a later stamp taken on
// another CU of the same XCD gave 1.5 ... 3.3 "GHz" over a few milliseconds), so a stamp records one (s_memtime, s_memrealtime) pair PER CU --
// slot = XCC_ID x 256 + HW_ID bits 15:8 (CU, shader array, shader engine) -- and two stamps are compared slot by slot: the offsets cancel.
// 2048 one-wave workgroups, eight per CU on average, so practically every CU is reached by both stamps; the reader skips empty slots.
__global__ void clock_stamp_kernel(unsigned long long* __restrict__ out) {
    if (threadIdx.x != 0) return;
    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 7u;      // HW_REG_XCC_ID
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);            // HW_REG_HW_ID: CU_ID 11:8, SH_ID 12, SE_ID 15:13
    const unsigned slot = xcc * 256u + ((hw >> 8) & 255u);
    const unsigned long long t = __builtin_amdgcn_s_memtime(), r = __builtin_amdgcn_s_memrealtime();
    // several workgroups may land on one CU: the pair is written as one 16-byte store, so whichever wins leaves a consistent pair
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    *reinterpret_cast<u64x2*>(out + 2 * slot) = u64x2{t, r};
}

int ee_clock_stamp(uint64_t* out_dev, void* stream) {
    if (!out_dev) return fail(nullptr, "ee_clock_stamp: null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, "ee_clock_stamp: no HIP device");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(out_dev, 0, MMEE_CLOCK_STAMP_WORDS * sizeof(uint64_t), s) != hipSuccess) return fail(nullptr, "ee_clock_stamp: memset failed");
    hipLaunchKernelGGL(clock_stamp_kernel, dim3(2048), dim3(64), 0, s, reinterpret_cast<unsigned long long*>(out_dev));
    return launch_status(nullptr, "ee_clock_stamp");
}

int ee_last_flops(ee_handle* h, double* gemm_flops, double* attn_flops, void* stream) {
    if (!h || !h->rec.last_stages) return fail(h, "ee_last_flops: no forward has run");
    const ForwardRecord& r = h->rec;
    std::vector<StageCounts> sc;
    if (read_stage_counts(h, stream, r.last_stages, sc)) return 1;
    const ee_config& c = h->cfg;
    const double H = c.hidden_size, I = c.intermediate_size;
    const int G = c.input_size / c.patch_size;
    double gf = 2.0 * r.last_B * G * G * (double)(c.num_channels * c.patch_size * c.patch_size) * H, af = 0.0;
    for (int l = 0; l < c.num_hidden_layers; ++l) {      // the CLS probes are not in here: ee_last_layer_plan reports them
        if (r.layer_qkv_stage[l] >= 0) gf += 2.0 * sc[r.layer_qkv_stage[l]].n_rows * 3.0 * H * H;
        if (r.layer_stage[l] >= 0) {
            const StageCounts& s = sc[r.layer_stage[l]];
            gf += 2.0 * s.n_rows * (H * H + 2.0 * H * I);
            af += 4.0 * (double)s.sum_len_sq * H;
        }
    }
    const int E = r.last_stages - 1;
    const double ko = c.strategy == MMEE_STRATEGY_RAMP ? c.num_labels : 2;
    for (int e = 0; e <= E; ++e) {
        const double n = sc[r.exit_stage[e]].n_docs;
        const bool fin = e == E;
        const double dense = (fin || c.exit_head_num_layers == 2) ? 2.0 * H * H : 0.0;
        const bool gate = !fin && c.strategy == MMEE_STRATEGY_GATE;
        if (!gate || r.last_gate_heads) gf += n * (dense + 2.0 * H * (fin ? c.num_labels : ko));
        if (gate) gf += n * (2.0 * H * H + 2.0 * H * c.num_labels);
    }
    if (gemm_flops) *gemm_flops = gf;
    if (attn_flops) *attn_flops = af;
    return 0;
}

int ee_last_layer_plan(ee_handle* h, int32_t* rows_qkv, int32_t* rows_main, int32_t* docs_probe, int32_t cap, double* probe_flops, void* stream) {
    if (!h || !h->rec.last_stages) return fail(h, "ee_last_layer_plan: no forward has run");
    const ForwardRecord& r = h->rec;
    std::vector<StageCounts> sc;
    if (read_stage_counts(h, stream, r.last_stages, sc)) return 1;
    const ee_config& c = h->cfg;
    const double H = c.hidden_size, I = c.intermediate_size;
    double pf = 0.0;
    for (int l = 0; l < c.num_hidden_layers; ++l) {
        const int q = r.layer_qkv_stage[l], m = r.layer_stage[l], p = r.layer_probe_stage[l];
        if (l < cap) {
            if (rows_qkv) rows_qkv[l] = q >= 0 ? sc[q].n_rows : 0;
            if (rows_main) rows_main[l] = m >= 0 ? sc[m].n_rows : 0;
            if (docs_probe) docs_probe[l] = p >= 0 ? sc[p].n_docs : 0;
        }
        // probe: 32 queries x every key of the document (QK^T and PV), then attention-out + FFN on one row per document
        if (p >= 0) {
            if (r.layer_xprobe[l])      // X space: q, u, v projections of one row per document + two passes of heads x H per row
                pf += 6.0 * sc[p].n_docs * H * H + 4.0 * (double)sc[p].n_rows * c.num_attention_heads * H + 2.0 * sc[p].n_docs * (H * H + 2.0 * H * I);
            else pf += 4.0 * 32.0 * sc[p].n_rows * H + 2.0 * sc[p].n_docs * (H * H + 2.0 * H * I);
        }
    }
    if (probe_flops) *probe_flops = pf;
    return 0;
}

int ee_policy_scan(const double* logits, int32_t E1, int32_t N, int32_t K, const double* thresholds, int32_t* exits,
                   double* predictions, double* confidence, int32_t* counts, void* stream) {
    if (!thresholds || E1 < 1 || E1 > 256 || N < 0 || K < 1 || (N > 0 && (!logits || !exits)))
        return fail(nullptr, "ee_policy_scan: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, "ee_policy_scan: no HIP device");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    double* thr_dev = nullptr;
    if (hipMallocAsync((void**)&thr_dev, sizeof(double) * E1, s) != hipSuccess) return fail(nullptr, "ee_policy_scan: hipMallocAsync failed");
    if (hipMemcpyAsync(thr_dev, thresholds, sizeof(double) * E1, hipMemcpyHostToDevice, s) != hipSuccess)
        return fail(nullptr, "ee_policy_scan: threshold copy failed");
    if (counts && hipMemsetAsync(counts, 0, sizeof(int) * E1, s) != hipSuccess) return fail(nullptr, "ee_policy_scan: memset failed");
    if (N > 0) launch_policy_scan(logits, E1, N, K, thr_dev, exits, predictions, confidence, counts, s);
    (void)hipFreeAsync(thr_dev, s);
    return launch_status(nullptr, "ee_policy_scan");
}

int ee_patience_scan(const double* logits, int32_t E1, int32_t N, int32_t K, int32_t patience, int32_t* exits, double* predictions,
                     double* confidence, int32_t* counts, void* stream) {
    if (patience < 1 || E1 < 1 || N < 0 || K < 1 || (N > 0 && (!logits || !exits))) return fail(nullptr, "ee_patience_scan: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, "ee_patience_scan: no HIP device");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (counts && hipMemsetAsync(counts, 0, sizeof(int) * E1, s) != hipSuccess) return fail(nullptr, "ee_patience_scan: memset failed");
    if (N > 0) launch_patience_scan(logits, E1, N, K, patience, exits, predictions, confidence, counts, s);
    return launch_status(nullptr, "ee_patience_scan");
}

int ee_patience_sweep(const double* logits, const int64_t* references, int32_t E1, int32_t N, int32_t K, const int32_t* patiences, int32_t V,
                      double* acc, double* mean_exit, int32_t* exit_hist, void* stream) {
    if (!logits || !references || !patiences || !acc || !mean_exit || E1 < 1 || E1 > 128 || N < 1 || K < 1 || V < 0)
        return fail(nullptr, "ee_patience_sweep: bad argument (E1 <= 128, N >= 1)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, "ee_patience_sweep: no HIP device");
    if (V > 0 && !launch_patience_sweep(logits, reinterpret_cast<const long long*>(references), E1, N, K, patiences, V, acc, mean_exit, exit_hist,
                                        reinterpret_cast<hipStream_t>(stream)))
        return fail(nullptr, "ee_patience_sweep: hipMallocAsync failed");
    return launch_status(nullptr, "ee_patience_sweep");
}

int ee_pack_results(const float* logits, const int32_t* exit_layer, const float* confidence, int32_t n, int32_t K, int32_t* rows, void* stream) {
    if (n < 0 || K < 1 || (n > 0 && (!logits || !exit_layer || !confidence || !rows))) return fail(nullptr, "ee_pack_results: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, "ee_pack_results: no HIP device");
    if (n > 0) launch_pack_results(logits, exit_layer, confidence, n, K, rows, reinterpret_cast<hipStream_t>(stream));
    return launch_status(nullptr, "ee_pack_results");
}

int ee_unpack_results(const int32_t* rows, int32_t n, int32_t K, float* logits, int32_t* exit_layer, float* confidence, void* stream) {
    if (n < 0 || K < 1 || (n > 0 && !rows)) return fail(nullptr, "ee_unpack_results: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, "ee_unpack_results: no HIP device");
    if (n > 0) launch_unpack_results(rows, n, K, logits, exit_layer, confidence, reinterpret_cast<hipStream_t>(stream));
    return launch_status(nullptr, "ee_unpack_results");
}

int ee_threshold_sweep(const double* conf, const uint8_t* correct, int32_t E1, int32_t N, const double* thr, int32_t V, double* acc,
                       double* mean_exit, int32_t* exit_hist, void* stream) {
    if (!conf || !correct || !thr || !acc || !mean_exit || E1 < 1 || E1 > 64 || N < 1 || V < 0)
        return fail(nullptr, "ee_threshold_sweep: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, "ee_threshold_sweep: no HIP device");
    if (V > 0) launch_threshold_sweep(conf, correct, E1, N, thr, V, acc, mean_exit, exit_hist, reinterpret_cast<hipStream_t>(stream));
    return launch_status(nullptr, "ee_threshold_sweep");
}

int ee_msp_table(const double* logits, const int64_t* references, int32_t E1, int32_t N, int32_t K, double* conf, uint8_t* correct,
                 void* stream) {
    if (!logits || !conf || E1 < 1 || N < 1 || K < 1) return fail(nullptr, "ee_msp_table: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, "ee_msp_table: no HIP device");
    launch_msp_table(logits, (const long long*)references, E1, N, K, conf, correct, reinterpret_cast<hipStream_t>(stream));
    return launch_status(nullptr, "ee_msp_table");
}

int ee_temperature_fit(const double* logits, const int64_t* labels, int32_t E1, int32_t N, int32_t K, int32_t max_iter,
                       double* temperature, double* nll, double* accuracy, double* avg_confidence, int32_t* iterations, void* stream) {
    if (!logits || !labels || !temperature || E1 < 1 || N < 1 || K < 2) return fail(nullptr, "ee_temperature_fit: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, "ee_temperature_fit: no HIP device");
    launch_temperature_fit(logits, (const long long*)labels, E1, N, K, max_iter > 0 ? max_iter : 100, temperature, nll, accuracy,
                           avg_confidence, iterations, reinterpret_cast<hipStream_t>(stream));
    return launch_status(nullptr, "ee_temperature_fit");
}

// ---- device-side input feed (N2) ----------------------------------------------------------------------------------------
int ee_preprocess_images(const uint8_t* images, const void* desc, int32_t B, int32_t R, int32_t max_h, void* workspace,
                         size_t workspace_bytes, float* pixel_values, uint8_t* resized_u8, void* stream) {
    constexpr int KMAX = 64;
    if (!images || !desc || !workspace || !pixel_values || B < 1 || R < 1 || max_h < 1) return fail(nullptr, "ee_preprocess_images: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, "ee_preprocess_images: no HIP device");
    // workspace layout: lut[256] f32 | bounds[B*2*R] int2 | kk[B*2*R*KMAX] int | tmp[B*max_h*R*3] u8
    const size_t o_lut = 0, o_b = 1024, o_k = o_b + sizeof(int2) * (size_t)B * 2 * R;
    const size_t o_t = (o_k + sizeof(int) * (size_t)B * 2 * R * KMAX + 255) & ~(size_t)255;
    const size_t need = o_t + (size_t)B * max_h * R * 3;
    if (workspace_bytes < need) return fail(nullptr, "ee_preprocess_images: workspace needs %zu bytes", need);
    char* ws = static_cast<char*>(workspace);
    float lut[256];
    for (int u = 0; u < 256; ++u) {              // HF rescale (float64 product -> float32) then normalize in float32
        const float v = (float)((double)u * (1.0 / 255.0));
        lut[u] = (v - 0.5f) / 0.5f;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemcpyAsync(ws + o_lut, lut, sizeof(lut), hipMemcpyHostToDevice, s) != hipSuccess) return fail(nullptr, "ee_preprocess_images: lut copy failed");
    launch_preprocess_images(images, static_cast<const ImageDesc*>(desc), B, R, KMAX, max_h, reinterpret_cast<int2*>(ws + o_b),
                             reinterpret_cast<int*>(ws + o_k), reinterpret_cast<unsigned char*>(ws + o_t),
                             reinterpret_cast<const float*>(ws + o_lut), pixel_values, resized_u8, s);
    return launch_status(nullptr, "ee_preprocess_images");
}

size_t ee_preprocess_workspace_bytes(int32_t B, int32_t R, int32_t max_h) {
    constexpr int KMAX = 64;
    const size_t o_b = 1024, o_k = o_b + sizeof(int2) * (size_t)B * 2 * R;
    const size_t o_t = (o_k + sizeof(int) * (size_t)B * 2 * R * KMAX + 255) & ~(size_t)255;
    return o_t + (size_t)B * max_h * R * 3;
}

int ee_collate_pad(const int64_t* ids, const int64_t* boxes, const int64_t* offsets, int32_t B, int32_t T, int64_t pad_id,
                   int64_t* out_ids, int64_t* out_mask, int64_t* out_bbox, void* stream) {
    if (!ids || !boxes || !offsets || !out_ids || !out_mask || !out_bbox || B < 1 || T < 1) return fail(nullptr, "ee_collate_pad: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, "ee_collate_pad: no HIP device");
    launch_collate_pad((const long long*)ids, (const long long*)boxes, (const long long*)offsets, B, T, pad_id,
                       (long long*)out_ids, (long long*)out_mask, (long long*)out_bbox, reinterpret_cast<hipStream_t>(stream));
    return launch_status(nullptr, "ee_collate_pad");
}

// ---- debug / micro-benchmark hooks: run ONE kernel of the path on caller-provided device buffers ------------------------
int ee_debug_gemm(const float* A, const float* W, const float* bias, const float* resid, float* Cout, int32_t M, int32_t N,
                  int32_t K, int32_t epi, int32_t wgs_per_cu, const int32_t* row_src, uint64_t* clk_probe, void* stream) {
    if (!A || !W || !Cout || M < 1 || N % 128 || K % 32 || epi < 0 || (epi & 15) > 3) return fail(nullptr, "ee_debug_gemm: bad argument");
    hipDeviceProp_t prop;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return fail(nullptr, "ee_debug_gemm: no device");
    GemmArgs g{};
    g.A = A; g.lda = K; g.W = W; g.bias = bias; g.C = Cout; g.ldc = N; g.resid = resid; g.ldr = N; g.m_static = M; g.N = N; g.K = K;
    g.scale = 1.f;
    g.clk_probe = (unsigned long long*)clk_probe;
    static int* dbg_head = nullptr;
    if (!dbg_head && hipMalloc((void**)&dbg_head, 512) != hipSuccess) return fail(nullptr, "ee_debug_gemm: hipMalloc failed");
    if (hipMemsetAsync(dbg_head, 0, 512, reinterpret_cast<hipStream_t>(stream)) != hipSuccess) return fail(nullptr, "ee_debug_gemm: memset failed");
#ifndef MMEE_DIAG
    if (epi & (32 | 512 | 1024)) return fail(nullptr, "ee_debug_gemm: timing variants (wrong results) exist in the diagnostic library only (make diag)");
#endif
    g.tile_counter = (epi & 16) ? nullptr : dbg_head;    // epi | 16 = static grid stride (A/B switch)
    g.dbg_noload = ((epi & 32) ? 1 : 0) | ((epi & 512) ? 2 : 0) | ((epi & 1024) ? 4 : 0) | (((epi >> 12) & 255) << 8);   // epi bits 12..19: stagger (x 8128 cycles) for odd wave slots   // epi | 512 = no k-loop barrier (DMA variant; timing diagnostic, wrong results)
    g.prio_mode = (epi >> 6) & 3;                         // epi | 64 / 128: static priority variants
    g.use_dma = ((epi >> 8) & 1) ? 1 : 2;                 // epi | 256: LDS-DMA staging kernel, else the register-staged one                    // epi | 32 = no in-loop global loads (timing diagnostic)
    epi &= 15;
    g.row_src = row_src;
    g.resid_row_src = row_src;
    if (epi == EPI_RESID && !resid) return fail(nullptr, "ee_debug_gemm: residual epilogue without a residual");
    if (wgs_per_cu < 0) {   // diagnostic: stamped build, |wgs_per_cu| workgroups per CU, 8 uint64 per workgroup in clk_probe
        launch_gemm_f32_stamped(g, epi, -wgs_per_cu * prop.multiProcessorCount, reinterpret_cast<hipStream_t>(stream));
    } else {
        set_gemm_wgs_per_cu(wgs_per_cu);
        launch_gemm_f32(g, epi, AMODE_ROWS, M, prop.multiProcessorCount, reinterpret_cast<hipStream_t>(stream));
        set_gemm_wgs_per_cu(0);
    }
    return launch_status(nullptr, "ee_debug_gemm");
}

int ee_debug_attn_stamps(uint64_t* out8) {
    unsigned long long* d = mmee::attention_idx_stamps() ? mmee::attention_idx_stamps() : mmee::attention_pair_stamps();
    if (!out8 || !d) return fail(nullptr, "ee_debug_attn_stamps: no stamped launch has run (set MMEE_ATTN_STAMPS=1 before the first forward)");
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out8, d, 64, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(nullptr, "ee_debug_attn_stamps: copy failed");
    (void)hipMemset(d, 0, 64);
    return 0;
}

int ee_debug_gemm_split(const float* A, const float* W, const float* bias, const float* resid, float* Cout, int32_t M, int32_t N,
                        int32_t K, int32_t epi, int32_t out_split, float a_scale, float w_scale, float out_scale,
                        const int32_t* row_src, int32_t rows_A, int32_t iters, float* ms_out, void* stream) {
    const int dbg = epi >> 4;            // diagnostic bits (timing only): 16 no in-loop DMA, 32 no barrier, 64 no DMA wait, 128 no epilogue
    epi &= 15;
#ifndef MMEE_DIAG
    if (dbg) return fail(nullptr, "ee_debug_gemm_split: timing variants (wrong results) exist in the diagnostic library only (make diag)");
#endif
    if (!A || !W || !Cout || M < 1 || rows_A < 1 || !mmee::gemm_split_supports(N, K) || epi < 0 || epi > 3 || iters < 1)
        return fail(nullptr, "ee_debug_gemm_split: bad argument (N %% 256, K %% 32)");
    if (epi == EPI_RESID && !resid) return fail(nullptr, "ee_debug_gemm_split: residual epilogue without a residual");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipDeviceProp_t prop;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return fail(nullptr, "ee_debug_gemm_split: no device");
    float *As = nullptr, *Ws = nullptr;
    int* heads = nullptr;
    if (hipMalloc((void**)&As, (size_t)rows_A * K * 4) != hipSuccess || hipMalloc((void**)&Ws, (size_t)N * K * 4) != hipSuccess ||
        hipMalloc((void**)&heads, 512) != hipSuccess) {
        (void)hipFree(As); (void)hipFree(Ws); (void)hipFree(heads);
        return fail(nullptr, "ee_debug_gemm_split: hipMalloc failed");
    }
    mmee::launch_split_rows(A, As, nullptr, rows_A, rows_A, K, a_scale, prop.multiProcessorCount, s);
    mmee::launch_split_rows(W, Ws, nullptr, N, N, K, w_scale, prop.multiProcessorCount, s);
    GemmArgs g{};
    g.A = As; g.lda = K; g.W = Ws; g.bias = bias; g.C = Cout; g.ldc = N; g.resid = resid; g.ldr = N; g.m_static = M; g.N = N; g.K = K;
    g.scale = 1.f; g.alpha = 1.0f / (a_scale * w_scale); g.out_split = out_split ? 1 : 0; g.out_scale = out_scale;
    g.row_src = row_src; g.resid_row_src = row_src; g.tile_counter = heads; g.dbg_noload = dbg;
    // diagnostic builds (any dbg bit; bit 256 = "diagnostic build, nothing removed") report the shader clock they ran at:
    // ms_out[1] = GHz averaged over the workgroups of the last launch
    unsigned long long* clk = nullptr;
    const int n_clk = 2 * 2 * prop.multiProcessorCount;
    if (dbg && ms_out) {
        if (hipMalloc((void**)&clk, n_clk * 8) == hipSuccess) (void)hipMemsetAsync(clk, 0, n_clk * 8, s);
        g.clk_probe = clk;
    }
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipMemsetAsync(heads, 0, 512, s);
    launch_gemm_split(g, epi, M, prop.multiProcessorCount, s);          // first launch untimed (code object load)
    (void)hipEventRecord(e0, s);
    for (int i = 1; i < iters; ++i) {
        (void)hipMemsetAsync(heads, 0, 512, s);
        launch_gemm_split(g, epi, M, prop.multiProcessorCount, s);
    }
    (void)hipEventRecord(e1, s);
    const hipError_t err = hipStreamSynchronize(s);
    float ms = 0.f;
    if (iters > 1) (void)hipEventElapsedTime(&ms, e0, e1);
    if (ms_out) *ms_out = iters > 1 ? ms / (float)(iters - 1) : 0.f;
    if (clk) {
        std::vector<unsigned long long> hc(n_clk);
        (void)hipMemcpy(hc.data(), clk, n_clk * 8, hipMemcpyDeviceToHost);
        double sum = 0;
        int n = 0;
        for (int i = 0; i + 1 < n_clk; i += 2)
            if (hc[i + 1]) { sum += (double)hc[i] / (double)hc[i + 1] * 0.1; ++n; }
        ms_out[1] = n ? (float)(sum / n) : 0.f;
        (void)hipFree(clk);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(As); (void)hipFree(Ws); (void)hipFree(heads);
    if (err != hipSuccess || hipGetLastError() != hipSuccess) return fail(nullptr, "ee_debug_gemm_split: launch failed: %s", hipGetErrorString(err));
    return 0;
}

}  // extern "C"
