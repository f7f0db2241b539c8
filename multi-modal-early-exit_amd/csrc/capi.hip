// C-ABI of libmmee_hip.so (include/mmee.h), the handle and the loader: the error helpers every entry point returns through, the parameter
// registry and workspace (ee_create), ee_load_tensor, ee_finalize, ee_destroy.  The other parts of the C-ABI: capi_internal.h.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "capi_internal.h"

using namespace mmee;
using namespace mmee::capi;

namespace {

std::string g_create_error;

}  // namespace

namespace mmee {
namespace capi {

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

int launch_status(ee_handle* h, const char* who) {
    char lds_msg[192];
    if (mmee::take_lds_error(lds_msg, sizeof(lds_msg))) { (void)hipGetLastError(); return fail(h, "%s: %s", who, lds_msg); }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, "%s: launch failed: %s", who, hipGetErrorString(e));
    return 0;
}

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
        return fail(h, "ee_forward: split-precision overflow or a NaN in %s (flags %d): an activation left the range of the split-f16 planes (|LayerNorm out|, "
                       "|Q/sqrt(d)|, |K|, |V|, |GELU out|, |pixel_values| <= 3750, |attention context| <= 937) and was clamped, or an input or activation "
                       "is a NaN, so its results are WRONG; run this checkpoint with precision \"fp32\" (which runs no such check)", whose, err);
    if (err)
        return fail(h, "ee_forward: input out of range in %s (flags %d: 1 = token id, 2 = bbox outside [0, max_2d), 4 = position id, 8 = token_type id); "
                       "its results are invalid", whose, err);
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

// per-tensor power-of-two scale by split_weight_exponent (capi_internal.h)
int split_weight_rows(ee_handle* h, const char* who, const float* w, int N, int K, float* out, float* absmax_dev, int num_cus, hipStream_t s, float* inv) {
    mmee::launch_absmax(w, (size_t)N * K, absmax_dev, s);
    float mx = 0.f;
    if (hipMemcpyAsync(&mx, absmax_dev, sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return fail(h, "%s: the maximum of a weight tensor could not be read", who);
    if (!(mx < 3.0e38f)) return fail(h, "%s: a weight tensor holds inf/nan", who);      // launch_absmax hands back inf / a NaN if one element is
    const int e = split_weight_exponent(mx);
    *inv = std::ldexp(1.0f, -e);
    mmee::launch_split_rows(w, out, nullptr, N, N, K, std::ldexp(1.0f, e), num_cus, s);
    return 0;
}

}  // namespace capi
}  // namespace mmee

namespace {

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

// ee_create, step 1: every rejection of a configuration.  None needs a device: all of them come before the first HIP call.
int check_config(const ee_config& c) {
    if (c.abi_version != MMEE_ABI_VERSION) return fail(nullptr, "ee_create: abi_version %d != %d", c.abi_version, MMEE_ABI_VERSION);
    const int H = c.hidden_size, I = c.intermediate_size, L = c.num_hidden_layers, K = c.num_labels;
    if (H % 128 || I % 128 || H > 1024) return fail(nullptr, "hidden_size/intermediate_size must be multiples of 128, hidden_size <= 1024");
    if (H % c.num_attention_heads || H / c.num_attention_heads != 64) return fail(nullptr, "head dim must be 64");
    const bool beit = c.arch == MMEE_ARCH_BEIT;
    if (c.arch != MMEE_ARCH_LAYOUTLMV3 && !beit) return fail(nullptr, "unknown arch %d", c.arch);
    if (!beit && 4 * c.coordinate_size + 2 * c.shape_size != H) return fail(nullptr, "4*coordinate_size + 2*shape_size != hidden_size");
    if (beit && c.n_embedding_exits) return fail(nullptr, "the BEiT / DiT variant has encoder-layer exits only");
    if (beit && !c.use_mean_pooling) return fail(nullptr, "BEiT / DiT: only use_mean_pooling = 1 is built");
    if (!patch_geometry_ok(c.num_channels, c.input_size, c.patch_size)) return fail(nullptr, "unsupported patch geometry");
    if (K < 1 || K > 64) return fail(nullptr, "num_labels must be in [1,64]");
    if (c.n_embedding_exits < 0 || c.n_embedding_exits > 3 || c.n_encoder_exits < 0 || c.n_encoder_exits > MMEE_MAX_ENCODER_EXITS)
        return fail(nullptr, "bad exit counts");
    for (int i = 0; i < c.n_encoder_exits; ++i) {
        const int l = c.encoder_exit_layers[i];
        if (l < 1 || l > L || (i && l <= c.encoder_exit_layers[i - 1])) return fail(nullptr, "encoder_exit_layers must be ascending in [1,L]");
    }
    if (c.max_docs < 1 || c.max_text_len < (beit ? 0 : 1) || c.max_text_len > 1024) return fail(nullptr, "max_docs >= 1, 1 <= max_text_len <= 1024");
    if (c.precision != MMEE_PREC_F32 && c.precision != MMEE_PREC_F32_SPLIT)
        return fail(nullptr, "precision %d not built (MMEE_PREC_F32 and MMEE_PREC_F32_SPLIT are; bf16 cannot meet the 1e-4 logit tolerance)", c.precision);
    if (c.precision == MMEE_PREC_F32_SPLIT &&
        !(mmee::gemm_split_supports(3 * H, H) && mmee::gemm_split_supports(H, H) && mmee::gemm_split_supports(I, H) && mmee::gemm_split_supports(H, I)))
        return fail(nullptr, "MMEE_PREC_F32_SPLIT needs hidden_size and intermediate_size to be multiples of 256 (got %d, %d)", H, I);
    {   // the split GEMM addresses a gathered A row by a 32-bit byte offset from the tile's first source row
        const double x_bytes = (double)c.max_docs * (double)(c.max_text_len + (c.input_size / c.patch_size) * (c.input_size / c.patch_size) + 1) * H * 4.0;
        if (c.precision == MMEE_PREC_F32_SPLIT && x_bytes >= 4294967296.0)
            return fail(nullptr, "MMEE_PREC_F32_SPLIT: max_docs * rows per document * hidden_size * 4 must stay below 4 GiB (got %.2f GiB); "
                                 "use a smaller max_docs per handle", x_bytes / 1073741824.0);
    }
    if (c.precision == MMEE_PREC_F32_SPLIT && !beit && !(c.rel_pos_bins <= 64 && c.rel_2d_pos_bins <= 64) &&
        !(c.max_rel_pos <= 128 && c.max_rel_2d_pos <= 256))
        return fail(nullptr, "MMEE_PREC_F32_SPLIT: the split-precision attention kernels hold bucket tables of <= 64 bins (attention_idx) or "
                             "distances <= 128 / 256 (attention_pair); got bins %d / %d, distances %d / %d: use MMEE_PREC_F32",
                    c.rel_pos_bins, c.rel_2d_pos_bins, c.max_rel_pos, c.max_rel_2d_pos);
    if (c.precision == MMEE_PREC_F32_SPLIT && (c.num_attention_heads < 1 || c.rel_pos_bins < 2 || c.rel_2d_pos_bins < 2) && !beit)
        return fail(nullptr, "bad relative-position configuration");
    if (c.exit_head_num_layers != 1 && c.exit_head_num_layers != 2) return fail(nullptr, "exit_head_num_layers must be 1 or 2");
    if (c.criterion != MMEE_CRIT_MAX_CONFIDENCE && c.criterion != MMEE_CRIT_ENTROPY && c.criterion != MMEE_CRIT_PATIENCE && c.criterion != MMEE_CRIT_MARGIN &&
        c.criterion != MMEE_CRIT_GATE)
        return fail(nullptr, "ee_create: unknown criterion %d", c.criterion);
    if (c.criterion == MMEE_CRIT_GATE && c.strategy != MMEE_STRATEGY_GATE)
        return fail(nullptr, "ee_create: MMEE_CRIT_GATE needs MMEE_STRATEGY_GATE: a ramp handle has no 2-way gate heads to score");
    if (c.criterion == MMEE_CRIT_GATE && c.use_lte)
        return fail(nullptr, "use_lte: learning-to-exit and MMEE_CRIT_GATE are two exit decisions; a handle takes one of them");
    if (c.use_lte && beit)
        return fail(nullptr, "use_lte: learning-to-exit is built for MMEE_ARCH_LAYOUTLMV3 only (the BEiT / DiT variant has no lte_classifier)");
    if (c.use_lte && c.criterion == MMEE_CRIT_PATIENCE)
        return fail(nullptr, "use_lte: learning-to-exit and MMEE_CRIT_PATIENCE are two exit decisions; a handle takes one of them");
    return 0;
}

// HF names of the ten per-layer parameters both architectures have, below "<model>.encoder.layer.<l>."
struct LayerNames { const char *attn, *ln_attn, *ln_ffn; };
const LayerNames kBeitLayer = {"attention.attention.", "layernorm_before", "layernorm_after"};
const LayerNames kLayoutLMv3Layer = {"attention.self.", "attention.output.LayerNorm", "output.LayerNorm"};

// One encoder layer's parameters, q = "<model>.encoder.layer.<l>.".  The order of the names is ABI (ee_expected_tensor_name).
// key_bias = false (BEiT): the key projection has no bias; its third of qkv_b stays zero and is not registered
int add_layer(ee_handle* h, const std::string& q, const LayerNames& nm, bool key_bias, LayerW& w) {
    const int H = h->cfg.hidden_size, I = h->cfg.intermediate_size;
    int rc = 0;
    rc |= dev_alloc(h, &w.qkv_w, (size_t)3 * H * H);
    rc |= dev_alloc(h, &w.qkv_b, (size_t)3 * H);
    if (rc) return rc;
    if (!key_bias && hipMemset(w.qkv_b, 0, sizeof(float) * 3 * H) != hipSuccess) return fail(h, "hipMemset failed");
    const char* proj[3] = {"query", "key", "value"};
    for (int t = 0; t < 3; ++t) {           // fused [3H][H] weight: Q rows, K rows, V rows
        rc |= add_param(h, q + nm.attn + proj[t] + ".weight", nullptr, {H, H}, w.qkv_w + (size_t)t * H * H);
        if (t != 1 || key_bias) rc |= add_param(h, q + nm.attn + proj[t] + ".bias", nullptr, {H}, w.qkv_b + (size_t)t * H);
    }
    rc |= add_param(h, q + "attention.output.dense.weight", &w.ao_w, {H, H});
    rc |= add_param(h, q + "attention.output.dense.bias", &w.ao_b, {H});
    rc |= add_param(h, q + nm.ln_attn + ".weight", &w.ao_g, {H});
    rc |= add_param(h, q + nm.ln_attn + ".bias", &w.ao_beta, {H});
    rc |= add_param(h, q + "intermediate.dense.weight", &w.f1_w, {I, H});
    rc |= add_param(h, q + "intermediate.dense.bias", &w.f1_b, {I});
    rc |= add_param(h, q + "output.dense.weight", &w.f2_w, {H, I});
    rc |= add_param(h, q + "output.dense.bias", &w.f2_b, {H});
    rc |= add_param(h, q + nm.ln_ffn + ".weight", &w.f_g, {H});
    rc |= add_param(h, q + nm.ln_ffn + ".bias", &w.f_beta, {H});
    return rc;
}

// ee_create, step 2: the parameter registry (HF names), one function per architecture.
// BEiT / DiT (transformers 4.x parameter names, as in the DiT checkpoints the reference's "dit" branch loads,
// EE/configs.py:429-449).  Exit heads are this build's extrapolation: the reference has none.
int register_beit(ee_handle* h) {
    const ee_config& c = h->cfg;
    const int H = c.hidden_size, L = c.num_hidden_layers, K = c.num_labels;
    const int NP = (c.input_size / c.patch_size) * (c.input_size / c.patch_size);
    const bool two = c.exit_head_num_layers == 2;
    const int out_dim = c.strategy == MMEE_STRATEGY_RAMP ? K : 2;     // EE/models/LayoutLMv3.py:83
    int rc = 0;
    const std::string p = "beit.";
    rc |= add_param(h, p + "embeddings.cls_token", &h->cls_token, {1, 1, H});
    if (c.use_abs_pos) rc |= add_param(h, p + "embeddings.position_embeddings", &h->pos_embed, {1, NP + 1, H});
    rc |= add_param(h, p + "embeddings.patch_embeddings.projection.weight", &h->patch_w, {H, c.num_channels, c.patch_size, c.patch_size});
    rc |= add_param(h, p + "embeddings.patch_embeddings.projection.bias", &h->patch_b, {H});
    for (int l = 0; l < L && !rc; ++l) {
        LayerW& w = h->layers[l];
        const std::string q = p + "encoder.layer." + std::to_string(l) + ".";
        rc |= add_layer(h, q, kBeitLayer, false, w);
        if (c.layer_scale && !rc) {
            rc |= add_param(h, q + "lambda_1", &w.lam1, {H});
            rc |= add_param(h, q + "lambda_2", &w.lam2, {H});
        }
    }
    if (c.use_mean_pooling) {
        rc |= add_param(h, p + "pooler.layernorm.weight", &h->ln_g, {H});
        rc |= add_param(h, p + "pooler.layernorm.bias", &h->ln_b, {H});
    } else {
        rc |= add_param(h, p + "layernorm.weight", &h->ln_g, {H});
        rc |= add_param(h, p + "layernorm.bias", &h->ln_b, {H});
    }
    for (int k = 0; k < c.n_encoder_exits && !rc; ++k)
        rc |= add_head(h, p + "encoder.early_exits." + std::to_string(k), &h->enc_heads[k], H, out_dim, two);
    h->classifier.out_dim = K;                                     // BeitForImageClassification.classifier = Linear(H, K)
    rc |= add_param(h, "classifier.weight", &h->classifier.out_w, {K, H});
    rc |= add_param(h, "classifier.bias", &h->classifier.out_b, {K});
    return rc;
}

int register_layoutlmv3(ee_handle* h) {
    const ee_config& c = h->cfg;
    const int H = c.hidden_size, L = c.num_hidden_layers, K = c.num_labels;
    const int NP = (c.input_size / c.patch_size) * (c.input_size / c.patch_size);
    const bool two = c.exit_head_num_layers == 2;
    const int out_dim = c.strategy == MMEE_STRATEGY_RAMP ? K : 2;     // EE/models/LayoutLMv3.py:83
    int rc = 0;
    const std::string p = "layoutlmv3.";
    rc |= add_param(h, p + "embeddings.word_embeddings.weight", &h->word, {c.vocab_size, H});
    rc |= add_param(h, p + "embeddings.token_type_embeddings.weight", &h->type, {c.type_vocab_size, H});
    rc |= add_param(h, p + "embeddings.position_embeddings.weight", &h->pos, {c.max_position_embeddings, H});
    rc |= add_param(h, p + "embeddings.x_position_embeddings.weight", &h->xtab, {c.max_2d_position_embeddings, c.coordinate_size});
    rc |= add_param(h, p + "embeddings.y_position_embeddings.weight", &h->ytab, {c.max_2d_position_embeddings, c.coordinate_size});
    rc |= add_param(h, p + "embeddings.h_position_embeddings.weight", &h->htab, {c.max_2d_position_embeddings, c.shape_size});
    rc |= add_param(h, p + "embeddings.w_position_embeddings.weight", &h->wtab, {c.max_2d_position_embeddings, c.shape_size});
    rc |= add_param(h, p + "embeddings.LayerNorm.weight", &h->emb_g, {H});
    rc |= add_param(h, p + "embeddings.LayerNorm.bias", &h->emb_b, {H});
    rc |= add_param(h, p + "patch_embed.proj.weight", &h->patch_w, {H, c.num_channels, c.patch_size, c.patch_size});
    rc |= add_param(h, p + "patch_embed.proj.bias", &h->patch_b, {H});
    rc |= add_param(h, p + "cls_token", &h->cls_token, {1, 1, H});
    rc |= add_param(h, p + "pos_embed", &h->pos_embed, {1, NP + 1, H});
    rc |= add_param(h, p + "norm.weight", &h->norm_g, {H});
    rc |= add_param(h, p + "norm.bias", &h->norm_b, {H});
    rc |= add_param(h, p + "LayerNorm.weight", &h->ln_g, {H});
    rc |= add_param(h, p + "LayerNorm.bias", &h->ln_b, {H});
    rc |= add_param(h, p + "encoder.rel_pos_bias.weight", &h->rel1, {c.num_attention_heads, c.rel_pos_bins});
    rc |= add_param(h, p + "encoder.rel_pos_x_bias.weight", &h->relx, {c.num_attention_heads, c.rel_2d_pos_bins});
    rc |= add_param(h, p + "encoder.rel_pos_y_bias.weight", &h->rely, {c.num_attention_heads, c.rel_2d_pos_bins});
    for (int l = 0; l < L && !rc; ++l)
        rc |= add_layer(h, p + "encoder.layer." + std::to_string(l) + ".", kLayoutLMv3Layer, true, h->layers[l]);
    const char* emb_nm[3] = {"vision_exit_embeddings", "text_exit_embeddings", "concat_exit_embeddings"};
    for (int i = 0; i < c.n_embedding_exits && !rc; ++i) {
        const int kind = c.embedding_exits[i];
        if (kind < 0 || kind > 2) { rc = fail(nullptr, "bad embedding exit kind"); break; }
        rc |= add_head(h, p + emb_nm[kind], &h->emb_heads[kind], H, out_dim, two);
    }
    for (int k = 0; k < c.n_encoder_exits && !rc; ++k)
        rc |= add_head(h, p + "encoder.early_exits." + std::to_string(k), &h->enc_heads[k], H, out_dim, two);
    rc |= add_head(h, "classifier", &h->classifier, H, K, true);       // HF:799-823, always dense + out_proj
    if (c.use_lte) {                                                   // one gate shared by all exits, EE/models/LayoutLMv3.py:140-142
        rc |= add_param(h, p + "encoder.lte_classifier.weight", &h->lte_w, {1, H});
        rc |= add_param(h, p + "encoder.lte_classifier.bias", &h->lte_b, {1});
    }
    return rc;
}

// ee_create, step 3: the workspace of a forward of max_docs documents
int alloc_workspace(ee_handle* h) {
    const ee_config& c = h->cfg;
    const int H = c.hidden_size, I = c.intermediate_size, L = c.num_hidden_layers;
    const bool beit = c.arch == MMEE_ARCH_BEIT;
    const int NP = (c.input_size / c.patch_size) * (c.input_size / c.patch_size);
    int rc = 0;
    const size_t Bm = c.max_docs, Tm = c.max_text_len, Pv = NP + 1;
    const size_t rows = Bm * (Tm + Pv);
    const int E = c.n_embedding_exits + c.n_encoder_exits;
    const size_t tch = (Tm + 31) / 32, vch = (Pv + 31) / 32;
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
                rc |= dev_alloc(h, &h->xp_u, Bm * (size_t)c.num_attention_heads * H);
                rc |= dev_alloc(h, &h->xp_s0, Bm * (size_t)c.num_attention_heads * 2);
                rc |= dev_alloc(h, &h->xp_order, Bm + 1);
                rc |= dev_alloc(h, &h->xp_c, Bm * (size_t)c.num_attention_heads * H);
                rc |= dev_alloc(h, &h->xp_part, 4 * Bm * H);      // split-K parts of the probe's FFN-down rows
                // MMEE_FLAG_LOW_LATENCY: the parts of a layer's residual GEMM.  ee_low_latency_k_splits keeps (128 x 128 tiles) x S <= 2 * num_cus,
                // so the buffer is that many tiles (33.5 MB at 256 CUs) whatever H and max_docs are
                h->ll_part_floats = (size_t)2 * h->num_cus * 128 * 128;
                rc |= dev_alloc(h, &h->ll_part, h->ll_part_floats);
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
            h->idx16 = idx_env == 16 && mmee::attention_idx16_fits(c.rel_pos_bins, c.rel_2d_pos_bins, 2 * maxpos - 1);
            h->idx_stride = (size_t)h->idx_nb * h->idx_nb * (h->idx16 ? 512 : 1024);
            rc |= dev_alloc(h, &h->pair_idx, Bm * h->idx_stride);
            if (h->idx16) {
                rc |= dev_alloc(h, &h->pair_idx0, Bm * (size_t)h->idx_nb * 1024);
                rc |= dev_alloc(h, &h->keymask, Bm * (size_t)h->idx_nb);
            }
            rc |= dev_alloc(h, &h->doc_flags, Bm);      // attention_pair.hip (and IDX16): "a key inside the document is masked", by original document
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
    const size_t st = (size_t)(E + 3) * (Bm + 1);      // stages 0 .. E of a forward; E + 1, E + 2: scratch of ee_embedding_inputs / ee_forward_vision
    rc |= dev_alloc(h, &h->doc_orig, st);
    rc |= dev_alloc(h, &h->doc_off, st);
    rc |= dev_alloc(h, &h->x_src, st);
    rc |= dev_alloc(h, &h->meta_src, st);
    rc |= dev_alloc(h, &h->counts, (size_t)(E + 3));
    rc |= dev_alloc(h, &h->thr_dev, 256);
    rc |= dev_alloc(h, &h->pat_state, 2 * Bm);
    if (c.use_lte) rc |= dev_alloc(h, &h->lte_score, Bm);
    return rc;
}

// ee_finalize, step 1: every registered parameter has been loaded
int report_missing(ee_handle* h) {
    std::string missing;
    int nmiss = 0;
    for (auto& n : h->names)
        if (!h->params[n].loaded) {
            if (nmiss < 8) missing += n + " ";
            ++nmiss;
        }
    if (nmiss) return fail(h, "ee_finalize: %d parameter(s) not loaded: %s%s", nmiss, missing.c_str(), nmiss > 8 ? "..." : "");
    return 0;
}

// One weight as split-f16 rows; per-tensor power-of-two scale that puts max|w| in [2^12, 2^13) (capped at 2^8: typical |w| ~ 0.02 then
// sits near 5, its lo plane well inside the f16 normal range)
int build_split(ee_handle* h, const float* w, int N, int K, float** out, float* inv) {
    if (!*out && dev_alloc(h, out, (size_t)N * K)) return 1;
    return split_weight_rows(h, "ee_finalize", w, N, K, *out, h->absmax_dev, h->num_cus, nullptr, inv);
}

// ee_finalize, step 2 (MMEE_PREC_F32_SPLIT): split-f16 rows of the four big weights of every layer, of the heads' dense layers and of the
// patch projection
int build_split_weights(ee_handle* h) {
    const ee_config& c = h->cfg;
    const int H = c.hidden_size, I = c.intermediate_size;
    for (auto& w : h->layers) {
        if (build_split(h, w.qkv_w, 3 * H, H, &w.qkv_s, &w.qkv_inv)) return 1;
        if (build_split(h, w.ao_w, H, H, &w.ao_s, &w.ao_inv)) return 1;
        if (build_split(h, w.f1_w, I, H, &w.f1_s, &w.f1_inv)) return 1;
        if (build_split(h, w.f2_w, H, I, &w.f2_s, &w.f2_inv)) return 1;
    }
    // the dense layer of every exit head and of the classifier (EE/models/LayoutLMv3.py:86-93, HF:799-823): H x H, on CLS rows
    if (mmee::gemm_split_supports(H, H) && c.arch != MMEE_ARCH_BEIT) {
        auto head = [&](HeadW& hw) -> int { return hw.dense_w ? build_split(h, hw.dense_w, H, H, &hw.dense_s, &hw.dense_inv) : 0; };
        for (auto& hw : h->enc_heads) if (head(hw)) return 1;
        if (head(h->classifier)) return 1;
    }
    const int Kp = c.num_channels * c.patch_size * c.patch_size;
    const size_t NPp = (size_t)(c.input_size / c.patch_size) * (c.input_size / c.patch_size);
    const bool fits = NPp * Kp <= ((size_t)c.max_text_len + NPp + 1) * I;      // the split patches are staged in H1
    if (mmee::gemm_split_supports(H, Kp) && c.patch_size % 4 == 0 && fits && build_split(h, h->patch_w, H, Kp, &h->patch_s, &h->patch_inv)) return 1;
    HIP_OK(h, hipDeviceSynchronize());
    return 0;
}

// ee_finalize, step 3: the bias tables the attention kernels read
int build_bias_tables(ee_handle* h) {
    const ee_config& c = h->cfg;
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
    return 0;
}

}  // namespace

extern "C" {

const char* ee_last_error(const ee_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int ee_create(const ee_config* c, ee_handle** out) {
    if (!c || !out) return fail(nullptr, "ee_create: null argument");
    if (check_config(*c)) return 1;
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
    h->layers.resize(c->num_hidden_layers);
    h->enc_heads.resize(c->n_encoder_exits);

    int rc = c->arch == MMEE_ARCH_BEIT ? register_beit(h) : register_layoutlmv3(h);
    if (!rc) rc = alloc_workspace(h);
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
    for (auto& ev : h->stream_ev) (void)hipEventDestroy(ev);
    if (h->stream_host) (void)hipHostFree(h->stream_host);
    if (h->dl_word) (void)hipHostFree(h->dl_word);
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
    if (report_missing(h)) return 1;
    if (h->split && build_split_weights(h)) return 1;
    if (build_bias_tables(h)) return 1;
    h->finalized = true;
    return 0;
}

}  // extern "C"
