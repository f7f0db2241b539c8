// ee_debug_prep, ee_debug_embed, ee_debug_ln_rows: the row kernels of prep_embed.hip alone, on caller-provided device buffers; no handle.
// Each entry point makes the calls of the path's own launchers that capi_forward.hip makes (launch_prep; launch_embed_text,
// launch_embed_visual, launch_pool_finish; launch_ln_rows), synchronises and hands the kernels' error word to a host int32.  No kernel is
// defined here; what the launchers cannot take is refused, not launched.  tests/test_gpu_rows.py drives them against tests/rows_ref.py.
#include "capi_debug.h"

using namespace mmee;
using namespace mmee::capi;

namespace {

// what launch_prep reads and the sizes it writes by
int check_prep(const char* who, const void* input_ids, const void* bbox, int B, int T, int G, int pad_id, int vocab, int max_2d, int max_pos,
               int type_vocab) {
    if (!input_ids || !bbox) return fail(nullptr, "%s: input_ids and bbox must not be NULL", who);
    if (B < 1 || T < 1 || G < 1 || G > 64 || (long long)B * ((long long)T + G * G + 1) > (1ll << 30))
        return fail(nullptr, "%s: bad shape (B >= 1, T >= 1, 1 <= G <= 64, B (T + G G + 1) <= 2^30), got B %d, T %d, G %d", who, B, T, G);
    if (vocab < 1 || max_2d < 1 || max_pos < 1 || type_vocab < 1 || pad_id < 0 || pad_id >= max_pos)
        return fail(nullptr, "%s: bad range limits (vocab, max_2d, max_pos, type_vocab >= 1, 0 <= pad_id < max_pos)", who);
    return 0;
}

// launch_prep's arguments from the caller's inputs and ranges (checked by check_prep) and the buffers it writes
PrepArgs prep_args(const int64_t* input_ids, const int64_t* attention_mask, const int64_t* bbox, const int64_t* position_ids, const int64_t* token_type_ids,
                   int B, int T, int G, int pad_id, int vocab, int max_2d, int max_pos, int type_vocab, int dense_rows, int* text_dst, int* emb_pos,
                   int* ntext, int* doc_off, int* x_src, int* doc_orig, RowMeta* meta, StageCounts* counts, int* err_flag) {
    PrepArgs pa{};
    pa.input_ids = (const long long*)input_ids; pa.attention_mask = (const long long*)attention_mask; pa.bbox = (const long long*)bbox;
    pa.position_ids = (const long long*)position_ids; pa.token_type_ids = (const long long*)token_type_ids;
    pa.B = B; pa.T = T; pa.G = G; pa.Pv = G * G + 1;
    pa.pad_id = pad_id; pa.vocab = vocab; pa.max_2d = max_2d; pa.max_pos = max_pos; pa.type_vocab = type_vocab;
    pa.dense_rows = dense_rows ? 1 : 0;
    pa.text_dst = text_dst; pa.emb_pos = emb_pos; pa.ntext = ntext; pa.doc_off = doc_off; pa.x_src = x_src; pa.doc_orig = doc_orig;
    pa.meta = meta; pa.counts = counts; pa.err_flag = err_flag;
    return pa;
}

}  // namespace

extern "C" {

int ee_debug_prep(const int64_t* input_ids, const int64_t* attention_mask, const int64_t* bbox, const int64_t* position_ids,
                  const int64_t* token_type_ids, int32_t B, int32_t T, int32_t G, int32_t pad_id, int32_t vocab, int32_t max_2d, int32_t max_pos,
                  int32_t type_vocab, int32_t dense_rows, int32_t* text_dst, int32_t* emb_pos, int32_t* ntext, int32_t* doc_off, int32_t* x_src,
                  int32_t* doc_orig, int32_t* meta, void* counts, int32_t* err_flag_out, void* stream) {
    const char* who = "ee_debug_prep";
    if (int rc = check_prep(who, input_ids, bbox, B, T, G, pad_id, vocab, max_2d, max_pos, type_vocab)) return rc;
    if (!text_dst || !emb_pos || !ntext || !doc_off || !x_src || !doc_orig || !meta || !counts || !err_flag_out)
        return fail(nullptr, "%s: every output pointer must be given", who);
    if (!have_device(who)) return 1;
    static_assert(sizeof(RowMeta) == 16 && sizeof(StageCounts) == 16, "the layouts include/mmee.h documents");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Scratch sc;
    int* err_flag = nullptr;
    if (!sc.get(&err_flag, 1)) return fail(nullptr, kScratchFailed, who);
    const PrepArgs pa = prep_args(input_ids, attention_mask, bbox, position_ids, token_type_ids, B, T, G, pad_id, vocab, max_2d, max_pos, type_vocab, dense_rows,
                                  text_dst, emb_pos, ntext, doc_off, x_src, doc_orig, reinterpret_cast<RowMeta*>(meta),
                                  reinterpret_cast<StageCounts*>(counts), err_flag);
    launch_prep(pa, s);
    return finish(who, s, err_flag, err_flag_out);
}

int ee_debug_embed(const ee_debug_embed_args* a, int32_t* err_flag_out, void* stream) {
    const char* who = "ee_debug_embed";
    if (!a || !err_flag_out) return fail(nullptr, "%s: args and err_flag_out must not be NULL", who);
    if (int rc = check_prep(who, a->input_ids, a->bbox, a->B, a->T, a->G, a->pad_id, a->vocab, a->max_2d, a->max_pos, a->type_vocab)) return rc;
    if (int rc = check_hidden(who, a->H)) return rc;
    const int B = a->B, T = a->T, H = a->H, Pv = a->G * a->G + 1;
    if (a->cs < 1 || a->ss < 1 || 4 * a->cs + 2 * a->ss != H)
        return fail(nullptr, "%s: 4 coordinate_size + 2 shape_size = %d is not the hidden size %d", who, 4 * a->cs + 2 * a->ss, H);
    if (!a->type || !a->pos || !a->xtab || !a->ytab || !a->htab || !a->wtab || !a->text_ln_g || !a->text_ln_b || !a->vis_ln_g || !a->vis_ln_b ||
        !a->ln2_g || !a->ln2_b || !a->cls_token || !a->pos_embed || !a->vis_raw || (!a->word && !a->inputs_embeds))
        return fail(nullptr, "%s: a table, LayerNorm vector or visual input is NULL (word may be NULL with inputs_embeds)", who);
    if ((a->X != nullptr) == (a->Xs != nullptr)) return fail(nullptr, "%s: exactly one of X and Xs receives the rows", who);
    if (a->Xs && H % 256 != 0) return fail(nullptr, "%s: split rows need a hidden size that is a multiple of 256 (got %d)", who, H);
    if (a->Xs && !(a->split_scale > 0.f)) return fail(nullptr, "%s: split_scale must be positive", who);
    if ((a->text_part != nullptr) != (a->pooled_text != nullptr) || (a->vis_part != nullptr) != (a->pooled_vis != nullptr) ||
        (a->cat_part != nullptr) != (a->pooled_cat != nullptr))
        return fail(nullptr, "%s: a partial-sum buffer and its pooled output are given together or not at all", who);
    if (!have_device(who)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);

    Scratch sc;
    const size_t rows = (size_t)B * ((size_t)T + Pv);
    int *text_dst = nullptr, *emb_pos = nullptr, *ntext = nullptr, *doc_off = nullptr, *x_src = nullptr, *doc_orig = nullptr, *err_flag = nullptr;
    RowMeta* meta = nullptr;
    StageCounts* counts = nullptr;
    if (!sc.get(&text_dst, (size_t)B * T) || !sc.get(&emb_pos, (size_t)B * T) || !sc.get(&ntext, B) || !sc.get(&doc_off, (size_t)B + 1) ||
        !sc.get(&x_src, B) || !sc.get(&doc_orig, B) || !sc.get(&meta, rows) || !sc.get(&counts, 1) || !sc.get(&err_flag, 1))
        return fail(nullptr, kScratchFailed, who);
    const PrepArgs pa = prep_args(a->input_ids, a->attention_mask, a->bbox, a->position_ids, a->token_type_ids, B, T, a->G, a->pad_id, a->vocab, a->max_2d,
                                  a->max_pos, a->type_vocab, a->dense_rows, text_dst, emb_pos, ntext, doc_off, x_src, doc_orig, meta, counts, err_flag);
    launch_prep(pa, s);

    const int tch = (T + 31) / 32, vch = (Pv + 31) / 32;
    EmbedArgs ea{};
    ea.input_ids = pa.input_ids; ea.token_type_ids = pa.token_type_ids; ea.bbox = pa.bbox;
    ea.emb_pos = emb_pos; ea.text_dst = text_dst; ea.ntext = ntext; ea.doc_off = doc_off;
    ea.B = B; ea.T = T; ea.Pv = Pv; ea.H = H; ea.cs = a->cs; ea.ss = a->ss; ea.max_2d = a->max_2d; ea.vocab = a->vocab; ea.type_vocab = a->type_vocab;
    ea.inputs_embeds = a->inputs_embeds;
    ea.word = a->word; ea.type = a->type; ea.pos = a->pos; ea.xtab = a->xtab; ea.ytab = a->ytab; ea.htab = a->htab; ea.wtab = a->wtab;
    ea.ln1_g = a->text_ln_g; ea.ln1_b = a->text_ln_b; ea.eps1 = a->text_eps;
    ea.ln2_g = a->ln2_g; ea.ln2_b = a->ln2_b; ea.eps2 = a->eps2;
    ea.X = a->X;
    if (a->Xs) { ea.Xs = a->Xs; ea.split_scale = a->split_scale; }
    ea.err_flag = err_flag;
    ea.text_part = a->text_part; ea.cat_part = a->cat_part; ea.cat_chunks = tch + vch;
    launch_embed_text(ea, s);

    EmbedArgs va = ea;
    va.ln1_g = a->vis_ln_g; va.ln1_b = a->vis_ln_b; va.eps1 = a->vis_eps;
    va.cls_token = a->cls_token; va.pos_embed = a->pos_embed; va.vis_raw = a->vis_raw;
    va.vis_part = a->vis_part;
    launch_embed_visual(va, s);
    if (a->vis_part) launch_pool_finish(a->vis_part, vch, H, (float)Pv, a->pooled_vis, B, s);
    if (a->text_part) launch_pool_finish(a->text_part, tch, H, (float)T, a->pooled_text, B, s);
    if (a->cat_part) launch_pool_finish(a->cat_part, tch + vch, H, (float)(T + Pv), a->pooled_cat, B, s);
    return finish(who, s, err_flag, err_flag_out);
}

int ee_debug_ln_rows(const float* src, float* dst, const int32_t* row_src, const int32_t* n_rows, int32_t max_rows, int32_t H, const float* gamma,
                     const float* beta, float eps, void* dst_split, float split_scale, int32_t pre_parts, size_t pre_stride,
                     const float* pre_bias, const void* pre_resid, const int32_t* pre_resid_rows, float pre_resid_inv, int32_t* err_flag_out,
                     void* stream) {
    const char* who = "ee_debug_ln_rows";
    if (!src || !n_rows || !gamma || !beta || !err_flag_out || max_rows < 0) return fail(nullptr, "%s: src, n_rows, gamma, beta, err_flag_out must not be NULL, max_rows >= 0", who);
    if (int rc = check_hidden(who, H)) return rc;
    if (!dst && !dst_split) return fail(nullptr, "%s: neither dst nor dst_split is given", who);
    if (dst_split && H % 256 != 0) return fail(nullptr, "%s: split rows need a hidden size that is a multiple of 256 (got %d)", who, H);
    if (dst_split && !(split_scale > 0.f)) return fail(nullptr, "%s: split_scale must be positive", who);
    if (pre_parts < 0 || pre_parts > 8) return fail(nullptr, "%s: pre_parts %d outside [0, 8]", who, pre_parts);
    if (pre_parts == 0 && (pre_bias || pre_resid || pre_resid_rows)) return fail(nullptr, "%s: a bias or residual needs pre_parts >= 1", who);
    if (pre_resid_rows && !pre_resid) return fail(nullptr, "%s: pre_resid_rows without pre_resid", who);
    if (!have_device(who)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipStreamSynchronize(s) != hipSuccess) return fail(nullptr, "%s: the stream is in error", who);
    int n = 0;
    if (hipMemcpy(&n, n_rows, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail(nullptr, "%s: copy of n_rows failed", who);
    if (n < 0 || n > max_rows) return fail(nullptr, "%s: n_rows = %d outside [0, max_rows = %d] (the buffers are sized by max_rows)", who, n, max_rows);
    const int cus = device_cus(who);
    if (!cus) return 1;
    Scratch sc;
    int* err_flag = nullptr;
    if (!sc.get(&err_flag, 1)) return fail(nullptr, kScratchFailed, who);
    launch_ln_rows(src, dst, row_src, n_rows, max_rows, H, gamma, beta, eps, cus, s, dst_split, split_scale, err_flag, pre_parts, pre_stride, pre_bias,
                   pre_resid, pre_resid_rows, pre_resid_inv);
    return finish(who, s, err_flag, err_flag_out);
}

}  // extern "C"
