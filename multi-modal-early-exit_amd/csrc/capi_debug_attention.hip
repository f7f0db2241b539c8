// ee_debug_attention: one of the fused attention kernels (attention_f32.hip, attention_pair.hip, attention_idx.hip) alone, on caller-provided
// ragged documents; no handle.  The operands are built by the path's own code; what the *_supports() predicates refuse is refused, not launched,
// and so is every row outside the caller's buffers.  It synchronises and hands the kernels' error word to a host int32.
// tests/test_gpu_attention.py drives it against tests/attn_ref.py.  The one kernel here is the hooks' own (ee_debug_xprobe launches it too).
#include "capi_debug.h"

using namespace mmee;
using namespace mmee::capi;

namespace {

// ee_debug_attention, ee_debug_xprobe: the rows' metadata from the caller's integers, by the expression of row_meta_kernel (make_row_meta)
__global__ void debug_row_meta_kernel(const int* __restrict__ pos, const int* __restrict__ x0, const int* __restrict__ y1,
                                      const int* __restrict__ masked, int rows, int coord_hi, RowMeta* __restrict__ meta) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < rows) meta[i] = make_row_meta(pos[i], x0[i], y1[i], coord_hi, masked[i] == 0);
}

}  // namespace

void mmee::capi::launch_debug_row_meta(const int* pos, const int* x0, const int* y1, const int* masked, int rows, int coord_hi, RowMeta* meta, hipStream_t s) {
    hipLaunchKernelGGL(debug_row_meta_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, pos, x0, y1, masked, rows, coord_hi, meta);
}

extern "C" {

int ee_debug_attention(const float* qkv, int32_t qkv_rows, const int32_t* doc_off, int32_t n_docs, const int32_t* qkv_doc_off, const int32_t* pos,
                       const int32_t* x0, const int32_t* y1, const int32_t* masked, const float* w1, const float* wx, const float* wy, int32_t heads,
                       int32_t bins1, int32_t bins2, int32_t max_rel_pos, int32_t max_rel_2d_pos, int32_t max_pos, int32_t max_coord, int32_t kernel,
                       int32_t use_queue, int32_t q_limit, int32_t terms, void* ctx, int32_t* err_flag_out, void* stream) {
    const char* who = "ee_debug_attention";
    const bool f32k = kernel == MMEE_ATTN_KERNEL_F32, pairk = kernel == MMEE_ATTN_KERNEL_PAIR, idxk = kernel == MMEE_ATTN_KERNEL_IDX,
               plaink = kernel == MMEE_ATTN_KERNEL_IDX_NOBIAS;
    if (!f32k && !pairk && !idxk && !plaink) return fail(nullptr, "%s: kernel %d is none of MMEE_ATTN_KERNEL_F32, _PAIR, _IDX, _IDX_NOBIAS", who, kernel);
    if (!qkv || !doc_off || !pos || !x0 || !y1 || !masked || !ctx || !err_flag_out || n_docs < 1 || heads < 1 || heads > 64 || qkv_rows < 1 ||
        q_limit < 0 || max_pos < 0 || max_pos > 4095 || max_coord < 0 || max_coord > 65535)
        return fail(nullptr, "%s: bad argument (pointers not NULL, n_docs >= 1, 1 <= heads <= 64, q_limit >= 0, max_pos <= 4095, max_coord <= 65535)", who);
    if (!plaink && (!w1 || !wx || !wy || bins1 < 4 || bins1 > 256 || bins2 < 4 || bins2 > 256 || max_rel_pos < 1 || max_rel_2d_pos < 1))
        return fail(nullptr, "%s: the bias needs w1 / wx / wy, 4 <= bins <= 256 and max_rel_pos, max_rel_2d_pos >= 1", who);
    if (terms != 3 && !(terms == 1 && idxk)) return fail(nullptr, "%s: terms is 3, or 1 for MMEE_ATTN_KERNEL_IDX (the one-term mode is built for that kernel only)", who);
    if (f32k && (q_limit > 0 || qkv_doc_off)) return fail(nullptr, "%s: attention_f32 takes neither q_limit nor qkv_doc_off (probe-first layers are split-precision)", who);
    if (!have_device(who)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int cus = device_cus(who), H = 64 * heads;
    if (!cus) return 1;

    // ---- the documents: offsets, lengths, every row inside the buffers, every integer inside its range (host copies: this is a test hook) ----
    DocTable docs;
    std::vector<int> qoff, hm;
    if (!docs.read(doc_off, n_docs)) return fail(nullptr, "%s: copy of doc_off failed", who);
    if (qkv_doc_off && !to_host(qoff, qkv_doc_off, (size_t)n_docs)) return fail(nullptr, "%s: copy of qkv_doc_off failed", who);
    if (docs.off[0] != 0) return fail(nullptr, "%s: doc_off[0] = %d, must be 0", who, docs.off[0]);
    for (int d = 0; d < n_docs; ++d) {
        const int len = docs.len(d);
        if (len < 1) return fail(nullptr, "%s: document %d has %d rows", who, d, len);
        const int q = qkv_doc_off ? qoff[d] : docs.off[d];
        if (q < 0 || (long)q + len > qkv_rows) return fail(nullptr, "%s: the Q | K | V rows of document %d (%d .. %d) leave the %d rows of qkv", who, d, q, q + len, qkv_rows);
    }
    const int rows = docs.rows, max_len = docs.max_len;
    if (int rc = check_row_ints(who, pos, x0, y1, rows, max_pos, max_coord)) return rc;
    if (!to_host(hm, masked, (size_t)rows)) return fail(nullptr, "%s: copy of the row integers failed", who);
    for (int i = 0; i < rows; ++i)
        if (plaink && hm[i] != 0) return fail(nullptr, "%s: row %d is masked, and the image-only form of attention_idx (no pair index) has no key mask", who, i);

    // ---- the operands, by the path's own code ----
    Scratch sc;
    BiasLuts b(max_pos, max_coord);
    AttnArgs at{};
    at.c1 = b.c1; at.n1 = b.n1; at.c2 = b.c2; at.n2 = b.n2;
    at.H = H; at.heads = heads; at.max_len = max_len; at.ld = 3 * H; at.ldc = H; at.ctx = static_cast<float*>(ctx);
    at.doc_off = doc_off; at.qkv_doc_off = qkv_doc_off; at.q_limit = q_limit; at.terms = terms;
    at.ctx_split = f32k ? 0 : 1; at.ctx_scale = kSplitScaleCtx; at.qkv_scale = kSplitScaleQKV;
    at.w1 = w1; at.wx = wx; at.wy = wy; at.bins1 = bins1; at.bins2 = bins2; at.inv_sqrt_d = 0.125f;      // 1 / sqrt(64)
    RowMeta* meta = nullptr;
    StageCounts* counts = nullptr;
    int *err_flag = nullptr, *heads_q = nullptr, *doc_orig = nullptr, *doc_flags = nullptr;
    if (!sc.get(&meta, rows) || !sc.get(&counts, 1) || !sc.get(&err_flag, 1) || !sc.get(&heads_q, 128) || !sc.get(&doc_orig, n_docs) || !sc.get(&doc_flags, n_docs))
        return fail(nullptr, kScratchFailed, who);
    launch_debug_row_meta(pos, x0, y1, masked, rows, max_coord, meta, s);
    const StageCounts hc{n_docs, rows, docs.sum_sq};
    std::vector<int> iota(n_docs);
    for (int d = 0; d < n_docs; ++d) iota[d] = d;
    if (hipMemcpyAsync(counts, &hc, sizeof(hc), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(doc_orig, iota.data(), sizeof(int) * n_docs, hipMemcpyHostToDevice, s) != hipSuccess)
        return fail(nullptr, kUploadFailed, who);
    launch_doc_flags(meta, doc_off, n_docs, doc_flags, s);
    at.meta = meta; at.counts = counts; at.err_flag = err_flag; at.doc_orig = doc_orig; at.doc_flags = doc_flags;
    at.item_counter = use_queue ? heads_q : nullptr;      // 8 XCD-local counters x 16 ints, zeroed
    if (!plaink) {
        float *t1 = nullptr, *tx = nullptr, *ty = nullptr;
        if (!sc.get(&t1, (size_t)heads * at.n1) || !sc.get(&tx, (size_t)heads * at.n2) || !sc.get(&ty, (size_t)heads * at.n2)) return fail(nullptr, kScratchFailed, who);
        if (int rc = upload_bias_luts(who, b, sc, bins1, max_rel_pos, bins2, max_rel_2d_pos, s)) return rc;
        launch_build_value_tables(w1, wx, wy, b.lut1, b.lut2, heads, bins1, bins2, at.n1, at.n2, at.inv_sqrt_d, t1, tx, ty, s);
        at.t1 = t1; at.tx = tx; at.ty = ty; at.lut1 = b.lut1;
    }
    if (f32k) {
        at.qkv = qkv;
        if (attention_f32_lds_bytes(at) > 160 * 1024) return fail(nullptr, "%s: the value tables of max_pos %d / max_coord %d do not fit attention_f32's LDS", who, max_pos, max_coord);
        launch_attention_f32(at, n_docs, cus, s);
    } else {
        float* qkv_s = nullptr;
        if (!sc.get(&qkv_s, (size_t)qkv_rows * 3 * H)) return fail(nullptr, kScratchFailed, who);
        launch_split_rows(qkv, qkv_s, nullptr, qkv_rows, qkv_rows, 3 * H, kSplitScaleQKV, cus, s, err_flag);
        at.qkv = qkv_s;
        if (idxk) {
            at.idx_nb = (max_len + 31) / 32;
            at.idx_doc_stride = (size_t)at.idx_nb * at.idx_nb * 1024;
            unsigned* pair_idx = nullptr;
            if (!sc.get(&pair_idx, (size_t)n_docs * at.idx_doc_stride)) return fail(nullptr, kScratchFailed, who);
            at.pair_idx = pair_idx;
        }
        if (pairk) {
            if (!attention_pair_supports(at, max_rel_pos, max_rel_2d_pos))
                return fail(nullptr, "%s: attention_pair holds Delta tables of distances <= 128 / 256 (got %d / %d)", who, max_rel_pos, max_rel_2d_pos);
            launch_attention_pair(at, n_docs, cus, max_rel_pos, max_rel_2d_pos, s);
        } else {
            if (!attention_idx_supports(at)) return fail(nullptr, "%s: attention_idx holds bucket tables of <= 64 bins (got %d / %d)", who, bins1, bins2);
            if (idxk) {
                if (int rc = check_pair_index_staging(who, b, max_len)) return rc;
                launch_pair_index(meta, doc_off, n_docs, at.idx_nb, b.lut1, at.c1, at.n1, b.lut2, at.c2, at.n2, bins1, const_cast<unsigned*>(at.pair_idx), at.idx_doc_stride, max_len, s);
            }
            launch_attention_idx(at, n_docs, cus, s);
        }
    }
    return finish(who, s, err_flag, err_flag_out);
}

}  // extern "C"
