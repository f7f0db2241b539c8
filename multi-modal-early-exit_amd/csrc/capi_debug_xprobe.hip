// ee_debug_xprobe: the X-space CLS probe of xprobe.hip alone, on caller-provided device buffers; no handle.  The entry point makes the
// calls layer_probe() of capi_forward.hip makes for an X-space layer (launch_xprobe) and what feeds it: the row metadata and pair index of
// the stage-0 batch as ee_forward builds them (launch_pair_index; launch_pair_index16 in the diagnostic library, where the forward can pick
// it) and the split-f16 rows of the value weight as ee_finalize builds them (split_weight_rows).  No kernel is defined here; what
// xprobe_supports() refuses is refused, not launched, and so is every row, document or offset outside the caller's buffers.  It
// synchronises and hands the kernels' error word to a host int32.  tests/test_gpu_xprobe.py drives it against tests/xprobe_ref.py.
#include "capi_debug.h"

using namespace mmee;
using namespace mmee::capi;

extern "C" {

int ee_debug_xprobe(const ee_debug_xprobe_args* a, int32_t* err_flag_out, void* stream) {
    const char* who = "ee_debug_xprobe";
    if (!a || !err_flag_out) return fail(nullptr, "%s: args and err_flag_out must not be NULL", who);
    if (!a->orig_doc_off || !a->pos || !a->x0 || !a->y1 || !a->masked || !a->doc_off || !a->doc_orig || !a->x_phys || !a->xs || !a->qc || !a->wk ||
        !a->bk || !a->bv || !a->wv || !a->w1 || !a->wx || !a->wy || !a->ctx)
        return fail(nullptr, "%s: an input pointer or ctx is NULL (only u_out, s0_out, cvec_out and order_out may be)", who);
    if (a->n_orig < 1 || a->n_docs < 0 || a->max_docs < 1 || a->max_docs < a->n_docs || a->max_docs > (1 << 20) || a->x_rows < 1 || a->ctx_rows < 1)
        return fail(nullptr, "%s: bad counts (n_orig >= 1, 0 <= n_docs <= max_docs, 1 <= max_docs <= 2^20, x_rows >= 1, ctx_rows >= 1)", who);
    if (a->H < 64 || a->H > 4096 || a->heads < 1 || a->heads > 64) return fail(nullptr, "%s: hidden size %d outside [64, 4096] or %d heads outside [1, 64]", who, a->H, a->heads);
    if (a->bins1 < 4 || a->bins1 > 256 || a->bins2 < 4 || a->bins2 > 256 || a->max_rel_pos < 1 || a->max_rel_2d_pos < 1 || a->max_pos < 0 ||
        a->max_pos > 4095 || a->max_coord < 0 || a->max_coord > 65535)
        return fail(nullptr, "%s: the bias needs 4 <= bins <= 256, max_rel_pos, max_rel_2d_pos >= 1, max_pos <= 4095, max_coord <= 65535", who);
    if (a->index_form != 0 && a->index_form != 1) return fail(nullptr, "%s: index_form %d is neither 0 (32-bit pair index) nor 1 (query block 0 of the 16-bit form)", who, a->index_form);
    if (a->cus < 0 || a->cus > 4096) return fail(nullptr, "%s: cus %d outside [0, 4096] (0: the device's count)", who, a->cus);
    if (!have_device(who)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int dev_cus = device_cus(who), cus = a->cus ? a->cus : dev_cus;
    if (!dev_cus) return 1;
    const int H = a->H, heads = a->heads, n_orig = a->n_orig, n_docs = a->n_docs, max_docs = a->max_docs;
    if (hipStreamSynchronize(s) != hipSuccess) return fail(nullptr, "%s: the stream is in error", who);

    // ---- the stage-0 batch and the stage on host copies: every length, row, document and offset inside the caller's buffers ----
    DocTable orig, stage;
    std::vector<int> dorig, xphys;
    if (!orig.read(a->orig_doc_off, n_orig) || !stage.read(a->doc_off, n_docs) || !to_host(dorig, a->doc_orig, (size_t)n_docs) ||
        !to_host(xphys, a->x_phys, (size_t)n_docs))
        return fail(nullptr, "%s: copy of the document tables failed", who);
    const std::vector<int> &ooff = orig.off, &off = stage.off;
    if (ooff[0] != 0 || off[0] != 0) return fail(nullptr, "%s: orig_doc_off[0] = %d, doc_off[0] = %d, both must be 0", who, ooff[0], off[0]);
    for (int d = 0; d < n_orig; ++d)
        if (orig.len(d) < 1 || ooff[d + 1] > (1 << 28)) return fail(nullptr, "%s: original document %d has %d rows (or the batch more than 2^28)", who, d, orig.len(d));
    const int rows = orig.rows, max_len = orig.max_len;
    for (int d = 0; d < n_docs; ++d) {
        const int len = stage.len(d), o = dorig[d];
        if (len < 1) return fail(nullptr, "%s: stage document %d has %d rows", who, d, len);
        if (o < 0 || o >= n_orig) return fail(nullptr, "%s: doc_orig[%d] = %d outside the %d original documents", who, d, o, n_orig);
        if (len != ooff[o + 1] - ooff[o])
            return fail(nullptr, "%s: stage document %d has %d rows, its original %d has %d (the pair index is built from the original)", who, d, len, o, ooff[o + 1] - ooff[o]);
        if (xphys[d] < 0 || (long long)xphys[d] + len > a->x_rows)
            return fail(nullptr, "%s: the rows of stage document %d (%d .. %d) leave the %d rows of xs", who, d, xphys[d], xphys[d] + len, a->x_rows);
        if (off[d] >= a->ctx_rows) return fail(nullptr, "%s: the context row %d of stage document %d leaves the %d rows of ctx", who, off[d], d, a->ctx_rows);
    }
    if (int rc = check_row_ints(who, a->pos, a->x0, a->y1, rows, a->max_pos, a->max_coord)) return rc;

    // ---- the operands, by the path's own code ----
    Scratch sc;
    BiasLuts b(a->max_pos, a->max_coord);
    const int nb = (max_len + 31) / 32;
    XProbeArgs xa{};
    xa.xs = reinterpret_cast<const char*>(a->xs); xa.xs_inv = 1.0f / kSplitScaleX; xa.x_phys = a->x_phys; xa.doc_off = a->doc_off; xa.doc_orig = a->doc_orig;
    xa.qc = a->qc; xa.wk = a->wk; xa.bk = a->bk; xa.bv = a->bv;
    xa.ctx = a->ctx; xa.ctx_scale = kSplitScaleCtx;
    xa.idx_doc_stride = a->index_form ? (size_t)nb * 1024 : (size_t)nb * nb * 1024;
    xa.w1 = a->w1; xa.wx = a->wx; xa.wy = a->wy; xa.bins1 = a->bins1; xa.bins2 = a->bins2; xa.inv_sqrt_d = 1.0f / std::sqrt((float)(H / heads));
    xa.H = H; xa.heads = heads;
    xa.pair_idx = reinterpret_cast<const unsigned*>(a->xs);      // any non-null value: xprobe_supports asks whether there is an index at all
    if (!xprobe_supports(xa, max_len))
        return fail(nullptr, "%s: xprobe_supports refuses %d heads x %d with %d / %d bins at max_len %d (12 x 768 or 16 x 1024, bins <= 255, 160 KB of LDS)", who,
                    heads, H, a->bins1, a->bins2, max_len);
    if (int rc = check_pair_index_staging(who, b, max_len)) return rc;
    if (a->index_form == 1) {
#ifdef MMEE_DIAG
        if (!attention_idx16_fits(a->bins1, a->bins2, b.n1)) return fail(nullptr, "%s: attention_idx16_fits refuses %d / %d bins with %d position deltas", who, a->bins1, a->bins2, b.n1);
#else
        return fail(nullptr, "%s: index_form 1 needs the diagnostic library: the 16-bit pair index is not part of the release library", who);
#endif
    }

    RowMeta* meta = nullptr;
    StageCounts* counts = nullptr;
    int *err_flag = nullptr, *order = nullptr, *ticket = nullptr;
    unsigned* pair_idx = nullptr;
    float *absmax = nullptr, *wv_s = nullptr, *u = nullptr, *s0 = nullptr, *cvec = nullptr;
    const size_t per_doc = (size_t)heads * H;
    if (!sc.get(&meta, (size_t)rows) || !sc.get(&counts, 1) || !sc.get(&err_flag, 1) || !sc.get(&pair_idx, (size_t)n_orig * xa.idx_doc_stride) ||
        !sc.get(&absmax, 1) || !sc.get(&wv_s, (size_t)H * H) || !get_dirty(sc, &u, (size_t)max_docs * per_doc, s) || !get_dirty(sc, &s0, (size_t)max_docs * heads * 2, s) || !get_dirty(sc, &cvec, (size_t)max_docs * per_doc, s) || !get_dirty(sc, &order, (size_t)max_docs, s) || !get_dirty(sc, &ticket, 1, s))
        return fail(nullptr, kScratchFailed, who);
    launch_debug_row_meta(a->pos, a->x0, a->y1, a->masked, rows, a->max_coord, meta, s);
    const StageCounts hc{n_docs, stage.rows, stage.sum_sq};
    if (hipMemcpyAsync(counts, &hc, sizeof(hc), hipMemcpyHostToDevice, s) != hipSuccess) return fail(nullptr, kUploadFailed, who);
    if (int rc = upload_bias_luts(who, b, sc, a->bins1, a->max_rel_pos, a->bins2, a->max_rel_2d_pos, s)) return rc;
    if (a->index_form == 0) {
        launch_pair_index(meta, a->orig_doc_off, n_orig, nb, b.lut1, b.c1, b.n1, b.lut2, b.c2, b.n2, a->bins1, pair_idx, xa.idx_doc_stride, max_len, s);
    } else {
#ifdef MMEE_DIAG
        unsigned *idx16 = nullptr, *keymask = nullptr;
        int* doc_flags = nullptr;
        const size_t stride16 = (size_t)nb * nb * 512;
        if (!sc.get(&idx16, (size_t)n_orig * stride16) || !sc.get(&keymask, (size_t)n_orig * nb) || !sc.get(&doc_flags, (size_t)n_orig)) return fail(nullptr, kScratchFailed, who);
        launch_pair_index16(meta, a->orig_doc_off, n_orig, nb, b.lut1, b.c1, b.n1, b.lut2, b.c2, b.n2, a->bins1, idx16, stride16, pair_idx, keymask, doc_flags, max_len, s);
#endif
    }
    // the value weight as split-f16 rows, with ee_finalize's per-tensor scale
    if (int rc = split_weight_rows(nullptr, who, a->wv, H, H, wv_s, absmax, dev_cus, s, &xa.wv_inv)) return rc;
    xa.wv_s = wv_s;
    xa.pair_idx = pair_idx; xa.counts = counts; xa.err_flag = err_flag;
    xa.u = u; xa.s0 = s0; xa.cvec = cvec; xa.order = order; xa.ticket = ticket;
    launch_xprobe(xa, max_docs, max_len, cus, s);
    if ((a->u_out && n_docs && hipMemcpyAsync(a->u_out, u, sizeof(float) * n_docs * per_doc, hipMemcpyDeviceToDevice, s) != hipSuccess) ||
        (a->s0_out && n_docs && hipMemcpyAsync(a->s0_out, s0, sizeof(float) * n_docs * heads * 2, hipMemcpyDeviceToDevice, s) != hipSuccess) ||
        (a->cvec_out && n_docs && hipMemcpyAsync(a->cvec_out, cvec, sizeof(float) * n_docs * per_doc, hipMemcpyDeviceToDevice, s) != hipSuccess) ||
        (a->order_out && n_docs && hipMemcpyAsync(a->order_out, order, sizeof(int) * n_docs, hipMemcpyDeviceToDevice, s) != hipSuccess))
        return fail(nullptr, "%s: copy of the intermediates failed", who);
    return finish(who, s, err_flag, err_flag_out);
}

}  // extern "C"
