// ee_debug_xprobe: the X-space CLS probe of xprobe.hip alone, on caller-provided device buffers; no handle.  The entry point makes the
// calls layer_probe() of capi_forward.hip makes for an X-space layer (launch_xprobe) and what feeds it: the row metadata and pair index of
// the stage-0 batch as ee_forward builds them (launch_pair_index; launch_pair_index16 in the diagnostic library, where the forward can pick
// it) and the split-f16 rows of the value weight as ee_finalize builds them (the scale rule of build_split).  No kernel is defined here; what
// xprobe_supports() refuses is refused, not launched, and so is every row, document or offset outside the caller's buffers.  It
// synchronises and hands the kernels' error word to a host int32.  tests/test_gpu_xprobe.py drives it against tests/xprobe_ref.py.
#include <vector>

#include "capi_internal.h"

using namespace mmee;
using namespace mmee::capi;

namespace {

template <typename T>
bool to_host(std::vector<T>& dst, const T* dev, size_t n) {
    dst.resize(n);
    return n == 0 || hipMemcpy(dst.data(), dev, sizeof(T) * n, hipMemcpyDeviceToHost) == hipSuccess;
}

// scratch that the forward takes from a workspace nobody zeroes between launches: a non-zero byte pattern (negative as an int, a NaN as a float)
template <typename T>
bool get_dirty(Scratch& sc, T** out, size_t count, hipStream_t s) {
    return sc.get(out, count) && hipMemsetAsync(*out, 0xA5, count * sizeof(T), s) == hipSuccess;
}

}  // namespace

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
    hipDeviceProp_t prop;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return fail(nullptr, "%s: no device", who);
    const int dev_cus = prop.multiProcessorCount, cus = a->cus ? a->cus : dev_cus;
    const int H = a->H, heads = a->heads, n_orig = a->n_orig, n_docs = a->n_docs, max_docs = a->max_docs;
    if (hipStreamSynchronize(s) != hipSuccess) return fail(nullptr, "%s: the stream is in error", who);

    // ---- the stage-0 batch and the stage on host copies: every length, row, document and offset inside the caller's buffers ----
    std::vector<int> ooff, off, dorig, xphys;
    if (!to_host(ooff, a->orig_doc_off, (size_t)n_orig + 1) || !to_host(off, a->doc_off, (size_t)n_docs + 1) || !to_host(dorig, a->doc_orig, (size_t)n_docs) ||
        !to_host(xphys, a->x_phys, (size_t)n_docs))
        return fail(nullptr, "%s: copy of the document tables failed", who);
    if (ooff[0] != 0 || off[0] != 0) return fail(nullptr, "%s: orig_doc_off[0] = %d, doc_off[0] = %d, both must be 0", who, ooff[0], off[0]);
    int max_len = 0;
    for (int d = 0; d < n_orig; ++d) {
        const int len = ooff[d + 1] - ooff[d];
        if (len < 1 || ooff[d + 1] > (1 << 28)) return fail(nullptr, "%s: original document %d has %d rows (or the batch more than 2^28)", who, d, len);
        max_len = len > max_len ? len : max_len;
    }
    const int rows = ooff[n_orig];
    for (int d = 0; d < n_docs; ++d) {
        const int len = off[d + 1] - off[d], o = dorig[d];
        if (len < 1) return fail(nullptr, "%s: stage document %d has %d rows", who, d, len);
        if (o < 0 || o >= n_orig) return fail(nullptr, "%s: doc_orig[%d] = %d outside the %d original documents", who, d, o, n_orig);
        if (len != ooff[o + 1] - ooff[o])
            return fail(nullptr, "%s: stage document %d has %d rows, its original %d has %d (the pair index is built from the original)", who, d, len, o, ooff[o + 1] - ooff[o]);
        if (xphys[d] < 0 || (long long)xphys[d] + len > a->x_rows)
            return fail(nullptr, "%s: the rows of stage document %d (%d .. %d) leave the %d rows of xs", who, d, xphys[d], xphys[d] + len, a->x_rows);
        if (off[d] >= a->ctx_rows) return fail(nullptr, "%s: the context row %d of stage document %d leaves the %d rows of ctx", who, off[d], d, a->ctx_rows);
    }
    {
        std::vector<int> hp, hx, hy;
        if (!to_host(hp, a->pos, (size_t)rows) || !to_host(hx, a->x0, (size_t)rows) || !to_host(hy, a->y1, (size_t)rows))
            return fail(nullptr, "%s: copy of the row integers failed", who);
        for (int i = 0; i < rows; ++i) {
            if (hp[i] < 0 || hp[i] > a->max_pos) return fail(nullptr, "%s: pos[%d] = %d outside [0, max_pos = %d]", who, i, hp[i], a->max_pos);
            if (hx[i] < 0 || hx[i] > a->max_coord || hy[i] < 0 || hy[i] > a->max_coord)
                return fail(nullptr, "%s: x0 / y1 of row %d = %d / %d outside [0, max_coord = %d]", who, i, hx[i], hy[i], a->max_coord);
        }
    }

    // ---- the operands, by the path's own code ----
    Scratch sc;
    const char* oom = "%s: hipMalloc of the scratch failed";
    const int c1 = a->max_pos, n1 = 2 * a->max_pos + 1, c2 = a->max_coord, n2 = 2 * a->max_coord + 1;
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
    if ((size_t)max_len * sizeof(RowMeta) + (size_t)n1 + n2 + 32 > 64 * 1024)
        return fail(nullptr, "%s: the pair-index kernel stages max_len rows and both LUTs in 64 KB of LDS (max_len %d, max_pos %d, max_coord %d)", who, max_len,
                    a->max_pos, a->max_coord);
    if (a->index_form == 1) {
#ifdef MMEE_DIAG
        if (!attention_idx16_fits(a->bins1, a->bins2, n1)) return fail(nullptr, "%s: attention_idx16_fits refuses %d / %d bins with %d position deltas", who, a->bins1, a->bins2, n1);
#else
        return fail(nullptr, "%s: index_form 1 needs the diagnostic library: the 16-bit pair index is not part of the release library", who);
#endif
    }

    RowMeta* meta = nullptr;
    StageCounts* counts = nullptr;
    int *err_flag = nullptr, *order = nullptr, *ticket = nullptr;
    unsigned* pair_idx = nullptr;
    unsigned char *lut1 = nullptr, *lut2 = nullptr;
    float *absmax = nullptr, *wv_s = nullptr, *u = nullptr, *s0 = nullptr, *cvec = nullptr;
    const size_t per_doc = (size_t)heads * H;
    if (!sc.get(&meta, (size_t)rows) || !sc.get(&counts, 1) || !sc.get(&err_flag, 1) || !sc.get(&pair_idx, (size_t)n_orig * xa.idx_doc_stride) ||
        !sc.get(&lut1, (size_t)n1 + 4) || !sc.get(&lut2, (size_t)n2 + 4) || !sc.get(&absmax, 1) || !sc.get(&wv_s, (size_t)H * H) ||
        !get_dirty(sc, &u, (size_t)max_docs * per_doc, s) || !get_dirty(sc, &s0, (size_t)max_docs * heads * 2, s) ||
        !get_dirty(sc, &cvec, (size_t)max_docs * per_doc, s) || !get_dirty(sc, &order, (size_t)max_docs, s) || !get_dirty(sc, &ticket, 1, s))
        return fail(nullptr, oom, who);
    launch_debug_row_meta(a->pos, a->x0, a->y1, a->masked, rows, a->max_coord, meta, s);
    unsigned long long sum_sq = 0;
    for (int d = 0; d < n_docs; ++d) sum_sq += (unsigned long long)(off[d + 1] - off[d]) * (off[d + 1] - off[d]);
    const StageCounts hc{n_docs, off[n_docs], sum_sq};
    std::vector<unsigned char> l1(n1), l2(n2);      // outlive the asynchronous copies below: the stream is synchronised before the return
    bucket_lut_host(a->bins1, a->max_rel_pos, c1, l1.data());
    bucket_lut_host(a->bins2, a->max_rel_2d_pos, c2, l2.data());
    if (hipMemcpyAsync(counts, &hc, sizeof(hc), hipMemcpyHostToDevice, s) != hipSuccess || hipMemcpyAsync(lut1, l1.data(), n1, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(lut2, l2.data(), n2, hipMemcpyHostToDevice, s) != hipSuccess)
        return fail(nullptr, "%s: host-to-device copy failed", who);
    if (a->index_form == 0) {
        launch_pair_index(meta, a->orig_doc_off, n_orig, nb, lut1, c1, n1, lut2, c2, n2, a->bins1, pair_idx, xa.idx_doc_stride, max_len, s);
    } else {
#ifdef MMEE_DIAG
        unsigned *idx16 = nullptr, *keymask = nullptr;
        int* doc_flags = nullptr;
        const size_t stride16 = (size_t)nb * nb * 512;
        if (!sc.get(&idx16, (size_t)n_orig * stride16) || !sc.get(&keymask, (size_t)n_orig * nb) || !sc.get(&doc_flags, (size_t)n_orig)) return fail(nullptr, oom, who);
        launch_pair_index16(meta, a->orig_doc_off, n_orig, nb, lut1, c1, n1, lut2, c2, n2, a->bins1, idx16, stride16, pair_idx, keymask, doc_flags, max_len, s);
#endif
    }
    // the value weight as split-f16 rows, with ee_finalize's per-tensor scale
    launch_absmax(a->wv, (size_t)H * H, absmax, s);
    float mx = 0.f;
    if (hipMemcpyAsync(&mx, absmax, sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return fail(nullptr, "%s: the maximum of wv could not be read", who);
    if (!(mx < 3.0e38f)) return fail(nullptr, "%s: wv holds inf/nan", who);
    const int e = split_weight_exponent(mx);
    launch_split_rows(a->wv, wv_s, nullptr, H, H, H, std::ldexp(1.0f, e), dev_cus, s);
    xa.wv_s = wv_s; xa.wv_inv = std::ldexp(1.0f, -e);
    xa.pair_idx = pair_idx; xa.counts = counts; xa.err_flag = err_flag;
    xa.u = u; xa.s0 = s0; xa.cvec = cvec; xa.order = order; xa.ticket = ticket;
    launch_xprobe(xa, max_docs, max_len, cus, s);
    if ((a->u_out && n_docs && hipMemcpyAsync(a->u_out, u, sizeof(float) * n_docs * per_doc, hipMemcpyDeviceToDevice, s) != hipSuccess) ||
        (a->s0_out && n_docs && hipMemcpyAsync(a->s0_out, s0, sizeof(float) * n_docs * heads * 2, hipMemcpyDeviceToDevice, s) != hipSuccess) ||
        (a->cvec_out && n_docs && hipMemcpyAsync(a->cvec_out, cvec, sizeof(float) * n_docs * per_doc, hipMemcpyDeviceToDevice, s) != hipSuccess) ||
        (a->order_out && n_docs && hipMemcpyAsync(a->order_out, order, sizeof(int) * n_docs, hipMemcpyDeviceToDevice, s) != hipSuccess))
        return fail(nullptr, "%s: copy of the intermediates failed", who);
    const hipError_t err = hipStreamSynchronize(s);
    if (err != hipSuccess) return fail(nullptr, "%s: launch failed: %s", who, hipGetErrorString(err));
    if (hipMemcpy(err_flag_out, err_flag, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail(nullptr, "%s: copy of err_flag failed", who);
    return launch_status(nullptr, who);
}

}  // extern "C"
