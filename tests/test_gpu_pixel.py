"""The pixel path alone, against tests/pixel_ref.py: page bytes through ee_preprocess_images (equality with Pillow's 8-bit BILINEAR and the
rescale / normalise table), ragged tokens through ee_collate_pad (equality with a loop), pixel_values through the patch projection by
ee_debug_patch_project (float64, per row: max|got - ref64| <= max(2 err32, 1e-6), err32 = torch float32 on the GPU on the same operands) at every
geometry class ee_create accepts, and one forward at patch_size 8.  Every output is followed by sentinel words that must survive; every
measured error goes through report_measured (profiles/pixel_path.txt holds a run's lines)."""
import ctypes as C

import numpy as np
import pytest

from . import pixel_ref as X
from .conftest import H256_KW, report_measured
from .hook_util import ERR_SPLIT_OVERFLOW, SENTINEL, _decode_split, _dev, _f32, _ptr, _stream

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4
GUARD_WORDS = 64


def _torch():
    import torch
    return torch


def _guarded_bytes(nbytes):
    """A device buffer of nbytes and GUARD_WORDS sentinel words behind it (uint8 view), every byte of it sentinel."""
    torch = _torch()
    return torch.full(((nbytes + 3) // 4 + GUARD_WORDS,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.uint8)


def _tail_kept(buf, nbytes, what):
    torch = _torch()
    pattern = torch.tensor(list(int(SENTINEL).to_bytes(4, "little")), dtype=torch.uint8, device="cuda")
    assert torch.equal(buf[nbytes:], pattern[torch.arange(nbytes, buf.numel(), device="cuda") % 4]), f"{what}: a write past its {nbytes} bytes"


# ---------------------------------------------------------------------------------------------------------------------------------------
# resize
# ---------------------------------------------------------------------------------------------------------------------------------------
_REF = {}


def _ref(pkg, R, shape):
    """(page, resized_u8, pixel_values) of a case, computed once."""
    if (R, shape) not in _REF:
        page = X.make_page(pkg.synth, R, shape)
        _REF[R, shape] = (page,) + X.resize_ref(page, R)
    return _REF[R, shape]


def _resize(pkg, pages, R, align=16, lead=0):
    """One ee_preprocess_images call on the C entry point: (resized_u8 [B, R, R, 3], pixel_values [B, 3, R, R]) as numpy, after the guards
    behind both outputs and behind the workspace were checked."""
    torch = _torch()
    lib = pkg.capi.load()
    buf, desc = X.pack_pages(pages, align, lead)
    rec = np.zeros(len(pages), dtype=pkg.feed._DESC)
    for i, (off, h, w, c) in enumerate(desc):
        rec[i] = (off, h, w, c, 0)
    B, max_h = len(pages), max(d[1] for d in desc)
    d_img, d_desc = torch.from_numpy(buf).cuda(), torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
    ws_bytes = lib.ee_preprocess_workspace_bytes(B, R, max_h)
    n_px, n_u8 = B * 3 * R * R * 4, B * R * R * 3
    ws, px, u8 = _guarded_bytes(ws_bytes), _guarded_bytes(n_px), _guarded_bytes(n_u8)
    pkg.capi.check(lib.ee_preprocess_images(_ptr(d_img), _ptr(d_desc), B, R, max_h, _ptr(ws), ws_bytes, _ptr(px), _ptr(u8), _stream()), None,
                   "ee_preprocess_images")
    torch.cuda.synchronize()
    for b, n, what in ((ws, ws_bytes, "workspace"), (px, n_px, "pixel_values"), (u8, n_u8, "resized_u8")):
        _tail_kept(b, n, what)
    return u8[:n_u8].cpu().numpy().reshape(B, R, R, 3), px[:n_px].view(torch.float32).cpu().numpy().reshape(B, 3, R, R)


def _same(got_u8, got_px, want_u8, want_px, what):
    assert np.array_equal(got_u8, want_u8), (what, int((got_u8 != want_u8).sum()), "bytes differ")
    assert got_px.dtype == np.float32 and np.array_equal(got_px.view(np.int32), want_px.view(np.int32)), what


@pytest.mark.parametrize("R,shape", X.RESIZE_CASES, ids=[f"R{R}-{'x'.join(map(str, s))}" for R, s in X.RESIZE_CASES])
def test_resize_equals_pillow_at_every_edge(pkg, R, shape):
    page, want_u8, want_px = _ref(pkg, R, shape)
    u8, px = _resize(pkg, [page], R)
    _same(u8[0], px[0], want_u8, want_px, (R, shape))


def test_resize_mixed_call_equals_the_single_pages(pkg):
    """Grey and RGB pages of very different heights in one call, the tallest not first: every page as alone."""
    R, shapes = X.MIXED_CALL
    refs = [_ref(pkg, R, s) for s in shapes]
    u8, px = _resize(pkg, [r[0] for r in refs], R)
    for i, (page, want_u8, want_px) in enumerate(refs):
        _same(u8[i], px[i], want_u8, want_px, ("mixed", shapes[i]))
        alone_u8, alone_px = _resize(pkg, [page], R)
        _same(u8[i], px[i], alone_u8[0], alone_px[0], ("mixed against alone", shapes[i]))


def test_resize_takes_pages_at_any_byte_offset(pkg):
    """include/mmee.h promises "packed back to back": no page but the first starts on a 16-byte boundary here, and the first not either."""
    R, shapes = 224, [(2, 3, 3), (1, 500, 1), (223, 225, 3), (225, 223, 1), (1, 1, 1)]
    refs = [_ref(pkg, R, s) for s in shapes]
    offs = [d[0] for d in X.pack_pages([r[0] for r in refs], 1, 3)[1]]
    assert all(o % 16 for o in offs) and len({o % 4 for o in offs}) > 1
    u8, px = _resize(pkg, [r[0] for r in refs], R, align=1, lead=3)
    for i, (_, want_u8, want_px) in enumerate(refs):
        _same(u8[i], px[i], want_u8, want_px, ("unaligned", shapes[i]))


def test_the_feed_refuses_a_side_above_31_r(pkg):
    R = 32
    for shape in ((X.MAX_RATIO * R + 1, 8, 3), (8, X.MAX_RATIO * R + 1, 1)):
        with pytest.raises(ValueError, match="must be <= 31"):
            pkg.feed.preprocess_images([np.zeros(shape[:2] if shape[2] == 1 else shape, np.uint8)], R)
    for shape in ((992, 8, 3), (992, 992, 1)):
        page, want_u8, want_px = _ref(pkg, R, shape)
        px, u8 = pkg.feed.preprocess_images([page], R, return_u8=True)
        _same(u8[0].cpu().numpy(), px[0].cpu().numpy(), want_u8, want_px, ("feed", shape))
    with pytest.raises(pkg.capi.MMEEError, match="max_h 993 is above 31 R = 992"):      # what the C entry point can see of it: the height
        pkg.feed._preprocess_on_device(_dev(np.zeros(993 * 8, np.uint8)), _dev(np.zeros(24, np.uint8)), 1, R, 993, "cuda")


# ---------------------------------------------------------------------------------------------------------------------------------------
# collation
# ---------------------------------------------------------------------------------------------------------------------------------------
def _collate(pkg, ids, boxes, offs, T, pad_id):
    torch = _torch()
    B = len(offs) - 1
    outs = [_guarded_bytes(n) for n in (B * T * 8, B * T * 8, B * T * 4 * 8)]
    d = [_dev(a) for a in (ids, boxes, offs)]
    pkg.capi.check(pkg.capi.load().ee_collate_pad(_ptr(d[0]), _ptr(d[1]), _ptr(d[2]), B, T, pad_id, _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _stream()),
                   None, "ee_collate_pad")
    torch.cuda.synchronize()
    res = []
    for o, n, shape, what in zip(outs, (B * T * 8, B * T * 8, B * T * 32), ((B, T), (B, T), (B, T, 4)), ("input_ids", "attention_mask", "bbox")):
        _tail_kept(o, n, what)
        res.append(o[:n].view(torch.int64).cpu().numpy().reshape(shape))
    return res


@pytest.mark.parametrize("T", X.COLLATE_T)
def test_collation_equals_the_loop(pkg, T):
    """T on either side of the 256-thread stride; documents of 0, 1, T - 1, T, T + 1 and 5 T tokens, an empty one first and last; pad ids
    and values beyond 32 bits."""
    for B in X.COLLATE_B:
        for i, lengths in enumerate(X.collate_lengths(B, T)):
            ids, boxes, offs = X.collate_inputs(lengths, 1000 * T + 10 * B + i)
            for pad in X.COLLATE_PAD:
                got, want = _collate(pkg, ids, boxes, offs, T, pad), X.collate_ref(ids, boxes, offs, T, pad)
                for g, w, what in zip(got, want, ("input_ids", "attention_mask", "bbox")):
                    assert np.array_equal(g, w), (what, T, B, lengths, pad)


# ---------------------------------------------------------------------------------------------------------------------------------------
# patch projection
# ---------------------------------------------------------------------------------------------------------------------------------------
FORMS = {0: "f32 dma", 1: "f32 registers", 2: "split"}


def _project(pkg, geo, B, H, form, pix, W, b, want_rows=False, expect_err=0):
    """One ee_debug_patch_project call: (out words [M, H] on the device, split rows [M, K] words or None), guards checked."""
    torch = _torch()
    Cn, R, P = geo
    M, K = B * (R // P) ** 2, Cn * P * P
    out = torch.full((M + X.GUARD, H), SENTINEL, dtype=torch.int32, device="cuda")
    rows = torch.full((M + X.GUARD, K), SENTINEL, dtype=torch.int32, device="cuda") if want_rows else None
    a = pkg.capi.DebugPatchProjectArgs()
    hold = [_dev(pix), _dev(W), _dev(b)]
    a.pixel_values, a.weight, a.bias = (t.data_ptr() for t in hold)
    a.B, a.C, a.R, a.P, a.H, a.form = B, Cn, R, P, H, form
    a.out, a.a_split_out = out.data_ptr(), rows.data_ptr() if want_rows else None
    err = C.c_int32(-1)
    a.err_flag_out = C.pointer(err)
    pkg.capi.check(pkg.capi.load().ee_debug_patch_project(C.byref(a), _stream()), None, "ee_debug_patch_project")
    torch.cuda.synchronize()
    assert err.value == expect_err, f"err_flag {err.value}"
    for buf, what in ((out, "out"), (rows, "a_split_out")):
        if buf is not None:
            assert torch.equal(buf[M:], torch.full_like(buf[M:], SENTINEL)), f"{what}: a write at or past row {M}"
    return out[:M], None if rows is None else rows[:M]


def _y32(pix, W, b, P):
    """The float32 yardsticks of a GEMM kernel, as tests/test_gpu_kernels.py (test_f32_gemm_against_float64) takes them, both torch float32 on
    the GPU with TF32 off, on the same operands: torch's GEMM, and the textbook loop with one float32 accumulator per output and k in order.
    The kernels here ARE such a chain (one MFMA accumulator per output, k in order), whatever M; torch's GEMM at a few hundred rows with
    K >= 768 sums in blocks and errs less than a one-accumulator chain does (measured on the worst row at K = 800, 132 rows: torch
    3.6e-07, the loop 8.7e-07, both kernels 1.48e-06; with torch's GEMM alone the rule fails at every K >= 768 geometry by 1.0 to 1.3 e-06
    against the 1e-6 floor), so alone it is no fixed yardstick.  A row's err32 is the larger of the two."""
    torch = _torch()
    tf32, torch.backends.cuda.matmul.allow_tf32 = torch.backends.cuda.matmul.allow_tf32, False
    try:
        with torch.no_grad():
            A, Wd, bd = _dev(X.im2col(pix, P)), _dev(W), _dev(b)
            At, Wt = A.t().contiguous(), Wd.t().contiguous()
            acc = torch.zeros(A.shape[0], Wd.shape[0], dtype=torch.float32, device="cuda")
            for k in range(At.shape[0]):
                acc.addcmul_(At[k][:, None], Wt[k][None, :])
            return (A @ Wd.T + bd).cpu().numpy(), (acc + bd).cpu().numpy()
    finally:
        torch.backends.cuda.matmul.allow_tf32 = tf32


def _check(tag, got, ref, y32):
    """The acceptance rule on every row (y32: one yardstick or several, a row's err32 is the largest); err, err32 and err / tol are recorded
    before the assertion."""
    each = [X.per_row_max(np.asarray(y, np.float64) - ref) for y in (y32 if isinstance(y32, tuple) else (y32,))]
    err, err32 = X.per_row_max(got - ref), np.maximum.reduce(each)
    tol = X.tolerance(err32)
    worst = int(np.argmax(err / tol))
    report_measured(f"pixel[{tag}]", f"max|err| over {len(err)} rows (worst row {worst}: err32 " + " / ".join(f"{e[worst]:.3e}" for e in each)
                    + f", err / tol {err[worst] / tol[worst]:.3f})", float(err.max()))
    assert not np.isnan(got).any(), tag
    bad = [(int(r), float(err[r]), float(err32[r])) for r in np.nonzero(~(err <= tol))[0]]
    assert not bad, (tag, bad[:8])


@pytest.mark.parametrize("geo,B", X.project_cases(), ids=[f"C{g[0]}-R{g[1]}-P{g[2]}-B{B}" for g, B in X.project_cases()])
def test_patch_projection_against_float64(pkg, geo, B):
    """Forms 0 and 1 at every hidden size, form 2 where the split kernel takes it; the real value set and general floats; guard rows kept;
    the split rows are exactly the planes of the patches; two calls give the same bits."""
    torch = _torch()
    P = geo[2]
    for H in X.HIDDEN:
        for draw in ("lut", "general"):
            pix, W, b = X.project_operands(geo, B, H, draw)
            ref, y32 = X.project_ref(pix, W, b, P), _y32(pix, W, b, P)
            for form in (0, 1, 2) if H % 256 == 0 else (0, 1):
                tag = f"C{geo[0]} R{geo[1]} P{P} B{B} H{H} {draw} {FORMS[form]}"
                out, rows = _project(pkg, geo, B, H, form, pix, W, b, want_rows=form == 2)
                _check(tag, _f32(out), ref, y32)
                again, rows2 = _project(pkg, geo, B, H, form, pix, W, b, want_rows=form == 2)
                assert torch.equal(out, again), f"{tag}: two calls differ"
                if form == 2:
                    A64 = X.im2col(pix, P).astype(np.float64)
                    got = _decode_split(rows, A64.shape[1], X.SPLIT_SCALE).cpu().numpy()
                    _check(tag + " rows", got, A64, X.split_values(pix, P))
                    assert np.array_equal(got, X.split_values(pix, P)), f"{tag}: the split rows are not the planes of the patches"
                    assert torch.equal(rows, rows2)
                    plain, _ = _project(pkg, geo, B, H, form, pix, W, b)
                    assert torch.equal(out, plain), f"{tag}: the rows staged in scratch give other bits"


def test_a_pixel_beyond_the_split_planes_raises_the_error_word(pkg):
    geo, B, H = (2, 32, 8), 2, 256
    pix, W, b = X.project_operands(geo, B, H, "lut")
    pix[1, 1, 17, 5] = 5000.0
    assert 5000.0 * X.SPLIT_SCALE > X.SPLIT_LIMIT
    _project(pkg, geo, B, H, 2, pix, W, b, want_rows=True, expect_err=ERR_SPLIT_OVERFLOW)
    ref, y32 = X.project_ref(pix, W, b, geo[2]), _y32(pix, W, b, geo[2])
    for form in (0, 1):
        out, _ = _project(pkg, geo, B, H, form, pix, W, b, expect_err=0)
        _check(f"pixel 5000 {FORMS[form]}", _f32(out), ref, y32)


def test_the_hook_refuses_what_the_kernels_cannot_take(pkg):
    pix, W, b = X.project_operands((2, 32, 8), 1, 128, "lut")
    with pytest.raises(pkg.capi.MMEEError, match="form 2 needs a shape gemm_split_supports takes"):
        _project(pkg, (2, 32, 8), 1, 128, 2, pix, W, b)
    with pytest.raises(pkg.capi.MMEEError, match="unsupported patch geometry"):
        _project(pkg, (1, 32, 4), 1, 128, 0, pix, W, b)          # C P P = 16


# ---------------------------------------------------------------------------------------------------------------------------------------
# one tie to the forward: a geometry other than 16 through ee_forward
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["tiny", "h256"])
def test_a_forward_at_patch_size_8_against_the_oracle(pkg, oracle, shape):
    """patch_size 8, input_size 32 (K = 192, 16 patches): f32 at H = 128 through the im2col GEMM, split at H = 256 through patch_split and
    the split GEMM -- the profile's roles show which the forward launched; both are launch_patch_projection, what the hook calls."""
    ee = dict(exits=["vision_avg", "text_visual_concat", 1, 2, 3], encoder_layer_strategy="ramp", inference_strategy="max_confidence")
    kw = dict(H256_KW) if shape == "h256" else dict(num_hidden_layers=3)
    cfg = pkg.ModelConfig.tiny(EE_config=ee, patch_size=8, input_size=32, **kw)
    W = pkg.synth.make_weights(cfg, seed=61)
    docs = pkg.synth.make_documents(cfg, 5, seed=62, text_len=40, min_words=2)
    assert docs["pixel_values"].shape == (5, 3, 32, 32) and W["layoutlmv3.patch_embed.proj.weight"].shape == (cfg.hidden_size, 3, 8, 8)
    ref = oracle.forward_all(cfg, W, docs, ee["exits"])
    precision = "split" if shape == "h256" else "fp32"
    eng = pkg.EarlyExitEngine(cfg, max_docs=8, max_text_len=40, precision=precision, xprobe=False)
    assert eng.precision == precision
    eng.load_weights(W)
    args = (docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"])
    out = eng.forward(*args, dump_all=True, want_all=True, want_head=True, validate=True)
    al = out.all_logits.cpu().numpy()
    report_measured(f"pixel[forward P8 {shape}]", "max|dlogit|", float(np.abs(al - ref["logits_store"]).max()))
    np.testing.assert_allclose(al, ref["logits_store"], rtol=0, atol=LOGIT_TOL)
    np.testing.assert_allclose(out.head_logits.cpu().numpy(), ref["exit_logits"], rtol=0, atol=LOGIT_TOL)
    eng.profile(True)
    eng.forward(*args, dump_all=True, want_all=True)
    prof = eng.profile_read()
    eng.profile(False)
    assert prof["gemm_patch"]["launches"] == 1 and prof["patch_split"]["launches"] == (1 if precision == "split" else 0), prof
    # the hook on the forward's own pixels and weights, in the form the forward ran: vis_raw, against float64
    H, form = cfg.hidden_size, 2 if precision == "split" else 0
    Wp, bp = W["layoutlmv3.patch_embed.proj.weight"].reshape(H, -1), W["layoutlmv3.patch_embed.proj.bias"]
    vis, _ = _project(pkg, (3, 32, 8), 5, H, form, docs["pixel_values"], np.ascontiguousarray(Wp), bp)
    _check(f"forward P8 {shape} vis_raw", _f32(vis), X.project_ref(docs["pixel_values"], Wp, bp, 8), _y32(docs["pixel_values"], np.ascontiguousarray(Wp), bp, 8))
    eng.close()
