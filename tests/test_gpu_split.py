"""The split-f16 encoders alone (csrc/mmee_common.h "Split-f16 operand rows"), against the numpy model of tests/split_ref.py.  Every comparison
here is on bit patterns: the planes of a finite value are what the model says or they are wrong, so nothing carries a tolerance.

  encoders at the edge set   split_ref.edge_values (rows of 256) through the clamp form (ee_debug_split_rows: split_rows_kernel -> store_split4 ->
                             split_f16x4) at scales 16, 64, 256; through the quad form (ee_debug_patch_project form 2: patch_split_kernel ->
                             store_split4_quad -> split_pair) at its scale of 16; and through the GEMM epilogues (ee_debug_gemm_routes, out_split
                             = 1, W = the identity: split_store_tile16 -> split_pair) on every route launch_gemm_split has for a split output.
  decoder round trip         the residual epilogue with A = 0: Cout = decode(encode(resid)), both residual routes, role tags 2 and 3.
  weight split               ee_debug_split_weight = ee_finalize's split_weight_rows: scale, planes, 1 / scale; inf / nan refused.
  the flag                   one +inf, -inf or NaN in the input of every hook that ends in an encoder raises bit 16; without it the word is 0.
  end to end                 a NaN pixel, a NaN row of inputs_embeds and a NaN / inf weight are refused in precision "split".

What ee_debug_attention cannot do is run attention_f32 with a split context (the hook gives that kernel an f32 one), so its store_split4 calls
are reached here only through the function they share with split_rows_kernel.  In the attention cases the bad V element is flagged where the
hook converts Q | K | V to planes (launch_split_rows, as the QKV GEMM's epilogue would in a forward)."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from . import attn_ref as A
from . import pixel_ref as X
from . import rows_ref as R
from . import split_ref as S
from . import xprobe_ref as XP
from .hook_util import ERR_SPLIT_OVERFLOW, SENTINEL, _dev, _ptr, _stream, _torch
from .test_gpu_attention import IDX, NOBIAS, PAIR
from .test_gpu_attention import _launch as _attention
from .test_gpu_config3_and_robustness import _small_split_cfg
from .test_gpu_pixel import _project
from .test_gpu_rows import _embed, _ln
from .test_gpu_xprobe import _launch as _xprobe

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 4                                # sentinel rows behind every output
EPI_BIAS, EPI_GELU, EPI_RESID = 0, 1, 2
BAD = {"+inf": np.inf, "-inf": -np.inf, "nan": np.nan}
GEO = (4, 8, 4)                          # C, R, P: the smallest geometry patch_geometry_ok takes with K = C P P >= 64 (K = 64, 2 x 2 patches)


def _sent(rows, cols):
    torch = _torch()
    return torch.full((rows + GUARD, cols), SENTINEL, dtype=torch.int32, device="cuda")


def _kept(buf, rows, what):
    torch = _torch()
    assert torch.equal(buf[rows:], torch.full_like(buf[rows:], SENTINEL)), f"{what}: a write at or past row {rows}"


def _same_words(got, want, what):
    """int32 words [rows, N] against the model's, with the first differing element spelled out."""
    got = np.ascontiguousarray(got)
    if np.array_equal(got, want):
        return
    gh, gl = S.unpack(got)
    wh, wl = S.unpack(want)
    bad = np.argwhere((gh != wh) | (gl != wl))
    r, c = bad[0]
    raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ; first at ({r}, {c}): got hi {gh[r, c]:#06x} lo {gl[r, c]:#06x}, "
                         f"want hi {wh[r, c]:#06x} lo {wl[r, c]:#06x}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the clamp form
# ---------------------------------------------------------------------------------------------------------------------------------------
def _split_rows(pkg, x, scale):
    """One ee_debug_split_rows call on f32 rows x: (words [rows, K] numpy, error word)."""
    torch = _torch()
    rows, K = x.shape
    src, dst = _dev(x, torch.float32), _sent(rows, K)
    err = C.c_int32(-1)
    pkg.capi.check(pkg.capi.load().ee_debug_split_rows(_ptr(src), rows, K, scale, _ptr(dst), C.byref(err), _stream()), None, "ee_debug_split_rows")
    torch.cuda.synchronize()
    _kept(dst, rows, "dst_words")
    return dst[:rows].cpu().numpy(), err.value


@pytest.mark.parametrize("overflow", [True, False], ids=["all", "no_overflow"])
@pytest.mark.parametrize("scale", S.SCALES)
def test_clamp_form_at_the_edge_set(pkg, scale, overflow):
    x = S.edge_rows(scale, overflow)
    want, flag = S.encode_words(x, scale, "clamp")
    assert flag == overflow
    got, err = _split_rows(pkg, x, scale)
    _same_words(got, want, f"clamp form, scale {scale}")
    assert err == (ERR_SPLIT_OVERFLOW if flag else 0), err


# ---------------------------------------------------------------------------------------------------------------------------------------
# the quad form
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _patch_operands(H=256):
    rng = np.random.default_rng(11)
    K = GEO[0] * GEO[2] ** 2
    return (0.02 * rng.standard_normal((H, K))).astype(F32), np.zeros(H, F32)


def _pixels(x):
    """A flat f32 vector as the pixel tensor [B, C, R, R] of GEO."""
    Cn, Rn, _ = GEO
    return np.ascontiguousarray(x, F32).reshape(-1, Cn, Rn, Rn)


def _quad_rows(pkg, pix, expect_err):
    W, b = _patch_operands()
    _, rows = _project(pkg, GEO, pix.shape[0], 256, 2, pix, W, b, want_rows=True, expect_err=expect_err)
    return rows.cpu().numpy()


@pytest.mark.parametrize("overflow", [True, False], ids=["all", "no_overflow"])
def test_quad_form_at_the_edge_set_and_against_the_clamp_form(pkg, overflow):
    """The pixel tensor is the edge set: the rows patch_split_kernel writes are the model's pair form, and on every value inside the planes'
    range they are the rows split_rows_kernel writes for the same matrix (the two encoder forms write the same bits)."""
    scale = X.SPLIT_SCALE
    assert scale == 16.0 and GEO[0] * GEO[2] ** 2 == 64
    x = S.edge_values(scale) if overflow else S.without_overflow(S.edge_values(scale), scale)
    pix = _pixels(x)
    hi, lo, flag = S.encode(pix, scale, "pair")
    assert flag == overflow
    want = S.pack(X.im2col(hi, GEO[2]), X.im2col(lo, GEO[2]))
    got = _quad_rows(pkg, pix, ERR_SPLIT_OVERFLOW if flag else 0)
    _same_words(got, want, "quad form")
    mat = np.ascontiguousarray(X.im2col(pix, GEO[2]))
    clamp, err = _split_rows(pkg, mat, scale)
    assert err == (ERR_SPLIT_OVERFLOW if flag else 0)
    inside = ~S.overflows(mat, scale)
    (qh, ql), (ch, cl) = S.unpack(got), S.unpack(clamp)
    assert inside.sum() > 2000 and np.array_equal(qh[inside], ch[inside]) and np.array_equal(ql[inside], cl[inside]), "the two device forms differ"
    if not overflow:
        assert np.array_equal(got, clamp)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the GEMM epilogues
# ---------------------------------------------------------------------------------------------------------------------------------------
N_ID = 256                               # the smallest N and K gemm_split_supports takes with rows of the edge set's 256 columns
W_SCALE = 256.0                          # ee_finalize's scale of the identity (max |w| = 1: 2^8, the cap)
GELU_EXACT = 6.0                         # x >= 4 sqrt 2 = 5.657: 1 - Phi(x) <= 7.7e-9 < 2^-25, so GELU(x) rounds to x in f32


def _gemm(pkg, Am, M, a_scale, out_scale, epi, out_split=1, want_err=True, **kw):
    """ee_debug_gemm_routes with W = the identity: (out words [M, N] numpy, error word)."""
    torch = _torch()
    out = _sent(M, N_ID)
    a = pkg.capi.DebugGemmRoutesArgs()
    W = torch.eye(N_ID, dtype=torch.float32, device="cuda")
    At = _dev(Am, torch.float32)
    vals = dict(M=M, N=N_ID, K=N_ID, epi=epi, out_split=out_split, a_scale=a_scale, w_scale=W_SCALE, out_scale=out_scale, resid_scale=0.0, rows_A=At.shape[0],
                rows_resid=0, route=0, role_tag=0, probe=0, terms=3, k_splits=1, split_stride=0, scale_cols=0, scale=1.0, max_m=0, m_on_device=0, iters=1)
    hold = dict(A=At, W=W, Cout=out)
    for k, v in kw.items():
        if hasattr(v, "data_ptr"):
            hold[k] = v
        else:
            vals[k] = v
    if "resid" in hold:
        vals["rows_resid"] = hold["resid"].shape[0]
    for k, v in hold.items():
        setattr(a, k, v.data_ptr())
    for k, v in vals.items():
        setattr(a, k, v)
    err = C.c_int32(-1)
    if want_err:
        a.err_flag_out = C.pointer(err)
    pkg.capi.check(pkg.capi.load().ee_debug_gemm_routes(C.byref(a), None, _stream()), None, "ee_debug_gemm_routes")
    torch.cuda.synchronize()
    _kept(out, M, "Cout")
    return out[:M].cpu().numpy(), err.value


def _held_exactly(v, a_scale, terms):
    """Which elements of v A's own planes hand to the matrix cores exactly: hi + lo == v inside the planes' range (one term: hi alone)."""
    hi, lo, _ = S.encode(v, a_scale, "clamp")
    h, l = hi.view(np.float16).astype(np.float64), lo.view(np.float16).astype(np.float64)
    held = (h if terms == 1 else h + l) / a_scale
    return (held == v.astype(np.float64)) & ~S.overflows(v, a_scale)


# route of the hook -> the instantiation launch_gemm_split picks at these 10 rows: the small-batch rule's 128 x 128 kernels, route 2 past it to
# the 256 x 256 ones (bias: CfgC; GELU: gemm_split_ffn_up), terms = 1 the one-term kernels
GEMM_ROUTES = {"bias-P": (EPI_BIAS, 0, 3), "bias-C": (EPI_BIAS, 2, 3), "gelu-P": (EPI_GELU, 0, 3), "gelu-ffn_up": (EPI_GELU, 2, 3),
               "bias-one_term": (EPI_BIAS, 0, 1), "gelu-one_term": (EPI_GELU, 0, 1)}


@pytest.mark.parametrize("a_scale", [4.0, 64.0], ids=["a4", "a64"])
@pytest.mark.parametrize("name", list(GEMM_ROUTES))
def test_gemm_epilogues_at_the_edge_set(pkg, name, a_scale):
    """Output planes of out_scale 16 from A = the edge set, W = I, no bias: acc = 256 a_scale v exactly, so the epilogue encodes v (GELU: v where
    GELU(v) is v, else 0).  A holds only values its own planes hold exactly (asserted); a_scale 4 keeps the overflow edge inside A's planes,
    a_scale 64 the values with a subnormal lo."""
    epi, route, terms = GEMM_ROUTES[name]
    out_scale = 16.0
    v = S.edge_rows(out_scale).copy()
    keep = _held_exactly(v, a_scale, terms)
    if epi == EPI_GELU:
        keep &= v >= GELU_EXACT
    v[~keep] = 0.0
    assert np.array_equal(S.plane_values(v, a_scale)[keep], v.astype(np.float64)[keep]) and not S.encode(v, a_scale)[2]
    floor = {(EPI_BIAS, 3): 500, (EPI_BIAS, 1): 150, (EPI_GELU, 3): 100, (EPI_GELU, 1): 20}[epi, terms]
    assert keep.sum() >= floor, (name, int(keep.sum()))
    want, flag = S.encode_words(v + F32(0.0), out_scale, "pair")           # (the accumulator starts at +0: -0 comes out as +0)
    assert flag == bool(a_scale == 4.0)                                    # the overflow edge survives in A only at the small scale
    got, err = _gemm(pkg, v, v.shape[0], a_scale, out_scale, epi, route=route, terms=terms)
    _same_words(got, want, f"GEMM epilogue {name}, a_scale {a_scale}")
    assert err == (ERR_SPLIT_OVERFLOW if flag else 0), err


# ---------------------------------------------------------------------------------------------------------------------------------------
# the decoder
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role_tag", [2, 3])
@pytest.mark.parametrize("route", [0, 1, 2], ids=["routed", "direct", "lds_dma"])
@pytest.mark.parametrize("scale", [16.0, 64.0])
def test_decoder_round_trip(pkg, scale, route, role_tag):
    """A = 0, no bias, the residual epilogue with a split residual: Cout = 0 + (hi + lo) / scale, the f32 of decode(encode(resid)), on the
    router's choice, the direct read (128 x 128) and the LDS-DMA staging (256 x 256)."""
    resid = S.edge_rows(scale)
    M = resid.shape[0]
    want_words, flag = S.encode_words(resid, scale, "clamp")
    want = S.decode(want_words, scale).astype(F32) + F32(0.0)
    assert flag and np.array_equal(want.astype(np.float64), S.decode(want_words, scale))
    got, err = _gemm(pkg, np.zeros((M, N_ID), F32), M, 16.0, 1.0, EPI_RESID, out_split=0, resid=_dev(resid, _torch().float32), resid_scale=scale, route=route,
                     role_tag=role_tag)
    assert np.array_equal(got, want.view(np.int32)), int((got != want.view(np.int32)).sum())
    assert err == ERR_SPLIT_OVERFLOW                                       # the residual's own conversion saw the overflow edge


# ---------------------------------------------------------------------------------------------------------------------------------------
# the weight split
# ---------------------------------------------------------------------------------------------------------------------------------------
def _split_weight(pkg, w, refused=False):
    torch = _torch()
    N, K = w.shape
    src, dst = _dev(w, torch.float32), _sent(N, K)
    inv = C.c_float(-1.0)
    rc = pkg.capi.load().ee_debug_split_weight(_ptr(src), N, K, _ptr(dst), C.byref(inv), _stream())
    torch.cuda.synchronize()
    if refused:
        assert rc != 0, "the hook accepted what it must refuse"
        assert torch.equal(dst, torch.full_like(dst, SENTINEL)), "a refused call wrote to dst_words"
        assert inv.value == -1.0
        return pkg.capi.last_error()
    pkg.capi.check(rc, None, "ee_debug_split_weight")
    _kept(dst, N, "dst_words")
    return dst[:N].cpu().numpy(), inv.value


def _weight(mx, at, shape=(8, 64), seed=0):
    """A tensor of magnitudes below |mx| / 2 with mx at flat index `at`."""
    rng = np.random.default_rng(seed)
    w = (rng.uniform(-0.5, 0.5, shape) * abs(float(mx))).astype(F32)
    w.reshape(-1)[at] = mx
    assert np.abs(w).max() == abs(F32(mx))
    return w


WEIGHTS = {f"2^{k}{'-' if below else ''}": (np.nextafter(F32(2.0 ** k), F32(0)) if below else F32(2.0 ** k), 100) for k in (-6, 4, 5) for below in (False, True)}
WEIGHTS.update({"first": (F32(0.07), 0), "last": (F32(0.07), -1), "negative": (F32(-0.07), 300), "1e6": (F32(1e6), 5)})


@pytest.mark.parametrize("name", list(WEIGHTS))
def test_weight_split_scale_and_planes(pkg, name):
    mx, at = WEIGHTS[name]
    w = _weight(mx, at)
    want, inv, e = S.encode_weight(w)
    if name in ("2^4-", "2^5"):
        assert (e, S.weight_exponent(np.nextafter(F32(32.0), F32(0))), S.weight_exponent(32.0), S.weight_exponent(16.0)) == (8 if name == "2^4-" else 7, 8, 7, 8)
    got, got_inv = _split_weight(pkg, w)
    assert got_inv == inv, (got_inv, inv, e)
    _same_words(got, want, f"weight {name}")


def test_weight_split_of_zero_and_tiny_tensors(pkg):
    for w in (np.zeros((8, 64), F32), np.full((8, 64), 1e-30, F32)):
        want, inv, e = S.encode_weight(w)
        assert e == 8 and not want.any()
        got, got_inv = _split_weight(pkg, w)
        assert got_inv == inv == F32(2.0 ** -8)
        _same_words(got, want, "zero / 1e-30")


def test_weight_split_where_the_maximum_is_past_the_first_sweep(pkg):
    """1040 x 256: more than the 1024 x 256 threads of absmax_kernel's grid, and the maximum in the part only the second sweep reads."""
    w = _weight(F32(100.0), 1040 * 256 - 7, shape=(1040, 256), seed=1)
    assert 1040 * 256 - 7 >= 1024 * 256
    want, inv, e = S.encode_weight(w)
    assert e == 6 and S.weight_exponent(np.abs(w[:1024]).max()) > 6          # 100 = 0.78 x 2^7; without it every |w| < 50: another scale
    got, got_inv = _split_weight(pkg, w)
    assert got_inv == inv
    _same_words(got, want, "weight 1040 x 256")


@pytest.mark.parametrize("at", [0, 257, -1], ids=["first", "middle", "last"])
@pytest.mark.parametrize("bad", list(BAD))
def test_weight_split_refuses_inf_and_nan(pkg, bad, at):
    w = _weight(F32(0.07), 100)
    w.reshape(-1)[at] = BAD[bad]
    assert S.encode_weight(w) is None
    assert "ee_debug_split_weight: a weight tensor holds inf/nan" == _split_weight(pkg, w, refused=True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the flag on non-finite input
# ---------------------------------------------------------------------------------------------------------------------------------------
def _flag_split_rows(pkg, bad):
    x = S.edge_rows(16.0, overflow=False).copy()
    if bad is not None:
        x[3, 77] = bad
    return _split_rows(pkg, x, 16.0)[1]


def _flag_patch_project(pkg, bad):
    pix = _pixels(S.without_overflow(S.edge_values(16.0), 16.0)).copy()
    if bad is not None:
        pix[2, 1, 5, 3] = bad
    want = 0 if bad is None else ERR_SPLIT_OVERFLOW
    _quad_rows(pkg, pix, want)           # _project asserts the error word
    return want


def _flag_ln_rows(pkg, bad):
    c = R.LnCase(256, 5, gather=False)
    if bad is not None:
        c.parts[0, 3, 9] = bad
    want = 0 if bad is None else ERR_SPLIT_OVERFLOW
    _ln(pkg, c, "split", expect_err=want)
    return want


def _flag_embed(pkg, bad):
    c = copy.copy(R.EmbedCase(256, 48, 32))
    c.word = c.word.copy()
    if bad is not None:
        assert c.mask[1, 4] == 1
        c.word[c.ids[1, 4], 17] = bad
    want = 0 if bad is None else ERR_SPLIT_OVERFLOW
    _embed(pkg, c, split=True, expect_err=want)
    return want


def _flag_gemm(pkg, bad):
    v = (np.random.default_rng(5).integers(-2 ** 15, 2 ** 15, (10, N_ID)) * 2.0 ** -12).astype(F32)      # |v| < 8, 16 bits: exact in any plane
    if bad is not None:
        v[6, 130] = bad
    return _gemm(pkg, v, 10, 16.0, 16.0, EPI_BIAS)[1]


def _flag_attention(kernel):
    def run(pkg, bad):
        b = A.make_batch(lengths=(33, 64), heads=2, seed=9, holes=False)
        qkv = b.qkv.copy()
        if bad is not None:
            qkv[40, 2 * 128 + 70] = bad      # V of key 7 of document 1, head 1
        want = 0 if bad is None else ERR_SPLIT_OVERFLOW
        _attention(pkg, b, kernel, qkv=qkv, expect_err=want)
        return want
    return run


def _flag_xprobe(pkg, bad):
    c = XP.count_case(12, 3)
    bv = c.bv.copy()
    if bad is not None:
        bv[5] = bad
    want = 0 if bad is None else ERR_SPLIT_OVERFLOW
    _xprobe(pkg, c, bv=bv, expect_err=want)
    return want


FLAG_HOOKS = {"split_rows": _flag_split_rows, "patch_project": _flag_patch_project, "ln_rows": _flag_ln_rows, "embed": _flag_embed, "gemm_routes": _flag_gemm,
              "attention_pair": _flag_attention(PAIR), "attention_idx": _flag_attention(IDX), "attention_nobias": _flag_attention(NOBIAS),
              "xprobe": _flag_xprobe}


@pytest.mark.parametrize("hook", list(FLAG_HOOKS))
def test_clean_input_raises_no_flag(pkg, hook):
    assert FLAG_HOOKS[hook](pkg, None) == 0


@pytest.mark.parametrize("bad", list(BAD))
@pytest.mark.parametrize("hook", list(FLAG_HOOKS))
def test_a_non_finite_input_raises_the_flag(pkg, hook, bad):
    """One element +inf, -inf or NaN: bit 16 of the error word (the helpers of the other hook tests assert the word itself)."""
    assert FLAG_HOOKS[hook](pkg, F32(BAD[bad])) & ERR_SPLIT_OVERFLOW


# ---------------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _e2e(pkg):
    ee, cfg = _small_split_cfg(pkg)
    W = pkg.synth.make_weights(cfg, seed=61)
    docs = pkg.synth.make_documents(cfg, 4, seed=62, text_len=40, min_words=2)
    return cfg, W, docs


def _engine(pkg, precision, W=None):
    cfg, W0, _ = _e2e(pkg)
    eng = pkg.EarlyExitEngine(cfg, max_docs=4, max_text_len=40, precision=precision, xprobe=False)
    eng.load_weights(W0 if W is None else W)
    return eng


def test_a_nan_pixel_is_refused_in_split_precision_and_reaches_the_logits_in_fp32(pkg):
    _, _, docs = _e2e(pkg)
    pix = docs["pixel_values"].copy()
    pix[2, 1, 7, 9] = np.nan
    args = (docs["input_ids"], docs["attention_mask"], docs["bbox"])
    eng = _engine(pkg, "split")
    eng.forward(*args, docs["pixel_values"], dump_all=True, validate=True)      # the clean batch runs
    with pytest.raises(pkg.capi.MMEEError, match="overflow"):
        eng.forward(*args, pix, dump_all=True, validate=True)
    eng.close()
    e32 = _engine(pkg, "fp32")                                                   # no such check: today's behaviour, pinned
    logits = e32.forward(*args, pix, dump_all=True, want_all=True).all_logits.cpu().numpy()
    e32.close()
    assert np.isnan(logits[:, 2]).all() and np.isfinite(np.delete(logits, 2, axis=1)).all()


def test_a_nan_row_of_inputs_embeds_is_refused_in_split_precision(pkg):
    cfg, W, docs = _e2e(pkg)
    emb = W["layoutlmv3.embeddings.word_embeddings.weight"][docs["input_ids"]].astype(F32)
    kw = dict(attention_mask=docs["attention_mask"], bbox=docs["bbox"], pixel_values=docs["pixel_values"])
    eng = _engine(pkg, "split")
    eng.forward(inputs_embeds=emb, **kw, dump_all=True, validate=True)
    assert docs["attention_mask"][1, 3] == 1
    emb[1, 3, :] = np.nan
    with pytest.raises(pkg.capi.MMEEError, match="overflow"):
        eng.forward(inputs_embeds=emb, **kw, dump_all=True, validate=True)
    eng.close()


@pytest.mark.parametrize("bad", ["nan", "+inf"])
def test_a_non_finite_weight_is_refused_at_load_in_split_precision(pkg, bad):
    cfg, W, _ = _e2e(pkg)
    name = "layoutlmv3.encoder.layer.1.attention.self.query.weight"
    W = dict(W)
    W[name] = W[name].copy()
    W[name][17, 33] = BAD[bad]
    eng = pkg.EarlyExitEngine(cfg, max_docs=4, max_text_len=40, precision="split", xprobe=False)
    with pytest.raises(pkg.capi.MMEEError, match="holds inf/nan"):
        eng.load_weights(W)
    eng.close()
