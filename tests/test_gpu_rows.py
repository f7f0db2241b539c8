"""The row kernels of csrc/prep_embed.hip alone, through ee_debug_prep / ee_debug_embed / ee_debug_ln_rows, against the float64 restatement of
tests/rows_ref.py at every hidden-size route.

Acceptance, float outputs, per row (as test_gpu_kernels.py and test_gpu_attention.py): max |got - ref64| <= max(2 * err32, 1e-6), err32 = the
error of the same operation in torch float32 on the CPU.  Split-plane outputs are decoded in float64 and their yardstick is the float32 result
passed through the plane model at the same scale.  Integer outputs (prep): equality.  Every output buffer ends in guard rows of a NaN bit
pattern that must survive.  tests/test_host_rows_ref.py shows that the inputs see each of sixteen subtle faults at 10 times these tolerances.

Which case reaches which instantiation (NV = ceil(H / 256), FULL = (H == 256 NV), FAST = cs, ss multiples of 4):
  embed_text<1, slow, POOLED>                 128 24/16, every mode           embed_text<2, slow, POOLED>        256, 384 (both), 512, every mode
  embed_text<3, FAST, POOLED / plain>         640 96/128  pooled, text_avg / rows, embeds, types
  embed_text<3, FAST, *, FULL>                768 128/128 (same modes)        embed_text<3, slow, *>             768 127/130
  embed_text<4, FAST, POOLED / plain>         896 160/128                     embed_text<4, FAST, *, FULL>       1024 192/128
  embed_text<4, slow, *>                      1024 171/170
  embed_visual_rows<NV[, FULL]>               every configuration, modes rows, text_avg, embeds, types (no vis / cat partial sums)
  embed_visual<NV[, FULL]> + pool_finish      every configuration, mode pooled;  split rows: 256, 512, 768, 1024 in modes rows and pooled
  ln_rows<1, plain, FULL / not>               256 / 128                       ln_rows<2, plain>                  384, 512
  ln_rows<3 / 4, plain, FULL / not>           768, 1024 / 640, 896            ln_rows<NV, PRE[, FULL]>           all eight sizes, parts 1, 2, 4, 8
  doc_prep with two and more positions per thread: T = 257, 512;  doc_scan's second sweep: B = 1025."""
import ctypes as C
import functools

import numpy as np
import pytest

from . import rows_ref as R
from .conftest import report_measured
from .hook_util import ERR_SPLIT_OVERFLOW, SENTINEL, _dev, _encode_split, _f32, _ptr, _stream, _torch
from .hook_util import _decode_split as _decode_split_dev

pytestmark = pytest.mark.gpu

GUARD = 4                                               # rows (or 16-byte words) past the last one in every output buffer


def _sent(rows, cols):
    torch = _torch()
    return torch.full((rows + GUARD, cols), SENTINEL, dtype=torch.int32, device="cuda")


def _kept(buf, first, what):
    torch = _torch()
    assert torch.equal(buf[first:], torch.full_like(buf[first:], SENTINEL)), f"{what}: a write at or past row {first}"


def _decode_split(rows_i32, N, scale):
    return _decode_split_dev(rows_i32, N, scale).cpu().numpy()


def _check(tag, got, ref, y32):
    """The acceptance rule on every row; every err, err32 and err / tol is recorded before the assertion."""
    err = R.per_row_max(got - ref)
    err32 = R.per_row_max(np.asarray(y32, np.float64) - ref)
    tol = R.tolerance(err32)
    worst = int(np.argmax(err / tol)) if len(err) else 0
    if len(err):
        report_measured(f"rows[{tag}]", f"max|err| over {len(err)} rows (worst row {worst}: err32 {err32[worst]:.3e}, err / err32 "
                        f"{err[worst] / max(err32[worst], 1e-30):.2f}, err / tol {err[worst] / tol[worst]:.2f})", float(err.max()))
    assert not np.isnan(got).any(), tag
    bad = [(int(r), float(err[r]), float(err32[r])) for r in np.nonzero(~(err <= tol))[0]]
    assert not bad, (tag, bad[:8])


# ---------------------------------------------------------------------------------------------------------------------------------------
# prep
# ---------------------------------------------------------------------------------------------------------------------------------------
def _prep(pkg, ids, am, bbox, G, pos_ids=None, tt=None, dense=False, max_pos=None, type_vocab=1):
    """One ee_debug_prep call.  Returns what the kernels wrote as a dict shaped like rows_ref.prep_ref's, guard rows checked."""
    torch = _torch()
    B, T = ids.shape
    Pv = G * G + 1
    cap = B * (T + Pv)
    i64 = lambda a: None if a is None else _dev(a, torch.int64)
    t_in = [i64(a) for a in (ids, am, bbox, pos_ids, tt)]
    out = dict(text_dst=_sent(B * T, 1), emb_pos=_sent(B * T, 1), ntext=_sent(B, 1), doc_off=_sent(B + 1, 1), x_src=_sent(B, 1), doc_orig=_sent(B, 1),
               meta=_sent(cap, 4), counts=_sent(4, 1))
    err = C.c_int32(-1)
    lib = pkg.capi.load()
    pkg.capi.check(lib.ee_debug_prep(*[_ptr(t) for t in t_in], B, T, G, R.PAD, R.VOCAB, R.MAX_2D, max_pos or T + 2, type_vocab, int(dense),
                                     *[_ptr(out[k]) for k in ("text_dst", "emb_pos", "ntext", "doc_off", "x_src", "doc_orig", "meta", "counts")],
                                     C.byref(err), _stream()), None, "ee_debug_prep")
    torch.cuda.synchronize()
    counts = out["counts"][:4, 0].cpu().numpy()
    n_rows = int(counts[1])
    assert 0 <= n_rows <= cap
    for k, n in (("text_dst", B * T), ("emb_pos", B * T), ("ntext", B), ("doc_off", B + 1), ("x_src", B), ("doc_orig", B), ("meta", n_rows), ("counts", 4)):
        _kept(out[k], n, k)
    got = {k: out[k][:n, 0].cpu().numpy() for k, n in (("ntext", B), ("doc_off", B + 1), ("x_src", B), ("doc_orig", B))}
    got.update(text_dst=out["text_dst"][:B * T, 0].cpu().numpy().reshape(B, T), emb_pos=out["emb_pos"][:B * T, 0].cpu().numpy().reshape(B, T),
               meta=out["meta"][:n_rows].cpu().numpy(), n_docs=int(counts[0]), n_rows=n_rows,
               sum_len_sq=int(counts[2:4].copy().view(np.uint64)[0]), err=err.value)
    return got


def _same_prep(got, want):
    for k in ("n_docs", "n_rows", "sum_len_sq", "err"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("text_dst", "emb_pos", "ntext", "doc_off", "x_src", "doc_orig", "meta"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4] if got[k].shape == want[k].shape else got[k].shape)


@pytest.mark.parametrize("dense", [False, True], ids=["ragged", "dense"])
@pytest.mark.parametrize("kind", R.MASKS)
@pytest.mark.parametrize("T", [1, 8, 9, 33, 257, 512])
def test_prep_against_the_restatement(pkg, T, kind, dense):
    """B = 3 (and B = 1 at two lengths); T = 257, 512: two positions per thread of doc_prep."""
    for B in ((3, 1) if T in (9, 257) else (3,)):
        ids, am, bbox = R.make_prep_inputs(B, T, kind, seed=T)
        _same_prep(_prep(pkg, ids, am, bbox, 2, dense=dense), R.prep_ref(ids, am, bbox, 2, dense_rows=dense, max_pos=T + 2))


@pytest.mark.parametrize("dense", [False, True], ids=["ragged", "dense"])
@pytest.mark.parametrize("kind", R.MASKS)
def test_prep_second_sweep_of_the_document_scan(pkg, kind, dense):
    """B = 1025: doc_scan's loop runs twice and carries the offset of document 1024 over."""
    ids, am, bbox = R.make_prep_inputs(1025, 8, kind, seed=1025)
    _same_prep(_prep(pkg, ids, am, bbox, 2, dense=dense), R.prep_ref(ids, am, bbox, 2, dense_rows=dense, max_pos=10))


@pytest.mark.parametrize("G", [2, 6, 14])
def test_prep_visual_boxes_and_custom_positions(pkg, G):
    ids, am, bbox = R.make_prep_inputs(3, 33, "hole", seed=G)
    pos = np.random.default_rng(G).integers(0, 35, (3, 33))
    _same_prep(_prep(pkg, ids, am, bbox, G), R.prep_ref(ids, am, bbox, G, max_pos=35))
    _same_prep(_prep(pkg, ids, am, bbox, G, pos_ids=pos), R.prep_ref(ids, am, bbox, G, pos_ids=pos, max_pos=35))


def test_prep_flags_and_clamps_what_is_out_of_range(pkg):
    """One out-of-range value per input kind: exactly its bit of the error word, and outputs inside their ranges."""
    T = 33
    ids, am, bbox = R.make_prep_inputs(3, T, "trailing", seed=7)
    tt = np.zeros((3, T), np.int64)
    pos = np.random.default_rng(7).integers(0, T + 2, (3, T))
    cases = {}
    a = ids.copy(); a[0, 1] = R.VOCAB
    cases[1] = dict(ids=a)
    a = ids.copy(); a[1, 2] = -1
    cases["1 (negative)"] = dict(ids=a)
    a = bbox.copy(); a[0, 1, 0] = R.MAX_2D + 5; a[0, 2, 3] = -3
    cases[2] = dict(bbox=a)
    a = pos.copy(); a[0, 3] = T + 2; a[1, 0] = -1
    cases[4] = dict(pos_ids=a)
    cases["4 (computed)"] = dict(max_pos=T + 1, am=np.ones((3, T), np.int64), ids=np.where(ids == R.PAD, 5, ids))       # the last token's id is T + 1
    a = tt.copy(); a[2, 0] = 1
    cases[8] = dict(tt=a)
    for bit, over in cases.items():
        kw = dict(ids=ids, am=am, bbox=bbox, pos_ids=None, tt=tt, max_pos=T + 2)
        kw.update(over)
        got = _prep(pkg, kw["ids"], kw["am"], kw["bbox"], 2, pos_ids=kw["pos_ids"], tt=kw["tt"], max_pos=kw["max_pos"])
        want = R.prep_ref(kw["ids"], kw["am"], kw["bbox"], 2, pos_ids=kw["pos_ids"], tt=kw["tt"], max_pos=kw["max_pos"])
        assert want["err"] == int(str(bit).split()[0]), bit
        _same_prep(got, want)
        assert got["emb_pos"].min() >= 0 and got["emb_pos"].max() < kw["max_pos"]
        assert got["meta"][:, 1:3].min() >= 0 and got["meta"][:, 1].max() <= 4 * 999


# ---------------------------------------------------------------------------------------------------------------------------------------
# embed
# ---------------------------------------------------------------------------------------------------------------------------------------
MODES = {      # name -> (pooled outputs, inputs_embeds, type_vocab)
    "rows": ((), False, 1), "pooled": (("text", "vis", "cat"), False, 1), "text_avg": (("text",), False, 1), "embeds": ((), True, 1),
    "types": ((), False, 2),
}
cid = lambda c: f"H{c[0]}_cs{c[1]}_ss{c[2]}"


@functools.lru_cache(maxsize=None)
def _case(cfg, type_vocab=1):
    return R.EmbedCase(*cfg, type_vocab=type_vocab)


@functools.lru_cache(maxsize=None)
def _embed_reference(cfg, type_vocab, use_embeds, dense=False):
    """Reference and yardstick of one configuration: computed once, shared, never written to."""
    c = _case(cfg, type_vocab)
    return R.embed_ref(c, dense, use_embeds), R.embed_f32_torch(c, dense, use_embeds)


def _embed(pkg, c, pooled=(), use_embeds=False, split=False, dense=False, expect_err=0, lay=None, **over):
    """One ee_debug_embed call.  Returns (X words [n_rows, H] on the device, {pooled name: float64 [B, H]})."""
    torch = _torch()
    lay = lay or c.prep(dense)
    n_rows, B, T, H, Pv = lay["n_rows"], c.B, c.T, c.H, c.Pv
    tch, vch = (T + 31) // 32, (Pv + 31) // 32
    hold = {}
    a = pkg.capi.DebugEmbedArgs()
    for k, v in dict(B=B, T=T, G=c.G, pad_id=R.PAD, vocab=R.VOCAB, max_2d=R.MAX_2D, max_pos=c.max_pos, type_vocab=c.type_vocab, dense_rows=int(dense),
                     H=H, cs=c.cs, ss=c.ss, text_eps=R.EPS, vis_eps=R.VIS_EPS, eps2=R.EPS, split_scale=R.SPLIT_SCALE if split else 0.0).items():
        setattr(a, k, over.get(k, v))
    ints = dict(input_ids=c.ids, attention_mask=c.mask, bbox=c.bbox, token_type_ids=c.tt if c.type_vocab > 1 else None)
    floats = dict(word=c.word, type=c.type, pos=c.pos, xtab=c.xtab, ytab=c.ytab, htab=c.htab, wtab=c.wtab, inputs_embeds=c.inputs_embeds if use_embeds else None,
                  text_ln_g=c.text_g, text_ln_b=c.text_b, vis_ln_g=c.vis_g, vis_ln_b=c.vis_b, ln2_g=over.get("ln2_g", c.ln2_g), ln2_b=over.get("ln2_b", c.ln2_b),
                  cls_token=c.cls_token, pos_embed=c.pos_embed, vis_raw=c.vis_raw)
    for k, v in ints.items():
        hold[k] = None if v is None else _dev(v, torch.int64)
    for k, v in floats.items():
        hold[k] = None if v is None else _dev(v, torch.float32)
    hold["out"] = _sent(n_rows, H)
    hold["Xs" if split else "X"] = hold["out"]
    chunks = dict(text=tch, vis=vch, cat=tch + vch)
    for k in pooled:
        hold[k + "_part"] = torch.zeros((B * chunks[k] + 1, H), dtype=torch.float32, device="cuda")
        hold["pooled_" + k] = _sent(B, H)
    for name, _ in a._fields_:
        if name in hold and hold[name] is not None:
            setattr(a, name, hold[name].data_ptr())
    err = C.c_int32(-1)
    lib = pkg.capi.load()
    pkg.capi.check(lib.ee_debug_embed(C.byref(a), C.byref(err), _stream()), None, "ee_debug_embed")
    torch.cuda.synchronize()
    assert err.value == expect_err, f"err_flag {err.value}"
    _kept(hold["out"], n_rows, "X")
    res = {}
    for k in pooled:
        _kept(hold["pooled_" + k], B, "pooled " + k)
        res[k] = _f32(hold["pooled_" + k][:B])
    return hold["out"][:n_rows], res


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("cfg", R.EMBED_CONFIGS, ids=cid)
def test_embed_against_float64(pkg, cfg, mode):
    """f32 rows and pooled vectors of B = 2, T = 41, G = 6 at every (hidden size, coordinate / shape size) route."""
    pooled, use_embeds, type_vocab = MODES[mode]
    c = _case(cfg, type_vocab)
    ref, y32 = _embed_reference(cfg, type_vocab, use_embeds)
    words, pool = _embed(pkg, c, pooled, use_embeds)
    tag = f"embed {cid(cfg)} {mode}"
    _check(tag + " X", _f32(words), ref["X"], y32["X"])
    for k in pooled:
        _check(f"{tag} {k}", pool[k], ref[k], y32[k])


@pytest.mark.parametrize("mode", ["rows", "pooled"])
@pytest.mark.parametrize("cfg", [c for c in R.EMBED_CONFIGS if c[0] % 256 == 0], ids=cid)
def test_embed_split_rows_against_float64(pkg, cfg, mode):
    """Split-f16 rows (scale 16): the acceptance rule on the decoded planes, error word 0, and the planes are the split of the f32 run's bits."""
    pooled = MODES[mode][0]
    c = _case(cfg)
    ref, y32 = _embed_reference(cfg, 1, False)
    words, pool = _embed(pkg, c, pooled, split=True)
    got = _decode_split(words, c.H, R.SPLIT_SCALE)
    tag = f"embed {cid(cfg)} {mode} split"
    _check(tag + " X", got, ref["X"], R.split_yardstick(y32["X"]))
    for k in pooled:
        _check(f"{tag} {k}", pool[k], ref[k], y32[k])
    f32_words, _ = _embed(pkg, c, pooled)
    assert np.array_equal(got, R.split_round(_f32(f32_words).astype(np.float32), R.SPLIT_SCALE)), "the split rows are not the split of the f32 rows"


def test_the_acceptance_rule_sees_a_wrong_eps(pkg):
    """The hook handed the visual LayerNorm's eps as 1e-5 instead of 1e-6 (what a kernel with the two swapped would compute for those rows):
    the same check that passes above must fail, on the visual rows."""
    cfg = (640, 96, 128)
    c = _case(cfg)
    ref, y32 = _embed_reference(cfg, 1, False)
    words, _ = _embed(pkg, c, vis_eps=R.EPS)
    with pytest.raises(AssertionError, match="wrong eps"):
        _check("wrong eps", _f32(words), ref["X"], y32["X"])


def test_embed_split_overflow_is_flagged(pkg):
    """One column of the model-level LayerNorm's bias at 4000 > 60000 / 16: bit 16.  (Every run above asserts an error word of 0.)"""
    c = _case((256, 48, 32))
    b = c.ln2_b.copy()
    b[5] = 4000.0
    assert 4000.0 * R.SPLIT_SCALE > R.SPLIT_LIMIT and np.abs(_embed_reference((256, 48, 32), 1, False)[0]["X"]).max() * R.SPLIT_SCALE < R.SPLIT_LIMIT
    _embed(pkg, c, split=True, expect_err=ERR_SPLIT_OVERFLOW, ln2_b=b)


@pytest.mark.parametrize("dense", [False, True], ids=["ragged", "dense"])
def test_embed_dense_rows_and_their_layout(pkg, dense):
    """MMEE_FLAG_DENSE_ROWS keeps the trailing pad rows: every position becomes a row, at two routes."""
    for cfg in ((128, 24, 16), (640, 96, 128)):
        c = _case(cfg)
        ref, y32 = _embed_reference(cfg, 1, False, dense)
        assert ref["lay"]["n_rows"] == (2 * 78 if dense else 142)
        words, pool = _embed(pkg, c, ("text", "cat"), dense=dense)
        _check(f"embed {cid(cfg)} dense={dense} X", _f32(words), ref["X"], y32["X"])
        for k in ("text", "cat"):
            _check(f"embed {cid(cfg)} dense={dense} {k}", pool[k], ref[k], y32[k])


@pytest.mark.parametrize("cfg", R.EMBED_CONFIGS, ids=cid)
def test_embed_visual_routes_write_the_same_bits(pkg, cfg):
    """embed_visual_rows (no pooled exit) and embed_visual (chunked, with the partial sums) write the same visual rows, bit for bit, as the
    comment in prep_embed.hip claims; in f32 and, where the hidden size allows them, in split rows."""
    torch = _torch()
    c = _case(cfg)
    lay = c.prep()
    vis = _dev(np.concatenate([np.arange(lay["doc_off"][b] + lay["ntext"][b], lay["doc_off"][b + 1]) for b in range(c.B)]), torch.int64)
    for split in ((False, True) if c.H % 256 == 0 else (False,)):
        rows, _ = _embed(pkg, c, (), split=split)
        chunked, _ = _embed(pkg, c, ("vis", "cat"), split=split)
        assert torch.equal(rows[vis], chunked[vis]), f"split={split}"


@pytest.mark.parametrize("pooled", [(), ("text", "vis", "cat")], ids=["rows", "pooled"])
@pytest.mark.parametrize("cfg", [(128, 24, 16), (512, 96, 64), (640, 96, 128), (1024, 171, 170)], ids=cid)
def test_a_documents_rows_do_not_depend_on_the_batch(pkg, cfg, pooled):
    """A document alone = inside the batch = in the other slot: rows and pooled vectors, bit for bit."""
    torch = _torch()
    c = _case(cfg)
    lay = c.prep()
    full, fp = _embed(pkg, c, pooled)
    swapped, sp = _embed(pkg, c.select([1, 0]), pooled)
    r = [slice(int(lay["doc_off"][b]), int(lay["doc_off"][b + 1])) for b in range(2)]
    n1 = r[1].stop - r[1].start
    assert torch.equal(swapped[:n1], full[r[1]]) and torch.equal(swapped[n1:], full[r[0]])
    for b in range(2):
        alone, ap = _embed(pkg, c.select([b]), pooled)
        assert torch.equal(alone, full[r[b]]), b
        for k in pooled:
            assert np.array_equal(ap[k][0], fp[k][b]) and np.array_equal(sp[k][1 - b], fp[k][b]), (k, b)


def test_the_embed_hook_refuses_what_the_launchers_cannot_take(pkg):
    c = _case((128, 24, 16))
    with pytest.raises(pkg.capi.MMEEError, match="multiple of 128"):
        _embed(pkg, c, H=192, cs=32, ss=32)
    with pytest.raises(pkg.capi.MMEEError, match="multiple of 128"):
        _embed(pkg, c, H=1152, cs=192, ss=192)
    with pytest.raises(pkg.capi.MMEEError, match="is not the hidden size"):
        _embed(pkg, c, cs=25)
    with pytest.raises(pkg.capi.MMEEError, match="multiple of 256"):
        _embed(pkg, c, split=True)
    with pytest.raises(pkg.capi.MMEEError, match="multiple of 256"):
        _embed(pkg, _case((384, 64, 64)), split=True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# ln_rows
# ---------------------------------------------------------------------------------------------------------------------------------------
def _ln(pkg, c, out="dst", max_rows=None, expect_err=0, H=None, n_word=None):
    """One ee_debug_ln_rows call on an LnCase.  out: "dst", "split", "both" or "inplace".  Returns {"dst": float64 rows, "split": decoded rows}."""
    torch = _torch()
    n, Hc = c.n, c.H
    max_rows = n + 2 if max_rows is None else max_rows
    src = _dev(c.src, torch.float32)
    if out == "inplace":
        assert not c.pre_parts and c.row_src is None
        src = torch.cat([src.view(torch.int32).view(c.src_rows, Hc), _sent(0, Hc)])
    dst = src if out == "inplace" else _sent(max_rows, Hc) if out in ("dst", "both") else None
    dsp = _sent(max_rows, Hc) if out in ("split", "both") else None
    t = dict(row_src=None if c.row_src is None else _dev(c.row_src, torch.int32), n=_dev(np.array([n if n_word is None else n_word], np.int32)),
             g=_dev(c.g), b=_dev(c.b), bias=None if c.bias is None else _dev(c.bias),
             resid=None if c.resid is None else _dev(_encode_split(c.resid, R.SPLIT_SCALE)),
             resid_rows=None if c.resid_rows is None else _dev(c.resid_rows, torch.int32))
    err = C.c_int32(-1)
    lib = pkg.capi.load()
    pkg.capi.check(lib.ee_debug_ln_rows(_ptr(src), _ptr(dst), _ptr(t["row_src"]), _ptr(t["n"]), max_rows, H or Hc, _ptr(t["g"]), _ptr(t["b"]), R.EPS,
                                        _ptr(dsp), R.SPLIT_SCALE if dsp is not None else 0.0, c.pre_parts, c.stride, _ptr(t["bias"]), _ptr(t["resid"]),
                                        _ptr(t["resid_rows"]), 1.0 / R.SPLIT_SCALE if c.resid is not None else 0.0, C.byref(err), _stream()),
                   None, "ee_debug_ln_rows")
    torch.cuda.synchronize()
    assert err.value == expect_err, f"err_flag {err.value}"
    res = {}
    if out == "inplace":
        _kept(dst, c.src_rows, "dst == src")
        assert torch.equal(dst[n:c.src_rows].view(torch.float32).cpu(), torch.from_numpy(c.parts[0, n:])), "source rows at and past n changed"
        res["dst"], res["dst_words"] = _f32(dst[:n]), dst[:n]
    elif dst is not None:
        _kept(dst, n, "dst")
        res["dst"], res["dst_words"] = _f32(dst[:n]), dst[:n]
    if dsp is not None:
        _kept(dsp, n, "dst_split")
        res["split"] = _decode_split(dsp[:n], Hc, R.SPLIT_SCALE)
    return res


def _ln_check(tag, c, res):
    ref, y32 = R.ln_rows_ref(c), R.ln_rows_f32_torch(c)
    if "dst" in res:
        _check(tag, res["dst"], ref, y32)
        if c.const_ok:      # a constant row: (x - mean) is 0, so the row is beta, whatever the variance made of eps
            assert np.array_equal(res["dst_words"][R.CONST_ROW].cpu().numpy(), c.b.view(np.int32)), "the constant row is not beta"
    if "split" in res:
        _check(tag + " split", res["split"], ref, R.split_yardstick(y32))
        if "dst" in res:
            assert np.array_equal(res["split"], R.split_round(res["dst"].astype(np.float32), R.SPLIT_SCALE)), "split rows are not the split of the f32 rows"


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5])
@pytest.mark.parametrize("H", R.HIDDEN_SIZES)
def test_ln_rows_against_float64(pkg, H, n):
    """The plain form: a gather with repeats, rows past n untouched, f32 / split / both outputs, and dst == src (the BEiT pooler's use)."""
    c = R.LnCase(H, n)
    for out in (("dst", "split", "both") if H % 256 == 0 else ("dst",)):
        _ln_check(f"ln_rows H={H} n={n} {out}", c, _ln(pkg, c, out))
    d = R.LnCase(H, n, gather=False)
    _ln_check(f"ln_rows H={H} n={n} inplace", d, _ln(pkg, d, "inplace"))


@pytest.mark.parametrize("parts", [1, 2, 4, 8])
@pytest.mark.parametrize("H", R.HIDDEN_SIZES)
def test_ln_rows_completes_the_row_from_split_k_parts(pkg, H, parts):
    """The PRE form: parts a stride larger than n H apart, with and without the bias, the split-plane residual gathered, dense and absent."""
    for bias, resid in ((True, "gather"), (False, "dense"), (True, None), (False, "gather")):
        c = R.LnCase(H, 5, pre_parts=parts, bias=bias, resid=resid)
        assert c.stride > c.n * H
        for out in (("dst", "both") if H % 256 == 0 else ("dst",)):
            _ln_check(f"ln_rows H={H} parts={parts} bias={bias} resid={resid} {out}", c, _ln(pkg, c, out))


def test_ln_rows_grid_stride_loop(pkg):
    """More rows than 4 x 8 x CUs at H = 128: every wave takes a second row; max_rows larger than n."""
    cus = _torch().cuda.get_device_properties(0).multi_processor_count
    n = 4 * 8 * cus + 37
    c = R.LnCase(128, n)
    _ln_check(f"ln_rows H=128 n={n}", c, _ln(pkg, c, "dst", max_rows=n + 100))
    d = R.LnCase(128, n, pre_parts=2)
    _ln_check(f"ln_rows H=128 n={n} parts=2", d, _ln(pkg, d, "dst", max_rows=n + 100))


def test_ln_rows_split_overflow_is_flagged(pkg):
    """gamma = 400 in one column: ordinary rows stay below 60000 / 16 there (error word 0); a row that is constant but for that column is
    sqrt(H - 1) deviations out and crosses the limit (bit 16)."""
    c = R.LnCase(256, 5, gather=False)
    c.g[7] = 400.0
    assert np.abs(R.ln_rows_ref(c)).max() * R.SPLIT_SCALE < R.SPLIT_LIMIT
    _ln(pkg, c, "split")
    c.parts[0, 3] = 0.25
    c.parts[0, 3, 7] = 1.0
    assert np.abs(R.ln_rows_ref(c)[3, 7]) * R.SPLIT_SCALE > R.SPLIT_LIMIT
    _ln(pkg, c, "split", expect_err=ERR_SPLIT_OVERFLOW)


def test_the_ln_rows_hook_refuses_what_the_launcher_cannot_take(pkg):
    c = R.LnCase(384, 3)
    with pytest.raises(pkg.capi.MMEEError, match="multiple of 128"):
        _ln(pkg, c, H=192)
    with pytest.raises(pkg.capi.MMEEError, match="multiple of 256"):
        _ln(pkg, c, "split")
    with pytest.raises(pkg.capi.MMEEError, match="max_rows"):
        _ln(pkg, c, n_word=6)
