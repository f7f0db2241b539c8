"""The three fused attention kernels alone (csrc/attention_f32.hip, attention_pair.hip, attention_idx.hip) through ee_debug_attention, against
the float64 restatement of tests/attn_ref.py, at every edge of the 32-key tile loop and of the 128-query tiles.

Acceptance rule, per document (as test_gpu_kernels.py for the GEMMs): max |ctx - ref64| <= max(FACTOR * err32, 1e-6), err32 = the error of the
same attention in torch float32 on the CPU.  FACTOR = 2 is the project's convention; tests/test_host_attention_ref.py shows that every mutation
of a subtly wrong kernel moves every document by at least 100 times that tolerance.  Reference, yardstick and kernel read the same Q, K, V,
pre-rounded to what the split planes hold (attn_ref.split_round), and the split kernels' context is decoded from its planes in float64, so the
rule charges a kernel for its own arithmetic only.

Bit-identity properties carry no tolerance: a document's context does not depend on its neighbours, on the order of the batch, on the work
queues, on q_limit or on where its Q | K | V rows lie."""
import ctypes as C
import functools

import numpy as np
import pytest

from . import attn_ref as R
from .conftest import report_measured
from .hook_util import ERR_SPLIT_OVERFLOW, SENTINEL, _decode_split, _dev, _ptr, _stream, _torch

pytestmark = pytest.mark.gpu

F32K, PAIR, IDX, NOBIAS = 0, 1, 2, 3                    # include/mmee.h MMEE_ATTN_KERNEL_*
NAMES = {F32K: "f32", PAIR: "pair", IDX: "idx", NOBIAS: "idx_nobias"}
SPLIT_KERNELS = [PAIR, IDX, NOBIAS]
MASKING_KERNELS = [F32K, PAIR, IDX]                     # the image-only form of attention_idx has no key mask
GUARD = 8                                               # rows past the last one in every context buffer; they must keep SENTINEL's bits
kid = lambda k: NAMES[k]


def _launch(pkg, b, kernel, queue=1, q_limit=0, qkv=None, qkv_doc_off=None, terms=3, expect_err=0, **over):
    """One ee_debug_attention call on batch b.  Returns the context rows as the kernel wrote them (int32 words [rows, H], on the device)."""
    torch = _torch()
    H = 64 * b.heads
    rows = int(b.doc_off[-1])
    t_qkv = _dev(b.qkv if qkv is None else qkv, torch.float32)
    t = [_dev(a, torch.int32) for a in (b.doc_off, b.pos, b.x0, b.y1, b.masked)]
    t_qoff = None if qkv_doc_off is None else _dev(qkv_doc_off, torch.int32)
    w = [None] * 3 if kernel == NOBIAS else [_dev(a, torch.float32) for a in (b.w1, b.wx, b.wy)]
    ctx = torch.full((rows + GUARD, H), SENTINEL, dtype=torch.int32, device="cuda")
    err = C.c_int32(-1)
    a = dict(bins1=b.w1.shape[1], bins2=b.wx.shape[1], max_rel_pos=R.MAX_REL_POS, max_rel_2d_pos=R.MAX_REL_2D_POS, max_pos=b.max_pos,
             max_coord=R.MAX_COORD)
    a.update(over)
    lib = pkg.capi.load()
    pkg.capi.check(lib.ee_debug_attention(_ptr(t_qkv), t_qkv.shape[0], _ptr(t[0]), b.n_docs, _ptr(t_qoff), *[_ptr(x) for x in t[1:] + w], b.heads, a["bins1"],
                                          a["bins2"], a["max_rel_pos"], a["max_rel_2d_pos"], a["max_pos"], a["max_coord"], kernel, queue, q_limit, terms,
                                          _ptr(ctx), C.byref(err), _stream()),
                   None, "ee_debug_attention")
    torch.cuda.synchronize()
    assert err.value == expect_err, f"err_flag {err.value}"
    assert torch.equal(ctx[rows:], torch.full_like(ctx[rows:], SENTINEL)), "a write past the last row"
    return ctx[:rows]


def _values(words, kernel, heads):
    torch = _torch()
    v = words.view(torch.float32).double() if kernel == F32K else _decode_split(words, 64 * heads, R.SCALE_CTX)
    return v.cpu().numpy()


def _reference(b, bias):
    ref = R.attention_ref(b, bias=bias)
    return ref, R.per_doc_max(b, R.attention_f32_torch(b, bias=bias).astype(np.float64) - ref)


@functools.lru_cache(maxsize=None)
def _ragged(heads, kernel_has_bias):
    """The ragged batch (its holes only where the kernel has a key mask), its float64 reference and the yardstick's error per document: computed
    once, shared by every test, never written to."""
    b = R.make_batch(heads=heads, holes=kernel_has_bias)
    return (b,) + _reference(b, kernel_has_bias)


def _check(tag, b, got, ref, err32, rows=None):
    """The acceptance rule on every document; every err / err32 is recorded before the assertion."""
    bad = []
    for d, L in enumerate(b.lengths):
        r = b.rows(d) if rows is None else rows[d]
        err = float(np.abs(got[r] - ref[r]).max())
        tol = float(R.tolerance(err32[d]))
        report_measured(f"attention[{tag},L={L}]", f"max|err| (err32 {err32[d]:.3e}, err / err32 {err / max(err32[d], 1e-30):.2f}, err / tol {err / tol:.2f})", err)
        if not err <= tol:
            bad.append((int(L), err, float(err32[d])))
    assert not np.isnan(got).any()
    assert not bad, (tag, bad)


# ---------------------------------------------------------------------------------------------------------------------------------------
# accuracy
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("queue", [1, 0], ids=["queue", "static"])
@pytest.mark.parametrize("heads", [3, 2], ids=["heads3", "heads2"])
@pytest.mark.parametrize("kernel", [F32K, PAIR, IDX, NOBIAS], ids=kid)
def test_attention_kernel_against_float64(pkg, kernel, heads, queue):
    """Lengths 1 ... 257 in one launch: 1-9 key tiles, exact multiples of 32, a third query tile that holds one query; three heads (the pair
    kernel's one-head items) and two (its two-head items); holes in the documents of 33 rows and more."""
    b, ref, err32 = _ragged(heads, kernel != NOBIAS)
    got = _values(_launch(pkg, b, kernel, queue), kernel, heads)
    _check(f"{NAMES[kernel]},heads={heads},queue={queue}", b, got, ref, err32)


def test_pair_kernel_masks_holes_inside_full_key_tiles(pkg):
    """attention_pair takes its fast tiles (which never read the key flags) only in documents without a masked key: holes inside FULL key tiles,
    launched as the forward launches the kernel without dense rows.  The kernel-level twin of
    test_gpu_parity.py::test_wide_bucket_tables_mask_holes_in_full_key_tiles."""
    for heads in (3, 2):
        b, ref, err32 = _ragged(heads, True)
        inside = [int(((np.nonzero(b.masked[b.rows(d)])[0] // 32 + 1) * 32 <= L).sum()) for d, L in enumerate(b.lengths)]
        assert sum(1 for n in inside if n) >= 10, inside                       # holes in whole tiles, in most documents
        assert all(b.masked[b.rows(d)].sum() == 0 for d, L in enumerate(b.lengths) if L < 33)      # and documents that keep the fast tiles
        got = _values(_launch(pkg, b, PAIR), PAIR, heads)
        _check(f"pair holes,heads={heads}", b, got, ref, err32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# bit identity
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [F32K, PAIR, IDX, NOBIAS], ids=kid)
def test_a_documents_context_does_not_depend_on_the_batch(pkg, kernel):
    """A document alone = that document inside the batch; the batch reversed = the same bits per document; work queues = static grid."""
    torch = _torch()
    b = _ragged(3, kernel != NOBIAS)[0]
    full = _launch(pkg, b, kernel, 1)
    assert torch.equal(full, _launch(pkg, b, kernel, 0)), "work queues and static grid differ"
    assert torch.equal(full, _launch(pkg, b, kernel, 1)), "two launches differ"
    order = list(range(b.n_docs))[::-1]
    rev = _launch(pkg, b.select(order), kernel, 1)
    o = 0
    for d in order:
        r = b.rows(d)
        L = r.stop - r.start
        assert torch.equal(rev[o:o + L], full[r]), f"document of {L} rows differs in the reversed batch"
        o += L
        alone = _launch(pkg, b.select([d]), kernel, d & 1)
        assert torch.equal(alone, full[r]), f"document of {L} rows alone differs from the batch"


@pytest.mark.parametrize("kernel", SPLIT_KERNELS, ids=kid)
def test_q_limit_writes_the_first_block_only(pkg, kernel):
    """q_limit = 32 (the CLS probe's launch): the first 32 rows of every document carry the bits of the full run, every other row keeps the
    sentinel."""
    torch = _torch()
    b = _ragged(3, kernel != NOBIAS)[0]
    full, lim = _launch(pkg, b, kernel), _launch(pkg, b, kernel, q_limit=32)
    for d, L in enumerate(b.lengths):
        r = b.rows(d)
        n = min(32, int(L))
        assert torch.equal(lim[r.start:r.start + n], full[r.start:r.start + n]), L
        assert torch.equal(lim[r.start + n:r.stop], torch.full_like(lim[r.start + n:r.stop], SENTINEL)), L


@pytest.mark.parametrize("kernel", SPLIT_KERNELS, ids=kid)
def test_qkv_rows_laid_out_with_gaps(pkg, kernel):
    """qkv_doc_off (a probe-first layer reads Q | K | V in the previous stage's numbering): rows with gaps between the documents give the bits
    of the dense layout."""
    torch = _torch()
    b = _ragged(2, kernel != NOBIAS)[0]
    gaps = np.array([3 + 5 * (d % 4) for d in range(b.n_docs)])
    qoff = b.doc_off[:-1] + np.cumsum(gaps)
    qkv = np.full((int(b.doc_off[-1] + gaps.sum() + 7), b.qkv.shape[1]), 777.0, np.float32)
    for d in range(b.n_docs):
        qkv[qoff[d]:qoff[d] + b.lengths[d]] = b.qkv[b.rows(d)]
    assert torch.equal(_launch(pkg, b, kernel, qkv=qkv, qkv_doc_off=qoff), _launch(pkg, b, kernel))


@pytest.mark.parametrize("kernel", MASKING_KERNELS, ids=kid)
def test_masked_keys_are_removed_rows(pkg, kernel):
    """Masking a key = the document without that row (a tolerance, not bits: the tiles differ).  Separates the mask from everything else: the
    kept rows of the run WITHOUT the masked rows are held to the reference of the run with them."""
    b, ref, err32 = _ragged(3, True)
    small, keep = b.without_masked_rows()
    got = _values(_launch(pkg, small, kernel), kernel, 3)
    _check(f"{NAMES[kernel]},masked rows removed", small, got, ref[keep], err32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# softmax edges: the lazy rescaling of the split kernels at its threshold
# ---------------------------------------------------------------------------------------------------------------------------------------
STAIRS = {
    "step4.0": dict(step=4.0),                               # above the 2^5 lag (5 ln 2 = 3.47): the reference maximum moves in every tile
    "step3.0": dict(step=3.0),                               # moves it every second tile
    "step3.4_once": dict(step=3.4, flat_after_first=True),   # never moves it: probabilities reach 2^10 e^3.4 ~ 2^15 in the f16 hi plane
    "step-40": dict(step=-40.0),                             # everything after tile 0 underflows
    "step4.0_query5": dict(step=4.0, only_query=5),          # one lane of a wave crosses the threshold: a wave-wide vote with per-lane maxima
}


@functools.lru_cache(maxsize=None)
def _stairs(name):
    b = R.staircase_batch(**STAIRS[name])
    return (b,) + _reference(b, True)


@pytest.mark.parametrize("name", list(STAIRS))
@pytest.mark.parametrize("kernel", [PAIR, IDX], ids=kid)
def test_lazy_rescaling_at_its_threshold(pkg, kernel, name):
    """Documents of 96 and 161 rows (3 and 6 key tiles), two heads, the maximum of key tile t a fixed step above tile t - 1."""
    b, ref, err32 = _stairs(name)
    s = R.attention_doc(b, 1)[0]
    tile_max = np.stack([s[:, :, 32 * t:32 * t + 32].max(-1) for t in range(6)], -1)        # [head, query, key tile]
    lag = 5 * np.log(2)
    if name == "step4.0":
        assert (np.diff(tile_max, axis=-1) > lag).all()
    if name == "step3.4_once":
        assert (tile_max[..., 1:] - tile_max[..., :1] < lag).all() and (tile_max[..., 1] - tile_max[..., 0] > 3.3).all()
    if name == "step4.0_query5":
        assert ((np.diff(tile_max, axis=-1) > lag).all(-1) == (np.arange(s.shape[1]) % 32 == 5)).all()
    got = _values(_launch(pkg, b, kernel), kernel, 2)
    _check(f"{NAMES[kernel]},{name}", b, got, ref, err32)


@pytest.mark.parametrize("kernel", [PAIR, IDX], ids=kid)
def test_context_overflow_is_flagged(pkg, kernel):
    """V = 2000 fits the Q | K | V planes at scale 16 (32000) and not the context planes at 64 (128000 > 65504): kErrSplitOverflow."""
    b = R.make_batch((96, 161), heads=2, holes=False)
    b.qkv[:, 2 * 128:] = 2000.0
    _launch(pkg, b, kernel, expect_err=ERR_SPLIT_OVERFLOW)


# ---------------------------------------------------------------------------------------------------------------------------------------
# masks at the front
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _front():
    b = R.make_batch((97, 97), heads=2, holes=False, seed=5)
    b.masked[1:41] = 1                 # key tile 0 keeps the CLS key alone, tile 1 starts masked
    b.masked[97:97 + 41] = 1           # key 0 masked as well (left padding): the first key tile is all masked
    return (b,) + _reference(b, True)


@pytest.mark.parametrize("kernel", MASKING_KERNELS, ids=kid)
def test_masks_at_the_front(pkg, kernel):
    """Keys 1 .. 40 masked (tile 0 keeps the CLS key alone), and keys 0 .. 40 masked (left padding: the first key tile is ALL masked).  The
    second document is the regression test of a fault this file found: with the running maximum started AT the masked-key sentinel, the
    split kernels formed the tile's exponents as the difference of two products of 1e30 rounded apart and left inf, then NaN, in the
    context (attention_idx: NaN; attention_pair: max |err| 940).  csrc/attention_idx.hip, attention_pair.hip: kMrefInit."""
    b, ref, err32 = _front()
    got = _values(_launch(pkg, b, kernel), kernel, 2)
    _check(f"{NAMES[kernel]},front masks", b, got, ref, err32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# what the hook refuses
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_hook_refuses_what_the_kernels_do_not_support(pkg):
    b = R.make_batch((33, 64), heads=2)
    with pytest.raises(pkg.capi.MMEEError, match="64 bins"):
        wide = b.copy()
        wide.w1 = np.zeros((2, 128), np.float32)
        _launch(pkg, wide, IDX)
    with pytest.raises(pkg.capi.MMEEError, match="Delta tables"):
        _launch(pkg, b, PAIR, max_rel_pos=129, max_pos=200)
    with pytest.raises(pkg.capi.MMEEError, match="q_limit"):
        _launch(pkg, b, F32K, q_limit=32)
    with pytest.raises(pkg.capi.MMEEError, match="no key mask"):
        _launch(pkg, b, NOBIAS)
    with pytest.raises(pkg.capi.MMEEError, match="terms"):
        _launch(pkg, b, PAIR, terms=1)
    with pytest.raises(pkg.capi.MMEEError, match="max_pos"):
        _launch(pkg, b, IDX, max_pos=3)
