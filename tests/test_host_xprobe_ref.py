"""The float64 restatement of the X-space CLS probe (tests/xprobe_ref.py), checked without a GPU: it agrees with attn_ref.attention_doc fed the
float64 projections, the re-associated form equals the plain one, the inputs are what their docstrings promise, and they can SEE a subtly wrong
kernel -- every mutation of xprobe_ref.kernel_model below moves the context of the documents it concerns by at least 10 times the tolerance
those documents are held to in tests/test_gpu_xprobe.py (the printout of `moved / tol` is the evidence)."""
import functools

import numpy as np
import pytest

from . import attn_ref as R
from . import xprobe_ref as X

HEADS = [12, 16]


@functools.lru_cache(maxsize=None)
def _case(kind, heads):
    c = getattr(X, kind + "_case")(heads)
    ref = X.reference(c)
    return c, ref, R.tolerance(X.yardstick(c, ref))


@functools.lru_cache(maxsize=None)
def _model(kind, heads):
    return X.model_launch(_case(kind, heads)[0])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", HEADS)
def test_reference_is_row_0_of_the_attention_reference_and_of_the_x_space_form(heads):
    """Row 0 of attn_ref.attention_doc on Q | K | V = (q in row 0 | X W_k^T + b_k | X W_v^T + b_v) in float64 (a float32 Q | K | V would round the
    projections); and the re-associated float64 form equals the plain one to 1e-12 relative, which also pins that q . b_k cancels in the
    softmax: the X-space form carries it, and the same form WITHOUT it gives the same context."""
    c = X.scale_case(heads)
    H = c.H
    for d in range(c.n_docs):
        K, V = X.projections(c, d)
        Q = np.zeros_like(K)
        Q[0] = c.qc[d]
        o = int(c.doc_orig[d])
        r = c.orig.rows(o)
        b = R.Batch(np.concatenate([Q, K, V], axis=1), [0, len(K)], c.orig.pos[r], c.orig.x0[r], c.orig.y1[r], c.orig.masked[r], c.orig.w1, c.orig.wx,
                    c.orig.wy, heads)
        want = R.attention_doc(b, 0)[2][0]
        got = X.reference_doc(c, d)[0]
        scale = np.abs(want).max()
        assert np.abs(got - want).max() <= 1e-12 * scale
        assert np.abs(X.xspace_f64(c, d) - got).max() <= 1e-12 * scale
        c0 = X.Case(c.orig, c.doc_orig, c.x_phys, c.xs, c.qc, (c.wk, np.zeros_like(c.bk), c.bv, c.wv))
        assert np.abs(X.xspace_f64(c0, d) - got).max() <= 1e-12 * scale
    assert not c.qc[0].any() and np.abs(X.reference_doc(c, 1)[1][np.isfinite(X.reference_doc(c, 1)[1])]).max() > 100      # q = 0; scores in the hundreds


def test_planes_round_trip_and_scale_rules():
    rng = np.random.default_rng(2)
    x = R.split_round(rng.standard_normal((5, 768)) * 3, X.SCALE_X)
    assert np.array_equal(X.decode_planes(X.encode_planes(x, X.SCALE_X), X.SCALE_X), x)
    hi, lo = X.planes(x, X.SCALE_X)
    assert np.array_equal(hi + lo, x)
    w = (0.03 * rng.standard_normal((64, 64))).astype(np.float32)
    s = X.weight_scale(w)
    assert s == 256.0 and X.weight_scale(np.zeros(3)) == 256.0 and X.weight_scale(np.array([40.0])) == 128.0       # capped at 2^8; 40 * 128 in [2^12, 2^13)
    assert X.u_scale(np.zeros(4)) == 1.0 and 4096 <= 0.37 * X.u_scale(np.array([0.37, -0.1])) < 8192


# ---------------------------------------------------------------------------------------------------------------------------------------
# the inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", HEADS)
def test_the_inputs_are_what_their_docstrings_promise(heads):
    c = X.edge_case(heads)
    assert tuple(c.lengths[:16]) == X.EDGE_LENGTHS and tuple(c.lengths[16:]) == (49, 64)
    m = c.masked(X.TILE_MASKED_DOC)
    assert m[16:32].all() and m.sum() == 16
    m = c.masked(X.PAD_ROWS_DOC)
    assert m[38:47].all() and m.sum() == 9
    cases = [c, X.staircase_case(heads), X.scale_case(heads), X.ticket_case(heads), X.stage_case(heads)] + [X.count_case(heads, n) for n in (1, 9, 65)]
    for k in cases:
        assert np.array_equal(X.decode_planes(X.encode_planes(k.xs, X.SCALE_X), X.SCALE_X), k.xs)          # the planes hold X exactly
        assert np.array_equal(R.split_round(k.wv, X.weight_scale(k.wv)), k.wv.astype(np.float64))         # ... and W_v
        assert np.abs(k.xs).max() * X.SCALE_X < 60000
        for d in range(k.n_docs):
            assert not k.masked(d)[0]                                                                     # key 0 is never masked
            assert int(k.x_phys[d]) + int(k.lengths[d]) <= len(k.xs)
    for d in range(c.n_docs):                                               # masked rows hold the top of the plane range, the others do not
        big = np.abs(c.X(d)).min(axis=1) > 3600
        assert np.array_equal(big, c.masked(d))
    assert all(c.masked(d).sum() == L // 6 for d, L in enumerate(X.EDGE_LENGTHS) if L >= 33)


@pytest.mark.parametrize("heads", HEADS)
def test_staircase_steps_keep_their_margin_from_the_lazy_threshold(heads):
    """Every (head, tile) of the staircase documents: the tile's maximum sits at least STAIR_MARGIN log2 units away from `running maximum + 5`;
    the designed moves happen: in the even heads of document 0 (0, 4.9, 9.8, 14.9, 19.8, 19.8) tile 1 does not move the maximum, tiles 2 and 3 do,
    tile 4 does not; document 1 steps by 300 (alpha underflows); the even heads of document 2 never move after the first tile."""
    c = X.staircase_case(heads)
    for d in range(c.n_docs):
        s2 = X.reference_doc(c, d)[1] * X.LOG2E
        tr = X.lazy_trace(s2, int(c.lengths[d]))
        assert tr.shape == (heads, 6)
        assert (np.abs(tr[:, 1:] - X.LAZY) >= X.STAIR_MARGIN).all(), (d, tr)
        want = np.array(X.STAIR_LEVELS[d])
        tmax = np.array([s2[:, t * 16:(t + 1) * 16].max(axis=1) for t in range(6)]).T
        tmax -= (c.qc[d].astype(np.float64) * c.bk).reshape(heads, 64).sum(1)[:, None] * X.LOG2E       # q . b_k shifts a head's scores as a whole
        assert np.abs(tmax[0::2] - want).max() < 0.03 and np.abs(tmax[1::2] - want[::-1]).max() < 0.03
        moves = tr[:, 1:] > X.LAZY
        if d == 0:
            assert (moves[0::2] == [False, True, True, False, False]).all()
        if d == 1:
            assert (moves[0::2] == [True, False, True, False, True]).all() and np.exp2(np.float32(-290.0)) == 0
        if d == 2:
            assert not moves[0::2].any() and moves[1::2].any()


@pytest.mark.parametrize("heads", HEADS)
def test_masked_rows_are_equivalent_to_removed_rows(heads):
    """The reference of the edge batch equals the reference of the same batch with its masked rows (and their plane-top data) removed."""
    c, ref, tol = _case("edge", heads)
    c2 = X.without_masked_rows(c)
    assert c2.n_docs == c.n_docs and c2.lengths.sum() == c.lengths.sum() - c.orig.masked.sum() and not c2.orig.masked.any()
    assert np.abs(X.reference(c2) - ref).max() <= 2.0 ** -20            # two float64 sums in another order, through the same planes (lo steps 2^-30)


def test_order_is_by_falling_length_then_rising_index():
    for n in (33, 65):
        L = X.count_case(12, n, equal=True).lengths
        o = X.order_ref(L)
        assert sorted(o) == list(range(n)) and all((L[a], -a) >= (L[b], -b) for a, b in zip(o[:-1], o[1:]))
        assert (np.bincount(L)[1:] >= 7).all()                                              # many equal lengths
        assert not np.array_equal(o, X.order_ref(L, ties_reversed=True))                    # a tie broken the other way shows
    assert list(X.order_ref([2, 5, 2, 5, 1])) == [1, 3, 0, 2, 4]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the inputs can see a subtly wrong kernel
# ---------------------------------------------------------------------------------------------------------------------------------------
def _last_live(c, d):
    return not c.masked(d)[-1]


def _swap_shows(c, d):
    """bx and by of (query 0, key j) differ for some live key, and not by the same bias for all of them (a common shift cancels in the softmax)"""
    o = int(c.doc_orig[d])
    diff = (X.bias_rows(c.orig, o, swap=True) - X.bias_rows(c.orig, o))[:, ~c.masked(d)]
    return bool((np.ptp(diff, axis=1) > 1e-3).all())


# mutation -> (case, the documents it concerns)
TABLE = {
    "u_lo": ("edge", lambda c, d: c.lengths[d] >= 2),
    "p_lo": ("edge", lambda c, d: c.lengths[d] >= 2),
    "c_lo": ("edge", lambda c, d: True),
    "no_bv": ("edge", lambda c, d: True),
    "bias_q1": ("edge", lambda c, d: c.lengths[d] >= 2),
    "swap_xy": ("edge", lambda c, d: _swap_shows(c, d)),
    "no_sqrt_d": ("edge", lambda c, d: c.lengths[d] >= 2),
    "pad_weight": ("edge", lambda c, d: c.lengths[d] >= 2 and c.lengths[d] % 16 != 0 and _last_live(c, d)),
    "mask_through": ("edge", lambda c, d: c.masked(d).any()),
    "wave_missing": ("edge", lambda c, d: c.lengths[d] >= 2),
    "tile_ring": ("edge", lambda c, d: c.lengths[d] > 16 * X.RING[c.heads]),
    "heads_alias": ("edge", lambda c, d: c.heads == 12 and c.lengths[d] >= 2),
    "no_acc_rescale": ("staircase", lambda c, d: True),
    "no_l_rescale": ("staircase", lambda c, d: True),
    "headroom": ("staircase", lambda c, d: d == 3),
    "slab_d": ("stage", lambda c, d: True),
    "rows_at_doc_off": ("stage", lambda c, d: True),
    "ctx_row_d": ("stage", lambda c, d: d >= 1),
}


def test_the_table_names_every_mutation():
    assert set(TABLE) == set(X.MUTATIONS)


@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("kind", ["edge", "staircase", "scale", "stage", "ticket"])
def test_the_unmutated_model_and_the_yardsticks_stay_within_the_rule(kind, heads):
    """kernel_model without a mutation meets the acceptance rule the GPU test applies, on every document of every shared case."""
    c, ref, tol = _case(kind, heads)
    got = _model(kind, heads)[c.doc_off[:-1]]
    err = np.abs(got - ref).max(axis=1)
    print(f"{kind}, {heads} heads: model err / tol per document:", ", ".join(f"L={L}: {e / t:.2f}" for L, e, t in zip(c.lengths, err, tol)))
    assert np.isfinite(ref).all() and (err <= tol).all(), (err / tol).max()


@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("mut", X.MUTATIONS)
def test_a_mutation_moves_the_documents_it_concerns(mut, heads):
    kind, concerns = TABLE[mut]
    c, ref, tol = _case(kind, heads)
    docs = [d for d in range(c.n_docs) if concerns(c, d)]
    if mut == "heads_alias" and heads == 16:
        assert not docs                                   # the 16-head instance has no absent head
        return
    assert docs
    base, got = _model(kind, heads), X.model_launch(c, mut)
    ratios = []
    for d in docs:
        r = int(c.doc_off[d])
        with np.errstate(invalid="ignore"):
            diff = np.abs(got[r] - base[r])
        moved = np.inf if np.isnan(diff).any() else float(diff.max())
        ratios.append(moved / float(tol[d]))
    print(f"{mut}, {heads} heads: moved / tol per document:", ", ".join(f"L={c.lengths[d]}: {x:.3g}" for d, x in zip(docs, ratios)))
    assert min(ratios) >= 10, (mut, [(int(c.lengths[d]), x) for d, x in zip(docs, ratios) if x < 10])
