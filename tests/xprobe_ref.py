"""The X-space CLS probe (csrc/xprobe.hip) restated plainly in numpy float64 (no GPU), with the inputs the probe's tests share.

The reference is the PLAIN form of what the probe computes for the CLS query of a document, deliberately not the kernel's re-association:

    K = X W_k^T + b_k,  V = X W_v^T + b_v                                  (the document's rows X)
    score[h, j] = q[h] . K[j, h] + (w1[h, b1(0, j)] + (wx[h, bx(0, j)] + wy[h, by(0, j)])) / sqrt(d);   masked keys: -inf
    p = softmax over j (max-shifted);   ctx[h] = p[h] @ V[:, h]

q arrives already divided by sqrt(d); buckets, split_round, FACTOR / FLOOR and tolerance() are those of tests/attn_ref.py.  X is pre-rounded
to what its split planes hold (scale 16) and W_v to what ee_finalize's planes hold (weight_scale), so reference, yardstick and kernel read
identical inputs.  The yardstick of a document is the larger of the errors against float64 of (a) the same plain attention in torch float32
and (b) the X-space form in float32 with u, p and c passed through the planes at the kernel's scales (``xspace_f32``); both sides are decoded
through the context planes (scale 64).

``kernel_model`` follows the kernel's own steps in float64 (16-row tiles, copy-of-last-row padding, lazy running maximum, planes of u, p, c,
the three-term products) and takes named MUTATIONS: tests/test_host_xprobe_ref.py uses it to show that the inputs below can see each of
them."""
import math

import numpy as np

from . import attn_ref as R
from .attn_ref import F32, F64, split_round

SCALE_X, SCALE_CTX = 16.0, 64.0             # csrc/mmee_common.h kSplitScaleX, kSplitScaleCtx
LOG2E = 1.44269504088896340736
LAZY, PSHIFT, TILE = 5.0, 10.0, 16          # xprobe_attn_kernel: the maximum moves when exceeded by 2^5, p carries 2^10, 16-row tiles
RING = {12: 3, 16: 2}                       # heads -> depth of the LDS ring (12 x 768, 16 x 1024)
PLANE_TOP = 3700.0                          # 16 x 3700 = 59200 < kSplitClamp = 60000: the top of the X planes' range
EDGE_LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 197, 198, 709)
TILE_MASKED_DOC, PAD_ROWS_DOC = 16, 17      # edge_case: a 49-row document whose tile 1 is masked, a 64-row one with pad rows behind its text
STAIR_MARGIN = 0.05                         # log2 units every staircase step keeps from the lazy threshold


def weight_scale(w):
    """ee_finalize's per-tensor scale (split_weight_exponent in csrc/capi_internal.h): the power of two that puts max |w| in [2^12, 2^13), capped at 2^8."""
    mx = float(np.abs(w).max())
    return 2.0 ** (8 if mx == 0 else min(8, 13 - math.frexp(mx)[1]))


def u_scale(u):
    """xprobe_u_kernel's plane scale of one head's u: the power of two that puts max |s u| in [2^12, 2^13); 1 for u = 0."""
    mx = float(np.abs(np.asarray(u, F32)).max())
    return 1.0 if mx == 0 else 2.0 ** (13 - math.frexp(mx)[1])


def planes(x, scale):
    """(hi, lo) of x's split planes as float64 values (already divided by the scale)."""
    xs = np.asarray(x, dtype=F32) * F32(scale)
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(F32)).astype(np.float16)
    return hi.astype(F64) / scale, lo.astype(F64) / scale


def encode_planes(x, scale):
    """Rows [r, N] as the int32 words of split-f16 rows: 64-byte groups [hi 16 f16 | lo 16 f16]."""
    xs = np.asarray(x, dtype=F32) * F32(scale)
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(F32)).astype(np.float16)
    r, N = xs.shape
    return np.ascontiguousarray(np.stack([hi.reshape(r, N // 16, 16), lo.reshape(r, N // 16, 16)], axis=2)).reshape(r, 2 * N).view(np.int32)


def decode_planes(words, scale):
    h = np.ascontiguousarray(words).view(np.float16).reshape(words.shape[0], -1, 2, 16).astype(F64)
    return (h[:, :, 0] + h[:, :, 1]).reshape(words.shape[0], -1) / scale


class Case:
    """One launch: the stage-0 batch `orig` (an attn_ref.Batch: row integers and tables; its qkv is not used), the stage (doc_orig, x_phys; the
    lengths are the originals'), the rows xs [x_rows, H] float64, qc [n_docs, H] float32 and the weights."""

    def __init__(self, orig, doc_orig, x_phys, xs, qc, w, max_docs=None):
        self.orig, self.heads, self.H = orig, orig.heads, 64 * orig.heads
        self.doc_orig, self.x_phys = np.asarray(doc_orig, np.int32), np.asarray(x_phys, np.int32)
        self.xs, self.qc = xs, np.ascontiguousarray(qc, dtype=F32).reshape(len(self.doc_orig), self.H)
        self.wk, self.bk, self.bv, self.wv = w
        self.lengths = orig.lengths[self.doc_orig].astype(np.int64) if len(self.doc_orig) else np.zeros(0, np.int64)
        self.doc_off = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int32)
        self.max_docs = max(self.n_docs, 1) if max_docs is None else max_docs

    @property
    def n_docs(self):
        return len(self.doc_orig)

    @property
    def ctx_rows(self):
        return max(int(self.doc_off[-1]), 1)

    def X(self, d, first=None):
        f = int(self.x_phys[d]) if first is None else int(first)
        return self.xs[f:f + int(self.lengths[d])]

    def masked(self, d, o=None):
        return self.orig.masked[self.orig.rows(int(self.doc_orig[d]) if o is None else o)] != 0


def bias_rows(orig, o, query=0, swap=False, divide=True):
    """(w1[h, b1] + (wx[h, bx] + wy[h, by])) / sqrt(d) of (query, every key) of original document o: [heads, L] float64."""
    r = orig.rows(o)
    rel = lambda c: c[r].astype(np.int64) - int(c[r][query])
    b1 = R.relative_position_bucket(rel(orig.pos), orig.w1.shape[1], R.MAX_REL_POS)
    bx = R.relative_position_bucket(rel(orig.x0), orig.wx.shape[1], R.MAX_REL_2D_POS)
    by = R.relative_position_bucket(rel(orig.y1), orig.wy.shape[1], R.MAX_REL_2D_POS)
    if swap:
        bx, by = by, bx
    b = orig.w1.astype(F64)[:, b1] + (orig.wx.astype(F64)[:, bx] + orig.wy.astype(F64)[:, by])
    return b / 8.0 if divide else b


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference and the yardsticks
# ---------------------------------------------------------------------------------------------------------------------------------------
def projections(c, d):
    """K, V [L, H] of document d in float64."""
    X = c.X(d)
    return X @ c.wk.astype(F64).T + c.bk.astype(F64), X @ c.wv.astype(F64).T + c.bv.astype(F64)


def reference_doc(c, d):
    """(ctx [H], scores [heads, L], p [heads, L]) of document d: the plain form in float64."""
    nh, L = c.heads, int(c.lengths[d])
    K, V = projections(c, d)
    q = c.qc[d].astype(F64).reshape(nh, 64)
    s = np.einsum("lhd,hd->hl", K.reshape(L, nh, 64), q) + bias_rows(c.orig, int(c.doc_orig[d]))
    s = np.where(c.masked(d)[None, :], -np.inf, s)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    return np.einsum("hl,lhd->hd", p, V.reshape(L, nh, 64)).reshape(c.H), s, p


def xspace_f64(c, d):
    """The re-associated form in float64, no planes: u = W_k^T q, scores = X u + q . b_k + bias, c = sum p x, ctx = W_v c + b_v."""
    nh, H = c.heads, c.H
    X, q = c.X(d), c.qc[d].astype(F64).reshape(nh, 64)
    wk, wv = c.wk.astype(F64).reshape(nh, 64, H), c.wv.astype(F64).reshape(nh, 64, H)
    u = np.einsum("hd,hdc->hc", q, wk)
    s = u @ X.T + (q * c.bk.astype(F64).reshape(nh, 64)).sum(1)[:, None] + bias_rows(c.orig, int(c.doc_orig[d]))
    s = np.where(c.masked(d)[None, :], -np.inf, s)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    cv = (e / e.sum(axis=1, keepdims=True)) @ X
    return (np.einsum("hdc,hc->hd", wv, cv) + c.bv.astype(F64).reshape(nh, 64)).reshape(H)


def plain_f32_torch(c, d):
    """The plain form in torch float32 on the CPU (matmul, softmax, matmul): yardstick (a)."""
    import torch
    nh, L = c.heads, int(c.lengths[d])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=F32))
    X = t(c.X(d))
    K, V = X @ t(c.wk).T + t(c.bk), X @ t(c.wv).T + t(c.bv)
    s = (K.reshape(L, nh, 64).permute(1, 0, 2) @ t(c.qc[d]).reshape(nh, 64, 1))[:, :, 0] + t(bias_rows(c.orig, int(c.doc_orig[d])))
    s = s.masked_fill(torch.from_numpy(c.masked(d))[None, :], float("-inf"))
    out = (torch.softmax(s, dim=-1)[:, None, :] @ V.reshape(L, nh, 64).permute(1, 0, 2))[:, 0, :].reshape(c.H).numpy()
    assert out.dtype == F32
    return out


def xspace_f32(c, d):
    """The X-space form in float32 with u, p and c through the planes at the kernel's scales: yardstick (b)."""
    nh, H = c.heads, c.H
    X = c.X(d).astype(F32)
    bias = bias_rows(c.orig, int(c.doc_orig[d])).astype(F32)
    msk = c.masked(d)
    out = np.zeros(H, F32)
    for h in range(nh):
        sl = slice(64 * h, 64 * h + 64)
        q = c.qc[d][sl]
        u = (c.wk[sl].T @ q).astype(F32)
        u2 = split_round(u, u_scale(u)).astype(F32)
        s = ((X @ u2).astype(F32) + F32(q @ c.bk[sl]) + bias[h]).astype(F32)
        s = np.where(msk, F32(-np.inf), s)
        p = np.exp2(((s - s.max()) * F32(LOG2E)).astype(F32) + F32(PSHIFT)).astype(F32)
        p2 = split_round(p, 1.0).astype(F32)
        cv = ((p2 @ X).astype(F32) / p.sum(dtype=F32)).astype(F32)
        c2 = split_round(cv, SCALE_X).astype(F32)
        out[sl] = (c.wv[sl] @ c2).astype(F32) + c.bv[sl]
    return out


def ctx_planes(x):
    """A context row as its planes hold it (scale 64)."""
    return split_round(x, SCALE_CTX)


def reference(c):
    """[n_docs, H] float64: every document's context row, decoded through the context planes."""
    return np.stack([ctx_planes(reference_doc(c, d)[0]) for d in range(c.n_docs)]) if c.n_docs else np.zeros((0, c.H))


def yardstick(c, ref=None):
    """Per document: the larger error against the reference of the two float32 forms."""
    ref = reference(c) if ref is None else ref
    ea = np.array([np.abs(ctx_planes(plain_f32_torch(c, d)) - ref[d]).max() for d in range(c.n_docs)])
    eb = np.array([np.abs(ctx_planes(xspace_f32(c, d)) - ref[d]).max() for d in range(c.n_docs)])
    return np.maximum(ea, eb)


def order_ref(lengths, ties_reversed=False):
    """xprobe_u_kernel's work order: documents by falling length, ties by rising index."""
    return np.array(sorted(range(len(lengths)), key=lambda d: (-int(lengths[d]), -d if ties_reversed else d)), dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the kernel's steps in float64, with mutations
# ---------------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("u_lo", "p_lo", "c_lo", "no_bv", "bias_q1", "swap_xy", "no_sqrt_d", "pad_weight", "mask_through", "no_acc_rescale", "no_l_rescale",
             "headroom", "slab_d", "rows_at_doc_off", "ctx_row_d", "wave_missing", "tile_ring", "heads_alias")


def lazy_trace(s2, L):
    """Per head and tile of log2-unit scores s2 [heads, L]: (tile maximum - running maximum before the tile); the first tile's entry is +inf."""
    nh = s2.shape[0]
    m_run = np.full(nh, -np.inf)
    out = []
    for t in range((L + TILE - 1) // TILE):
        tmax = s2[:, t * TILE:(t + 1) * TILE].max(axis=1)
        with np.errstate(invalid="ignore"):
            out.append(np.where(np.isfinite(m_run), tmax - m_run, np.inf))
        m_run = np.where(tmax > m_run + LAZY, tmax, m_run)
    return np.array(out).T


def kernel_model(c, d, mut=()):
    """Document d's context row [H] (before the context planes) by the kernel's steps in float64.  mut: names of MUTATIONS."""
    mut = frozenset([mut] if isinstance(mut, str) else mut)
    assert mut <= set(MUTATIONS), mut
    nh, H, L = c.heads, c.H, int(c.lengths[d])
    n_orig = c.orig.n_docs
    o = min(d, n_orig - 1) if "slab_d" in mut else int(c.doc_orig[d])
    X = c.X(d, c.doc_off[d] if "rows_at_doc_off" in mut else None)
    assert X.shape[0] == L, "the mutated read leaves xs: give the case rows behind its last document"
    Xhi = planes(X, SCALE_X)[0]
    q = c.qc[d].astype(F64).reshape(nh, 64)
    # xprobe_u_kernel
    u = np.einsum("hd,hdc->hc", q, c.wk.astype(F64).reshape(nh, 64, H)).astype(F32)
    s0 = (q * c.bk.astype(F64).reshape(nh, 64)).sum(1)
    uh, ul = np.zeros((nh, H)), np.zeros((nh, H))
    for h in range(nh):
        uh[h], ul[h] = planes(u[h], u_scale(u[h]))
    if "u_lo" in mut:
        ul[:] = 0
    if "wave_missing" in mut:              # wave 3's k-steps: columns 3 H / 8 .. 4 H / 8
        uh[:, 3 * H // 8:4 * H // 8] = 0
        ul[:, 3 * H // 8:4 * H // 8] = 0
    # scores in log2 units: x_hi u_hi + x_hi u_lo + x_lo u_hi (no lo x lo term), q . b_k, the bias of query 0, the masked-key sentinel
    dot = Xhi @ (uh + ul).T + (X - Xhi) @ uh.T                                     # [L, heads]
    Lo = int(c.orig.lengths[o])
    bias = np.zeros((nh, L))
    n = min(L, Lo)
    bias[:, :n] = bias_rows(c.orig, o, query=1 if ("bias_q1" in mut and Lo > 1) else 0, swap="swap_xy" in mut, divide="no_sqrt_d" not in mut)[:, :n]
    msk = np.ones(L, bool)                                                        # keys past the slab's document carry the sentinel bucket
    msk[:n] = c.masked(d, o)[:n]
    if "mask_through" in mut:
        msk[:] = False
    s2 = (dot.T + s0[:, None] + bias) * LOG2E
    s2 = np.where(msk[None, :], -np.inf, s2)
    ring = RING[nh]
    n_rt = (L + TILE - 1) // TILE
    acc, l_run, m_run = np.zeros((nh, H)), np.zeros(nh), np.full(nh, -np.inf)
    acc2, l2 = np.zeros((nh, H)), np.zeros(nh)                                      # heads_alias: what the absent heads' lanes would add
    lazy = 8.0 if "headroom" in mut else LAZY
    for t in range(n_rt):
        rows = np.minimum(np.arange(t * TILE, (t + 1) * TILE), L - 1)              # rows past the end: a copy of the last row ...
        st = s2[:, rows].copy()
        if "pad_weight" not in mut:
            st[:, np.arange(t * TILE, (t + 1) * TILE) >= L] = -np.inf              # ... with weight 0
        tmax = st.max(axis=1)
        move = tmax > m_run + lazy
        with np.errstate(invalid="ignore"):
            alpha = np.where(move, np.exp2(np.where(move, m_run - tmax, 0.0)), 1.0)
        m_run = np.where(move, tmax, m_run)
        if "no_l_rescale" not in mut:
            l_run *= alpha
            l2 *= alpha
        if "no_acc_rescale" not in mut:
            acc *= alpha[:, None]
            acc2 *= alpha[:, None]
        p = np.exp2(st - m_run[:, None] + PSHIFT).astype(F32)
        l_run += p.sum(axis=1, dtype=F64)
        p = np.minimum(p, F32(65504.0))                                           # (only the headroom mutation gets there)
        ph, pl = planes(p, 1.0)
        if "p_lo" in mut:
            pl[:] = 0
        xr = rows
        if "tile_ring" in mut and t + ring < n_rt:
            xr = np.minimum(np.arange((t + ring) * TILE, (t + ring + 1) * TILE), L - 1)
        acc += ph @ X[xr] + pl @ Xhi[xr]                                           # p_hi x_hi + p_hi x_lo + p_lo x_hi
        if "heads_alias" in mut and nh == 12:
            # lanes 12 .. 15 hold the u of heads 0 .. 3 and head 0's bias table: their scores, let through into heads 0 .. 3
            sa = (dot.T[:4] + s0[:4, None] + bias[0][None, :]) * LOG2E
            sa = np.where(msk[None, :], -np.inf, sa)[:, rows]
            sa[:, np.arange(t * TILE, (t + 1) * TILE) >= L] = -np.inf
            pa = np.exp2(sa - m_run[:4, None] + PSHIFT)
            l2[:4] += pa.sum(axis=1)
            acc2[:4] += pa @ X[xr]
    cv = ((acc + acc2) / (l_run + l2)[:, None]).astype(F32)
    # xprobe_v_kernel: c through the planes of X, c_hi w_hi + c_hi w_lo + c_lo w_hi, b_v
    ch, cl = planes(cv, SCALE_X)
    if "c_lo" in mut:
        cl[:] = 0
    wv = c.wv.astype(F64).reshape(nh, 64, H)
    wh = planes(c.wv, weight_scale(c.wv))[0].reshape(nh, 64, H)
    y = np.einsum("hdc,hc->hd", wv, ch) + np.einsum("hdc,hc->hd", wh, cl)
    if "no_bv" not in mut:
        y = y + c.bv.astype(F64).reshape(nh, 64)
    return y.reshape(H)


def model_launch(c, mut=()):
    """ctx [ctx_rows, H] of a whole launch by kernel_model (through the context planes); rows nobody writes hold NaN."""
    mut = frozenset([mut] if isinstance(mut, str) else mut)
    ctx = np.full((max(c.ctx_rows, c.n_docs), c.H), np.nan)
    for d in range(c.n_docs):
        ctx[d if "ctx_row_d" in mut else int(c.doc_off[d])] = ctx_planes(kernel_model(c, d, mut - {"ctx_row_d"}))
    return ctx


# ---------------------------------------------------------------------------------------------------------------------------------------
# the inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def make_weights(heads, seed=100):
    """W_k, b_k, b_v float32 and W_v pre-rounded to what ee_finalize's planes hold."""
    rng = np.random.default_rng(seed + heads)
    H = 64 * heads
    wk = (0.03 * rng.standard_normal((H, H))).astype(F32)
    bk, bv = (0.1 * rng.standard_normal(H)).astype(F32), (0.1 * rng.standard_normal(H)).astype(F32)
    wv = (0.03 * rng.standard_normal((H, H))).astype(F32)
    return wk, bk, bv, split_round(wv, weight_scale(wv)).astype(F32)


def make_rows(orig, rng, doc_scale=(1.0, 4.0), fill_masked=True, extra_rows=0):
    """LayerNorm-like rows for every row of `orig` (documents alternate between the magnitudes of doc_scale), masked rows at the top of the
    plane range, pre-rounded to the planes; extra_rows rows of the same kind behind the last document."""
    H = 64 * orig.heads
    rows = int(orig.doc_off[-1])
    x = rng.standard_normal((rows + extra_rows, H))
    for d in range(orig.n_docs):
        x[orig.rows(d)] *= doc_scale[d % len(doc_scale)]
    if fill_masked:
        m = np.nonzero(orig.masked)[0]
        x[m] = PLANE_TOP * np.where(rng.random((len(m), H)) < 0.5, -1.0, 1.0) * (1.0 - 0.01 * rng.random((len(m), H)))
    return split_round(x, SCALE_X)


def identity_case(orig, seed, q_scale=0.35, max_docs=None, **kw):
    """Every document of `orig` in its own order, rows contiguous: what stage 0 of a forward looks like."""
    rng = np.random.default_rng(seed)
    xs = make_rows(orig, rng, **kw)
    qc = (q_scale * rng.standard_normal((orig.n_docs, 64 * orig.heads))).astype(F32)
    return Case(orig, np.arange(orig.n_docs), orig.doc_off[:-1], xs, qc, make_weights(orig.heads), max_docs)


def edge_case(heads):
    """Every edge of the 16-row tile loop and of both rings in one launch: EDGE_LENGTHS with holes from 33 rows on, a 49-row document whose whole
    tile 1 (rows 16 .. 31) is masked, and a 64-row one whose last nine text rows are masked pad rows (MMEE_FLAG_DENSE_ROWS).  The queries of the
    documents shorter than 16 rows are scaled by 0.25 (see below), which also tames what the kernel finds hardest -- a few rows at |x| ~ 4 with
    scores of 30: THAT accuracy risk is carried by count_case (test_document_counts) alone, whose documents keep the full scale."""
    orig = R.make_batch(EDGE_LENGTHS + (49, 64), heads, seed=5, holes=True)
    r = orig.rows(TILE_MASKED_DOC)
    orig.masked[r] = 0
    orig.masked[r.start + 16:r.start + 32] = 1
    r = orig.rows(PAD_ROWS_DOC)
    orig.masked[r] = 0
    orig.masked[r.start + 38:r.start + 47] = 1                     # 47 text rows, then 17 patch rows
    c = identity_case(orig, seed=6)
    c.qc[c.lengths < 16] *= 0.25                                    # no key of a document of a few rows carries a negligible weight
    return c


def without_masked_rows(c):
    """The same launch with the masked rows removed from the batch and from xs (identity cases only)."""
    assert np.array_equal(c.x_phys, c.doc_off[:-1])
    o2, keep = c.orig.without_masked_rows()
    return Case(o2, np.arange(o2.n_docs), o2.doc_off[:-1], c.xs[keep], c.qc, (c.wk, c.bk, c.bv, c.wv), c.max_docs)


STAIR_LEVELS = ((0.0, 4.9, 9.8, 14.9, 19.8, 19.8),             # cumulative: no move, a move (9.8 > 5), a move by 5.1, no move by 4.9
                (0.0, 5.1, 10.0, 310.0, 310.0, 620.0),         # moves just above the threshold, then steps of several hundred: alpha underflows to 0
                (20.0, 15.1, 10.0, 4.9, 0.0, 0.0),             # descending: the maximum never moves after the first tile
                (0.0, 4.9, 0.0, 5.1, 12.1, 5.0))               # up and down around a maximum that lags; a step of 7: p reaches 2^15 without a move
STAIR_LENGTHS = (90, 96, 83, 81)


def staircase_case(heads):
    """attn_ref.staircase_batch with 16-row tiles, driven through u: W_k row 64 h is the unit vector of column 64 h, q[64 h] = 1, so that
    u_h = e_{64 h} (+ noise of 1e-4) and the score of key j is X[j, 64 h] = ln 2 x the level of its tile.  Tile t of document i sits at
    STAIR_LEVELS[i][t] log2 units in the even heads and at the reversed sequence in the odd ones (the heads of a wave then move at different
    tiles); inside a tile one row is at the level, the others up to 3 below.  The tables and the rest of q are tiny."""
    orig = R.make_batch(STAIR_LENGTHS, heads, seed=9, holes=False, table_scale=0.005)
    rng = np.random.default_rng(10)
    H = 64 * heads
    xs = make_rows(orig, rng, doc_scale=(1.0,))
    wk, bk, bv, wv = make_weights(heads)
    wk = wk.copy()
    qc = (0.0003 * rng.standard_normal((orig.n_docs, H))).astype(F32)
    for h in range(heads):
        wk[64 * h] = 0
        wk[:, 64 * h] = 0                                # column 64 h reaches a score through q[64 h] of head h alone
        qc[:, 64 * h] = 1
    wk[64 * np.arange(heads), 64 * np.arange(heads)] = 1
    for d, L in enumerate(STAIR_LENGTHS):
        r = orig.rows(d)
        tile = np.arange(L) // TILE
        for h in range(heads):
            lv = np.array(STAIR_LEVELS[d] if h % 2 == 0 else STAIR_LEVELS[d][::-1])[tile]
            below = 3.0 * rng.random(L)
            below[(np.arange(L) % TILE) == (3 * h + d) % TILE] = 0                 # one row of every full tile at the level
            below[L - 1] = 0 if (L - 1) % TILE < (3 * h + d) % TILE else below[L - 1]     # ... and of the partial last tile
            xs[r, 64 * h] = (lv - below) * math.log(2.0)
    return Case(orig, np.arange(orig.n_docs), orig.doc_off[:-1], split_round(xs, SCALE_X), qc, (wk, bk, bv, wv))


def scale_case(heads):
    """Degenerate plane scales of u: document 0 with q = 0 (u = 0, scale 1: the context is the bias-weighted mean), document 1 with a large
    q (scores in the hundreds), document 2 ordinary; 40, 55 and 33 rows."""
    orig = R.make_batch((40, 55, 33), heads, seed=13, holes=True)
    c = identity_case(orig, seed=14, doc_scale=(1.0,))
    c.qc[0] = 0
    c.qc[1] *= 60.0
    return c


def count_case(heads, n_docs, equal=False):
    """n_docs short documents (1 .. 5 rows; equal: runs of equal lengths, for the tie rule of the rank loop)."""
    rng = np.random.default_rng(1000 + n_docs)
    lengths = (1 + (np.arange(n_docs) // 7) % 3) if equal else rng.integers(1, 6, n_docs)
    orig = R.make_batch(tuple(int(L) for L in lengths), heads, seed=20 + n_docs, holes=False)
    return identity_case(orig, seed=21 + n_docs)


def ticket_case(heads):
    """Nine documents alternating long (709 / 198) and short (1 / 17): with one or two workgroups a short document follows a long one on the
    same LDS ring, bias tables and bucket bytes."""
    return identity_case(R.make_batch((709, 1, 198, 17, 709, 1, 198, 17, 709), heads, seed=30, holes=True), seed=31)


STAGE_ORIG_LENGTHS = (33, 17, 64, 5, 49, 1, 80, 16, 31, 65, 2, 48)
STAGE_DOCS = (9, 2, 11, 0, 6, 4, 7)                       # a shuffled subset of the twelve: doc_orig is not the identity
STAGE_X_PHYS = (400, 0, 700, 130, 200, 70, 320)           # gaps between the documents, not monotone; 64, 48, 33, 80, 49, 16 rows fit
STAGE_X_ROWS = 760


def stage_case(heads, docs=STAGE_DOCS, x_phys=STAGE_X_PHYS):
    """n_orig = 12, the stage a shuffled subset of 7 whose rows lie scattered in xs (every row of xs holds data, the gaps too)."""
    orig = R.make_batch(STAGE_ORIG_LENGTHS, heads, seed=40, holes=True)
    rng = np.random.default_rng(41)
    H = 64 * heads
    xs = split_round(rng.standard_normal((STAGE_X_ROWS, H)), SCALE_X)
    rows = {o: split_round(rng.standard_normal((int(orig.lengths[o]), H)) * (1.0 + 3.0 * (o % 2)), SCALE_X) for o in range(orig.n_docs)}
    qs = {o: (0.35 * rng.standard_normal(H)).astype(F32) for o in range(orig.n_docs)}
    for o, f in zip(docs, x_phys):
        L = int(orig.lengths[o])
        x = rows[o].copy()
        m = orig.masked[orig.rows(o)] != 0
        x[m] = split_round(np.where(x[m] < 0, -PLANE_TOP, PLANE_TOP), SCALE_X)
        xs[f:f + L] = x
    qc = np.stack([qs[o] for o in docs]) if len(docs) else np.zeros((0, H), F32)
    return Case(orig, docs, x_phys, xs, qc, make_weights(heads), max_docs=12)
