"""One layer's self-attention over ragged documents, restated plainly in numpy float64 (no GPU), with the inputs the attention tests share.

    scores[h, q, k] = Q[q, h] . K[k, h] + (w1[h, b1(pos_k - pos_q)] + (wx[h, b2(x0_k - x0_q)] + wy[h, b2(y1_k - y1_q)])) / sqrt(d)
    masked keys: -inf;  P = softmax over k (max-shifted);  ctx[q, h] = P[h, q] @ V[:, h]

Q arrives already divided by sqrt(d), as the Q | K | V projection of the path writes it (HF:263); the buckets are
``oracle.ee_oracle.relative_position_bucket`` (HF:392-413), the sum order of the bias is HF:268, 455.  ``attention_f32_torch`` is the same
attention in torch float32 on the CPU: the yardstick whose error against float64 bounds what a float32 kernel may err by.

``split_round`` emulates the split-f16 planes of csrc/mmee_common.h exactly; reference, yardstick and kernel all read Q, K, V after
``split_round(., 16)``, so the input quantisation of the split precision is charged to nobody (a kernel's own split of a pre-rounded value
reproduces it exactly)."""
import math

import numpy as np

from oracle.ee_oracle import relative_position_bucket

F32, F64 = np.float32, np.float64
SCALE_QKV, SCALE_CTX = 16.0, 64.0            # csrc/mmee_common.h kSplitScaleQKV, kSplitScaleCtx
BINS = (32, 64)
MAX_REL_POS, MAX_REL_2D_POS = 128, 256
MAX_COORD = 1023
# every edge of the 32-key tile loop and of the 128-query tiles: 19 documents = three rounds of the eight queues, three query tiles at 257
RAGGED_LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 160, 161, 255, 256, 257)


def split_round(x, scale):
    """The value a split-f16 row holds for x: hi = f16(x * s), lo = f16(x * s - hi), (hi + lo) / s; float32 arithmetic as the kernels'."""
    xs = np.asarray(x, dtype=F32) * F32(scale)
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(F32)).astype(np.float16)
    return (hi.astype(F64) + lo.astype(F64)) / scale


class Batch:
    """Ragged documents: qkv [rows, 3 H] float32, doc_off [n + 1], per-row pos / x0 / y1 / masked (int32), tables w1 / wx / wy [heads, bins]."""

    def __init__(self, qkv, doc_off, pos, x0, y1, masked, w1, wx, wy, heads):
        self.qkv, self.doc_off, self.pos, self.x0, self.y1, self.masked = qkv, np.asarray(doc_off, np.int32), pos, x0, y1, masked
        self.w1, self.wx, self.wy, self.heads = w1, wx, wy, heads

    @property
    def n_docs(self):
        return len(self.doc_off) - 1

    @property
    def lengths(self):
        return np.diff(self.doc_off)

    @property
    def max_pos(self):
        return int(self.pos.max())

    def rows(self, d):
        return slice(int(self.doc_off[d]), int(self.doc_off[d + 1]))

    def select(self, docs):
        """The documents `docs`, in that order, as a batch of their own."""
        docs = list(docs)
        idx = np.concatenate([np.arange(self.doc_off[d], self.doc_off[d + 1]) for d in docs])
        off = np.concatenate([[0], np.cumsum([self.lengths[d] for d in docs])])
        return Batch(self.qkv[idx], off, self.pos[idx], self.x0[idx], self.y1[idx], self.masked[idx], self.w1, self.wx, self.wy, self.heads)

    def without_masked_rows(self):
        """The same documents with their masked rows removed (what masking a key must be equivalent to), and the kept rows' old indices."""
        keep = np.nonzero(self.masked == 0)[0]
        doc_of = np.searchsorted(self.doc_off, keep, side="right") - 1
        off = np.concatenate([[0], np.cumsum(np.bincount(doc_of, minlength=self.n_docs))])
        return Batch(self.qkv[keep], off, self.pos[keep], self.x0[keep], self.y1[keep], self.masked[keep], self.w1, self.wx, self.wy, self.heads), keep

    def copy(self):
        return Batch(self.qkv.copy(), self.doc_off.copy(), self.pos.copy(), self.x0.copy(), self.y1.copy(), self.masked.copy(), self.w1, self.wx,
                     self.wy, self.heads)


def make_batch(lengths=RAGGED_LENGTHS, heads=3, seed=0, holes=True, q_scale=0.35, table_scale=1.0):
    """Rows of a document: text positions 2, 3, ... then min(17, L // 2) patch rows renumbered from 0; x0 random, y1 sorted; Q ~ q_scale N(0, 1),
    K, V ~ N(0, 1), tables ~ table_scale N(0, 1); in documents of 33 rows or more about L // 6 keys are masked, never key 0."""
    rng = np.random.default_rng(seed)
    H = 64 * heads
    rows = int(sum(lengths))
    qkv = rng.standard_normal((rows, 3 * H))
    qkv[:, :H] *= q_scale
    pos, x0, y1, masked = (np.zeros(rows, np.int32) for _ in range(4))
    o = 0
    for L in lengths:
        nv = min(17, L // 2)
        nt = L - nv
        pos[o:o + nt] = 2 + np.arange(nt)
        pos[o + nt:o + L] = np.arange(nv)
        x0[o:o + L] = rng.integers(0, 1000, L)
        y1[o:o + nt] = np.sort(rng.integers(0, 1000, nt))
        y1[o + nt:o + L] = np.sort(rng.integers(0, 1000, nv))
        if holes and L >= 33:
            masked[o + rng.choice(np.arange(1, L), size=L // 6, replace=False)] = 1
        o += L
    w1 = (table_scale * rng.standard_normal((heads, BINS[0]))).astype(F32)
    wx = (table_scale * rng.standard_normal((heads, BINS[1]))).astype(F32)
    wy = (table_scale * rng.standard_normal((heads, BINS[1]))).astype(F32)
    off = np.concatenate([[0], np.cumsum(lengths)])
    return Batch(split_round(qkv, SCALE_QKV).astype(F32), off, pos, x0, y1, masked, w1, wx, wy, heads)


def staircase_batch(step, lengths=(96, 161), heads=2, seed=0, only_query=None, flat_after_first=False):
    """Scores whose maximum in key tile t sits `step` (natural-log units) above tile t - 1: Q column 0 of every head is 1, the matching K
    column is step * (key // 32) (flat_after_first: step from tile 1 on), over noise small against the 0.07 between 3.4 and the 2^5 lag of the
    running maximum.  only_query: the staircase in query only_query of every 32-query block alone (a wave-wide vote with per-lane maxima)."""
    b = make_batch(lengths, heads, seed, holes=False, q_scale=0.001, table_scale=0.005)
    H = 64 * heads
    for d in range(b.n_docs):
        r = b.rows(d)
        L = r.stop - r.start
        tile = np.arange(L) // 32
        q = np.ones(L) if only_query is None else (np.arange(L) % 32 == only_query).astype(F64)
        for h in range(heads):
            b.qkv[r, 64 * h] = q
            b.qkv[r, H + 64 * h] = step * (np.minimum(tile, 1) if flat_after_first else tile)
    b.qkv = split_round(b.qkv, SCALE_QKV).astype(F32)
    return b


def _buckets(b, r, b1_hook=None, d=None):
    """(b1, bx, by)[q, k] of the rows r of a batch; relative coordinate = key - query (HF:415-457)."""
    rel = lambda c: c[r].astype(np.int64)[None, :] - c[r].astype(np.int64)[:, None]
    b1 = relative_position_bucket(rel(b.pos), b.w1.shape[1], MAX_REL_POS)
    if b1_hook is not None:
        b1 = b1_hook(d, b1)
    return b1, relative_position_bucket(rel(b.x0), b.wx.shape[1], MAX_REL_2D_POS), relative_position_bucket(rel(b.y1), b.wy.shape[1], MAX_REL_2D_POS)


def attention_doc(b, d, bias=True, b1_hook=None):
    """Document d of a batch in float64: (scores, probabilities, context), shapes (heads, L, L), (heads, L, L), (L, H)."""
    r, nh = b.rows(d), b.heads
    H = b.qkv.shape[1] // 3
    dh = H // nh
    L = r.stop - r.start
    Q, K, V = (b.qkv[r, i * H:(i + 1) * H].astype(F64).reshape(L, nh, dh).transpose(1, 0, 2) for i in range(3))
    s = Q @ K.transpose(0, 2, 1)
    if bias:
        b1, bx, by = _buckets(b, r, b1_hook, d)
        s = s + (b.w1.astype(F64)[:, b1] + (b.wx.astype(F64)[:, bx] + b.wy.astype(F64)[:, by])) / math.sqrt(dh)
    s = np.where(b.masked[r][None, None, :] != 0, -np.inf, s)
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True)
    return s, p, (p @ V).transpose(1, 0, 2).reshape(L, H)


def attention_ref(b, bias=True, b1_hook=None):
    """Context rows [rows, H] of every document, float64."""
    return np.concatenate([attention_doc(b, d, bias, b1_hook)[2] for d in range(b.n_docs)], axis=0)


def attention_f32_torch(b, bias=True):
    """The same attention in torch float32 on the CPU (matmul, softmax, matmul): the yardstick.  Context rows [rows, H] float32."""
    import torch
    nh = b.heads
    H = b.qkv.shape[1] // 3
    dh = H // nh
    out = []
    for d in range(b.n_docs):
        r = b.rows(d)
        L = r.stop - r.start
        Q, K, V = (torch.from_numpy(np.ascontiguousarray(b.qkv[r, i * H:(i + 1) * H])).reshape(L, nh, dh).permute(1, 0, 2) for i in range(3))
        s = Q @ K.transpose(1, 2)
        if bias:
            b1, bx, by = (torch.from_numpy(t) for t in _buckets(b, r))
            w1, wx, wy = (torch.from_numpy(t) for t in (b.w1, b.wx, b.wy))
            s = s + (w1[:, b1] + (wx[:, bx] + wy[:, by])) * torch.tensor(1.0 / math.sqrt(dh), dtype=torch.float32)
        s = s.masked_fill(torch.from_numpy(b.masked[r] != 0)[None, None, :], float("-inf"))
        out.append((torch.softmax(s, dim=-1) @ V).permute(1, 0, 2).reshape(L, H))
    res = torch.cat(out).numpy()
    assert res.dtype == np.float32
    return res


def per_doc_max(b, x):
    """max |x| over the rows of every document."""
    return np.array([np.abs(x[b.rows(d)]).max() for d in range(b.n_docs)])


# The acceptance rule of a kernel against float64 (test_gpu_kernels.py, test_split_gemm_kernel_against_float64): err <= max(FACTOR * err32, FLOOR),
# err32 = the float32 yardstick's error on the same document.
FACTOR, FLOOR = 2.0, 1e-6


def tolerance(err32):
    return np.maximum(FACTOR * np.asarray(err32), FLOOR)
