"""The row kernels of csrc/prep_embed.hip restated plainly in numpy float64 (no GPU), with the inputs the row-kernel tests share.

    prep     : which text positions become rows of the packed layout (everything up to the last position the mask keeps, row 0 always;
               MMEE_FLAG_DENSE_ROWS keeps all), the position ids of HF:138-146, per row 4 * (position, x0, y1) and the key mask's float bits;
               the visual rows' boxes are create_visual_bbox (HF:575-596).
    embed    : text rows = LayerNorm(word + type + position + cat(x0, y0, x1, y1, h, w rows))  (HF:160-199, 112-136), visual rows =
               LayerNorm_1e-6(cat(cls, patches) + pos_embed)  (EE/models/LayoutLMv3.py:358-373), both through the model-level LayerNorm (:565);
               text_avg (:519-520), vision_avg (:466) and text_visual_concat (:581-582) are means over EVERY position, pads included.
    ln_rows  : LayerNorm(sum of split-K parts + bias + residual row)  (HF:299-303, 508-512).

``mut`` names ONE deliberate fault of a subtly wrong kernel; tests/test_host_rows_ref.py shows that each moves a checked output by at least ten
times what tests/test_gpu_rows.py tolerates.  The ``*_f32_torch`` functions are the same operations in torch float32 on the CPU: the yardstick
whose error against float64 bounds what a float32 kernel may err by.

Every float input lies on a grid of 2^-12 with |x| < 4, so the sum of up to 1024 of them is exact in float32 in ANY order: the mean of a
LayerNorm's input row then carries one rounding (of sum / H) whoever computes it, the kernel's tree of lane sums and torch's own alike.  On rows
whose mean is 50 times their deviation that rounding is the whole error, and without the grid it would be a draw between two summation
orders, not a statement about the kernel.  The second LayerNorm of the embedding path reads the first one's output, arbitrary floats of mean
about 0."""
import numpy as np

from .attn_ref import FACTOR, FLOOR, split_round, tolerance  # noqa: F401  (the acceptance rule and the plane model are the attention tests')

F32, F64 = np.float32, np.float64
GRID = 2.0 ** -12
KEY_MASKED = np.array([-3.0e38], F32).view(np.int32)[0]        # csrc/mmee_common.h kKeyMasked
SPLIT_SCALE = 16.0                                            # csrc/mmee_common.h kSplitScaleX
SPLIT_LIMIT = 60000.0                                         # kSplitClamp: |x * scale| above it raises bit 16
PAD, VOCAB, MAX_2D = 1, 48, 96
EPS, VIS_EPS = 1e-5, 1e-6
N_LARGE = 6                                                   # word rows VOCAB - N_LARGE ... and as many patches: mean 50 x deviation


def on_grid(x, lim=3.9):
    return np.clip(np.round(np.asarray(x, F64) / GRID) * GRID, -lim, lim).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# prep
# ---------------------------------------------------------------------------------------------------------------------------------------
def position_ids(ids, pad, mut=""):
    """HF:138-146: cumsum(ids != pad) * (ids != pad) + pad."""
    m = (ids != pad).astype(np.int64)
    c = np.cumsum(m, axis=1)
    if mut == "posid_no_mask_factor":
        return c + pad
    if mut == "posid_start_at_pad":
        return (c - 1) * m + pad
    return c * m + pad


def visual_boxes(G):
    """HF:575-596: (x0, y1) of the cls box [1, 1, 999, 999] and of the G x G patch boxes, row-major, trunc(1000 k / G)."""
    x0, y1 = [1], [999]
    for py in range(G):
        for px in range(G):
            x0.append(1000 * px // G)
            y1.append(1000 * (py + 1) // G)
    return np.array(x0), np.array(y1)


def prep_ref(ids, mask, bbox, G, pos_ids=None, tt=None, dense_rows=False, pad=PAD, vocab=VOCAB, max_2d=MAX_2D, max_pos=None, type_vocab=1, mut=""):
    """The packed layout and every integer the prep kernels write.  Out-of-range inputs raise bits 1 (id), 2 (bbox), 4 (position), 8 (type) of
    `err`; a position id of the caller outside [0, max_pos) is read as 0, a computed one is capped at max_pos - 1, box coordinates are clamped."""
    ids, bbox = np.asarray(ids, np.int64), np.asarray(bbox, np.int64)
    B, T = ids.shape
    Pv = G * G + 1
    am = np.ones((B, T), np.int64) if mask is None else np.asarray(mask, np.int64)
    err = 0
    if ((ids < 0) | (ids >= vocab)).any():
        err |= 1
    if ((bbox < 0) | (bbox >= max_2d)).any():
        err |= 2
    if tt is not None and ((np.asarray(tt) < 0) | (np.asarray(tt) >= type_vocab)).any():
        err |= 8
    if pos_ids is not None:
        p = np.asarray(pos_ids, np.int64).copy()
        bad = (p < 0) | (p >= max_pos)
        p[bad] = 0
    else:
        p = position_ids(ids, pad, mut)
        bad = p >= max_pos
        p[bad] = max_pos - 1
    if bad.any():
        err |= 4
    text_dst = np.full((B, T), -1, np.int32)
    ntext = np.zeros(B, np.int32)
    vx0, vy1 = visual_boxes(G)
    meta = []
    for b in range(B):
        kept_pos = np.nonzero(am[b] != 0)[0]
        last = int(kept_pos[-1]) if len(kept_pos) else 0
        keep = np.arange(T) <= last
        if dense_rows or mut == "trailing_pads_kept":
            keep[:] = True
        if mut == "hole_dropped":
            keep &= (am[b] != 0) | (np.arange(T) == 0)
        text_dst[b, keep] = np.arange(keep.sum())
        ntext[b] = keep.sum()
        for j in np.nonzero(keep)[0]:
            y1 = bbox[b, j, 1] if mut == "y1_from_bbox1" else bbox[b, j, 3]
            meta.append((4 * j, 4 * min(max(bbox[b, j, 0], 0), max_2d - 1), 4 * min(max(y1, 0), max_2d - 1), 0 if am[b, j] != 0 else KEY_MASKED))
        meta += [(4 * v, 4 * vx0[v], 4 * vy1[v], 0) for v in range(Pv)]
    lens = ntext.astype(np.int64) + Pv
    doc_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return dict(text_dst=text_dst, emb_pos=p.astype(np.int32), ntext=ntext, doc_off=doc_off, x_src=doc_off[:-1].copy(), doc_orig=np.arange(B, dtype=np.int32),
                meta=np.array(meta, np.int64).astype(np.int32).reshape(-1, 4), n_docs=B, n_rows=int(doc_off[-1]), sum_len_sq=int((lens * lens).sum()), err=err)


MASKS = ("full", "null", "trailing", "zero", "hole", "last_only")


def make_prep_inputs(B, T, mask_kind, seed=0):
    """ids in [2, VOCAB) with the pad id where the mask is 0, boxes with independent corners (x1 < x0 in about half), and the mask."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(2, VOCAB, (B, T))
    bbox = rng.integers(0, MAX_2D, (B, T, 4))
    am = np.ones((B, T), np.int64)
    for b in range(B):
        if mask_kind == "trailing":
            am[b, max(1, T - (1 + (5 * b + 3) % T)):] = 0          # different lengths per document
        elif mask_kind == "zero":
            am[b] = 0
        elif mask_kind == "hole":
            am[b, max(1, T - 1 - b % 3):] = 0
            last = int(np.nonzero(am[b])[0][-1])
            if last >= 2:
                am[b, 1 + (7 * b + T // 3) % (last - 1)] = 0           # before the last kept position, never position 0
        elif mask_kind == "last_only":
            am[b, :-1] = 0
    ids[am == 0] = PAD
    return ids, (None if mask_kind == "null" else am), bbox


# ---------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------------------
def layer_norm(x, g, b, eps, mut=""):
    """torch.nn.LayerNorm over the last axis in float64: two passes, biased variance."""
    x = np.asarray(x, F64)
    H = x.shape[-1]
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).sum(-1, keepdims=True) / (H - 1 if mut == "var_h_minus_1" else H)
    if mut == "one_pass_var_f32":
        x32 = x.astype(F32)
        m32 = x32.mean(-1, keepdims=True, dtype=F32)
        var = np.maximum((x32 * x32).mean(-1, keepdims=True, dtype=F32) - m32 * m32, F32(0)).astype(F64)
    return (x - mu) / np.sqrt(var + eps) * np.asarray(g, F64) + np.asarray(b, F64)


def _torch_ln(x, g, b, eps):
    import torch
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), torch.from_numpy(g), torch.from_numpy(b), eps)


# ---------------------------------------------------------------------------------------------------------------------------------------
# embed
# ---------------------------------------------------------------------------------------------------------------------------------------
# hidden size -> (coordinate_size, shape_size) pairs of the kernel tests; 63 / 66, 127 / 130, 171 / 170 take the element-wise spatial path
EMBED_CONFIGS = ((128, 24, 16), (256, 48, 32), (384, 64, 64), (384, 63, 66), (512, 96, 64), (640, 96, 128), (768, 128, 128), (768, 127, 130),
                 (896, 160, 128), (1024, 192, 128), (1024, 171, 170))


class EmbedCase:
    """Tables, LayerNorm vectors and a batch: B = 2, T = 41 (two 32-position chunks, the second a part-filled wave), G = 6 (37 visual rows: past
    the 32-row chunk).  Document 0 ends in 11 pads; document 1 has a hole at position 17 and 3 pads.  Tables ~ 0.02 N(0, 1) as a checkpoint's;
    the last N_LARGE word rows and patches 1, 2, 30 ... 32 of every document have a mean 50 times their deviation."""
    B, T, G = 2, 41, 6

    def __init__(self, H, cs, ss, seed=0, type_vocab=1):
        rng = np.random.default_rng([seed, H, cs])
        B, T, G = self.B, self.T, self.G
        Pv = self.Pv = G * G + 1
        self.H, self.cs, self.ss, self.type_vocab, self.max_pos = H, cs, ss, type_vocab, T + 2
        tab = lambda *shape: on_grid(0.02 * rng.standard_normal(shape))
        self.word, self.type, self.pos = tab(VOCAB, H), tab(type_vocab, H), tab(self.max_pos, H)
        self.word[VOCAB - N_LARGE:] = on_grid(2.0 + 0.04 * rng.standard_normal((N_LARGE, H)))
        self.xtab, self.ytab, self.htab, self.wtab = tab(MAX_2D, cs), tab(MAX_2D, cs), tab(MAX_2D, ss), tab(MAX_2D, ss)
        self.cls_token, self.pos_embed = tab(H), tab(Pv, H)
        self.vis_raw = on_grid(0.05 * rng.standard_normal((B, Pv - 1, H)))
        self.large_patches = np.array([0, 1, 29, 30, 31])                                  # visual rows 1, 2, 30, 31, 32: both chunks
        self.vis_raw[:, self.large_patches] = on_grid(2.0 + 0.04 * rng.standard_normal((B, len(self.large_patches), H)))
        vec = lambda mean, dev: (mean + dev * rng.standard_normal(H)).astype(F32)
        self.text_g, self.text_b, self.vis_g, self.vis_b, self.ln2_g, self.ln2_b = vec(1, .1), vec(0, .05), vec(1, .1), vec(0, .05), vec(1, .1), vec(0, .05)
        self.inputs_embeds = on_grid(0.02 * rng.standard_normal((B, T, H)))
        self.inputs_embeds[:, 3::7] = on_grid(2.0 + 0.04 * rng.standard_normal(self.inputs_embeds[:, 3::7].shape))
        self.ids = rng.integers(2, VOCAB, (B, T))
        self.bbox = rng.integers(0, MAX_2D, (B, T, 4))
        self.tt = rng.integers(0, type_vocab, (B, T))
        self.mask = np.ones((B, T), np.int64)
        self.mask[0, 30:] = 0
        self.mask[1, 17] = 0
        self.mask[1, 38:] = 0
        self.ids[self.mask == 0] = PAD

    def prep(self, dense_rows=False, mut=""):
        return prep_ref(self.ids, self.mask, self.bbox, self.G, tt=self.tt, dense_rows=dense_rows, max_pos=self.max_pos, type_vocab=self.type_vocab, mut=mut)

    def select(self, docs):
        """The documents `docs`, in that order, as a case of their own (same tables)."""
        import copy
        c = copy.copy(self)
        d = list(docs)
        c.B = len(d)
        c.ids, c.bbox, c.tt, c.mask, c.vis_raw, c.inputs_embeds = self.ids[d], self.bbox[d], self.tt[d], self.mask[d], self.vis_raw[d], self.inputs_embeds[d]
        return c


def _spatial_index(c, mut=""):
    bb = c.bbox
    h, w = bb[..., 3] - bb[..., 1], bb[..., 2] - bb[..., 0]
    if mut == "height_from_x":
        h = w
    if mut == "no_clip":
        h, w = h % MAX_2D, w % MAX_2D              # an unclipped index leaves the table: here it wraps, as a negative numpy index does
    else:
        h, w = np.clip(h, 0, MAX_2D - 1), np.clip(w, 0, MAX_2D - 1)
    return bb[..., 0], bb[..., 1], bb[..., 2], bb[..., 3], h, w


def _pack(c, lay, t2, v2):
    """Rows of the packed layout: per document its kept text rows in order, then its visual rows."""
    return np.concatenate([np.concatenate([t2[b][lay["text_dst"][b] >= 0], v2[b]]) for b in range(c.B)])


def embed_ref(c, dense_rows=False, use_embeds=False, mut=""):
    """float64: dict(X packed rows, text / vis / cat pooled vectors (B, H), lay = the prep integers)."""
    lay = c.prep(dense_rows, mut)
    f = lambda a: np.asarray(a, F64)
    x0, y0, x1, y1, h, w = _spatial_index(c, mut)
    htab, wtab = (c.wtab, c.htab) if mut == "hw_swapped" else (c.htab, c.wtab)
    sp = np.concatenate([f(c.xtab)[x0], f(c.ytab)[y0], f(c.xtab)[x1], f(c.ytab)[y1], f(htab)[h], f(wtab)[w]], -1)
    e = (f(c.inputs_embeds) if use_embeds else f(c.word)[c.ids]) + f(c.type)[c.tt] + f(c.pos)[lay["emb_pos"]] + sp
    t1 = layer_norm(e, c.text_g, c.text_b, EPS, mut)
    t2 = layer_norm(t1, c.ln2_g, c.ln2_b, EPS, mut)
    v = np.concatenate([np.broadcast_to(f(c.cls_token), (c.B, 1, c.H)), f(c.vis_raw)], 1) + f(c.pos_embed)
    e1, e2 = (EPS, VIS_EPS) if mut == "eps_swapped" else (VIS_EPS, EPS)
    v1 = layer_norm(v, c.vis_g, c.vis_b, e1, mut)
    v2 = layer_norm(v1, c.ln2_g, c.ln2_b, e2, mut)
    kept = (lay["text_dst"] >= 0)[..., None]
    if mut == "pool_kept_only":
        text, cat = (t1 * kept).sum(1) / c.T, ((t2 * kept).sum(1) + v2.sum(1)) / (c.T + c.Pv)
    elif mut == "pool_div_kept":
        text, cat = t1.sum(1) / kept.sum(1), (t2.sum(1) + v2.sum(1)) / (kept.sum(1) + c.Pv)
    else:
        text, cat = t1.mean(1), np.concatenate([t2, v2], 1).mean(1)
    return dict(X=_pack(c, lay, t2, v2), text=text, vis=v1.mean(1), cat=cat, lay=lay)


def embed_f32_torch(c, dense_rows=False, use_embeds=False):
    """The same embedding rows and pooled vectors in torch float32 on the CPU: the yardstick."""
    import torch
    lay = c.prep(dense_rows)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    x0, y0, x1, y1, h, w = (t(i) for i in _spatial_index(c))
    sp = torch.cat([t(c.xtab)[x0], t(c.ytab)[y0], t(c.xtab)[x1], t(c.ytab)[y1], t(c.htab)[h], t(c.wtab)[w]], -1)
    e = (t(c.inputs_embeds) if use_embeds else t(c.word)[t(c.ids)]) + t(c.type)[t(c.tt)] + t(c.pos)[t(lay["emb_pos"]).long()] + sp
    t1 = _torch_ln(e, c.text_g, c.text_b, EPS)
    t2 = _torch_ln(t1, c.ln2_g, c.ln2_b, EPS)
    v = torch.cat([t(c.cls_token).expand(c.B, 1, c.H), t(c.vis_raw)], 1) + t(c.pos_embed)
    v1 = _torch_ln(v, c.vis_g, c.vis_b, VIS_EPS)
    v2 = _torch_ln(v1, c.ln2_g, c.ln2_b, EPS)
    out = dict(X=_pack(c, lay, t2.numpy(), v2.numpy()), text=t1.mean(1).numpy(), vis=v1.mean(1).numpy(), cat=torch.cat([t2, v2], 1).mean(1).numpy())
    assert all(a.dtype == F32 for a in out.values())
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# ln_rows
# ---------------------------------------------------------------------------------------------------------------------------------------
HIDDEN_SIZES = (128, 256, 384, 512, 640, 768, 896, 1024)
CONST_ROW, CONST_VALUE = 2, 1.5


class LnCase:
    """n output rows gathered (with repeats, out of order) from `src_rows` source rows; pre_parts > 0: split-K parts `stride` floats apart, a bias
    and a residual of its own rows (values a split-f16 plane at scale 16 holds exactly), read through resid_rows or densely.  Output row CONST_ROW
    completes to the constant CONST_VALUE exactly; output rows 1 and 4 have a mean 50 times their deviation."""

    def __init__(self, H, n, pre_parts=0, bias=True, resid="gather", gather=True, seed=0, src_rows=None):
        rng = np.random.default_rng([seed, H, n, pre_parts])
        self.H, self.n, self.pre_parts = H, n, pre_parts
        S = self.src_rows = src_rows or n + 3
        self.stride = S * H + 64 if pre_parts else 0                                        # larger than n * H
        self.row_src = ((5 * np.arange(n) + 2) % max(n - 1, 1)).astype(np.int32) if gather else None      # repeats: n outputs from n - 1 sources
        self.g, self.b = (1 + .1 * rng.standard_normal(H)).astype(F32), (.05 * rng.standard_normal(H)).astype(F32)
        self.bias = on_grid(0.05 * rng.standard_normal(H)) if pre_parts and bias else None
        self.resid = on_grid(0.2 * rng.standard_normal((n + 2, H))) if pre_parts and resid else None
        self.resid_rows = ((3 * np.arange(n) + 1) % (n + 2)).astype(np.int32) if pre_parts and resid == "gather" else None
        parts = on_grid(0.2 * rng.standard_normal((max(pre_parts, 1), S, H)))
        # the target of every output row, then part 0 of its source row = target - everything else (all on the grid: exact)
        target = on_grid(0.3 * rng.standard_normal((n, H)))
        for r in (1, 4):
            if r < n:
                target[r] = on_grid(2.0 + 0.04 * rng.standard_normal(H))
        if CONST_ROW < n:
            target[CONST_ROW] = CONST_VALUE
        src_of = self.row_src if gather else np.arange(n)
        last_writer = {int(src_of[r]): r for r in range(n)}
        self.free = np.array([last_writer[int(src_of[r])] == r for r in range(n)], bool)      # output rows no later row shares a source with: they hold their target
        for r in range(n):
            rest = parts[1:, src_of[r]].astype(F64).sum(0) if pre_parts > 1 else 0.0
            if self.bias is not None:
                rest = rest + self.bias
            if self.resid is not None:
                rest = rest + self.resid[self.resid_rows[r] if self.resid_rows is not None else r]
            parts[0, src_of[r]] = on_grid(target[r] - rest)
        self.parts = parts
        self.const_ok = CONST_ROW < n and bool(self.free[CONST_ROW])

    @property
    def src(self):
        """The source buffer as the kernel reads it: [src_rows, H] rows, or the parts `stride` floats apart."""
        if not self.pre_parts:
            return self.parts[0].ravel().copy()
        flat = np.zeros(self.pre_parts * self.stride, F32)
        for q in range(self.pre_parts):
            flat[q * self.stride:q * self.stride + self.src_rows * self.H] = self.parts[q].ravel()
        return flat

    def rows(self, r):
        return self.row_src[r] if self.row_src is not None else r


def ln_rows_ref(c, mut=""):
    """float64 [n, H]."""
    out = np.zeros((c.n, c.H))
    n_parts = c.pre_parts - 1 if mut == "drop_last_part" and c.pre_parts > 1 else max(c.pre_parts, 1)
    for r in range(c.n):
        x = c.parts[:n_parts, c.rows(r)].astype(F64).sum(0)
        if c.bias is not None:
            x = x + c.bias
        if c.resid is not None:
            rr = c.resid_rows[r] if c.resid_rows is not None and mut != "resid_not_gathered" else r
            x = x + c.resid[rr].astype(F64) * (2.0 if mut == "resid_inv_x2" else 1.0)
        out[r] = layer_norm(x, c.g, c.b, EPS, mut)
    return out


def ln_rows_f32_torch(c):
    """The same in torch float32 on the CPU, parts added in order, then the bias, then the residual: the yardstick."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    out = []
    for r in range(c.n):
        x = t(c.parts[0, c.rows(r)])
        for q in range(1, c.pre_parts):
            x = x + t(c.parts[q, c.rows(r)])
        if c.bias is not None:
            x = x + t(c.bias)
        if c.resid is not None:
            x = x + t(c.resid[c.resid_rows[r] if c.resid_rows is not None else r])
        out.append(_torch_ln(x[None], c.g, c.b, EPS)[0])
    res = torch.stack(out).numpy() if out else np.zeros((0, c.H), F32)
    assert res.dtype == F32
    return res


def per_row_max(x):
    return np.abs(x).max(-1)


def split_yardstick(y32, scale=SPLIT_SCALE):
    """What a split-f16 row holds of the float32 yardstick's values: the yardstick of a split output."""
    return split_round(y32, scale)
