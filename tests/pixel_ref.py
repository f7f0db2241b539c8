"""The pixel path restated plainly in numpy (no GPU), with the inputs the pixel tests share: page bytes -> ee_preprocess_images ->
pixel_values -> patch rows -> patch projection, and the collation beside it.

    resize      oracle.pil_bilinear_resize_u8 (Pillow's 8-bit BILINEAR) and oracle.rescale_normalize_lut: ``resize_ref``
    collation   a plain loop: ``collate_ref``
    projection  im2col as reshape + transpose, the way oracle.forward_all_beit writes it, then ``A @ W.T + b`` in float64: ``project_ref``;
                ``project_f32_torch`` is the same product in torch float32 on the CPU, the yardstick whose error against float64 bounds what a
                float32 kernel may err by (the acceptance rule of tests/attn_ref.py: per row, err <= max(2 err32, 1e-6))
    split rows  what launch_patch_split leaves of the patches: ``split_round`` of them at kSplitScaleX; ``split_words`` are those values as the
                32-bit words of the planes (hook_util._encode_split)

Beside each reference stands a model of the KERNEL's arithmetic with a switch per subtle fault (``resize_model``, ``collate_model``,
``im2col_model``): without a switch it must equal the reference, with one it shows what a kernel with that fault would write, so that
tests/test_host_pixel_ref.py can assert that the inputs of tests/test_gpu_pixel.py see the fault."""
import numpy as np

from oracle.ee_oracle import pil_bilinear_resize_u8, rescale_normalize_lut

from .attn_ref import FACTOR, FLOOR, split_round, tolerance  # noqa: F401  (the acceptance rule and the plane model are the attention tests')
from .hook_util import _encode_split

F32, F64 = np.float32, np.float64
SPLIT_SCALE = 16.0                                            # csrc/mmee_common.h kSplitScaleX
SPLIT_LIMIT = 60000.0                                         # kSplitClamp: |x * scale| above it raises bit 16
KMAX, MAX_RATIO = 64, 31                                      # csrc/capi_tools.hip: taps per output pixel, and the ratio they are sized for
PRECISION_BITS = 32 - 8 - 2                                   # libImaging/Resample.c
GUARD = 3                                                     # sentinel rows behind every output
TILE = 128                                                    # rows of an f32 GEMM tile (csrc/gemm_f32.hip BM)


# ---------------------------------------------------------------------------------------------------------------------------------------
# resize
# ---------------------------------------------------------------------------------------------------------------------------------------
# (R, [(h, w, c), ...]): every single-page case of tests/test_gpu_pixel.py
RESIZE_SHAPES = [
    (224, [(1, 1, 1), (1, 1, 3), (2, 3, 3), (1, 500, 1), (500, 1, 3)]),                                              # tiny sides
    (224, [(223, 225, 3), (225, 223, 1), (224, 224, 1), (447, 449, 3), (448, 448, 1), (112, 112, 3)]),               # around identity
    (224, [(1171, 224, 3), (2400, 230, 1)]),                              # the horizontal kernel's second and third grid-stride sweep
    (224, [(8, 6944, 3), (6944, 8, 1)]),                                  # the 31 x limit on one axis
    (32, [(992, 992, 1), (33, 65, 3), (640, 480, 3), (992, 8, 3)]),       # the limit on both axes; a vertical-first page in colour
    (1, [(31, 31, 3)]), (3, [(93, 93, 1)]), (7, [(17, 5, 3)]),
]
RESIZE_CASES = [(R, s) for R, shapes in RESIZE_SHAPES for s in shapes]
MIXED_CALL = (224, [(300, 224, 1), (2400, 230, 1), (1, 1, 3), (1171, 224, 3), (2, 3, 3)])      # the tallest page not first, short after tall, grey and RGB
# what tests/golden/preprocess_edges.npz holds of Pillow's own outputs: the small-R shapes and a few thin ones at R = 224
GOLDEN_CASES = [(R, s) for R, s in RESIZE_CASES if R < 224] + [(224, s) for s in ((1, 1, 1), (1, 1, 3), (2, 3, 3), (1, 500, 1), (500, 1, 3), (6944, 8, 1))]


def page_seed(R, shape):
    h, w, c = shape
    return 7000 + 131 * R + 17 * h + 5 * w + c


def make_page(synth, R, shape):
    """The page of a case, from its seed (synth.make_page_image): (h, w) uint8 greyscale or (h, w, 3)."""
    h, w, c = shape
    return synth.make_page_image(page_seed(R, shape), h, w, c)


def as_rgb(img):
    return img if img.ndim == 3 else np.repeat(img[:, :, None], 3, axis=2)          # Image.convert("RGB") of an "L" page


def resize_ref(img, R):
    """(resized_u8 [R, R, 3], pixel_values [3, R, R] float32) of one page."""
    u8 = pil_bilinear_resize_u8(as_rgb(img), R, R)
    return u8, rescale_normalize_lut()[u8].transpose(2, 0, 1).copy()


def pack_pages(pages, align=1, lead=0):
    """The pages back to back (every start rounded up to `align`, the first at `lead`): (bytes, [(offset, h, w, c)])."""
    chunks, desc, off = [np.zeros(lead, np.uint8)], [], lead
    for im in pages:
        pad = -off % align
        chunks.append(np.zeros(pad, np.uint8))
        off += pad
        desc.append((off, im.shape[0], im.shape[1], 1 if im.ndim == 2 else 3))
        chunks.append(np.ascontiguousarray(im).reshape(-1))
        off += im.size
    return np.concatenate(chunks), desc


RESIZE_FAULTS = ("no_rounding", "plane_stride_h", "xmax_unclipped", "unnormalised", "grey_channel0_only", "horizontal_always")


def vertical_first(h, w, R):
    """Image.resize's rule (PIL/Image.py): a page more than 100 times as tall as wide that shrinks vertically takes the vertical pass first."""
    return h > 100 * w and R < h


def _coeffs(in_size, R, mut):
    """resize_coeffs_kernel: per output index (xmin, n) and the n fixed-point taps."""
    scale = in_size / R
    support = max(scale, 1.0)
    ss = 1.0 / support
    out = []
    for xx in range(R):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = int(center + support + 0.5)
        if mut != "xmax_unclipped":
            xmax = min(xmax, in_size)
        n = min(xmax - xmin, KMAX)
        w = [max(1.0 - abs((x + xmin - center + 0.5) * ss), 0.0) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0 and mut != "unnormalised":
            w = [v / ww for v in w]
        out.append((xmin, np.array([int(0.5 + v * (1 << PRECISION_BITS)) for v in w], np.int64)))
    return out


def _clip8(acc):
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_model(pages, R, mut="", align=1, lead=0):
    """One ee_preprocess_images call as the kernels compute it: the packed byte buffer, the tap tables, the horizontal pass into tmp (rows of
    R x 3 bytes, plane stride max_h) and the vertical pass out of it.  Returns resized_u8 [B, R, R, 3]."""
    buf, desc = pack_pages(pages, align, lead)
    buf = np.concatenate([buf, np.zeros(3 * (KMAX + 2) + 16, np.uint8)]).astype(np.int64)          # what an unclipped tap reads past the last page
    B, max_h = len(pages), max(d[1] for d in desc)
    tmp = np.zeros((B * max_h + 2 * KMAX, R * 3), np.int64)
    rnd = 0 if mut == "no_rounding" else 1 << (PRECISION_BITS - 1)
    out = np.zeros((B, R, R, 3), np.uint8)
    for d, (off, h, w, c) in enumerate(desc):
        if vertical_first(h, w, R) and mut != "horizontal_always":          # straight from the page, then along the rows of w pixels
            src = buf[off:off + h * w * c].reshape(h, w, c)
            mid = np.stack([_clip8((src[ymin:ymin + len(k)] * k[:, None, None]).sum(0) + rnd) for ymin, k in _coeffs(h, R, mut)]).astype(np.int64)
            for xx, (xmin, k) in enumerate(_coeffs(w, R, mut)):
                taps = mid[:, xmin:xmin + len(k)]
                out[d, :, xx] = _clip8((taps * k[None, :taps.shape[1], None]).sum(1) + rnd)          # (R, c) into 3 channels
            continue
        rows = tmp[d * max_h:d * max_h + h].reshape(h, R, 3)
        ys = np.arange(h)[:, None]
        for xx, (xmin, k) in enumerate(_coeffs(w, R, mut)):
            x = np.arange(len(k))[None, :]
            if c == 1:
                v = _clip8((buf[off + ys * w + xmin + x] * k).sum(1) + rnd)
                rows[:, xx, 0] = v
                if mut != "grey_channel0_only":
                    rows[:, xx, 1] = rows[:, xx, 2] = v
            else:
                for ch in range(3):
                    rows[:, xx, ch] = _clip8((buf[off + (ys * w + xmin + x) * 3 + ch] * k).sum(1) + rnd)
        plane = h if mut == "plane_stride_h" else max_h
        for yy, (ymin, k) in enumerate(_coeffs(h, R, mut)):
            out[d, yy] = _clip8((tmp[d * plane + ymin:d * plane + ymin + len(k)] * k[:, None]).sum(0) + rnd).reshape(R, 3)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# collation
# ---------------------------------------------------------------------------------------------------------------------------------------
COLLATE_T = (1, 255, 256, 257, 512)
COLLATE_B = (1, 7)
COLLATE_PAD = (1, -7, 1 << 40)
COLLATE_FAULTS = ("truncate_t_minus_1", "pad_id_32_bits", "boxes_32_bits")
BIG = 1 << 33                                                 # ids and boxes at and above it


def collate_lengths(B, T):
    """Document lengths: an empty document first and last (B = 1: the one document is empty in a case of its own), and 1, T - 1, T, T + 1, 5 T."""
    if B == 1:
        return [[0], [1], [T - 1], [T], [T + 1], [5 * T]]
    return [[0, 1, T - 1, T, T + 1, 5 * T, 0][:B]]


def collate_inputs(lengths, seed):
    """Ragged ids [total] and boxes [total, 4] (int64, every fifth value at or above 2^33, some negative) and offsets [B + 1]."""
    rng = np.random.default_rng(seed)
    total = int(sum(lengths))
    ids = rng.integers(0, 50000, max(total, 1)).astype(np.int64)
    boxes = rng.integers(0, 1001, (max(total, 1), 4)).astype(np.int64)
    ids[::5] += BIG * rng.integers(1, 1 << 20, len(ids[::5]))
    boxes[::5] += BIG * rng.integers(1, 1 << 20, boxes[::5].shape)
    ids[1::7] *= -1
    return ids, boxes, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def _low32(v):
    return int(np.array([v], np.int64).astype(np.int32)[0])


def collate_model(ids, boxes, offsets, T, pad_id, mut=""):
    """DataCollatorWithPadding(padding="max_length") with truncation, as a loop: (input_ids [B, T], attention_mask [B, T], bbox [B, T, 4])."""
    B = len(offsets) - 1
    out_ids = np.empty((B, T), np.int64)
    out_mask = np.empty((B, T), np.int64)
    out_bbox = np.empty((B, T, 4), np.int64)
    pad = _low32(pad_id) if mut == "pad_id_32_bits" else pad_id
    for b in range(B):
        o = int(offsets[b])
        n = min(int(offsets[b + 1]) - o, T - 1 if mut == "truncate_t_minus_1" else T)
        for j in range(T):
            keep = j < n
            out_ids[b, j] = ids[o + j] if keep else pad
            out_mask[b, j] = 1 if keep else 0
            for c in range(4):
                v = int(boxes[o + j, c]) if keep else 0
                out_bbox[b, j, c] = _low32(v) if mut == "boxes_32_bits" else v
    return out_ids, out_mask, out_bbox


def collate_ref(ids, boxes, offsets, T, pad_id):
    return collate_model(ids, boxes, offsets, T, pad_id)


# ---------------------------------------------------------------------------------------------------------------------------------------
# patch projection
# ---------------------------------------------------------------------------------------------------------------------------------------
# ((C, R, P), batch sizes): every geometry class ee_create accepts
GEOMETRIES = [
    ((3, 224, 16), (1, 3)),                  # K 768.  B = 1: M = 196, one full and one partial tile; B = 3: M = 588, tiles straddle images at rows 196, 392
    ((3, 16, 16), (1, 127, 128, 129)),       # K 768.  NP = 1: every row another image
    ((2, 32, 8), (2,)),                      # K 128
    ((6, 32, 4), (3,)),                      # K 96.   P P = 16: a 32-wide slab spans two channels
    ((1, 64, 32), (5,)),                     # K 1024. a slab is one pixel row
    ((2, 48, 12), (9,)),                     # K 288.  kx changes from slab to slab
    ((2, 24, 12), (33,)),                    # K 288.  G = 2
    ((2, 40, 20), (33,)),                    # K 800.  P P = 400 = 12.5 slabs: every other channel starts in the middle of a slab
]
HIDDEN = (128, 256, 768)
PROJECT_FAULTS = ("kx_first_slab", "c_from_k0", "channel_stride_dropped", "image_of_tile_first_row")


def project_cases():
    return [(geo, B) for geo, batches in GEOMETRIES for B in batches]


def case_seed(geo, B, H, draw):
    C, R, P = geo
    return 11 + 1000003 * C + 10007 * R + 101 * P + 13 * B + 7 * H + (0 if draw == "lut" else 500000)


def project_operands(geo, B, H, draw):
    """pixel_values [B, C, R, R], W [H, C P P], b [H], float32.  draw "lut": the LUT of random bytes, the value set of real pixel_values;
    "general": normal floats with six k-columns near +-100 in every patch and a sprinkle of values below 1e-3 (whose lo plane is subnormal).
    W and b as tests/test_gpu_kernels._operands draws them."""
    C, R, P = geo
    rng = np.random.default_rng(case_seed(geo, B, H, draw))
    if draw == "lut":
        pix = rescale_normalize_lut()[rng.integers(0, 256, (B, C, R, R))]
    else:
        pix = rng.standard_normal((B, C, R, R)).astype(F32)
        K = C * P * P
        for k in rng.permutation(K)[:6]:
            c, ky, kx = k // (P * P), (k % (P * P)) // P, k % P
            v = pix[:, c, ky::P, kx::P]
            pix[:, c, ky::P, kx::P] = 100.0 * np.sign(v) + v
        pix = np.where(rng.random(pix.shape) < 0.05, pix * F32(1e-4), pix).astype(F32)
    W = (rng.standard_normal((H, C * P * P)) * 0.02).astype(F32)
    b = rng.standard_normal(H).astype(F32)
    return np.ascontiguousarray(pix, F32), W, b


def im2col(pix, P):
    """[B, C, R, R] -> [B (R / P)^2, C P P]: row (b, gy, gx), k = (c, ky, kx) as Conv2d's weight flattens (oracle.forward_all_beit)."""
    B, C, R, _ = pix.shape
    g = R // P
    return pix.reshape(B, C, g, P, g, P).transpose(0, 2, 4, 1, 3, 5).reshape(B * g * g, C * P * P)


def project_ref(pix, W, b, P):
    return im2col(pix, P).astype(F64) @ W.astype(F64).T + b.astype(F64)


def project_f32_torch(pix, W, b, P):
    import torch
    with torch.no_grad():
        return (torch.from_numpy(np.ascontiguousarray(im2col(pix, P))) @ torch.from_numpy(W).T + torch.from_numpy(b)).numpy()


def im2col_model(pix, P, mut=""):
    """The A operand as the kernels address it: element (row r, k) from the flat pixel buffer at
    b C R R + c R R + (gy P + ky) R + gx P + kx, with (c, ky, kx) taken from k slab by slab (k = k0 + lane offset, k0 a multiple of 32)."""
    B, C, R, _ = pix.shape
    g = R // P
    NP, K, pp = g * g, C * P * P, P * P
    flat = np.concatenate([pix.reshape(-1), np.zeros(4 * R * R, pix.dtype)])
    r = np.arange(B * NP)[:, None]
    k = np.arange(K)[None, :]
    b = r // NP
    if mut == "image_of_tile_first_row":
        b = (r // TILE * TILE) // NP
    p = r - (r // NP) * NP
    gy, gx = p // g, p % g
    k0, lane = k // 32 * 32, k % 32
    c = (k0 if mut == "c_from_k0" else k) // pp
    rem = k - c * pp
    ky, kx = rem // P, rem % P
    if mut == "kx_first_slab":
        kx = lane % P
    if mut == "channel_stride_dropped":
        c = np.zeros_like(c)
    return flat[b * C * R * R + c * R * R + (gy * P + ky) * R + gx * P + kx]


def rows_written(M, mut=""):
    """The output rows a launch over M rows stores: M, or whole tiles when the store is not masked."""
    return -(-M // TILE) * TILE if mut == "rows_past_m" else M


def split_values(pix, P, scale=SPLIT_SCALE):
    """What the split rows hold of the patches (float64)."""
    return split_round(im2col(pix, P), scale)


def split_words(pix, P, scale=SPLIT_SCALE):
    """The split rows as int32 words [B NP, C P P]: 64-byte groups [hi 16 f16 | lo 16 f16]."""
    return _encode_split(split_values(pix, P, scale).astype(F32), scale)


def decode_words(words, scale=SPLIT_SCALE):
    rows, N = words.shape
    h = np.ascontiguousarray(words).view(np.float16).reshape(rows, N // 16, 2, 16)
    return (h[:, :, 0].astype(F64) + h[:, :, 1].astype(F64)).reshape(rows, N) / scale


def per_row_max(x):
    return np.abs(x).max(-1)
