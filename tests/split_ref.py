"""The split-f16 codec of csrc/mmee_common.h ("Split-f16 operand rows") restated plainly in numpy (no GPU), with the one edge value set that
every test of tests/test_gpu_split.py feeds to an encoder.

    encode   : xs = f32(scale * x); hi = RNE f16 of xs, lo = RNE f16 of (xs - hi), the difference taken exactly.  form "clamp" (split_f16x4:
               split_rows_kernel, the attention context stores, the f32-staged GEMM epilogue) first clamps xs to +-60000; form "pair"
               (split_pair: patch_split_kernel, the row kernels, the GEMM epilogues) does not, so above 65504 hi rounds as f16 does, to inf
               from 65520.  The flag (kErrSplitOverflow, bit 16) is "max |xs| is not <= 60000, or an element is a NaN".
    decode   : (hi + lo) / scale in float64.
    weight_exponent : split_weight_exponent of csrc/capi_internal.h, the per-tensor scale 2^e of a weight under ee_finalize.

Planes travel as f16 bit patterns (uint16), so that +-0, subnormals and inf compare as what they are.  The 64-byte group layout of a row
([hi 16 | lo 16] per 16 columns) is not restated here: pack / unpack read it off hook_util._encode_split, decode goes through
hook_util._decode_split.

``mut`` names ONE deliberate fault of a subtly wrong encoder; tests/test_host_split_ref.py shows that each changes a word of
encode(edge_values) or the flag, so the bit comparisons of tests/test_gpu_split.py see it."""
import functools

import numpy as np

from .hook_util import _decode_split, _encode_split

F16, F32, F64 = np.float16, np.float32, np.float64
CLAMP = 60000.0                         # csrc/mmee_common.h kSplitClamp
F16_MAX = 65504.0
SCALES = (16.0, 64.0, 256.0)            # kSplitScaleX / QKV / H1, kSplitScaleCtx, the cap of a weight's scale
BINADES = range(-24, 16)                # f16 binades [2^e, 2^(e+1)) of |scale * x|: subnormal below -14
ROW = 256                               # the edge set is a whole number of rows of this many columns
MUTATIONS = ("trunc_hi", "lo_unscaled", "flush_lo", "clamp_65504", "scale_x2", "nan_unflagged", "swap_cols")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the row layout, read off hook_util._encode_split
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _layout(N):
    """(hi_pos [N], lo_pos [N]): where column k's hi and lo halves sit among the 2 N f16 halves of a row.  Column k is encoded as
    (k + 1)(1 + 2^-12): hi = k + 1 (the remainder is below half an f16 ulp for k + 1 <= 2048), lo = (k + 1) 2^-12, both exact."""
    assert N % 16 == 0 and N <= 2048
    k1 = np.arange(1, N + 1, dtype=F64)
    halves = _encode_split((k1 * (1.0 + 2.0 ** -12)).astype(F32)[None, :], 1.0).view(F16).reshape(2 * N).astype(F64)
    hi_pos, lo_pos = np.empty(N, np.int64), np.empty(N, np.int64)
    is_hi = halves >= 1.0
    hi_pos[(halves[is_hi] - 1).astype(np.int64)] = np.nonzero(is_hi)[0]
    lo_pos[(halves[~is_hi] * 4096.0 - 1).astype(np.int64)] = np.nonzero(~is_hi)[0]
    return hi_pos, lo_pos


def pack(hi, lo):
    """f16 bit patterns [rows, N] of the two planes -> the rows' int32 words [rows, N]."""
    rows, N = hi.shape
    hi_pos, lo_pos = _layout(N)
    halves = np.empty((rows, 2 * N), np.uint16)
    halves[:, hi_pos] = hi
    halves[:, lo_pos] = lo
    return halves.view(np.int32)


def unpack(words):
    """int32 words [rows, N] -> (hi, lo) f16 bit patterns [rows, N]."""
    words = np.ascontiguousarray(words, np.int32)
    hi_pos, lo_pos = _layout(words.shape[1])
    halves = words.view(np.uint16)
    return halves[:, hi_pos], halves[:, lo_pos]


def decode(words, scale):
    """(hi + lo) / scale of int32 words [rows, N], float64."""
    import torch
    words = np.ascontiguousarray(words, np.int32)
    return _decode_split(torch.from_numpy(words), words.shape[1], scale).numpy()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the encoder
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rne_f16(v64):
    """float64 -> f16, round to nearest even (numpy converts float64 to half in one rounding)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return v64.astype(F16)


def _trunc_f16(v64):
    """float64 -> f16 toward zero (the fault "trunc_hi")."""
    h = _rne_f16(v64)
    away = np.abs(h.astype(F64)) > np.abs(v64)
    bits = h.view(np.uint16).copy()
    bits[away] -= 1                      # one f16 step toward zero (sign-magnitude: the pattern minus one)
    return bits.view(F16)


def encode(x, scale, form="clamp", mut=""):
    """x f32 (any shape) -> (hi bits, lo bits, flag): uint16 arrays of x's shape and a bool."""
    assert form in ("clamp", "pair") and mut in ("",) + MUTATIONS
    x = np.asarray(x, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        xs = x * F32(scale * (2.0 if mut == "scale_x2" else 1.0))              # the f32 product: exact (a power of two) short of inf
    nan = np.isnan(xs)
    with np.errstate(invalid="ignore"):
        flag = bool(not (np.abs(xs[~nan]).max(initial=0.0) <= CLAMP)) or bool(nan.any() and mut != "nan_unflagged")
    if form == "clamp":
        lim = F32(F16_MAX if mut == "clamp_65504" else CLAMP)
        xs = np.where(nan, xs, np.minimum(np.maximum(xs, -lim), lim))
    xs64 = xs.astype(F64)
    hi = _trunc_f16(xs64) if mut == "trunc_hi" else _rne_f16(xs64)
    with np.errstate(invalid="ignore"):
        rest = (x.astype(F64) if mut == "lo_unscaled" else xs64) - hi.astype(F64)      # exact in float64 (and in f32, as the kernels take it)
    lo = _rne_f16(rest)
    if mut == "flush_lo":
        lo = np.where(np.abs(lo.astype(F64)) < 2.0 ** -14, F16(0.0) * np.sign(lo), lo).astype(F16)
    hi, lo = hi.view(np.uint16), lo.view(np.uint16)
    if mut == "swap_cols":               # columns 4 j + 2 and 4 j + 3 of every group of four
        assert x.shape[-1] % 4 == 0
        perm = np.arange(x.shape[-1]).reshape(-1, 4)[:, [0, 1, 3, 2]].reshape(-1)
        hi, lo = hi[..., perm], lo[..., perm]
    return hi, lo, flag


def encode_words(x, scale, form="clamp", mut=""):
    """encode of rows [rows, N] as the rows' int32 words, and the flag."""
    hi, lo, flag = encode(x, scale, form, mut)
    return pack(hi, lo), flag


def plane_values(x, scale, form="clamp"):
    """What the planes of x hold, (hi + lo) / scale, as float64 of x's shape."""
    hi, lo, _ = encode(x, scale, form)
    with np.errstate(invalid="ignore"):
        return (hi.view(F16).astype(F64) + lo.view(F16).astype(F64)) / scale


# ---------------------------------------------------------------------------------------------------------------------------------------
# the weight scale
# ---------------------------------------------------------------------------------------------------------------------------------------
def weight_exponent(max_abs):
    """split_weight_exponent: the e of a weight's scale 2^e -- max |w| 2^e in [2^12, 2^13), capped at 8; 8 for an all-zero tensor."""
    mx = float(F32(max_abs))
    if not mx > 0.0:
        return 8
    _, ex = np.frexp(mx)                 # mx = m 2^ex, m in [0.5, 1)
    return min(8, 13 - int(ex))


def encode_weight(w):
    """The weight split of ee_finalize on w [N, K]: (words, 1 / scale, e), or None where it refuses (inf / nan)."""
    w = np.asarray(w, F32)
    mx = np.abs(w).max()
    if not np.isfinite(w).all():
        return None
    e = weight_exponent(mx)
    words, flag = encode_words(w, 2.0 ** e, "clamp")
    return words, F32(2.0 ** -e), e


# ---------------------------------------------------------------------------------------------------------------------------------------
# the edge value set
# ---------------------------------------------------------------------------------------------------------------------------------------
def _f16_of_bits(p):
    return np.array(p, np.uint16).view(F16).astype(F64)


def _binade_patterns(e):
    """(first, last) f16 bit patterns of the positive binade [2^e, 2^(e+1))."""
    first = int(np.array(2.0 ** e, F16).view(np.uint16))
    last = int(np.array(2.0 ** (e + 1), F16).view(np.uint16)) - 1 if e < 15 else 0x7BFF
    return first, last


def overflow_edge(scale):
    """The values around the planes' upper end, as x: 60000, the f32 behind it, 65504, the f32 in front of 65520 (hi still 65504 in the pair
    form), 65520 (inf), each over the scale; 1e30; the largest f32."""
    s = [CLAMP, np.nextafter(F32(CLAMP), F32(np.inf)), F16_MAX, np.nextafter(F32(65520.0), F32(0.0)), 65520.0]
    return np.concatenate([np.array(s, F64) / scale, [1e30, float(np.finfo(F32).max)]]).astype(F32)


@functools.lru_cache(maxsize=None)
def edge_values(scale):
    """A seeded f32 vector (a whole number of ROW columns, read-only) at the f16 rounding edges of scale * x.  For every binade of BINADES:
    its first, a middle and its last f16 value (lo exactly 0); the ties between f16 neighbours with an even and an odd lower neighbour at both
    ends of the binade, and the f32 just below and above each; f16 values plus a few units of 2^-24 or one f32 ulp (lo f16-subnormal where the
    binade allows one); random significands.  Then +-0, f32 subnormals, the overflow edge, and the other sign of everything."""
    rng = np.random.default_rng(20240 + int(scale))
    s = []                               # scaled values, float64, every one exact in f32
    for e in BINADES:
        first, last = _binade_patterns(e)
        mid = (first + last) // 2 | 1
        s += [_f16_of_bits(p) for p in sorted({first, min(mid, last), last})]
        for p in sorted({first, min(first + 1, last), max(last - 1, first), last}):
            if p + 1 > 0x7BFF:
                continue                 # the tie above 65504 is 65520: overflow_edge
            tie = F32(0.5 * (_f16_of_bits(p) + _f16_of_bits(p + 1)))
            s += [float(tie), float(np.nextafter(tie, F32(0.0))), float(np.nextafter(tie, F32(np.inf)))]
        h = float(_f16_of_bits(min(mid, last)))
        for d in (2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** (e - 23), 2.0 ** -20 + 2.0 ** (e - 23), -2.0 ** -24, -(2.0 ** (e - 23))):
            if float(F32(h + d)) == h + d and abs(d) < 0.5 * max(2.0 ** (e - 10), 2.0 ** -24):      # an f32, and hi stays h
                s.append(h + d)
        s += list(np.ldexp(1.0 + rng.integers(0, 1 << 23, 12) / float(1 << 23), e))
    s.append(2.0 ** -25)                 # the tie between 0 and the smallest f16 subnormal, and its f32 neighbours
    s += [float(np.nextafter(F32(2.0 ** -25), F32(0.0))), float(np.nextafter(F32(2.0 ** -25), F32(1.0))), 2.0 ** -26, 2.0 ** -30]
    x = (np.array(s, F64) / scale).astype(F32)
    assert np.array_equal(x.astype(F64) * scale, np.array(s, F64))
    tiny = np.array([0.0, 1.4e-45, 1e-40, 1.1754942e-38], F32)                  # 0 and f32 subnormals (as x: scale * x encodes to 0)
    x = np.concatenate([x, tiny, overflow_edge(scale)])
    x = np.concatenate([x, -x])
    fill = (-len(x)) % ROW
    more = np.ldexp(1.0 + rng.integers(0, 1 << 23, fill) / float(1 << 23), rng.integers(-24, 15, fill)) * rng.choice([-1.0, 1.0], fill) / scale
    x = np.concatenate([x, more.astype(F32)])[rng.permutation(len(x) + fill)]
    x.setflags(write=False)
    return x


def overflows(x, scale):
    """Which elements leave the planes' range: |f32(scale x)| > 60000."""
    with np.errstate(over="ignore"):
        return ~(np.abs(np.asarray(x, F32) * F32(scale)) <= CLAMP)


def without_overflow(x, scale):
    """x with every overflowing element replaced by 0."""
    return np.where(overflows(x, scale), F32(0.0), np.asarray(x, F32)).astype(F32)


def edge_rows(scale, overflow=True):
    """edge_values as rows [n / ROW, ROW]; overflow = False: without_overflow of them."""
    x = edge_values(scale)
    return (x if overflow else without_overflow(x, scale)).reshape(-1, ROW)
