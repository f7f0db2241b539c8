"""The numpy restatement of the split-f16 codec (tests/split_ref.py), checked without a GPU: it keeps the promises csrc/mmee_common.h makes
about the planes, its edge value set holds what its header says, and the set can SEE a subtly wrong encoder -- every mutation changes at least
one word of encode(edge_values) or the flag, which is all tests/test_gpu_split.py compares."""
import numpy as np
import pytest

from . import split_ref as S
from .hook_util import _encode_split

F16, F32, F64 = np.float16, np.float32, np.float64
FORMS = ("clamp", "pair")


def _planes(x, scale, form):
    hi, lo, flag = S.encode(x, scale, form)
    return hi.view(F16), lo.view(F16), flag


@pytest.mark.parametrize("scale", S.SCALES)
def test_the_edge_set_holds_what_its_header_says(scale):
    with np.errstate(over="ignore"):     # the values beyond 65504 become inf as f16, knowingly
        _check_edge_set(scale)


def _check_edge_set(scale):
    x = S.edge_values(scale)
    assert x.dtype == F32 and x.ndim == 1 and len(x) % S.ROW == 0 and 2000 <= len(x) <= 64 * S.ROW and not x.flags.writeable
    assert np.array_equal(x, S.edge_values(scale)) and not np.isnan(x).any() and not np.isinf(x).any()
    have = set(x.tolist())
    assert {float(F32(v)) for v in (0.0, 1.4e-45, 1.1754942e-38, 1e30, np.finfo(F32).max)} <= {abs(v) for v in have} and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    for v in (60000.0, float(np.nextafter(F32(60000.0), F32(np.inf))), 65504.0, 65519.99609375, 65520.0):
        assert v / scale in have and -v / scale in have, v
    hi, lo, _ = _planes(x, scale, "pair")
    xs = x.astype(F64) * scale
    for e in S.BINADES:
        first, last = (float(np.array(p, np.uint16).view(F16)) for p in S._binade_patterns(e))
        inside = (np.abs(xs) >= 2.0 ** e) & (np.abs(xs) < 2.0 ** (e + 1))
        for sign in (1.0, -1.0):
            assert sign * first / scale in have and sign * last / scale in have, (e, sign)
            # a tie is the mean of two neighbouring f16 values: both parities of the lower one, and an f32 on either side of a tie
            m = inside & (np.sign(xs) == sign)
            a = np.abs(xs[m])
            lower = np.minimum(a.astype(F16).astype(F64), _other_neighbour(a))
            is_tie = (a != a.astype(F16).astype(F64)) & (np.abs(a - a.astype(F16).astype(F64)) == np.abs(a - _other_neighbour(a)))
            parities = {int(np.array(v, F16).view(np.uint16)) & 1 for v in lower[is_tie]}
            assert parities == ({0, 1} if e > -24 else {1}), (e, sign, parities)
            for t in a[is_tie]:
                t32 = F32(t)
                assert float(np.nextafter(t32, F32(0))) * sign / scale in have and float(np.nextafter(t32, F32(np.inf))) * sign / scale in have, (e, t)
        sub = inside & (lo != 0) & (np.abs(lo.astype(F64)) < 2.0 ** -14)
        assert (inside & (lo == 0)).any(), e
        if -11 <= e <= 8:                # h + d with d a few 2^-24, or one f32 ulp of h, is an f32 and d stays below half an f16 ulp
            assert sub.any(), e


def _other_neighbour(a):
    """The f16 neighbour of a on the other side of a than its nearest f16 value (float64)."""
    h = a.astype(F16)
    up = np.nextafter(h, F16(np.inf)).astype(F64)
    down = np.nextafter(h, F16(0)).astype(F64)
    return np.where(h.astype(F64) < a, up, down)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scale", S.SCALES)
def test_hi_plus_lo_is_exact_in_f32_and_carries_22_bits(scale, form):
    x = S.edge_values(scale)
    hi, lo, _ = _planes(x, scale, form)
    ok = np.isfinite(hi.astype(F64))
    s64 = hi.astype(F64)[ok] + lo.astype(F64)[ok]
    assert np.array_equal((hi.astype(F32)[ok] + lo.astype(F32)[ok]).astype(F64), s64), "hi + lo rounds in f32"
    xs = x.astype(F64) * scale
    claim = (np.abs(xs) >= 2.0 ** -3) & (np.abs(xs) <= (S.CLAMP if form == "clamp" else S.F16_MAX))
    got = S.plane_values(x, scale, form)
    assert claim.sum() > 500
    assert (np.abs(x.astype(F64)[claim] - got[claim]) <= 2.0 ** -22 * np.abs(x.astype(F64)[claim])).all()


@pytest.mark.parametrize("scale", S.SCALES)
def test_the_two_forms_agree_up_to_the_clamp(scale):
    x = S.edge_values(scale)
    a, b = S.encode(x, scale, "clamp"), S.encode(x, scale, "pair")
    inside = ~S.overflows(x, scale)
    assert inside.sum() > 2000 and (~inside).sum() >= 12
    assert np.array_equal(a[0][inside], b[0][inside]) and np.array_equal(a[1][inside], b[1][inside])
    assert a[2] and b[2]
    assert not np.array_equal(a[0][~inside], b[0][~inside])               # beyond it they differ: clamped against converted
    quiet = S.without_overflow(x, scale)
    assert not S.encode(quiet, scale, "clamp")[2] and not S.encode(quiet, scale, "pair")[2]
    assert np.array_equal(S.encode(quiet, scale, "clamp")[:2], S.encode(quiet, scale, "pair")[:2])


def test_the_flag_is_overflow_or_nan():
    x = np.zeros(16, F32)
    for form in FORMS:
        assert not S.encode(x, 16.0, form)[2]
        for bad, at in ((np.inf, 0), (-np.inf, 7), (np.nan, 15), (3750.0 + 2.0 ** -8, 3), (-1e30, 9)):
            y = x.copy()
            y[at] = bad
            assert S.encode(y, 16.0, form)[2], (form, bad)
        y = x.copy()
        y[5] = 3750.0                    # 16 x 3750 = 60000: the last value inside
        assert not S.encode(y, 16.0, form)[2]


def test_pack_and_decode_use_the_layout_of_the_hook_tests():
    rng = np.random.default_rng(3)
    for N in (16, 64, 256, 1024):
        x = (rng.integers(-2 ** 21, 2 ** 21, (3, N)) * 2.0 ** -14).astype(F32)          # 22 bits: the planes hold them exactly
        words, flag = S.encode_words(x, 16.0)
        assert not flag and np.array_equal(words, _encode_split(x, 16.0))
        assert np.array_equal(S.decode(words, 16.0), x.astype(F64))
        hi, lo = S.unpack(words)
        assert np.array_equal(S.pack(hi, lo), words)


def test_weight_exponent_puts_the_maximum_in_its_binade():
    rng = np.random.default_rng(4)
    mags = np.concatenate([np.ldexp(1.0 + rng.random(400), rng.integers(-60, 40, 400)), 2.0 ** np.arange(-40.0, 30.0),
                           np.nextafter((2.0 ** np.arange(-40.0, 30.0)).astype(F32), F32(0)).astype(F64)]).astype(F32)
    for mx in mags:
        e = S.weight_exponent(mx)
        assert e == 8 or (e < 8 and 2.0 ** 12 <= float(mx) * 2.0 ** e < 2.0 ** 13), (mx, e)
        if e == 8:
            assert float(mx) * 2.0 ** 8 < 2.0 ** 13
    assert S.weight_exponent(0.0) == 8 and S.weight_exponent(2.0 ** 5) == 7 and S.weight_exponent(np.nextafter(F32(32.0), F32(0))) == 8
    assert S.weight_exponent(1e6) == -7 and S.weight_exponent(1e-30) == 8
    assert S.encode_weight(np.array([[1.0, np.nan]], F32)) is None and S.encode_weight(np.array([[np.inf, 0.0]], F32)) is None


@pytest.mark.parametrize("form,mut", [(f, m) for m in S.MUTATIONS for f in FORMS if (f, m) != ("pair", "clamp_65504")])      # the pair form has no clamp
@pytest.mark.parametrize("scale", S.SCALES)
def test_the_edge_set_sees_each_seeded_fault(scale, form, mut):
    x = S.edge_rows(scale)
    if mut == "nan_unflagged":           # the flag's NaN half: on the set without its overflow values, one element a NaN
        x = S.edge_rows(scale, overflow=False).copy()
        x[1, 7] = np.nan
        assert S.encode(x, scale, form)[2] and not S.encode(x, scale, form, mut)[2]
        return
    want, got = S.encode_words(x, scale, form), S.encode_words(x, scale, form, mut)
    n = int((want[0] != got[0]).sum())
    assert n > 0 or want[1] != got[1], mut
    if mut != "clamp_65504":             # and without the overflow values, where only the words are left to differ
        q = S.edge_rows(scale, overflow=False)
        assert (S.encode_words(q, scale, form)[0] != S.encode_words(q, scale, form, mut)[0]).any(), mut
