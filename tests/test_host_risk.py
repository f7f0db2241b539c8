"""Risk control without a device: the restatement (tests/risk_ref.py) against scipy, the properties the definition in include/mmee.h
promises, and the refusals that come before any device call."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
from scipy import stats

from . import risk_ref as R
from .conftest import ROOT, report_measured

# n and alpha of the comparison with scipy.  The first seven n and the alphas but 0.2 are the stated grid; 5, 1031 and alpha = 0.2 are what
# tests/test_gpu_risk.py runs on top, so that the bar it derives from this measurement covers its own cases.
CDF_N = (1, 2, 59, 257, 1000, 2500, 4096, 5, 1031)
CDF_ALPHA = (0.01, 0.05, 0.1, 0.3, 0.2)
BOUND_CASES = ((10, 0), (10, 3), (257, 20), (1000, 999), (2500, 100), (4096, 0), (7, 7))
# What float64 allows the restatement.  A term's exponent is a sum of five numbers of magnitude up to lgamma(4097) = 2.998e4, where one ulp is
# 2^-38 = 3.6e-12: five roundings of the operands (lgamma and the two products, half an ulp each when correctly rounded, one ulp allowed for
# libm's lgamma) and four of the additions stay below 14 half-ulps = 2.6e-11 absolute in the exponent, which is the relative error of the
# term and so of the sum of terms; the running sum's own roundings (4097 x 1.1e-16) add 4.5e-13.  Rounded up:
CDF_REL_BOUND = 5e-11
# A bound is a root of F(theta) = delta.  An error eps (relative) in F moves it by eps delta / |F'(theta)|, and |F'| = n x (a binomial
# probability of n - 1 trials) is above 0.5 at every case below (the least: theta^7 = 0.05 at (7, 7), 7 theta^6 = 0.54): 5e-11 x 0.05 / 0.5
BOUND_ABS_BOUND = 1e-11


def test_binomial_cdf_against_scipy():
    worst = 0.0
    for n in CDF_N:
        for alpha in CDF_ALPHA:
            F, S = R.binom_cdf_table(n, alpha), stats.binom.cdf(np.arange(n + 1), n, alpha)
            big = S >= 1e-280
            worst = max(worst, float((np.abs(F[big] - S[big]) / S[big]).max()))
            assert (np.diff(F) >= 0).all() and F[-1] <= 1.0 and F[-1] > 1 - 1e-9
    report_measured("test_binomial_cdf_against_scipy", "restatement vs scipy.stats.binom.cdf, max relative deviation where scipy >= 1e-280", worst)
    assert worst <= CDF_REL_BOUND


def test_clopper_pearson_against_scipy_beta_ppf():
    delta, worst = 0.05, 0.0
    for n, k in BOUND_CASES:
        up, low = R.bounds(n, k, delta)
        want_up = 1.0 if k == n else float(stats.beta.ppf(1 - delta, k + 1, n - k))
        want_low = 0.0 if k == 0 else float(stats.beta.ppf(delta, k, n - k + 1))
        worst = max(worst, abs(up - want_up), abs(low - want_low))
        assert low <= k / n <= up
    report_measured("test_clopper_pearson_against_scipy_beta_ppf", "restatement vs scipy.stats.beta.ppf, max absolute deviation", worst)
    assert worst <= BOUND_ABS_BOUND
    assert R.bounds(7, 7, delta)[0] == 1.0 and R.bounds(10, 0, delta)[1] == 0.0
    assert R.bounds(10, 0, delta)[0] == pytest.approx(1 - delta ** 0.1, abs=1e-15)         # (1 - theta)^10 = delta in closed form


def test_hoeffding_bentkus_at_zero_loss_is_the_binomial_value():
    for n in (1, 59, 1000):
        for alpha in (0.05, 0.3):
            p = R.pvalues([0], n, alpha, R.HB)[0]
            assert p == pytest.approx((1 - alpha) ** n, rel=1e-12)                         # h(0, alpha) = -log(1 - alpha); e F(0) is larger
            assert p <= R.pvalues([0], n, alpha, R.BINOMIAL)[0] * (1 + 1e-12)
    # r >= alpha: Hoeffding's part is 1 and Bentkus's is e F(ceil) clamped
    assert R.pvalues([30 * R.ONE], 100, 0.3, R.HB)[0] == min(1.0, math.e * R.binom_cdf_table(100, 0.3)[30])
    # Bentkus's part reads the table at the sum rounded UP to whole losses: one unit above 399 reads F(400).  alpha = 0.5, n = 1000:
    # Hoeffding's part exp(-1000 h(0.4, 0.5)) = 1.8e-9 is the larger there, so the minimum is Bentkus's
    F = R.binom_cdf_table(1000, 0.5)
    assert math.e * F[400] < math.exp(-1000 * R.kl(0.4, 0.5))
    assert R.pvalues([399 * R.ONE + 1], 1000, 0.5, R.HB)[0] == math.e * F[400] and R.pvalues([399 * R.ONE], 1000, 0.5, R.HB)[0] == math.e * F[399]


def test_ceil_quantisation_never_lowers_a_sum():
    rng = np.random.default_rng(5)
    loss = rng.random((3, 4000))
    loss[0, :5] = (0.0, 1.0, 2.0 ** -31, 1 - 2.0 ** -40, 0.5)
    q = R.quantise(loss)
    assert q.min() >= 0 and q.max() <= R.ONE and (q[0, :5] == (0, R.ONE, 1, R.ONE, R.ONE // 2)).all()
    assert (q >= loss * R.ONE).all() and (q - loss * R.ONE < 1).all()                     # exact: the products are exact in float64
    assert int(q.sum()) >= math.fsum((loss * R.ONE).ravel())
    binary = (rng.random((3, 50)) < 0.5).astype(np.float64)
    assert set(np.unique(R.quantise(binary))) <= {0, R.ONE}


def test_fixed_sequence_stops_at_the_first_failure_and_bonferroni_does_not():
    """One exit below the final one, N = 1000, agreement by confidence: on the path [1.0, 0.9, 0.0, 0.95] the third vector (everybody leaves
    at exit 0) fails, the fourth passes on its own."""
    conf, agree = R.synthetic_table(11, 2, 1000)
    loss_q = (1 - agree.astype(np.int64)) * R.ONE
    thr = np.array([[1.0, 0.0], [0.9, 0.0], [0.0, 0.0], [0.95, 0.0]])
    alpha, delta = 0.1, 0.05
    fs = R.control(conf, 1.0, loss_q, None, thr, alpha, delta, R.BINOMIAL, R.FIXED_SEQUENCE)
    bf = R.control(conf, 1.0, loss_q, None, thr, alpha, delta, R.BINOMIAL, R.BONFERRONI)
    assert R.away_from_levels(fs["pvalue"], 4, delta)
    assert fs["pvalue"][2] > delta and fs["pvalue"][3] <= delta / 4
    assert fs["certified"].tolist() == [True, True, False, False] and bf["certified"].tolist() == [True, True, False, True]
    assert fs["n_certified"] == 2 and bf["n_certified"] == 3
    assert fs["selected"] == 1 and bf["selected"] == 1                                    # 0.9 releases more than 0.95: the cheaper of the certified
    assert fs["loss_sum"] == bf["loss_sum"] and fs["hist"][0].tolist() == [0, 1000]


def test_58_documents_certify_nothing_and_59_everything():
    alpha = delta = 0.05
    assert math.ceil(math.log(delta) / math.log(1 - alpha)) == 59
    for n, want in ((58, False), (59, True)):
        conf = np.random.default_rng(n).random((3, n))
        thr = np.linspace(1, 0, 11)[:, None] * np.ones((1, 3))
        for bound in (R.BINOMIAL, R.HB):
            r = R.control(conf, 1.0, np.zeros((3, n), dtype=np.int64), None, thr, alpha, delta, bound, R.FIXED_SEQUENCE)
            assert r["certified"].all() == want and r["certified"].any() == want
            assert r["selected"] == (10 if want else -1)                                   # the cheapest: everybody leaves at exit 0


def test_exit_rule_is_strict_skips_nan_and_never_reads_the_last_threshold():
    conf = np.array([[0.5, np.nan, 0.7], [0.9, 0.9, np.nan], [0.1, 0.1, 0.1]])
    assert R.exits_of(conf, 1.0, np.array([0.5, 0.9, np.nan])).tolist() == [2, 2, 0]
    assert R.exits_of(conf, 1.0, np.array([0.4, 0.8, np.nan])).tolist() == [0, 1, 0]
    assert R.exits_of(conf, -1.0, np.array([0.6, 0.95, np.nan])).tolist() == [0, 1, 2]


def test_the_header_states_the_definition_and_the_binding_knows_the_entry_points(pkg):
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    declared = set(re.findall(r"^\w[\w\s\*]*?\b(ee_\w+)\s*\(", header, flags=re.M))
    lib = pkg.capi.load()
    for name in ("ee_risk_control", "ee_binomial_bounds"):
        assert name in declared and name in pkg.capi.SYMBOLS and hasattr(lib, name), name
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", header))
    for words in ("the first e < E1-1 with sign conf[e][n] > sign thr[v][e], else E1-1", "min(2^30, ceil(l 2^30))",
                  "p_B = min(1, e F(ceil(loss_sum / 2^30)))", "ties to the lowest v; -1 when none is certified",
                  "A front searched on the same table does not qualify", "Not built: the WSR betting bound", "exactly 64 bisections of [0,1]"):
        assert words in flat, words
    for code, name in ((pkg.capi.RISK_BINOMIAL, "MMEE_RISK_BINOMIAL"), (pkg.capi.RISK_HB, "MMEE_RISK_HB"),
                       (pkg.capi.RISK_FIXED_SEQUENCE, "MMEE_RISK_FIXED_SEQUENCE"), (pkg.capi.RISK_BONFERRONI, "MMEE_RISK_BONFERRONI")):
        assert re.search(rf"\b{name} = {code}\b", header), name


def test_refusals_come_before_any_device_call(pkg):
    lib = pkg.capi.load()
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)

    def call(**kw):
        a = dict(conf=p, sign=1.0, loss_f64=None, loss_q=p, cost=None, E1=2, N=4, thr=p, V=1, alpha=0.1, delta=0.05, bound=0, method=0,
                 loss_sum=p, exit_sum=p, cost_sum=p, hist=None, pvalue=p, certified=p, n_certified=p, selected=p)
        a.update(kw)
        assert lib.ee_risk_control(*a.values(), None) != 0
        return pkg.capi.last_error()

    assert "NULL argument" in call(conf=None) and "NULL argument" in call(selected=None) and "NULL argument" in call(thr=None)
    assert "exactly one of loss_f64 and loss_q" in call(loss_f64=p) and "exactly one of loss_f64 and loss_q" in call(loss_q=None)
    assert "1 <= E1 <= 64" in call(E1=0) and "1 <= E1 <= 64" in call(E1=65)
    assert "1 <= N < 2^24" in call(N=0) and "1 <= N < 2^24" in call(N=1 << 24)
    assert "1 <= V <= 65536" in call(V=0) and "1 <= V <= 65536" in call(V=65537)
    assert "alpha" in call(alpha=0.0) and "alpha" in call(alpha=1.0) and "alpha" in call(alpha=float("nan"))
    assert "delta" in call(delta=0.0) and "delta" in call(delta=1.5)
    assert "sign is +1 or -1" in call(sign=0.5)
    assert "neither MMEE_RISK_BINOMIAL nor MMEE_RISK_HB" in call(bound=2)
    assert "neither MMEE_RISK_FIXED_SEQUENCE nor MMEE_RISK_BONFERRONI" in call(method=-1)

    def bounds(n, k, Q=1, delta=0.05, up=p, low=p):
        nn, kk = (C.c_int32 * 1)(n), (C.c_int32 * 1)(k)
        assert lib.ee_binomial_bounds(nn, kk, Q, delta, up, low, None) != 0
        return pkg.capi.last_error()

    assert "outside [0, n = 5]" in bounds(5, 6) and "outside [0, n = 5]" in bounds(5, -1)
    assert "1 <= n < 2^24" in bounds(0, 0) and "1 <= n < 2^24" in bounds(1 << 24, 0)
    assert "delta" in bounds(5, 1, delta=1.0) and "1 <= Q" in bounds(5, 1, Q=0) and "NULL argument" in bounds(5, 1, up=None)


def test_python_refusals_need_no_device(pkg):
    risk = pkg.risk
    t = (np.zeros((2, 4)), np.zeros((2, 4), dtype=np.uint8))
    with pytest.raises(ValueError, match="fixed_sequence"):
        risk.risk_control(t, alpha=0.1, delta=0.05, method="holm")
    with pytest.raises(ValueError, match="binomial"):
        risk.risk_control(t, alpha=0.1, delta=0.05, bound="wsr")
    with pytest.raises(ValueError, match="consistency"):
        risk.risk_control(t, alpha=0.1, delta=0.05, risk="brier")
    with pytest.raises(ValueError, match=r"\(0, 1\)"):
        risk.risk_control(t, alpha=0.0, delta=0.05)
    with pytest.raises(ValueError, match="not a threshold criterion"):
        risk.risk_control(t, alpha=0.1, delta=0.05, criterion="patience")
    with pytest.raises(ValueError, match="strictly towards the aggressive side"):
        risk._candidates([0.9, 0.9], None, 3, 1.0, "max_confidence")
    with pytest.raises(ValueError, match="strictly towards the aggressive side"):
        risk._candidates([0.5, 0.4], None, 3, -1.0, "entropy")
    with pytest.raises(ValueError, match="no default candidates"):
        risk._candidates(None, None, 3, -1.0, "entropy")
    with pytest.raises(ValueError, match="not both"):
        risk._candidates([0.5], np.zeros((1, 3)), 3, 1.0, "max_confidence")
    lam = risk._candidates(None, None, 3, 1.0, "margin")
    assert lam.shape == (101, 3) and lam[0, 0] == 1.0 and lam[-1, 2] == 0.0 and (np.diff(lam[:, 1]) < 0).all()
    with pytest.raises(ValueError, match="SearchResult or a RefineResult"):
        risk.path_from_front(np.zeros((2, 3)))
    with pytest.raises(ValueError, match="0 <= k <= n"):
        risk.binomial_bounds(5, 6, 0.05)
    # the message of an empty certificate names the smallest table that could pass
    r = risk.RiskResult(thresholds=np.zeros((3, 2)), loss_sum=np.zeros(3, dtype=np.uint64), exit_sum=np.zeros(3, dtype=np.int64),
                        cost_sum=np.zeros(3, dtype=np.uint64), risk=np.zeros(3), pvalue=np.full(3, 0.051), certified=np.zeros(3, dtype=bool),
                        n_certified=0, selected=-1, num_samples=58, alpha=0.05, delta=0.05, bound="binomial", method="fixed_sequence", binary=True)
    with pytest.raises(ValueError, match=r"= 59 calibration documents"):
        r.select()
