"""Risk control on the GPU (ee_risk_control / ee_binomial_bounds; risk.py, audit.consistency(delta=), audit.certify) against the restatement
(tests/risk_ref.py): the integers, histograms, masks and selections exactly, p-values and bounds against scipy within a bar derived from the
restatement's own deviation from scipy; then against what already ships (the scans, the audit's counts) and end to end into a forward."""
import ctypes as C
import math

import numpy as np
import pytest
from scipy import stats

from . import risk_ref as R
from .conftest import TINY_CASES, report_measured, sweep_ref_inputs

pytestmark = pytest.mark.gpu

# The restatement's own deviation from scipy over the cases of this file, measured by tests/test_host_risk.py (profiles/risk_control.txt):
# relative, against stats.binom.cdf where it is >= 1e-280; absolute, of both Clopper-Pearson bounds against stats.beta.ppf at delta = 0.05.
RESTATEMENT_REL, RESTATEMENT_ABS = 7.6e-12, 9.9e-15
# The device's bar: 16 x that, for another summation order and another libm.  Not to be widened: a miss is reported with its cause.
P_REL_BAR, BOUND_ABS_BAR = 16 * RESTATEMENT_REL, 16 * RESTATEMENT_ABS
P_TINY, P_TINY_ABS = 1e-280, 1e-300

SHAPES = ((1, 5), (2, 257), (4, 1000), (7, 2500), (24, 1031))
ALPHAS, DELTA = (0.05, 0.1, 0.2), 0.05
LAMBDAS = np.linspace(1.0, 0.0, 101)
BOUNDS = {"binomial": R.BINOMIAL, "hb": R.HB}
METHODS = {"fixed_sequence": R.FIXED_SEQUENCE, "bonferroni": R.BONFERRONI}
BOUND_CASES = ((10, 0), (10, 3), (257, 20), (1000, 999), (2500, 100), (4096, 0), (7, 7))


def _np(t):
    return t.detach().cpu().numpy()


def _ragged(E1, N):
    """tests/test_gpu_search_cost.py's: cost[e][n] = 2 e w_n + 3 (e + 1), a document's weight spans six orders of magnitude."""
    w = np.random.default_rng(1234).integers(1, 2 ** 20, N)
    e = np.arange(E1)[:, None]
    return 2 * e * w[None, :] + 3 * (e + 1)


def _paths(V, E1, lam=None):
    lam = np.linspace(1.0, 0.0, V) if lam is None else lam
    return np.ascontiguousarray(np.broadcast_to(lam[:, None], (len(lam), E1)))


@pytest.fixture(scope="module")
def tables():
    """Per shape, once: the synthetic table and the restatement's integers for the 101 shared thresholds (unit cost)."""
    out = {}
    for E1, N in SHAPES:
        conf, agree = R.synthetic_table(100 + E1, E1, N)
        loss_q = (1 - agree.astype(np.int64)) * R.ONE
        thr = _paths(101, E1, LAMBDAS)
        loss_sum, exit_sum, cost_sum, hist, exits = R.counts(conf, 1.0, loss_q, None, thr)
        out[(E1, N)] = dict(conf=conf, agree=agree, loss_q=loss_q, thr=thr, loss_sum=loss_sum, exit_sum=exit_sum, cost_sum=cost_sum, hist=hist)
    return out


def _scipy_pvalues(loss_sum, n, alpha, bound):
    out = []
    for ls in loss_sum:
        if bound == R.BINOMIAL:
            out.append(float(stats.binom.cdf(ls >> 30, n, alpha)))
        else:
            r = ls / (n * float(R.ONE))
            p_h = math.exp(-n * R.kl(r, alpha)) if r < alpha else 1.0
            out.append(min(p_h, min(1.0, math.e * float(stats.binom.cdf((ls + R.ONE - 1) >> 30, n, alpha)))))
    return np.array(out)


def _p_deviation(got, want):
    """(max relative deviation where want >= 1e-280, max absolute deviation below)"""
    big = want >= P_TINY
    rel = float((np.abs(got[big] - want[big]) / want[big]).max()) if big.any() else 0.0
    small = float(np.abs(got[~big] - want[~big]).max()) if (~big).any() else 0.0
    return rel, small


def _check(res, ref_counts, conf, alpha, delta, bound, method, tag, cost_sum=None):
    """One RiskResult against the restatement: integers equal, masks equal under the stated precondition, p-values within the bar of scipy."""
    N, V = conf.shape[1], len(ref_counts["loss_sum"])
    cost_sum = ref_counts["cost_sum"] if cost_sum is None else cost_sum
    assert res.loss_sum.dtype == np.uint64 and [int(x) for x in res.loss_sum] == ref_counts["loss_sum"], tag
    assert [int(x) for x in res.exit_sum] == ref_counts["exit_sum"] and [int(x) for x in res.cost_sum] == list(cost_sum), tag
    if res.hist is not None:
        assert res.hist.dtype == np.int32 and np.array_equal(res.hist, ref_counts["hist"]), tag
    p = R.pvalues(ref_counts["loss_sum"], N, alpha, BOUNDS[bound])
    assert R.away_from_levels(p, V, delta), (tag, "a p-value within 1e-6 relative of its level: the case is badly chosen")
    ok, n_ok, best = R.certify(p, cost_sum, delta, METHODS[method])
    assert np.array_equal(res.certified, ok) and res.n_certified == n_ok and res.selected == best, (tag, res.selected, best)
    rel, small = _p_deviation(res.pvalue, _scipy_pvalues(ref_counts["loss_sum"], N, alpha, BOUNDS[bound]))
    assert rel <= P_REL_BAR and small <= P_TINY_ABS, (tag, rel, small)
    assert np.array_equal(res.risk, np.array(ref_counts["loss_sum"]) / (float(N) * R.ONE))
    return rel


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"E1_{s[0]}_N_{s[1]}")
def test_sums_masks_and_pvalues_match_the_restatement(pkg, tables, shape):
    t = tables[shape]
    errors = np.array(t["loss_sum"]) >> 30
    if shape[0] > 1 and shape[1] >= 1000:
        assert (np.diff(errors) < 0).any() and (np.diff(errors) > 0).any()             # the error count is not monotone in lambda
    worst = 0.0
    for alpha in ALPHAS:
        for bound in BOUNDS:
            for method in METHODS:
                res = pkg.risk.risk_control((t["conf"], t["agree"]), alpha=alpha, delta=DELTA, method=method, bound=bound, want_hist=True)
                assert np.array_equal(res.thresholds, t["thr"]) and res.binary and res.num_samples == shape[1]
                worst = max(worst, _check(res, t, t["conf"], alpha, DELTA, bound, method, (shape, alpha, bound, method)))
    report_measured(f"test_sums_masks_and_pvalues_match_the_restatement[{shape}]", "device p-values vs scipy, max relative deviation", worst)


def test_costs_beyond_32_bits_a_tie_one_vector_and_three_hundred(pkg, tables):
    t = tables[(7, 2500)]
    cost = _ragged(7, 2500)
    cols = np.arange(2500)
    ragged_sum = [sum(int(c) for c in cost[R.exits_of(t["conf"], 1.0, th), cols]) for th in t["thr"]]
    assert max(ragged_sum) > 2 ** 32
    res = pkg.risk.risk_control((t["conf"], t["agree"]), alpha=0.2, delta=DELTA, cost=cost, want_hist=True)
    _check(res, t, t["conf"], 0.2, DELTA, "binomial", "fixed_sequence", "ragged", cost_sum=ragged_sum)
    assert res.selected >= 1 and res.cost_sum[res.selected] == min(ragged_sum[v] for v in range(101) if res.certified[v])
    # every vector costs the same: the tie goes to the lowest certified index
    flat = pkg.risk.risk_control((t["conf"], t["agree"]), alpha=0.2, delta=DELTA, cost=np.full((7,), 5, dtype=np.int64))
    assert flat.n_certified == res.n_certified > 1 and flat.selected == 0 and set(flat.cost_sum.tolist()) == {5 * 2500}
    # a per-exit cost vector is the (E1,N) table of its broadcast
    per_exit = pkg.risk.risk_control((t["conf"], t["agree"]), alpha=0.2, delta=DELTA, cost=np.arange(7) * 3 + 1)
    assert [int(x) for x in per_exit.cost_sum] == [3 * s + 2500 for s in t["exit_sum"]]
    # V = 1
    one = pkg.risk.risk_control((t["conf"], t["agree"]), alpha=0.2, delta=DELTA, thresholds=t["thr"][20:21], want_hist=True)
    sub = {k: t[k][20:21] for k in ("loss_sum", "exit_sum", "cost_sum", "hist")}
    assert one.selected == 0 and one.n_certified == 1
    _check(one, sub, t["conf"], 0.2, DELTA, "binomial", "fixed_sequence", "V=1")
    # V = 300: more than one pass of a 256-thread block; V = 1500: more than one pass of the selecting workgroup's 1024 threads, and
    # one workgroup per vector in the count (at 300 two share a vector, at the 101 vectors of the (7, 2500) table ten)
    s = tables[(2, 257)]
    for V in (300, 1500):
        thr = _paths(V, 2)
        loss_sum, exit_sum, cost_sum, hist, _ = R.counts(s["conf"], 1.0, s["loss_q"], None, thr)
        ref = dict(loss_sum=loss_sum, exit_sum=exit_sum, cost_sum=cost_sum, hist=hist)
        for method in METHODS:
            many = pkg.risk.risk_control((s["conf"], s["agree"]), alpha=0.2, delta=DELTA, lambdas=np.linspace(1.0, 0.0, V), method=method, want_hist=True)
            _check(many, ref, s["conf"], 0.2, DELTA, "binomial", method, (V, method))


def test_a_real_valued_loss_is_rounded_up_and_takes_hoeffding_bentkus(pkg, tables):
    t = tables[(4, 1000)]
    rng = np.random.default_rng(8)
    loss = np.clip((1 - t["conf"]) ** 2 * rng.random((4, 1000)) * 1.5, 0.0, 1.0)       # a Brier-like gap in [0, 1], zeros and ones included
    loss[3] = 0.0
    loss[0, :3] = (1.0, 2.0 ** -31, 0.0)
    q = R.quantise(loss)
    loss_sum, exit_sum, cost_sum, hist, _ = R.counts(t["conf"], 1.0, q, None, t["thr"])
    ref = dict(loss_sum=loss_sum, exit_sum=exit_sum, cost_sum=cost_sum, hist=hist)
    assert any(ls % R.ONE for ls in loss_sum)
    for method in METHODS:
        res = pkg.risk.risk_control((t["conf"], None), loss=loss, alpha=0.1, delta=DELTA, method=method, want_hist=True)
        assert res.bound == "hb" and not res.binary
        _check(res, ref, t["conf"], 0.1, DELTA, "hb", method, ("real loss", method))
        with pytest.raises(ValueError, match="not binary"):
            res.upper_bound(0)


def _scan_case(pkg, criterion, E1=5, N=300, K=8):
    """Logits, the criterion's own table, and threshold vectors made of table entries (conf == thr must not fire) and of values between."""
    logits, labels = sweep_ref_inputs(seed=31, E1=E1, N=N, K=K)
    table = _np(pkg.sweep.csf_table(logits, criterion=criterion)[0])
    rng = np.random.default_rng(2)
    med = np.median(table, axis=1)
    thr = np.stack([table[np.arange(E1), rng.integers(0, N, E1)] for _ in range(4)] + [med, np.sort(table, axis=1)[:, N // 4],
                                                                                      np.sort(table, axis=1)[:, -1], np.sort(table, axis=1)[:, 0]])
    assert sum(int((table[:E1 - 1] == th[:E1 - 1, None]).sum()) for th in thr) >= 4 * (E1 - 1)
    return logits, labels, table, thr


@pytest.mark.parametrize("criterion", ["max_confidence", "entropy", "margin"])
def test_exits_are_the_criterion_scan_s(pkg, criterion):
    logits, labels, table, thr = _scan_case(pkg, criterion)
    E1, N = table.shape
    res = pkg.risk.risk_control(logits, labels, criterion=criterion, risk="error", alpha=0.3, delta=DELTA, thresholds=thr, want_hist=True)
    wrong = logits.argmax(-1) != labels[None, :]
    sign = -1.0 if criterion == "entropy" else 1.0
    for v, th in enumerate(thr):
        exits, _, _, counts = pkg.criterion_scan_device(logits, th, criterion)
        ex = _np(exits).astype(np.int64)
        assert np.array_equal(res.hist[v], _np(counts)) and np.array_equal(np.bincount(ex, minlength=E1), res.hist[v]), (criterion, v)
        assert int(res.exit_sum[v]) == int(ex.sum()) and int(res.loss_sum[v]) == int(wrong[ex, np.arange(N)].sum()) * R.ONE, (criterion, v)
        assert np.array_equal(ex, R.exits_of(table, sign, th)), (criterion, v)
    # the other binary risks, from the same correct table: against the full model's own answers, and wrong where the full model is right
    v = 4
    ex = R.exits_of(table, sign, thr[v])
    final = logits[-1].argmax(-1)
    cons = pkg.risk.risk_control(logits, criterion=criterion, risk="consistency", alpha=0.3, delta=DELTA, thresholds=thr)
    gap = pkg.risk.risk_control(logits, labels, criterion=criterion, risk="gap", alpha=0.3, delta=DELTA, thresholds=thr)
    assert int(cons.loss_sum[v]) == int((logits.argmax(-1)[ex, np.arange(N)] != final).sum()) * R.ONE
    assert int(gap.loss_sum[v]) == int((wrong[ex, np.arange(N)] & ~wrong[-1]).sum()) * R.ONE
    assert np.array_equal(cons.exit_sum, res.exit_sum) and np.array_equal(gap.exit_sum, res.exit_sum)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_a_nan_criterion_never_fires_on_a_table(pkg, sign):
    """A precomputed table with NaN entries and a whole NaN column, against the scans that take a table: ee_gate_scan ('>') and ee_lte_scan
    ('<'), which are ee_criterion_scan's kernel reading its criterion from memory."""
    conf, agree = R.synthetic_table(9, 4, 300)
    conf[1, 5], conf[0, 6], conf[:, 7] = np.nan, np.nan, np.nan
    thr = np.stack([np.full(4, 0.5), conf[:, 20], np.array([0.9, 0.1, 0.5, np.nan]), np.full(4, np.nan)])
    thr[1, 1] = conf[1, 21]
    pair = (-conf if sign < 0 else conf, agree)                                        # the pair form hands a '<' table over negated (as_csf)
    res = pkg.risk.risk_control(pair, criterion="entropy" if sign < 0 else "max_confidence", alpha=0.3, delta=DELTA, thresholds=thr, want_hist=True)
    dummy = np.zeros((4, 300, 2))
    for v, th in enumerate(thr):
        scan = pkg.lte_scan_device(conf, dummy, th)[0] if sign < 0 else pkg.gate_scan_device(conf, dummy, th)[0]
        ex = _np(scan).astype(np.int64)
        assert np.array_equal(ex, R.exits_of(conf, sign, th)) and ex[7] == 3, v
        assert np.array_equal(res.hist[v], np.bincount(ex, minlength=4)), v
        assert int(res.loss_sum[v]) == int((1 - agree.astype(np.int64))[ex, np.arange(300)].sum()) * R.ONE, v
    assert res.hist[3].tolist() == [0, 0, 0, 300]


def test_fixed_sequence_against_bonferroni_on_a_path_that_recovers(pkg):
    conf, agree = R.synthetic_table(11, 2, 1000)
    thr = np.array([[1.0, 0.0], [0.9, 0.0], [0.0, 0.0], [0.95, 0.0]])
    loss_sum, exit_sum, cost_sum, hist, _ = R.counts(conf, 1.0, (1 - agree.astype(np.int64)) * R.ONE, None, thr)
    ref = dict(loss_sum=loss_sum, exit_sum=exit_sum, cost_sum=cost_sum, hist=hist)
    fs = pkg.risk.risk_control((conf, agree), alpha=0.1, delta=DELTA, thresholds=thr, method="fixed_sequence", want_hist=True)
    bf = pkg.risk.risk_control((conf, agree), alpha=0.1, delta=DELTA, thresholds=thr, method="bonferroni", want_hist=True)
    _check(fs, ref, conf, 0.1, DELTA, "binomial", "fixed_sequence", "fs")
    _check(bf, ref, conf, 0.1, DELTA, "binomial", "bonferroni", "bf")
    assert fs.certified.tolist() == [True, True, False, False] and bf.certified.tolist() == [True, True, False, True]
    assert fs.pvalue[3] <= DELTA / 4 < DELTA < fs.pvalue[2] and fs.selected == bf.selected == 1
    assert fs.select() == [0.9, 0.0]


def test_58_documents_certify_nothing_and_59_everything(pkg):
    for n, want in ((58, False), (59, True)):
        conf = np.random.default_rng(n).random((3, n))
        ones = np.ones((3, n), dtype=np.uint8)
        for bound in BOUNDS:
            res = pkg.risk.risk_control((conf, ones), alpha=0.05, delta=0.05, lambdas=np.linspace(1, 0, 11), bound=bound)
            assert res.n_certified == (11 if want else 0) and res.certified.all() == want and res.selected == (10 if want else -1), (n, bound)
            assert res.pvalue[0] == pytest.approx(0.95 ** n, rel=P_REL_BAR)
            if want:
                assert res.select() == [0.0, 0.0, 0.0]
            else:
                with pytest.raises(ValueError, match="= 59 calibration documents"):
                    res.select()


def test_a_bad_loss_fails_the_call_with_the_outputs_untouched(pkg):
    import torch
    lib = pkg.capi.load()
    E1, N, V = 3, 500, 7
    conf, _ = R.synthetic_table(4, E1, N)
    cf, th = torch.from_numpy(conf).cuda(), torch.from_numpy(_paths(V, E1)).cuda()
    good = np.random.default_rng(0).random((E1, N))
    ptr = lambda x: C.c_void_p(x.data_ptr())

    def run(loss, bound):
        ls = torch.from_numpy(np.ascontiguousarray(loss)).cuda()
        outs = [torch.full((V,), -7, dtype=torch.int64, device="cuda") for _ in range(3)] + [torch.full((V, E1), -7, dtype=torch.int32, device="cuda"),
                torch.full((V,), -7.0, dtype=torch.float64, device="cuda"), torch.full((V,), 77, dtype=torch.uint8, device="cuda"),
                torch.full((1,), -7, dtype=torch.int32, device="cuda"), torch.full((1,), -7, dtype=torch.int32, device="cuda")]
        rc = lib.ee_risk_control(ptr(cf), 1.0, ptr(ls), None, None, E1, N, ptr(th), V, 0.1, 0.05, bound, 0, *[ptr(o) for o in outs],
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc, pkg.capi.last_error() if rc else "", [_np(o) for o in outs]

    for value, bound, words in ((1.5, 1, "outside [0, 1]"), (-1e-300, 1, "outside [0, 1]"), (np.nan, 1, "not finite"), (np.inf, 1, "not finite"),
                                (0.5, 0, "not 0 or 1")):
        loss = good.copy() if bound == 1 else (good < 0.3).astype(np.float64)
        loss[E1 - 1, N - 1] = value
        rc, msg, outs = run(loss, bound)
        assert rc != 0 and words in msg and "no output was written" in msg, (value, msg)
        assert all((o == (77 if o.dtype == np.uint8 else -7)).all() for o in outs), value
    rc, _, outs = run(good, 1)
    assert rc == 0 and (outs[0] >= 0).all() and outs[6][0] >= 0 and (outs[5] <= 1).all()
    with pytest.raises(pkg.capi.MMEEError, match="not 0 or 1"):
        pkg.risk.risk_control((conf, None), loss=good, bound="binomial", alpha=0.1, delta=0.05)
    binary = pkg.risk.risk_control((conf, None), loss=(good < 0.02).astype(np.float64), bound="binomial", alpha=0.1, delta=0.05)
    same = pkg.risk.risk_control((conf, (good >= 0.02).astype(np.uint8)), alpha=0.1, delta=0.05)
    assert binary.binary and np.array_equal(binary.loss_sum, same.loss_sum) and np.array_equal(binary.pvalue, same.pvalue)


def test_binomial_bounds_against_scipy_and_bit_for_bit_again(pkg):
    n, k = np.array([c[0] for c in BOUND_CASES]), np.array([c[1] for c in BOUND_CASES])
    up, low = pkg.risk.binomial_bounds(n, k, DELTA)
    up2, low2 = pkg.risk.binomial_bounds(n, k, DELTA)
    assert np.array_equal(up.view(np.int64), up2.view(np.int64)) and np.array_equal(low.view(np.int64), low2.view(np.int64))
    worst = 0.0
    for i, (ni, ki) in enumerate(BOUND_CASES):
        want_up = 1.0 if ki == ni else float(stats.beta.ppf(1 - DELTA, ki + 1, ni - ki))
        want_low = 0.0 if ki == 0 else float(stats.beta.ppf(DELTA, ki, ni - ki + 1))
        worst = max(worst, abs(up[i] - want_up), abs(low[i] - want_low))
        assert low[i] <= ki / ni <= up[i]
        one = pkg.risk.binomial_bounds(ni, ki, DELTA)                                  # a query alone has the bits it has in a batch
        assert isinstance(one[0], float) and (np.float64(one[0]).view(np.int64), np.float64(one[1]).view(np.int64)) == \
            (up[i].view(np.int64), low[i].view(np.int64))
    report_measured("test_binomial_bounds_against_scipy_and_bit_for_bit_again", "device bounds vs scipy.stats.beta.ppf, max absolute deviation", worst)
    assert up[6] == 1.0 and low[0] == 0.0 and low[5] == 0.0
    assert worst <= BOUND_ABS_BAR, worst


@pytest.fixture(scope="module")
def ramp(pkg):
    import torch
    cfg = pkg.ModelConfig.tiny(EE_config=dict(TINY_CASES["tiny_ramp"]))
    W = pkg.synth.make_weights(cfg, seed=21, head_gain=4.0)
    B, T = 64, 16
    docs = pkg.synth.make_documents(cfg, B, seed=22, text_len=T, min_words=2)
    t = {k: torch.from_numpy(np.ascontiguousarray(docs[k])).cuda() for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}
    eng = pkg.EarlyExitEngine(cfg, xprobe=False, max_docs=B, max_text_len=T, precision="fp32")
    eng.load_weights(W)
    dump = eng.forward(**t, dump_all=True, want_all=True)
    yield eng, t, dump.all_logits.clone(), B
    eng.close()


def test_consistency_with_delta_adds_lower_bounds_and_changes_nothing_else(pkg, ramp):
    eng, t, all_logits, B = ramp
    conf = _np(pkg.sweep.csf_table(all_logits)[0])
    thr = np.median(conf, axis=1)
    assert np.abs(conf - thr[:, None]).min() > 1e-9
    out = eng.forward(**t, want_all=True, thresholds=thr.tolist(), audit_fraction=0.75, audit_seed=5)
    eng.set_audit(None)
    sample = pkg.audit.sample(out)
    plain, bounded = pkg.audit.consistency(sample), pkg.audit.consistency(sample, delta=DELTA)
    assert plain.rate_lower is None and plain.pooled_rate_lower is None and plain.pooled_delivered >= 10
    for name in ("delivered", "agree", "rate"):
        assert np.array_equal(getattr(plain, name), getattr(bounded, name), equal_nan=True), name
    assert (plain.num_samples, plain.pooled_delivered, plain.pooled_agree) == (bounded.num_samples, bounded.pooled_delivered, bounded.pooled_agree)
    assert np.float64(plain.pooled_rate).view(np.int64) == np.float64(bounded.pooled_rate).view(np.int64)
    d, a = plain.delivered, plain.agree
    at = np.nonzero(d > 0)[0]
    assert len(at) >= 2 and np.isnan(bounded.rate_lower[d == 0]).all()
    assert (bounded.rate_lower[at] <= plain.rate[at]).all() and bounded.pooled_rate_lower <= plain.pooled_rate
    want = 1.0 - pkg.risk.binomial_bounds(np.append(d[at], plain.pooled_delivered), np.append(d[at] - a[at], plain.pooled_delivered - plain.pooled_agree),
                                          DELTA)[0]
    assert np.array_equal(bounded.rate_lower[at], want[:-1]) and bounded.pooled_rate_lower == want[-1]
    for e in at:
        assert bounded.rate_lower[e] == pytest.approx(1.0 - R.bounds(int(d[e]), int(d[e] - a[e]), DELTA)[0], abs=BOUND_ABS_BAR)
    # certify is risk_control on the sample's table with the label-free risk
    cert = pkg.audit.certify(sample, 0.3, 0.2, want_hist=True)
    same = pkg.risk.risk_control(sample.logits, sample.references(), risk="error", alpha=0.3, delta=0.2, want_hist=True)
    assert cert.num_samples == sample.num_samples and np.array_equal(cert.loss_sum, same.loss_sum) and np.array_equal(cert.hist, same.hist)
    assert np.array_equal(cert.pvalue, same.pvalue) and cert.selected == same.selected


def test_end_to_end_the_selected_thresholds_run_in_a_forward(pkg, ramp):
    eng, t, all_logits, B = ramp
    res = pkg.risk.risk_control(all_logits, alpha=0.3, delta=0.2, want_hist=True)
    assert res.n_certified >= 2 and res.selected >= 1, res.pvalue[:5]
    thr = res.select()
    E1 = all_logits.shape[0]
    assert isinstance(thr, list) and len(thr) == E1 and all(type(x) is float for x in thr)
    conf = _np(pkg.sweep.csf_table(all_logits)[0])
    assert np.abs(conf[:E1 - 1] - np.array(thr)[:E1 - 1, None]).min() > 1e-6          # no criterion within rounding of its threshold
    out = eng.forward(**t, thresholds=thr)
    ex = _np(out.exit_layer).astype(np.int64)
    assert np.array_equal(np.bincount(ex, minlength=E1), res.hist[res.selected]) and int(ex.sum()) == int(res.exit_sum[res.selected])
    final = _np(all_logits)[-1].argmax(-1)
    assert int((_np(out.logits).argmax(-1) != final).sum()) * R.ONE == int(res.loss_sum[res.selected])
    assert 0.0 <= res.risk[res.selected] <= res.upper_bound() <= 1.0
    # a front found elsewhere, deepest first, is a path
    front = pkg.sweep.threshold_search(all_logits, pkg.sweep.final_predictions(all_logits), num_per_exit=3, mixtures=200, seed=1)
    path = pkg.risk.path_from_front(front)
    assert path.shape == (len(front.front_vector), E1) and np.array_equal(path[0], front.front_thresholds[-1])
    along = pkg.risk.risk_control(all_logits, alpha=0.3, delta=0.2, thresholds=path)
    assert [int(x) for x in along.exit_sum] == [int(x) for x in front.front_exit_sum[::-1]]
