"""CPU checks of budgeted exits (include/mmee.h MMEE_QUOTA_*): properties of the numpy restatement tests/quota_ref.py -- the oracle of
tests/test_gpu_quota.py -- and of the host helpers ``sweep.quotas_from_fractions`` / ``sweep.budget_quotas``; the C-ABI's declarations and
the refusals that need no device."""
import os
import re

import numpy as np
import pytest

from . import csf_ref
from . import quota_ref as Q
from .conftest import ROOT, sweep_ref_inputs

NEW_SYMBOLS = ("ee_set_quotas", "ee_has_quotas", "ee_quota_scan", "ee_debug_exit_quota")


def _criteria(rng, n, ties=True, nans=True):
    """Criteria with everything the order has to handle: ties (duplicated values), +-0, +-inf and NaNs."""
    c = rng.standard_normal(n)
    if ties and n > 3:
        c[rng.integers(0, n, n // 3)] = c[rng.integers(0, n, n // 3)]
        c[rng.integers(0, n, 2)] = (0.0, -0.0)
    if n > 6:
        c[rng.integers(0, n, 2)] = (np.inf, -np.inf)
    if nans and n > 2:
        c[rng.integers(0, n, max(1, n // 10))] = np.nan
    return c


@pytest.mark.parametrize("sign", [+1, -1])
@pytest.mark.parametrize("n", [0, 1, 2, 7, 64, 257, 1000])
def test_rank_is_a_permutation_and_counts_the_header_s_relation(n, sign):
    rng = np.random.default_rng(n + 5 * (sign + 1))
    c = _criteria(rng, n)
    slots = rng.permutation(n + 9)[:n]
    r = Q.rank(c, sign, slots)
    assert np.array_equal(np.sort(r), np.arange(n))
    P = Q.precedes(c, sign, slots)
    assert np.array_equal(r, P.sum(0))                                   # rank_i = #{j : j precedes i}
    assert not (P & P.T).any() and (P | P.T | np.eye(n, dtype=bool)).all()      # a strict total order
    nan = np.isnan(c)
    if nan.any() and (~nan).any():
        assert r[nan].min() > r[~nan].max()                              # NaNs rank last ...
        assert np.array_equal(np.argsort(r[nan]), np.argsort(slots[nan]))       # ... by slot among themselves
    for v in np.unique(c[~nan]):                                         # ties: the lower slot first
        idx = np.nonzero(c == v)[0]
        assert np.array_equal(np.argsort(r[idx]), np.argsort(slots[idx]))


def test_signed_zeros_tie_and_the_sign_reverses_the_order():
    c = np.array([0.0, -0.0, 1.0, -1.0])
    assert Q.rank(c, +1).tolist() == [1, 2, 0, 3] and Q.rank(c, -1).tolist() == [1, 2, 3, 0]


@pytest.mark.parametrize("G", [1, 7, 100, None])
def test_exact_releases_min_q_n_at_every_exit(G):
    store, _ = sweep_ref_inputs(seed=3, E1=6, N=400, K=5)
    table = csf_ref.max_softmax(store)
    table[2, 17] = np.nan
    rng = np.random.default_rng(1)
    for trial in range(6):
        g = G or 400
        quotas = rng.integers(0, max(2, g // 2), 5).tolist() if trial else [0, g + 5, 0, 0, 3]
        ex, cuts = Q.scan(table, +1, quotas, Q.EXACT, G=G)
        for s in range(0, 400, g):
            ng = min(g, 400 - s)
            sizes = Q.stage_sizes(ng, quotas)
            hist = np.bincount(ex[s:s + g], minlength=6)
            assert hist[:5].tolist() == [min(q, n) for q, n in zip(quotas, sizes)], (trial, s)
            assert hist[5] == sizes[5]
        # the cuts bracket the boundary in the criterion's direction wherever both sides exist and are numbers
        both = ~np.isnan(cuts).any(-1)
        assert (cuts[..., 0][both] >= cuts[..., 1][both]).all()


@pytest.mark.parametrize("criterion", csf_ref.CRITERIA)
def test_at_least_with_zero_quotas_is_the_threshold_scan(criterion):
    store, _ = sweep_ref_inputs(seed=4, E1=7, N=500, K=6)
    table, sign = csf_ref.csf(store, criterion), csf_ref.SIGN[criterion]
    thr, _ = csf_ref.gap_thresholds(table, 0.7 if sign > 0 else 0.3, 1e-9)
    for G in (1, 33, None):
        ex, _ = Q.scan(table, sign, [0] * 6, Q.AT_LEAST, thr, G=G)
        assert np.array_equal(ex, csf_ref.exits(table, thr, sign))


@pytest.mark.parametrize("sign", [+1, -1])
def test_at_least_never_keeps_a_document_exact_would_release(sign):
    store, _ = sweep_ref_inputs(seed=5, E1=6, N=300, K=4)
    table = csf_ref.csf(store, "max_confidence" if sign > 0 else "entropy")
    rng = np.random.default_rng(2)
    for trial in range(8):
        quotas = rng.integers(0, 40, 5).tolist()
        thr = np.quantile(table, rng.uniform(0.2, 0.9), axis=1)
        G = (None, 50)[trial % 2]
        ex_exact, _ = Q.scan(table, sign, quotas, Q.EXACT, G=G)
        ex_least, _ = Q.scan(table, sign, quotas, Q.AT_LEAST, thr, G=G)
        assert (ex_least <= ex_exact).all()
        # one exit of one stage: whoever EXACT releases, AT_LEAST releases
        lv_e, _ = Q.leave(table[0], sign, quotas[0], Q.EXACT)
        lv_a, _ = Q.leave(table[0], sign, quotas[0], Q.AT_LEAST, thr[0])
        assert not (lv_e & ~lv_a).any() and lv_a.sum() == max(lv_e.sum(), Q.fires(table[0], sign, thr[0]).sum())


def test_quota_fractions_rounding_never_drifts(pkg):
    rng = np.random.default_rng(9)
    R = lambda x: int(np.floor(x + 0.5))
    for trial in range(1000):
        B, E = int(rng.integers(0, 5000)), int(rng.integers(1, 12))
        f = rng.random(E) * rng.random()
        f = f / max(1.0, f.sum() / rng.uniform(0.3, 1.0))
        if trial % 10 == 0:
            f = f / f.sum()                                              # shares that sum to 1 (up to rounding)
        q = pkg.sweep.quotas_from_fractions(B, f)
        assert q == Q.quotas_from_fractions(B, f) and len(q) == E and min(q) >= 0
        cum = np.cumsum(f)
        assert sum(q) == R(B * cum[-1]) and sum(q) <= B
        assert [sum(q[:e + 1]) for e in range(E)] == [R(B * c) for c in cum]      # every prefix, not only the total
    assert pkg.sweep.quotas_from_fractions(10, [0.25, 0.25, 0.25, 0.25], num_exits=3) == [3, 2, 3]     # R(2.5) = 3, R(5) = 5, R(7.5) = 8
    assert pkg.sweep.quotas_from_fractions(7, [0.5, 0.5]) == [4, 3]
    for bad in ([0.7, 0.6], [-0.1, 0.2], [np.nan]):
        with pytest.raises(ValueError, match="shares"):
            pkg.sweep.quotas_from_fractions(10, bad)
    with pytest.raises(ValueError, match="exits below"):
        pkg.sweep.quotas_from_fractions(10, [0.1] * 5, num_exits=3)


def test_budget_quotas_meets_its_budget_and_refuses_what_is_out_of_range(pkg):
    rng = np.random.default_rng(11)
    for trial in range(200):
        E1 = int(rng.integers(2, 13))
        cost = np.cumsum(rng.uniform(0.1, 5.0, E1))
        budget = float(rng.uniform(cost[0], cost[-1])) if trial % 20 else (cost[0], cost[-1])[(trial // 20) % 2]
        B = int(rng.integers(1, 3000))
        quotas, p, q = pkg.sweep.budget_quotas(cost, budget, B)
        assert abs(float(p @ cost) - budget) <= 1e-9, (trial, float(p @ cost), budget)
        assert abs(p.sum() - 1.0) <= 1e-12 and (p >= 0).all() and q >= 0            # q = 0 / inf: everybody at the first / the final exit
        ratio = p[1:] / np.maximum(p[:-1], 1e-300)
        big = p[:-1] > 1e-200
        assert np.allclose(ratio[big], q, rtol=1e-9)                     # geometric
        assert quotas == Q.quotas_from_fractions(B, p[:-1]) and len(quotas) == E1 - 1 and sum(quotas) <= B
        # the integer quotas spend the budget up to the rounding of B documents: at most one document per exit off the shares
        hist = np.array(quotas + [B - sum(quotas)])
        assert np.abs(hist - B * p).max() <= 1.0 + 1e-9
    cost = np.array([1.0, 2.0, 4.0, 8.0])
    for bad in (0.99, 8.01, -1.0, np.nan):
        with pytest.raises(ValueError, match="outside"):
            pkg.sweep.budget_quotas(cost, bad, 100)
    quotas, p, q = pkg.sweep.budget_quotas(cost, None, 100, q=1.0)        # q given: uniform shares, the budget is not read
    assert np.allclose(p, 0.25) and quotas == [25, 25, 25]
    with pytest.raises(ValueError, match="non-decreasing"):
        pkg.sweep.budget_quotas([1.0, 0.5], 0.7, 10)


def test_the_c_abi_declares_the_new_entry_points_and_the_binding_knows_them(pkg):
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    declared = set(re.findall(r"^\w[\w\s\*]*?\b(ee_\w+)\s*\(", header, flags=re.M))
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg.capi.SYMBOLS, name
    assert re.search(r"MMEE_QUOTA_OFF = 0, MMEE_QUOTA_EXACT = 1, MMEE_QUOTA_AT_LEAST = 2", header)
    assert (pkg.capi.QUOTA_EXACT, pkg.capi.QUOTA_AT_LEAST) == (Q.EXACT, Q.AT_LEAST)
    # the header says, in these words, that only where a document leaves depends on its batch mates
    flat = re.sub(r"[\s\*]+", " ", header)
    assert "A document's logits still do not depend on its batch mates. Only WHERE IT LEAVES does" in flat
    lib = pkg.capi.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    # the stand-alone hook's struct is the decide hook's with four fields behind it
    import ctypes as C
    assert C.sizeof(pkg.capi.DebugExitQuotaArgs) == C.sizeof(pkg.capi.DebugExitDecideArgs) + 8 + 2 * C.sizeof(C.c_void_p)


def test_refusals_that_need_no_device(pkg):
    lib = pkg.capi.load()
    import ctypes as C
    q = (C.c_int32 * 2)(1, -1)
    thr = (C.c_double * 3)(0.5, 0.5, 0.5)
    cases = [(dict(sign=0.5), "sign"), (dict(E1=0), "E1"), (dict(G=0), "G >= 1"), (dict(mode=3), "unknown mode"), (dict(mode=2, thr=None), "needs the thresholds"),
             (dict(), r"quotas\[1\]=-1")]
    for over, match in cases:
        a = dict(sign=1.0, E1=3, N=0, mode=1, thr=thr, G=4)
        a.update(over)
        rc = lib.ee_quota_scan(None, a["sign"], a["E1"], a["N"], q, a["mode"], a["thr"], a["G"], None, None, None, None)
        assert rc != 0 and re.search(match, pkg.capi.last_error()), (over, pkg.capi.last_error())
    args = pkg.capi.DebugExitQuotaArgs()
    args.decide.mode, args.decide.rule = 1, 0
    assert lib.ee_debug_exit_quota(C.byref(args), None) != 0 and "mode must be 0" in pkg.capi.last_error()
    args.decide.mode, args.decide.is_final = 0, 1
    assert lib.ee_debug_exit_quota(C.byref(args), None) != 0 and "is_final" in pkg.capi.last_error()
    args.decide.is_final, args.quota_mode = 0, 0
    assert lib.ee_debug_exit_quota(C.byref(args), None) != 0 and "quota_mode" in pkg.capi.last_error()
    args.quota_mode, args.quota = 1, -2
    assert lib.ee_debug_exit_quota(C.byref(args), None) != 0 and "negative" in pkg.capi.last_error()
    args.quota = 2
    assert lib.ee_debug_exit_quota(C.byref(args), None) != 0 and "crit and rank" in pkg.capi.last_error()
