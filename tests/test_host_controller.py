"""Online exit control without a device: the restatement (tests/controller_ref.py) keeps the promise of include/mmee.h at every prefix, on the
three tables that matter; the log's word layout; the header's text; and the refusals that come before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import audit_ref as A
from . import controller_ref as CR
from .conftest import ROOT

NEW_SYMBOLS = ("ee_set_controller", "ee_has_controller", "ee_controller_state", "ee_controller_log", "ee_rolling_control", "ee_debug_audit_tally",
               "ee_debug_controller_step")
# The promise is an inequality of real numbers; the restatement sums T <= 400 float64 terms of magnitude <= 1, each quotient and each
# partial sum rounded once: at most 2 T ulps of 400 = 2 x 400 x 2^-44 < 1e-10 between the float sum and the real one.
SLACK = 1e-10


def _path(V, E1, sign):
    lam = np.linspace(0.95, 0.05, V) if sign > 0 else np.linspace(0.05, 1.3, V)
    return np.repeat(lam[:, None], E1, axis=1)


def _table(kind, E1, N, sign, seed):
    rng = np.random.default_rng(seed)
    conf = rng.uniform(0.0, 1.0, (E1, N)) if sign > 0 else rng.uniform(0.0, 1.4, (E1, N))
    if kind == "all_wrong":
        bad = np.ones((E1, N), np.uint8)
    elif kind == "none_wrong":
        bad = np.zeros((E1, N), np.uint8)
    else:
        bad = (rng.random((E1, N)) < 0.35).astype(np.uint8)
    return conf, bad


@pytest.mark.parametrize("kind", ["all_wrong", "none_wrong", "random"])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_the_inequality_holds_at_every_prefix(kind, sign):
    E1, V = 4, 7
    for (N, G, fraction, alpha, gamma, p0, seed) in ((4000, 16, 0.5, 0.1, 1.0, 2.0, 3), (3000, 8, 0.25, 0.05, 0.5, 6.0, 11), (2000, 5, 1.0, 0.3, 2.5, 0.0, 5),
                                                     (1200, 64, 0.1, 0.2, 0.3, 3.5, 7)):
        conf, bad = _table(kind, E1, N, sign, seed)
        path = _path(V, E1, sign)
        exits, log, p_end = CR.rolling(conf, bad, path, sign=sign, cut=A.cut_of(fraction), seed=seed, alpha=alpha, gamma=gamma, p0=p0, G=G)
        T = -(-N // G)
        assert log["call"].tolist() == list(range(T)) and exits.shape == (N,) and T <= 400
        ex = CR.excess(log, alpha)
        assert (ex <= CR.bound(p0, gamma, alpha) + SLACK).all(), (kind, sign, float(ex.max()), CR.bound(p0, gamma, alpha))
        # the argument itself: p never falls below -gamma (1 - alpha), never rises above V - 1, and below 0 nobody leaves early
        assert (log["p_after"] >= -gamma * (1 - alpha) - SLACK).all() and (log["p_after"] <= V - 1).all()
        below = log["p_before"] < 0
        assert (log["disagree"][below] == 0).all() and (log["delivered"][below] == 0).all()
        assert np.isinf(log["thresholds"][below][:, :E1 - 1]).all() and (np.sign(log["thresholds"][below][:, :E1 - 1]) == sign).all()
        assert np.array_equal(log["p_before"][1:], log["p_after"][:-1]) and log["p_before"][0] == p0 and p_end == log["p_after"][-1]
        assert (log["disagree"] <= log["delivered"].sum(1)).all() and (log["delivered"].sum(1) <= log["sampled"]).all()
        assert np.array_equal(log["delivered"].sum(1) - log["agree"].sum(1), log["disagree"])
        if kind == "all_wrong" and T >= 100 * max(1.0, p0 / gamma):         # enough calls: the loop is driven below 0 and comes back
            assert below.any() and (log["p_before"][np.nonzero(below)[0][0]:] >= 0).any()
        if kind == "none_wrong":
            assert (log["disagree"] == 0).all() and (np.diff(log["p_after"]) >= 0).all()
            assert p_end == V - 1 or T * gamma * alpha < V - 1 - p0 + 1                 # the clamp, once there were calls enough to reach it


def test_thresholds_and_step_of_the_restatement():
    path = np.array([[0.875, 0.75, 0.5], [0.625, 0.75, 0.5], [0.125, 0.25, 0.25]])              # dyadic: every lerp below is exact
    assert np.array_equal(CR.thresholds(path, 0.0, 1.0), [0.875, 0.75, 0.5]) and np.array_equal(CR.thresholds(path, 2.0, 1.0), [0.125, 0.25, 0.5])
    assert np.array_equal(CR.thresholds(path, 7.5, 1.0), [0.125, 0.25, 0.5])                    # clamped at V - 1: row V - 2 at t = 1
    assert np.array_equal(CR.thresholds(path, 1.0, 1.0), [0.625, 0.75, 0.5])                    # an integer position: the row itself, t = 0
    t = CR.thresholds(path, 0.25, 1.0)
    assert t[0] == 0.875 + (0.625 - 0.875) * 0.25 and t[1] == 0.75 and t[2] == 0.5
    u = CR.thresholds(np.array([[0.9, 0.5], [0.1, 0.5]]), 1.0 / 3.0, 1.0)                       # not exact: the product is rounded, then the sum
    assert u[0] == np.float64(0.9) + (np.float64(0.1) - np.float64(0.9)) * (np.float64(1.0) / np.float64(3.0))
    assert np.array_equal(CR.thresholds(path, -1e-300, 1.0), [np.inf, np.inf, 0.5]) and np.array_equal(CR.thresholds(path, -3.0, -1.0), [-np.inf, -np.inf, 0.5])
    assert CR.step(1.5, 0, 0, 0.1, 1.0, 3) == 1.5 and CR.step(1.5, 4, 4, 0.1, 1.0, 3) == 1.5 - 1.0 * (1.0 - 0.1)
    assert CR.step(1.95, 8, 0, 0.1, 1.0, 3) == 2.0 and CR.step(0.05, 3, 1, 0.1, 2.0, 3) == 0.05 - 2.0 * (np.float64(1) / np.float64(3) - 0.1)
    assert CR.first_argmax(np.array([[1.0, 3.0, 3.0], [np.nan, 5.0, 1.0], [-0.0, 0.0, -1.0]], np.float32)).tolist() == [1, 2, 0]


def test_log_rows_parse_into_the_dataclass(pkg):
    E1 = 4
    _, log, _ = CR.rolling(*_table("random", E1, 300, 1.0, 2), _path(5, E1, 1.0), sign=1.0, cut=A.cut_of(0.5), seed=9, alpha=0.1, gamma=1.0, p0=2.0, G=16)
    T = len(log["call"])
    f = lambda a: np.ascontiguousarray(a, np.float64).view(np.int64)
    rows = np.concatenate([log["call"][:, None], f(log["p_before"])[:, None], f(log["p_after"])[:, None], log["sampled"][:, None], log["disagree"][:, None],
                           log["delivered"], log["agree"], f(log["thresholds"])], axis=1).astype(np.int64)
    assert rows.shape == (T, CR.log_words(E1)) and pkg.capi.controller_log_words(E1) == CR.log_words(E1)
    got = pkg.ControllerLog.from_rows(rows, E1)
    for k in ("call", "p_before", "p_after", "sampled", "disagree", "delivered", "agree", "thresholds"):
        assert np.array_equal(np.asarray(getattr(got, k)).view(np.int64), np.asarray(log[k]).view(np.int64)), k
    assert np.allclose(got.excess(0.1), CR.excess(log, 0.1), rtol=0, atol=1e-12)
    assert np.array_equal(np.isnan(got.loss), log["sampled"] == 0)


def test_header_declares_the_entry_points_and_states_the_promise(pkg):
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    declared = set(re.findall(r"^\w[\w\s\*]*?\b(ee_\w+)\s*\(", header, flags=re.M))
    lib = pkg.capi.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg.capi.SYMBOLS and hasattr(lib, name), name
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", header))
    for words in ("sum_{t <= T} (l_t - alpha) <= p0 / gamma + 1 - alpha", "while p < 0 nobody leaves early", "The bound is on the AUDITED estimate",
                  "nothing is promised for a single call", "with no exchangeability assumed", "p <- min(V - 1, p - gamma ((double)disagree / (double)sampled - alpha))",
                  "(seed + t) mod 2^32", "a row with a NaN counts as K - 1", "Not built: controllers under captured graphs",
                  "one controller shared across ranks"):
        assert words in flat, words
    src = open(os.path.join(ROOT, "multi-modal-early-exit_amd", "csrc", "Makefile")).read()
    assert "controller.hip" in src


def test_c_refusals_come_before_any_device_call(pkg):
    lib = pkg.capi.load()
    buf = (C.c_double * 16)()
    p = C.cast(buf, C.c_void_p)

    def call(**kw):
        a = dict(table=p, sign=1.0, bad=p, E1=3, N=8, path=p, V=2, cut=1 << 31, seed=0, alpha=0.1, gamma=1.0, p0=0.0, G=4, exits=p, log=p, p_out=None)
        a.update(kw)
        assert lib.ee_rolling_control(*a.values(), None) != 0
        return pkg.capi.last_error()

    assert "NULL argument" in call(table=None) and "NULL argument" in call(bad=None) and "NULL argument" in call(log=None)
    assert "2 <= E1 <= 64" in call(E1=1) and "2 <= E1 <= 64" in call(E1=65)
    assert "1 <= N < 2^28" in call(N=0) and "a group holds at least one document" in call(G=0)
    assert "2 <= V" in call(V=1) and "sign is +1 or -1" in call(sign=0.0)
    assert "outside [1, 2^32]" in call(cut=0) and "outside [1, 2^32]" in call(cut=(1 << 32) + 1)
    assert "alpha" in call(alpha=0.0) and "alpha" in call(alpha=1.0) and "gamma" in call(gamma=0.0) and "gamma" in call(gamma=float("inf"))
    assert "p0 = 1.5 outside [0, V - 1 = 1]" in call(p0=1.5) and "outside" in call(p0=-0.1) and "outside" in call(p0=float("nan"))
    t, s = pkg.capi.DebugAuditTallyArgs(), pkg.capi.DebugControllerStepArgs()
    assert lib.ee_debug_audit_tally(None, None) != 0 and "args must not be NULL" in pkg.capi.last_error()
    assert lib.ee_debug_audit_tally(C.byref(t), None) != 0 and "must not be NULL" in pkg.capi.last_error()
    assert lib.ee_debug_controller_step(C.byref(s), None) != 0 and "path, state, tally and thr must not be NULL" in pkg.capi.last_error()
    assert lib.ee_has_controller(None) == 0


def test_python_refusals_need_no_device(pkg):
    risk = pkg.risk
    z, path = np.zeros((3, 8, 2)), np.array([[0.9, 0.9, 0.5], [0.1, 0.1, 0.5]])
    kw = dict(alpha=0.1, gamma=1.0, group_size=4, fraction=0.5)
    with pytest.raises(ValueError, match="not a threshold criterion"):
        risk.rolling_control(z, path, criterion="patience", **kw)
    with pytest.raises(ValueError, match=r"alpha must lie in \(0, 1\)"):
        risk.rolling_control(z, path, **dict(kw, alpha=1.0))
    with pytest.raises(ValueError, match="gamma must be positive and finite"):
        risk.rolling_control(z, path, **dict(kw, gamma=0.0))
    with pytest.raises(ValueError, match="gamma must be positive and finite"):
        risk.rolling_control(z, path, **dict(kw, gamma=float("inf")))
    with pytest.raises(ValueError, match="at least one document"):
        risk.rolling_control(z, path, **dict(kw, group_size=0))
    with pytest.raises(ValueError, match="audits nobody"):
        risk.rolling_control(z, path, **dict(kw, fraction=0.0))
    with pytest.raises(ValueError, match="outside"):
        risk.rolling_control(z, path, **dict(kw, fraction=1.5))
    r = risk.RollingResult(exits=None, log=None, position=0.0, alpha=0.1, gamma=2.0, start=3.0, group_size=4)
    assert r.bound() == 3.0 / 2.0 + 1.0 - 0.1
