"""Deadline exits without a device: the properties of the restatement (tests/deadline_ref.py) that the definition of include/mmee.h states,
``deadline.eta_from_logs`` on hand-made logs, the log's word layout, the header's text, and the refusals that come before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import deadline_ref as D
from .conftest import ROOT

NEW_SYMBOLS = ("ee_set_deadline", "ee_set_deadline_log", "ee_has_deadline", "ee_request_cut", "ee_deadline_log", "ee_debug_deadline_check")
KHZ = 100000                    # the 100 MHz counter: 10 ns a tick


def _rule(**kw):
    a = dict(t0=1000, now=1500, khz=KHZ, budget=10 ** 9, eta=0, host_word=0, call=3, exit_index=1, E1=4, prev_cut_exit=-1, prev_cut_by=0)
    a.update(kw)
    return D.rule(**a)


def test_ticks_to_ns_and_the_saturating_add():
    assert D.ticks_to_ns(500, KHZ) == 5000 and D.ticks_to_ns(1, 3) == 333333 and D.ticks_to_ns(0, 7) == 0
    assert D.ticks_to_ns(7, 27000) == 7 * 10 ** 6 // 27000                      # a rate that does not divide 10^6: rounded down
    for khz in (1, 3, 27000, KHZ, 2 ** 32 - 1):                                  # the integer formula is floor(d 10^6 / khz) wherever that fits
        for d in (0, 1, khz - 1, khz, khz + 1, 12345678901, 2 ** 40 + 17):
            assert D.ticks_to_ns(d, khz) == d * 10 ** 6 // khz, (d, khz)
    # 2^64 - 1 where the ns would not fit 64 bits, the exact value up to there
    top = (D.NONE - 999999) // 10 ** 6
    assert D.ticks_to_ns(D.NONE, 1) == D.NONE and D.ticks_to_ns(D.NONE, KHZ) == D.NONE and D.ticks_to_ns((top + 1) * KHZ, KHZ) == D.NONE
    assert D.ticks_to_ns(top * KHZ + KHZ - 1, KHZ) == (top * KHZ + KHZ - 1) * 10 < D.NONE
    assert D.sat_add(5, D.NONE) == D.NONE and D.sat_add(D.NONE, D.NONE) == D.NONE and D.sat_add(D.NONE - 1, 1) == D.NONE and D.sat_add(3, 4) == 7
    # eta = 2^64 - 1 saturates instead of wrapping to a small number: any finite budget is reached, NONE still never cuts
    assert _rule(eta=D.NONE, budget=D.NONE - 1)[1:] == (1, 1)
    assert _rule(eta=D.NONE, budget=D.NONE)[1:] == (-1, 0)
    # the clock difference is taken modulo 2^64
    assert _rule(t0=D.NONE - 4, now=5)[0] == 100


def test_budget_none_never_cuts_and_budget_zero_cuts_at_exit_0():
    for now in (1000, 10 ** 15, D.NONE):
        for eta in (0, 10 ** 12, D.NONE):
            assert _rule(now=now, eta=eta, budget=D.NONE)[1:] == (-1, 0)
    assert _rule(now=1000, eta=0, budget=0, exit_index=0) == (0, 0, 1)
    # one ns below, at and above the budget (10 ns a tick: elapsed 5000 ns)
    assert _rule(budget=5001)[1:] == (-1, 0) and _rule(budget=5000)[1:] == (1, 1) and _rule(budget=4999)[1:] == (1, 1)
    assert _rule(budget=5001, eta=1)[1:] == (1, 1) and _rule(budget=5002, eta=1)[1:] == (-1, 0)


def test_a_cut_is_sticky_is_the_first_one_and_the_final_exit_writes_nothing():
    assert _rule(budget=0, prev_cut_exit=0, prev_cut_by=2)[1:] == (0, 2)         # already cut by the host: the clock does not take it over
    assert _rule(budget=0, exit_index=3)[1:] == (-1, 0)                          # E1 = 4: the final exit
    assert _rule(host_word=9, exit_index=3)[1:] == (-1, 0)
    E1, thr = 5, np.array([0.9, 0.8, 0.7, 0.6, 0.5])
    nows = [100, 200, 300, 400, 500]                                            # elapsed 1000 .. 5000 ns from t0 = 0
    for sign in (1.0, -1.0):
        got, row = D.call_log(thr, sign, khz=KHZ, budget=2500, eta=[0] * E1, t0=0, nows=nows, host_words=[0] * E1, call=1)
        assert row[2] == 2 and row[3] == 1 and row[4:].tolist() == [1000, 2000, 3000, 4000, 5000]
        assert np.array_equal(got, D.cut_thresholds(thr, 2, sign)) and np.array_equal(got[:2], thr[:2]) and got[4] == thr[4]
        assert (got[2:4] == (np.inf if sign < 0 else -np.inf)).all()
        # lookahead: the cut moves to the last exit the budget still allows
        got, row = D.call_log(thr, sign, khz=KHZ, budget=2500, eta=[4000, 3000, 2000, 1000, 0], t0=0, nows=nows, host_words=[0] * E1, call=1)
        assert row[2] == 0 and np.array_equal(got, D.cut_thresholds(thr, 0, sign))
        # nobody cuts: the thresholds and the row's verdict stay, the stamps are there
        got, row = D.call_log(thr, sign, khz=KHZ, budget=D.NONE, eta=[D.NONE] * E1, t0=0, nows=nows, host_words=[0] * E1, call=1)
        assert np.array_equal(got, thr) and row[2] == -1 and row[3] == 0 and row[1] == -1 and row[4:].tolist() == [1000, 2000, 3000, 4000, 5000]
        # a budget that only the final exit's check would meet cuts nothing
        got, row = D.call_log(thr, sign, khz=KHZ, budget=4500, eta=[0] * E1, t0=0, nows=nows, host_words=[0] * E1, call=1)
        assert np.array_equal(got, thr) and row[2] == -1
    # the host asks between the checks of exits 1 and 2; the clock would have cut at exit 3: the first cut stands
    got, row = D.call_log(thr, 1.0, khz=KHZ, budget=3500, eta=[0] * E1, t0=0, nows=nows, host_words=[0, 0, 7, 7, 7], call=7)
    assert row[2] == 2 and row[3] == 2 and np.array_equal(got, D.cut_thresholds(thr, 2, 1.0))


def test_the_host_word_cuts_the_calls_enqueued_so_far_and_no_later_one():
    for k in (1, 2, 9, 2 ** 40):
        assert _rule(call=k, host_word=k - 1, budget=D.NONE)[1:] == (-1, 0)
        assert _rule(call=k, host_word=k, budget=D.NONE)[1:] == (1, 2)
        assert _rule(call=k, host_word=k + 5, budget=D.NONE)[1:] == (1, 2)
    assert _rule(call=4, host_word=4, budget=0)[1:] == (1, 1)                    # both hold: the clock is named


def _log(pkg, cut_exit, elapsed):
    elapsed = np.asarray(elapsed, np.uint64)
    n = len(cut_exit)
    return pkg.DeadlineLog(np.arange(1, n + 1), np.full(n, D.NONE, np.uint64), np.asarray(cut_exit, np.int64),
                           (np.asarray(cut_exit) >= 0).astype(np.int64), elapsed)


def test_eta_from_logs_on_a_hand_made_log(pkg):
    el = np.array([[100, 300, 600, 1000], [100, 200, 300, 2000], [50, 60, 70, 80], [10, 500, 900, 1500], [100, 400, 800, 1300]]) * 10 ** 6
    log = _log(pkg, [-1, -1, 2, -1, -1], el)                                    # call 3 was cut: its short tail must not count
    want = np.array([[900, 700, 400, 0], [1900, 1800, 1700, 0], [1490, 1000, 600, 0], [1200, 900, 500, 0]], np.float64)
    assert np.array_equal(pkg.eta_from_logs(log), want.max(0)) and pkg.eta_from_logs(log)[-1] == 0.0
    assert np.array_equal(pkg.eta_from_logs(log, quantile=0.5), np.sort(want, 0)[1])      # 2 of the 4 at or below it
    assert np.array_equal(pkg.eta_from_logs(log, quantile=0.75), np.sort(want, 0)[2])
    assert np.array_equal(pkg.eta_from_logs(log, quantile=0.76), want.max(0))
    assert np.array_equal(pkg.eta_from_logs(log, quantile=0.01), want.min(0))
    # several logs are one pool
    a, b = _log(pkg, [-1, -1], el[:2]), _log(pkg, [2, -1, -1], el[2:])
    assert np.array_equal(pkg.eta_from_logs([a, b]), want.max(0))
    assert pkg.deadline.eta_from_logs is pkg.eta_from_logs
    with pytest.raises(ValueError, match="every logged call was cut"):
        pkg.eta_from_logs(_log(pkg, [0, 1], el[:2]))
    with pytest.raises(ValueError, match="quantile"):
        pkg.eta_from_logs(log, quantile=0.0)
    with pytest.raises(ValueError, match="stamps decrease"):
        pkg.eta_from_logs(_log(pkg, [-1], [[5, 4, 6, 7]]))
    with pytest.raises(ValueError, match="disagree on the number of exits"):
        pkg.eta_from_logs([a, _log(pkg, [-1], [[1, 2, 3]])])
    with pytest.raises(ValueError, match="no log given"):
        pkg.eta_from_logs([])


def test_eta_to_next_exit_on_a_hand_made_log(pkg):
    el = np.array([[100, 300, 600, 1000], [100, 200, 300, 2000], [50, 60, 70, 80], [10, 500, 900, 1500]]) * 10 ** 6
    log = _log(pkg, [-1, -1, 2, -1], el)                                       # the cut call's stretches must not count
    full = pkg.eta_from_logs(log)
    got = pkg.eta_to_next_exit(log, 5.0)
    # exits 0 and 1: the longest stretch to the next check plus the tail; exit 2 cannot hand the cut on, the final exit never cuts
    assert np.array_equal(got, [490.0 + 5.0, 400.0 + 5.0, full[2], 0.0]) and full[2] == 1700.0
    assert np.array_equal(pkg.eta_to_next_exit(log, 0.0, quantile=0.34), [200.0, 300.0, 600.0, 0.0])      # 2 of the 3 at or below
    two = _log(pkg, [-1], [[1, 5]])                                             # one exit below the final one: nothing to hand on to
    assert np.array_equal(pkg.eta_to_next_exit(two, 7.0), pkg.eta_from_logs(two))
    with pytest.raises(ValueError, match="tail_ms"):
        pkg.eta_to_next_exit(log, -1.0)
    with pytest.raises(ValueError, match="every logged call was cut"):
        pkg.eta_to_next_exit(_log(pkg, [0], el[:1]), 1.0)


def test_log_rows_parse_into_the_dataclass(pkg):
    E1 = 3
    assert pkg.capi.deadline_log_words(E1) == D.log_words(E1) == 7 and pkg.capi.DL_STATE_WORDS == D.STATE_WORDS
    assert pkg.capi.DEADLINE_NONE == D.NONE and pkg.capi.DEADLINE_OFF == D.OFF
    _, row = D.call_log(np.array([0.5, 0.5, 0.5]), 1.0, khz=KHZ, budget=D.NONE, eta=[0] * E1, t0=0, nows=[1, 2, 2 ** 63 // 10 + 5], host_words=[0, 4, 4], call=4)
    log = pkg.DeadlineLog.from_rows(np.stack([row, row]), E1)
    assert log.call.tolist() == [4, 4] and log.budget_ns.dtype == np.uint64 and int(log.budget_ns[0]) == D.NONE
    assert log.cut_exit.tolist() == [1, 1] and log.cut_by.tolist() == [2, 2]
    assert log.elapsed_ns.dtype == np.uint64 and [int(x) for x in log.elapsed_ns[1]] == [10, 20, (2 ** 63 // 10 + 5) * 10]      # past 2^63: unsigned


def test_header_declares_the_entry_points_and_states_the_definition(pkg):
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    declared = set(re.findall(r"^\w[\w\s\*]*?\b(ee_\w+)\s*\(", header, flags=re.M))
    lib = pkg.capi.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg.capi.SYMBOLS and hasattr(lib, name), name
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", header))
    for words in ("sat_add(elapsed, eta_ns[e]) >= budget", "the host's request word >= k", "It is sticky", "The final exit's check stamps and writes nothing else",
                  "a NaN criterion does not fire", "IF NOBODY IS CUT THERE", "relaxed system-scope atomic load", "hipDeviceAttributeWallClockRate",
                  "Not built: deadlines in captured graphs", "a host <-> device clock correlation", "forcing out NaN documents; a learned eta"):
        assert words in flat, words
    assert header.index("Deadline exits (ee_set_deadline") > header.index("Online exit control (ee_set_controller")
    src = open(os.path.join(ROOT, "multi-modal-early-exit_amd", "csrc", "Makefile")).read()
    assert "deadline.hip" in src


def test_c_refusals_come_before_any_device_call(pkg):
    lib = pkg.capi.load()
    buf = (C.c_int64 * 16)()
    p = C.cast(buf, C.c_void_p)

    def hook(**kw):
        a = pkg.capi.DebugDeadlineCheckArgs()
        base = dict(E1=3, exit_index=0, khz=KHZ, sign=1.0, call=1, budget_ns=5, eta_ns=0, host_word=0, now=1, t0=0, state=p, thr=p, row=p)
        base.update(kw)
        for k, v in base.items():
            setattr(a, k, v)
        assert lib.ee_debug_deadline_check(C.byref(a), None) != 0
        return pkg.capi.last_error()

    assert lib.ee_debug_deadline_check(None, None) != 0 and "args must not be NULL" in pkg.capi.last_error()
    assert "state and thr must not be NULL" in hook(state=None) and "state and thr must not be NULL" in hook(thr=None)
    assert "2 <= E1 <= 64" in hook(E1=1) and "2 <= E1 <= 64" in hook(E1=65)
    assert "outside [0, E1 = 3)" in hook(exit_index=3) and "outside [0, E1 = 3)" in hook(exit_index=-1)
    assert "khz is 0" in hook(khz=0) and "sign is +1 or -1" in hook(sign=0.5) and "numbered from 1" in hook(call=0)
    assert lib.ee_has_deadline(None) == 0 and lib.ee_request_cut(None) != 0 and lib.ee_set_deadline(None, 5, None) != 0
