"""Deadline exits (include/mmee.h, behind the controller's) on the MI355X: the precondition that the 100 MHz counter is one clock chip-wide;
the check launch alone, through its hook with an injected clock, against the numpy restatement of tests/deadline_ref.py in every output word;
the forward with a cut forced at every exit, under a budget of 0, with stamps only, under real budgets and under a cut from the host, each
against the plain forward given the thresholds thr' the definition names, bit for bit; handle hygiene and the refusals.

Nothing here depends on how fast a launch runs: the forced cuts use budgets and lookaheads far outside any elapsed time (2^62 and 2^63 ns
against calls of milliseconds), and the host-cut test asserts what holds wherever the request lands.  Thresholds are gap midpoints of the
device's own criterion table, so no criterion sits on a threshold; the always-fires value is an infinity, which no criterion equals."""
import ctypes as C
import time

import numpy as np
import pytest

from . import csf_ref
from . import deadline_ref as D
from . import ensemble_ref as ER
from .conftest import H256_KW
from .hook_util import SENTINEL, _stream, _torch
from .test_gpu_controller import FIELDS, MIN_GAP, Case, _bits, _np, _table

pytestmark = pytest.mark.gpu

GUARD = 4
KHZ = 100000                    # 10 ns a tick
FAR_BUDGET_MS = 2.0 ** 62 / 1e6  # no call here runs for 2^62 ns
FAR_ETA_MS = 2.0 ** 63 / 1e6     # and elapsed + 2^63 ns is past that budget whatever elapsed is


@pytest.fixture(scope="module")
def cases(pkg):
    built = {}

    def get(name):
        if name not in built:
            built[name] = Case(pkg, name)
        return built[name]

    yield get
    for c in built.values():
        c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 0. the precondition: s_memrealtime is one clock on the whole chip
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_100_mhz_counter_is_one_clock_chip_wide(cases):
    """The begin and the check launches land on arbitrary CUs of arbitrary XCDs, so elapsed = now - t0 means something only if every CU reads
    the same counter.  Stamp A, synchronise, sleep 2 ms on the host, stamp B: over the CU slots filled in both, the values of A lie within
    less than the 2 ms gap of each other, and every value of B is later than every value of A."""
    torch = _torch()
    eng = cases("tiny_ramp").engine()
    a = eng.clock_stamp()
    torch.cuda.synchronize()
    time.sleep(0.002)
    b = eng.clock_stamp()
    torch.cuda.synchronize()
    ra, rb = _np(a)[1::2], _np(b)[1::2]
    both = (ra != 0) & (rb != 0)
    assert both.sum() >= 64, both.sum()
    gap_ticks = 0.002 * KHZ * 1e3
    spread = int(ra[both].max() - ra[both].min())
    print(f"s_memrealtime over {int(both.sum())} CU slots: spread within one stamp {spread} ticks = {spread * 10} ns; "
          f"min(B) - max(A) = {int(rb[both].min() - ra[both].max())} ticks; spread of B {int(rb[both].max() - rb[both].min())} ticks")
    assert spread < gap_ticks, (spread, gap_ticks)
    assert rb[both].min() > ra[both].max(), (int(rb[both].min()), int(ra[both].max()))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the check launch alone
# ---------------------------------------------------------------------------------------------------------------------------------------
def _u64(x):
    return np.array([int(x)], np.uint64).view(np.int64)[0]


def _check(pkg, *, thr, state, row, sign, khz, budget, eta, host_word, call, exit_index, now, t0, over=None):
    """One check launch on device copies of state, thr and row, each followed by GUARD sentinel words (one upload, one download)."""
    torch = _torch()
    E1 = len(thr)
    guard = np.full(GUARD, SENTINEL, np.int64)
    parts = dict(state=np.asarray(state, np.int64), thr=np.asarray(thr, np.float64).view(np.int64), row=np.asarray(row, np.int64))
    at, packed = {}, []
    for k, v in parts.items():
        at[k] = sum(len(x) for x in packed)
        packed += [v, guard]
    buf = torch.from_numpy(np.concatenate(packed)).cuda()
    a = pkg.capi.DebugDeadlineCheckArgs()
    a.E1, a.exit_index, a.khz, a.sign = E1, exit_index, khz, sign
    a.call, a.budget_ns, a.eta_ns, a.host_word, a.now, a.t0 = call, budget, eta, host_word, now, t0
    a.state, a.thr, a.row = (buf.data_ptr() + 8 * at[k] for k in ("state", "thr", "row"))
    for k, v in (over or {}).items():
        setattr(a, k, v)
    pkg.capi.check(pkg.capi.load().ee_debug_deadline_check(C.byref(a), _stream()), None, "ee_debug_deadline_check")
    got = buf.cpu().numpy()
    return {k: got[at[k]:at[k] + len(v) + GUARD] for k, v in parts.items()}


@pytest.mark.parametrize("E1", [2, 3, 7, 64])
def test_check_hook_is_the_restatement_in_every_output_word(pkg, E1):
    rng = np.random.default_rng(E1)
    thr = rng.uniform(0.1, 0.9, E1)
    W = D.log_words(E1)
    row0 = rng.integers(1, 1 << 40, W)                                          # a row with history: only the words the check owns may change
    t0, ticks, eta = 123456789, 4321, 777
    elapsed = D.ticks_to_ns(ticks, KHZ)
    seen = set()
    for e in range(E1):
        for rel in (-10, 0, 10):                                                # elapsed + eta one tick below, at, one tick above the budget
            budget = elapsed + eta - rel
            for prev in ((-1, 0), (0, 1), (max(e - 1, 0), 2)):                  # not cut yet / cut before by the clock / by the host
                for sign in (1.0, -1.0):
                    for word, call in ((4, 5), (5, 5), (6, 5)):                 # the host word below, at and above the call number
                        state = np.array([-99, prev[0], prev[1]], np.int64)     # state[0] is not read: t0 is injected
                        row = row0.copy()
                        kw = dict(sign=sign, khz=KHZ, budget=budget, eta=eta, host_word=word, call=call, exit_index=e, now=t0 + ticks, t0=t0)
                        w_state, w_thr, w_row = D.check(state, thr, row, **kw)
                        got = _check(pkg, thr=thr, state=state, row=row, **kw)
                        tag = (E1, e, rel, prev, sign, word)
                        assert np.array_equal(got["state"][:3], w_state) and (got["state"][3:] == SENTINEL).all(), (tag, got["state"], w_state)
                        assert np.array_equal(got["thr"][:E1], w_thr.view(np.int64)) and (got["thr"][E1:] == SENTINEL).all(), (tag, got["thr"][:E1].view(np.float64))
                        assert np.array_equal(got["row"][:W], w_row) and (got["row"][W:] == SENTINEL).all(), (tag, got["row"][:W], w_row)
                        assert w_row[4 + e] == elapsed
                        seen.add((int(w_state[1]) == e and prev[0] < 0, int(w_state[2])))
    # the grid reached what its axes name: fresh cuts by the clock and by the host, and checks that cut nothing
    assert {(True, 1), (True, 2), (False, 0)} <= seen, seen


def test_check_hook_other_clock_rates_the_wrap_and_no_row(pkg):
    thr = np.array([0.3, 0.6, 0.9, 0.5])
    fresh, row0 = np.array([0, -1, 0], np.int64), np.arange(10, 10 + D.log_words(4), dtype=np.int64)
    # a rate that does not divide 10^6; the difference taken modulo 2^64; an elapsed time past 2^63 ns; one that saturates
    for khz, t0, now in ((27000, 5, 5 + 123457), (KHZ, D.NONE - 4, 5), (1000, 0, 2 ** 63 // 1000 + 9), (1, 0, D.NONE), (2 ** 32 - 1, 17, 2 ** 50)):
        el = D.ticks_to_ns((now - t0) % D.M64, khz)
        for budget in (el, el + 1 if el < D.NONE else D.NONE, D.NONE):
            kw = dict(sign=1.0, khz=khz, budget=budget, eta=0, host_word=0, call=1, exit_index=1, now=now, t0=t0)
            w_state, w_thr, w_row = D.check(fresh, thr, row0, **kw)
            got = _check(pkg, thr=thr, state=fresh, row=row0, **kw)
            assert np.array_equal(got["state"][:3], w_state) and np.array_equal(got["thr"][:4], w_thr.view(np.int64)), (khz, budget)
            assert np.array_equal(got["row"][:len(row0)], w_row) and got["row"][5] == _u64(el), (khz, budget, got["row"], w_row)
    # eta = 2^64 - 1 saturates: a finite budget is met, MMEE_DEADLINE_NONE is not
    for budget, cut in ((D.NONE - 1, 1), (D.NONE, -1)):
        kw = dict(sign=-1.0, khz=KHZ, budget=budget, eta=D.NONE, host_word=0, call=1, exit_index=1, now=50, t0=0)
        got = _check(pkg, thr=thr, state=fresh, row=row0, **kw)
        w_state, w_thr, _ = D.check(fresh, thr, row0, **kw)
        assert got["state"][1] == cut == w_state[1] and np.array_equal(got["thr"][:4], w_thr.view(np.int64))
        assert (got["thr"][1:3].view(np.float64) == np.inf).all() == (cut == 1)
    # no row given: the state and the thresholds all the same, nothing else written
    kw = dict(sign=1.0, khz=KHZ, budget=0, eta=0, host_word=0, call=1, exit_index=2, now=50, t0=0)
    got = _check(pkg, thr=thr, state=fresh, row=row0, over=dict(row=None), **kw)
    w_state, w_thr, _ = D.check(fresh, thr, None, **kw)
    assert np.array_equal(got["state"][:3], w_state) and np.array_equal(got["thr"][:4], w_thr.view(np.int64)) and np.array_equal(got["row"][:len(row0)], row0)
    with pytest.raises(pkg.capi.MMEEError, match="2 <= E1 <= 64"):
        _check(pkg, thr=thr, state=fresh, row=row0, over=dict(E1=65), **kw)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the forward
# ---------------------------------------------------------------------------------------------------------------------------------------
def _setup(pkg, c, criterion):
    """(deadline engine, plain engine, thresholds, sign, the dump of call 0: all_logits, criterion table)."""
    eng, plain = c.engine(), c.engine()
    for e in (eng, plain):
        e.set_criterion(criterion)
    all_logits, head_logits = c.dump(plain)
    table, _, sign = _table(pkg, c, criterion, all_logits, head_logits)
    thr = csf_ref.gap_thresholds(table, 0.7 if sign > 0 else 0.3, MIN_GAP)[0]
    return eng, plain, thr, sign, all_logits[:, :c.B], table[:, :c.B]


def _fields(o):
    return {f: _np(getattr(o, f)) for f in FIELDS}


def _same(got, want, tag):
    for f in FIELDS:
        assert np.array_equal(_bits(got[f]), _bits(want[f])), (tag, f)


def _forced(c, e_star):
    """Arguments of set_deadline under which the clock cuts at exit e_star whatever the elapsed time is."""
    eta = np.zeros(c.E + 1)
    eta[e_star] = FAR_ETA_MS
    return dict(budget_ms=FAR_BUDGET_MS, eta_ms=eta)


def _scan(pkg, criterion, all_logits, table, thr):
    if criterion == "gate":
        return _np(pkg.gate_scan_device(table, all_logits, thr)[0])
    return _np(pkg.criterion_scan_device(all_logits, thr, criterion)[0])


FORWARD = [("tiny_ramp", "max_confidence"), ("tiny_ramp", "entropy"), ("tiny_ramp", "margin"), ("h256_gate", "gate")]


@pytest.mark.parametrize("name,criterion", FORWARD)
def test_a_cut_at_every_exit_is_the_plain_forward_under_thr_prime(cases, pkg, name, criterion):
    c = cases(name)
    eng, plain, thr, sign, all_logits, table = _setup(pkg, c, criterion)
    want_plain = _fields(plain.forward(**c.call(0), thresholds=thr))
    hist = []
    for e_star in range(c.E):
        eng.set_deadline(**_forced(c, e_star), log_cap=4)
        assert eng.has_deadline()
        got = _fields(eng.forward(**c.call(0), thresholds=thr))
        thr_p = D.cut_thresholds(thr, e_star, sign)
        _same(got, _fields(plain.forward(**c.call(0), thresholds=thr_p)), (name, criterion, e_star))
        assert np.array_equal(got["exit_layer"], _scan(pkg, criterion, all_logits, table, thr_p)), (name, criterion, e_star)
        assert got["exit_layer"].max() <= e_star and np.array_equal(got["exit_layer"], np.minimum(want_plain["exit_layer"], e_star))
        log = eng.deadline_log()
        # a new eta on an engine that has a deadline restarts nothing: the ring of 4 rows runs on, the call's row is the last
        assert len(log.call) == min(e_star + 1, 4) and log.call[-1] == e_star + 1 and log.cut_exit[-1] == e_star and log.cut_by[-1] == 1, (e_star, log)
        assert abs(int(log.budget_ns[-1]) - 2 ** 62) <= 2 ** 11                  # the ms -> ns conversion of a float64
        el = log.elapsed_ns[-1].astype(np.int64)
        assert (np.diff(el) >= 0).all() and 0 < el[-1] < 10 ** 10, el
        hist.append(int((got["exit_layer"] == e_star).sum()))
    eng.check()
    plain.check()
    # the case is a case: under the plain thresholds documents leave at several exits and somebody reaches the final one
    ex = want_plain["exit_layer"]
    print(name, criterion, "plain exits:", np.bincount(ex, minlength=c.E + 1).tolist(), "cut at e*, leaving there:", hist)
    assert len(np.unique(ex)) >= 3 and (ex == c.E).any(), np.bincount(ex, minlength=c.E + 1)


def test_an_ensemble_temperatures_low_latency_and_the_result_stream(cases, pkg):
    c = cases("tiny_ramp")
    eng, plain, thr, sign, _, _ = _setup(pkg, c, "max_confidence")
    temps = np.linspace(0.6, 2.0, c.E + 1)
    e_star = 3
    eng.set_deadline(**_forced(c, e_star), log_cap=8)
    for tag, ensemble, kw in (("temperatures", None, dict(temperatures=temps)),
                              ("ensemble", ER.random_weights(c.E + 1, c.K, seed=3), {}),
                              ("ensemble and temperatures", ER.random_weights(c.E + 1, c.K, seed=4), dict(temperatures=temps))):
        for e in (eng, plain):
            e.set_ensemble(ensemble)
        # thresholds in the gaps of the criteria THIS variant decides on.  The dump holds them rounded to float32 -- at most 2^-25 = 3e-8 away
        # for a criterion below 1 -- so the midpoint of a gap of 1e-6 or more lies on the same side of both neighbours' float64 values
        crit = _np(plain.forward(**c.call(1), dump_all=True, want_all=True, **kw).all_crit).astype(np.float64)
        v_thr = csf_ref.gap_thresholds(crit, 0.6, 1e-6)[0]
        got = _fields(eng.forward(**c.call(1), thresholds=v_thr, **kw))
        _same(got, _fields(plain.forward(**c.call(1), thresholds=D.cut_thresholds(v_thr, e_star, sign), **kw)), tag)
        uncut = _fields(plain.forward(**c.call(1), thresholds=v_thr, **kw))
        assert got["exit_layer"].max() <= e_star < uncut["exit_layer"].max(), tag       # the cut changed somebody's exit
    for e in (eng, plain):
        e.set_ensemble(None)
    thr_p = D.cut_thresholds(thr, e_star, sign)
    # the result stream: every document arrives exactly once, its row is the tensors' row
    st = eng.forward_stream(**c.call(2), thresholds=thr)
    chunks = list(st)
    out = _fields(st.output)
    _same(out, _fields(plain.forward(**c.call(2), thresholds=thr_p)), "forward_stream")
    assert [ch.exit_index for ch in chunks] == list(range(c.E + 1))
    idx = np.concatenate([ch.doc_index for ch in chunks])
    assert np.array_equal(np.sort(idx), np.arange(c.B))
    for ch in chunks:
        assert (ch.exit_layer == ch.exit_index).all() and np.array_equal(out["exit_layer"][ch.doc_index], ch.exit_layer)
        assert np.array_equal(_bits(ch.logits), _bits(out["logits"][ch.doc_index])) and np.array_equal(_bits(ch.confidence), _bits(out["confidence"][ch.doc_index]))
        assert ch.exit_index <= e_star or len(ch.doc_index) == 0
    log = eng.deadline_log()
    assert log.cut_exit.tolist() == [e_star] * 4 and log.call.tolist() == [1, 2, 3, 4]
    eng.check()
    plain.check()
    # low latency is a split-precision mode: the gate handle under its configured criterion
    g = cases("h256_gate")
    geng, gplain, gthr, gsign, _, _ = _setup(pkg, g, "max_confidence")
    geng.set_deadline(**_forced(g, 1))
    got = _fields(geng.forward(**g.call(0), thresholds=gthr, low_latency=True))
    _same(got, _fields(gplain.forward(**g.call(0), thresholds=D.cut_thresholds(gthr, 1, gsign), low_latency=True)), "low_latency")
    assert geng.deadline_log().cut_exit.tolist() == [1] and got["exit_layer"].max() <= 1
    geng.check()
    gplain.check()


def test_budget_zero_stamps_only_real_budgets_and_the_per_call_override(cases, pkg):
    c = cases("tiny_ramp")
    eng, plain, thr, sign, _, _ = _setup(pkg, c, "max_confidence")
    want = _fields(plain.forward(**c.call(0), thresholds=thr))
    at0 = _fields(plain.forward(**c.call(0), thresholds=D.cut_thresholds(thr, 0, sign)))
    assert (at0["exit_layer"] == 0).all() and (want["exit_layer"] > 0).any()
    # budget = 0: everybody leaves at exit 0
    eng.set_deadline(0.0)
    _same(_fields(eng.forward(**c.call(0), thresholds=thr)), at0, "budget 0")
    # 1 ns above zero eta: the first check has passed it
    eng.set_deadline(1e-6)
    _same(_fields(eng.forward(**c.call(0), thresholds=thr)), at0, "budget 1 ns")
    log = eng.deadline_log()
    assert log.cut_exit.tolist() == [0, 0] and log.cut_by.tolist() == [1, 1] and log.budget_ns.tolist() == [0, 1] and log.elapsed_ns[1, 0] >= 1
    # 10 s: no cut, the plain bits
    eng.set_deadline(10e3)
    _same(_fields(eng.forward(**c.call(0), thresholds=thr)), want, "budget 10 s")
    log = eng.deadline_log()
    assert log.cut_exit.tolist() == [0, 0, -1] and log.cut_by.tolist() == [1, 1, 0] and log.budget_ns.tolist() == [0, 1, 10 ** 10]
    # stamps only: the plain bits, a timeline per call; the per-call override cuts its own call and no other (another log_cap: the log restarts)
    eng.set_deadline(None, stamps_only=True, log_cap=4)
    _same(_fields(eng.forward(**c.call(0), thresholds=thr)), want, "stamps only")
    _same(_fields(eng.forward(**c.call(0), thresholds=thr, deadline_ms=0.0)), at0, "deadline_ms=0")
    _same(_fields(eng.forward(**c.call(0), thresholds=thr)), want, "the call after the override")
    log = eng.deadline_log()
    assert log.cut_exit.tolist() == [-1, 0, -1] and log.cut_by.tolist() == [0, 1, 0] and [int(b) for b in log.budget_ns] == [D.NONE, 0, D.NONE]
    assert (np.diff(log.elapsed_ns.astype(np.int64), axis=1) >= 0).all()
    eta = pkg.eta_from_logs(log)                                                # from the two uncut rows
    assert eta.shape == (c.E + 1,) and eta[-1] == 0 and (np.diff(eta) <= 0).all() and eta[0] > 0
    # the ring keeps the latest log_cap rows, oldest first
    for _ in range(3):
        eng.forward(**c.call(0), thresholds=thr)
    log = eng.deadline_log()
    assert len(log.call) == 4 and np.array_equal(np.diff(log.call), [1, 1, 1]) and log.cut_exit.tolist() == [-1] * 4
    # a dump-all call is no deadline call: no row, no number used
    last = int(log.call[-1])
    eng.forward(**c.call(0), dump_all=True, want_all=True)
    eng.forward(**c.call(0), thresholds=thr)
    assert int(eng.deadline_log().call[-1]) == last + 1
    with pytest.raises(ValueError, match="stamps_only=True goes with budget_ms=None"):
        eng.set_deadline(5.0, stamps_only=True)
    with pytest.raises(ValueError, match="one per exit"):
        eng.set_deadline(5.0, eta_ms=[0.0, 1.0])
    with pytest.raises(ValueError, match="set_deadline"):
        plain.forward(**c.call(0), thresholds=thr, deadline_ms=1.0)
    with pytest.raises(ValueError, match="deadline calls are eager"):
        plain.capture(**{k: v.clone() for k, v in c.call(0).items()}, thresholds=thr, deadline_ms=1.0)
    eng.check()
    plain.check()


def test_a_cut_from_the_host(cases, pkg):
    c = cases("tiny_ramp")
    eng, plain, thr, sign, _, _ = _setup(pkg, c, "max_confidence")
    assert not plain.request_cut()                                             # never had a deadline: nothing to cut
    eng.set_deadline(None, stamps_only=True, log_cap=16)
    # asked before any deadline forward: zero calls were enqueued, so none is cut
    assert eng.request_cut()
    first = _fields(eng.forward(**c.call(0), thresholds=thr))
    _same(first, _fields(plain.forward(**c.call(0), thresholds=thr)), "a request before the first call")
    # eight enqueued back to back, the request, one more
    outs = [eng.forward(**c.call(t % c.T), thresholds=thr) for t in range(8)]
    assert eng.request_cut()
    after = eng.forward(**c.call(1), thresholds=thr)
    log = eng.deadline_log()
    assert log.call.tolist() == list(range(1, 11)) and log.cut_exit[0] == -1
    _same(_fields(after), _fields(plain.forward(**c.call(1), thresholds=thr)), "the call after the request")
    assert log.cut_exit[-1] == -1 and log.cut_by[-1] == 0
    for t, o in enumerate(outs):                                                # wherever the request landed: the call is thr' of its logged cut
        ce, by = int(log.cut_exit[1 + t]), int(log.cut_by[1 + t])
        assert (ce == -1 and by == 0) or (0 <= ce < c.E and by == 2), (t, ce, by)
        _same(_fields(o), _fields(plain.forward(**c.call(t % c.T), thresholds=D.cut_thresholds(thr, ce, sign))), ("host cut", t, ce))
    print("host cut: cut_exit of the eight calls in flight:", log.cut_exit[1:9].tolist())
    # a request on a drained engine cuts nothing later either, and the clock's budget still works next to it
    assert eng.request_cut()
    _same(_fields(eng.forward(**c.call(0), thresholds=thr)), first, "a request between calls")
    eng.check()
    plain.check()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. hygiene and refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_handle_without_a_deadline_issues_the_parent_s_launches_and_bits(cases, pkg):
    c = cases("tiny_ramp")
    never, other, thr, _, _, _ = _setup(pkg, c, "max_confidence")

    def run(e, **kw):
        e.profile(True)
        o = e.forward(**c.call(0), **kw)
        prof = e.profile_read()
        e.profile(False)
        return _fields(o) if not kw.get("dump_all") else None, {role: v["launches"] for role, v in prof.items()}

    strip = lambda n: {k: v for k, v in n.items() if k != "deadline"}
    out_never, n_never = run(never, thresholds=thr)
    _, d_never = run(never, dump_all=True)
    assert n_never["exit_decide"] == c.E + 1 and n_never.get("deadline", 0) == 0
    other.set_deadline(10e3)
    out_dl, n_dl = run(other, thresholds=thr)
    assert n_dl["deadline"] == c.E + 2 and strip(n_dl) == strip(n_never), (n_dl, n_never)       # E1 + 1: the begin launch and one check per exit
    _, d_dl = run(other, dump_all=True)
    assert d_dl.get("deadline", 0) == 0 and strip(d_dl) == strip(d_never)
    other.set_deadline(None)
    assert not other.has_deadline() and other.deadline is None
    out_off, n_off = run(other, thresholds=thr)
    assert strip(n_off) == strip(n_never) and n_off.get("deadline", 0) == 0
    _same(out_dl, out_never, "a deadline that never cuts")
    _same(out_off, out_never, "after set_deadline(None)")
    assert len(other.deadline_log().call) == 1                                  # the log outlives the deadline; the dump-all call wrote no row
    never.check()
    other.check()


def test_refusals_say_why_and_leave_the_handle_usable(cases, pkg):
    c = cases("tiny_ramp")
    eng, plain, thr, sign, _, _ = _setup(pkg, c, "max_confidence")
    want = _fields(plain.forward(**c.call(0), thresholds=thr))
    Err = pkg.capi.MMEEError
    call = c.call(0)
    path = np.repeat(np.array([0.97, 0.8, 0.6, 0.4, 0.1])[:, None], c.E + 1, axis=1)
    ctl = dict(alpha=0.1, gamma=1.0, start=2.0, seed=1)

    def usable(deadline):
        assert eng.has_deadline() == deadline and (eng.deadline is not None) == deadline
        _same(_fields(eng.forward(**call, thresholds=thr)), want, "after a refusal")
        eng.check()

    # set_deadline on a handle whose decisions it cannot cut
    eng.set_criterion("patience")
    with pytest.raises(Err, match="ee_set_deadline: a handle under MMEE_CRIT_PATIENCE"):
        eng.set_deadline(5.0)
    eng.set_criterion("max_confidence")
    eng.set_patience(2)
    for rule in ("patient_confident", "patience_or_threshold"):
        eng.set_exit_rule(rule)
        with pytest.raises(Err, match="ee_set_deadline: a handle under MMEE_RULE_STREAK / MMEE_RULE_EITHER"):
            eng.set_deadline(5.0)
    eng.set_exit_rule("plain")
    for mode in ("exact", "at_least"):
        eng.set_quotas([1] * c.E, mode=mode)
        with pytest.raises(Err, match="ee_set_deadline: quotas are set"):
            eng.set_deadline(5.0)
    eng.set_quotas(None)
    eng.set_audit(0.5, seed=1)
    with pytest.raises(Err, match="ee_set_deadline: an audit is set"):
        eng.set_deadline(5.0)
    eng.set_controller(path, **ctl)
    with pytest.raises(Err, match="ee_set_deadline: a controller is set"):
        eng.set_deadline(None, stamps_only=True)
    eng.set_controller(None)
    eng.set_audit(None)
    usable(False)
    # the other order: while a deadline is set
    eng.set_deadline(10e3)
    with pytest.raises(Err, match="MMEE_CRIT_PATIENCE while a deadline is set"):
        eng.set_criterion("patience")
    with pytest.raises(Err, match="while a deadline is set"):
        eng.set_exit_rule("patient_confident")
    for mode in ("exact", "at_least"):
        with pytest.raises(Err, match="ee_set_quotas: a deadline is set"):
            eng.set_quotas([1] * c.E, mode=mode)
    with pytest.raises(Err, match="ee_set_audit: a deadline is set"):
        eng.set_audit(0.5, seed=1)
    with pytest.raises(Err, match="ee_set_controller: a deadline is set"):
        eng.set_controller(path, **ctl)
    assert not eng.has_audit() and not eng.has_controller() and not eng.has_quotas
    with pytest.raises(Err, match="ee_graph_capture: a deadline is set"):
        eng.capture(**{k: v.clone() for k, v in call.items()}, thresholds=thr)
    with pytest.raises(Err, match="ee_forward_vision: a deadline is set"):
        eng.forward_vision(call["pixel_values"], thresholds=thr)
    usable(True)
    # captured graphs held
    eng.set_deadline(None)
    cap = eng.capture(**{k: v.clone() for k, v in call.items()}, thresholds=thr)
    with pytest.raises(Err, match="ee_set_deadline: the handle holds captured graphs"):
        eng.set_deadline(5.0)
    cap.close()
    usable(False)
    # micro-batches and cascades
    mb = pkg.MicroBatchedEngine(c.cfg, xprobe=False, micro_batches=2, max_docs=c.B, max_text_len=c.text, precision=c.precision)
    mb.load_weights(c.W)
    with pytest.raises(ValueError, match="a deadline over micro-batches is not built"):
        mb.set_deadline(5.0)
    with pytest.raises(ValueError, match="a deadline over micro-batches is not built"):
        mb.set_deadline(None, stamps_only=True)
    assert mb.set_deadline(None) is None and not mb.has_deadline()
    with pytest.raises(ValueError, match="a deadline over micro-batches is not built"):
        mb.forward(**call, thresholds=thr, deadline_ms=5.0)
    mb.engines[0].set_deadline(5.0)
    with pytest.raises(ValueError, match="a deadline over micro-batches is not built"):
        mb.forward(**call, thresholds=thr)
    mb.close()
    eng.set_deadline(10e3)
    with pytest.raises(ValueError, match="deadlines on cascade stages are not built"):
        pkg.CascadeEngine([eng, plain]).forward(call)
    usable(True)
    eng.set_deadline(None)
    # learning-to-exit
    lte_cfg = pkg.ModelConfig.tiny(EE_config=dict(exits=[1, 2], encoder_layer_strategy="ramp", use_lte=True), **H256_KW)
    lte = pkg.EarlyExitEngine(lte_cfg, xprobe=False, max_docs=4, max_text_len=48, precision="split")
    with pytest.raises(Err, match="ee_set_deadline: a use_lte handle"):
        lte.set_deadline(5.0)
    assert not lte.has_deadline() and lte.deadline is None
    lte.close()
    # more exits than a wave has lanes
    deep_cfg = pkg.ModelConfig.tiny(EE_config=dict(exits=list(range(1, 65)), encoder_layer_strategy="ramp", inference_strategy="max_confidence"),
                                    num_hidden_layers=64)
    deep = pkg.EarlyExitEngine(deep_cfg, xprobe=False, max_docs=2, max_text_len=16, precision="fp32")
    assert deep.E + 1 == 65
    with pytest.raises(Err, match=r"E1 = 65 exits, a deadline takes E1 <= 64"):
        deep.set_deadline(5.0)
    assert not deep.has_deadline()
    deep.close()
    # the model wrapper passes through
    m = pkg.LayoutLMv3EEForSequenceClassification(c.cfg, weights=c.W, max_docs=c.B, max_text_len=c.text, precision=c.precision)
    assert m.set_deadline(0.0)["budget_ns"] == 0 and m.engine.has_deadline()
    o = m.early_exit(**call, thresholds=thr, xprobe=False)
    assert (_np(o.exit_layer) == 0).all() and m.engine.deadline_log().cut_exit.tolist() == [0]
    assert m.set_deadline(None) is None and not m.engine.has_deadline()
    assert np.array_equal(_np(m.early_exit(**call, thresholds=thr, xprobe=False).exit_layer), want["exit_layer"])
