"""The exit ensemble (include/mmee.h, at ee_set_ensemble) on the MI355X against the numpy restatement of tests/ensemble_ref.py: the launch alone
through ee_debug_exit_ensemble at the wave and block edges, the forward (eager, captured, streamed, low-latency) on ``tiny_ramp``, the
``h256`` ramp and gate configurations and the tiny DiT, the dumped-array tool ``sweep.ensemble_logits``, and the fit ``ee_ensemble_fit``.

The device's exp / log may differ from numpy's in the last place of float64, and the device accumulates with fma where numpy rounds every
product: either can move the float32 rounding of an ensemble row by one place.  So the launch alone is compared within 1 float32 ulp and
its float64 state within 1e-12 relative, while everything the forward returns is compared BIT FOR BIT with what the dumped-array tool makes
of the forward's own un-ensembled dump -- the two share their device functions.  Thresholds sit at midpoints of adjacent sorted reference
criteria more than 1e-9 apart, and a CPU assertion checks that no document is within 1e-12 of its threshold.

The fit's tolerances are derived: with g the reference gradient at the device's theta and g* the one at the reference optimum,
|theta - theta*| <= (|g| + |g*|) / l2 by strong convexity, and an ensemble row moves by at most that times max_n |(l_.,n, 1)|, plus one
float32 rounding."""
import ctypes as C

import numpy as np
import pytest

from . import csf_ref
from . import ensemble_ref as ER
from . import exit_stage_ref as R
from .conftest import DIT_EE, H256_KW, MATRIX_CASES, TINY_CASES, report_measured, sweep_ref_inputs
from .hook_util import SENTINEL, _stream, _torch

pytestmark = pytest.mark.gpu

GUARD = 4
STAGE_N = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
KS = (2, 16, 17)
E1_HOOK = 5
SENT64 = np.int64(0x7FF5A5A57FA5A5A5)                  # a NaN bit pattern no kernel writes
MIN_GAP, MIN_DIST = 1e-9, 1e-12


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the launch alone
# ---------------------------------------------------------------------------------------------------------------------------------------
def _i32(a):
    return _torch().from_numpy(np.concatenate([np.asarray(a, np.int64).reshape(-1), [SENTINEL]]).astype(np.int32)).cuda()


def _counts(stage):
    sq = stage["sum_len_sq"]
    return _torch().from_numpy(np.array([stage["n"], stage["n_rows"], sq & 0xFFFFFFFF, sq >> 32], np.int64).astype(np.int32)).cuda()


def _call_hook(pkg, stage, z, state_words, w, b, e, temp, B, by_pointer=0, E1=E1_HOOK, out_rows=None, pol_rows=None):
    """One ee_debug_exit_ensemble call: z (n,K) float32, state_words (E1,B,K) int64 bit patterns (returned updated), w (E1,E1), b (E1,K) | None.
    -> (y words (n + GUARD rows, K) int32, state words)."""
    torch = _torch()
    n, K = z.shape
    zt = torch.from_numpy(np.ascontiguousarray(z) if n else np.zeros((1, K), np.float32)).cuda()
    st = torch.from_numpy(np.ascontiguousarray(state_words)).cuda()
    out = torch.full(((n + GUARD) * K,), SENTINEL, dtype=torch.int32, device="cuda")
    wt = torch.from_numpy(np.ascontiguousarray(w, np.float64)).cuda()
    bt = None if b is None else torch.from_numpy(np.ascontiguousarray(b, np.float64)).cuda()
    keep = (_counts(stage), _i32(stage["doc_orig"]))
    a = pkg.capi.DebugExitEnsembleArgs()
    a.pol_logits, a.pol_rows, a.K, a.E1, a.exit_index, a.B = zt.data_ptr(), n if pol_rows is None else pol_rows, K, E1, e, B
    a.temp, a.by_pointer = float(temp), by_pointer
    a.counts, a.doc_orig, a.w, a.b = keep[0].data_ptr(), keep[1].data_ptr(), wt.data_ptr(), None if bt is None else bt.data_ptr()
    a.state, a.out, a.out_rows = st.data_ptr(), out.data_ptr(), n if out_rows is None else out_rows
    pkg.capi.check(pkg.capi.load().ee_debug_exit_ensemble(C.byref(a), _stream()), None, "ee_debug_exit_ensemble")
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(n + GUARD, K), st.cpu().numpy()


def _hook_case(n, K):
    rng = np.random.default_rng(4000 + 17 * n + K)
    B = n + 29
    sel = (n + K) % 3
    e = (0, 2, E1_HOOK - 1)[sel]
    temp = (1.0, 3.0, 0.5)[(n // 3 + K) % 3]
    stage = R.make_stage(n, B, seed=n + K)
    z = (rng.standard_normal((n, K)) * 2.0).astype(np.float32)
    w, b = ER.random_weights(E1_HOOK, K, seed=n + K)
    state = np.full((E1_HOOK, B, K), SENT64, np.int64)
    o = stage["doc_orig"]
    earlier = ER.logsoftmax64(rng.standard_normal((e, n, K)) * 2.0)              # what earlier launches left for the active slots
    state[:e, o] = earlier.view(np.int64)
    return dict(n=n, K=K, B=B, e=e, temp=temp, stage=stage, z=z, w=w, b=b if (n + K) % 2 else None, state=state, earlier=earlier,
                by_pointer=(n // 2 + K) % 2)


def _hook_reference(c):
    """(y (n,K) float32, l (n,K) float64) of the case by the restatement."""
    x = (c["z"].astype(np.float64) / c["temp"]).astype(np.float32)
    l = ER.logsoftmax64(x)
    e = c["e"]
    rows = np.concatenate([c["earlier"], l[None]], 0)                           # (e + 1, n, K)
    a = np.zeros_like(l) if c["b"] is None else np.broadcast_to(c["b"][e], l.shape).copy()
    for j in range(e + 1):
        a = a + c["w"][e, j] * rows[j]
    return a.astype(np.float32), l


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", STAGE_N)
def test_launch_alone_matches_the_restatement_and_touches_nothing_else(pkg, n, K):
    c = _hook_case(n, K)
    y, state = _call_hook(pkg, c["stage"], c["z"], c["state"].copy(), c["w"], c["b"], c["e"], c["temp"], c["B"], c["by_pointer"])
    want_y, want_l = _hook_reference(c)
    ok, near = ER.ulp_close_f32(y[:n].view(np.float32), want_y)
    assert ok.all(), (n, K, np.argwhere(~ok)[:4].tolist())
    assert np.all(y[n:] == SENTINEL)                                            # nothing behind the n rows
    o, e = c["stage"]["doc_orig"], c["e"]
    got_l = state[e, o].view(np.float64)
    assert np.all(np.abs(got_l - want_l) <= 1e-12 * np.abs(want_l)), (n, K)
    rel = float((np.abs(got_l - want_l) / np.maximum(np.abs(want_l), 1e-300)).max())
    rest = state.copy()
    rest[e, o] = c["state"][e, o]
    assert np.array_equal(rest, c["state"])                                     # earlier rows, later rows and untouched slots: bit for bit
    report_measured(f"ensemble.launch[n={n},K={K},e={e},T={c['temp']}]", "float32 neighbours of the restatement / max rel state error", near + rel)


def test_launch_chains_three_exits_over_a_shrinking_stage(pkg):
    """Exits 0, 1, 2 of one batch: each call's state is the next one's, a third of the documents leaves after each exit (their slots are never
    written again), and every y is the restatement's on the whole history within 1 ulp."""
    n0, K, B = 300, 16, 329
    rng = np.random.default_rng(8)
    stage = R.make_stage(n0, B, seed=5)
    w, b = ER.random_weights(E1_HOOK, K, seed=9)
    temps = (1.0, 3.0, 0.5)
    z = (rng.standard_normal((3, n0, K)) * 2.0).astype(np.float32)
    x = ER.scaled(z, temps)
    want = ER.ensemble(x, w[:3, :3], b[:3])                                     # (3, n0, K) by document of the first stage
    state = np.full((E1_HOOK, B, K), SENT64, np.int64)
    alive = np.arange(n0)
    for e in range(3):
        st = dict(stage, n=len(alive), doc_orig=stage["doc_orig"][alive], n_rows=len(alive), sum_len_sq=len(alive))
        y, state = _call_hook(pkg, st, z[e, alive], state, w, b, e, temps[e], B, by_pointer=e % 2)
        ok, _ = ER.ulp_close_f32(y[:len(alive)].view(np.float32), want[e, alive])
        assert ok.all(), (e, np.argwhere(~ok)[:4].tolist())
        gone = np.setdiff1d(np.arange(n0), alive)
        assert np.all(state[e, stage["doc_orig"][gone]] == SENT64)              # who left earlier is not written
        alive = alive[rng.random(len(alive)) > 1.0 / 3.0]
    free = np.setdiff1d(np.arange(B), stage["doc_orig"])
    assert np.all(state[:, free] == SENT64) and np.all(state[3:] == SENT64)


def test_launch_refusals(pkg):
    c = _hook_case(65, 16)
    args = (c["stage"], c["z"], c["state"].copy(), c["w"], c["b"], c["e"], c["temp"], c["B"])
    with pytest.raises(pkg.capi.MMEEError, match="exit_index"):
        _call_hook(pkg, *args[:5], E1_HOOK, c["temp"], c["B"])
    with pytest.raises(pkg.capi.MMEEError, match="exit_index"):
        _call_hook(pkg, *args[:5], -1, c["temp"], c["B"])
    with pytest.raises(pkg.capi.MMEEError, match="rows of out"):
        _call_hook(pkg, *args, out_rows=64)
    with pytest.raises(pkg.capi.MMEEError, match="rows of pol_logits"):
        _call_hook(pkg, *args, pol_rows=64)
    bad = dict(c["stage"], doc_orig=c["stage"]["doc_orig"].copy())
    bad["doc_orig"][7] = c["B"]
    with pytest.raises(pkg.capi.MMEEError, match="doc_orig"):
        _call_hook(pkg, bad, *args[1:])
    with pytest.raises(pkg.capi.MMEEError, match="n_docs"):
        _call_hook(pkg, c["stage"], *args[1:7], 64)                             # B below the stage's document count


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the forward
# ---------------------------------------------------------------------------------------------------------------------------------------
H256_RAMP = dict(MATRIX_CASES["h256_entropy_1layer"][1], inference_strategy="max_confidence")
# name -> (shape, EE_config, precision, documents, text length, per-exit temperatures)
CASES = {
    "tiny_ramp": ("tiny", dict(TINY_CASES["tiny_ramp"]), "fp32", 24, 16, False),
    "h256_ramp": ("h256", H256_RAMP, "split", 24, 48, True),
    "h256_gate": ("h256", dict(MATRIX_CASES["h256_gate"][1]), "split", 24, 48, True),
    "dit_tiny": ("dit", dict(DIT_EE), None, 24, 0, False),
}
FIELDS = ("logits", "exit_layer", "confidence")
SIGN = csf_ref.SIGN


class Case:
    """One configuration: the engine, the documents, its un-ensembled dump (once), a non-trivial (w, b) and the ensembled dump (once)."""

    def __init__(self, pkg, name):
        torch = _torch()
        shape, ee, precision, B, T, temps = CASES[name]
        self.pkg, self.name, self.B, self.T, self.dit, self.precision = pkg, name, B, T, shape == "dit", precision
        mk = {"tiny": lambda **kw: pkg.ModelConfig.tiny(**kw), "h256": lambda **kw: pkg.ModelConfig.tiny(**kw, **H256_KW),
              "dit": lambda **kw: pkg.ModelConfig.dit_tiny(**kw)}[shape]
        self.cfg = mk(EE_config=dict(ee))
        if self.dit:
            self.W = pkg.synth.make_weights_beit(self.cfg, seed=81, head_gain=4.0)
            docs = {"pixel_values": pkg.synth.make_documents(self.cfg, B, seed=82, text_len=8)["pixel_values"]}
        else:
            self.W = pkg.synth.make_weights(self.cfg, seed=81, head_gain=4.0)
            d = pkg.synth.make_documents(self.cfg, B, seed=82, text_len=T, min_words=2)
            docs = {k: d[k] for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}
        self.dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in docs.items()}
        self.E, self.K = self.cfg.exit_config.num_exits, self.cfg.num_labels
        self.tm = np.random.default_rng(5).uniform(0.5, 3.0, self.E + 1) if temps else None
        self.w, self.b = ER.random_weights(self.E + 1, self.K, seed=len(name))
        self.eng = self.engine()
        self._plain = self._ens = None

    def engine(self):
        size = dict(max_docs=self.B) if self.dit else dict(max_docs=self.B, max_text_len=self.T, precision=self.precision)
        eng = self.pkg.EarlyExitEngine(self.cfg, **size)
        eng.load_weights(self.W)
        return eng

    def inputs(self):
        return {k: v.contiguous() for k, v in self.dev.items()}

    def fwd(self, eng=None, **kw):
        return (eng or self.eng).forward(**self.inputs(), temperatures=self.tm, whole_layers=True, **kw)

    def plain(self):
        """The un-ensembled dump (numpy all_logits, all_crit, head_logits) of the case's engine, with no ensemble set."""
        if self._plain is None:
            assert not self.eng.has_ensemble
            o = self.fwd(dump_all=True, want_all=True, want_head=True)
            self.eng.check()
            self._plain = dict(al=_np(o.all_logits), ac=_np(o.all_crit), hl=_np(o.head_logits), hc=_np(o.head_crit))
            assert np.isfinite(self._plain["al"]).all()
        return self._plain

    def ensembled(self):
        """sweep.ensemble_logits of the un-ensembled dump: float64 (E1,B,K) on the host, every value a float32."""
        if self._ens is None:
            y = _np(self.pkg.sweep.ensemble_logits(self.plain()["al"], self.w, self.b))
            assert y.dtype == np.float64 and np.array_equal(y, y.astype(np.float32).astype(np.float64))
            self._ens = y
        return self._ens

    def thresholds(self, criterion, position=0.65):
        """(thr (E1,), reference table (E1,B)): gap midpoints of the reference criterion of the ensembled array, every document clear of them."""
        table = csf_ref.csf(self.ensembled(), criterion)
        thr, width = csf_ref.gap_thresholds(table, position if SIGN[criterion] > 0 else 1.0 - position, MIN_GAP)
        assert np.all(width > MIN_GAP), (self.name, criterion, width.tolist())
        dist = np.abs(table[:-1] - thr[:-1, None]).min()
        assert dist > MIN_DIST, (self.name, criterion, "a reference criterion within 1e-12 of its threshold", float(dist))
        return thr, table


@pytest.fixture(scope="module")
def cases(pkg):
    built = {}

    def get(name):
        if name not in built:
            built[name] = Case(pkg, name)
        c = built[name]
        c.plain()                                                               # before any test sets an ensemble
        c.eng.set_ensemble((c.w, c.b))
        c.eng.set_criterion("max_confidence")
        c.eng.set_exit_rule("plain")
        return c

    yield get
    for c in built.values():
        c.eng.close()


@pytest.mark.parametrize("name", list(CASES))
def test_dump_all_equals_the_tool_on_the_plain_dump_bit_for_bit(cases, name):
    c = cases(name)
    p, want = c.plain(), c.ensembled().astype(np.float32)
    o = c.fwd(dump_all=True, want_all=True, want_head=True)
    c.eng.check()
    al = _np(o.all_logits)
    assert np.array_equal(_bits(al), _bits(want)), (name, int((_bits(al) != _bits(want)).sum()))
    # 1 ulp of the restatement on the same rows (the scaled rows are what the plain dump stores)
    ok, near = ER.ulp_close_f32(al, ER.ensemble(p["al"], c.w, c.b))
    assert ok.all()
    report_measured(f"ensemble.forward[{name}]", f"float32 neighbours of the restatement, of {al.size}", float(near))
    # the criterion is the ensemble row's (temperature 1); the head's own outputs are untouched
    ref = csf_ref.max_softmax(al.astype(np.float64))
    assert np.abs(_np(o.all_crit) - ref).max() < 1e-6
    assert np.array_equal(_np(o.head_logits), p["hl"]) and np.array_equal(_np(o.head_crit), p["hc"])
    assert np.array_equal(_np(o.logits), al[c.E]) and np.all(_np(o.exit_layer) == c.E)
    assert not np.array_equal(al, p["al"])


def _check_rows(c, o, ex, dump, tag):
    rows = np.arange(c.B)
    assert np.array_equal(_np(o.exit_layer), ex), (tag, _np(o.exit_layer).tolist(), ex.tolist())
    assert np.array_equal(_bits(_np(o.logits)), _bits(_np(dump.all_logits)[ex, rows])), tag
    assert np.array_equal(_bits(_np(o.confidence)), _bits(_np(dump.all_crit)[ex, rows])), tag


@pytest.mark.parametrize("name,criterion", [(n, cr) for n in CASES for cr in csf_ref.CRITERIA if cr == "max_confidence" or n in ("tiny_ramp", "h256_ramp")])
def test_threshold_criteria_decide_on_the_ensemble_row(cases, pkg, name, criterion):
    c = cases(name)
    c.eng.set_criterion(criterion)
    thr, table = c.thresholds(criterion)
    ex_ref = csf_ref.exits(table, thr, SIGN[criterion])
    assert len(np.unique(ex_ref)) >= 3, np.bincount(ex_ref).tolist()
    exits, pred, conf, _ = pkg.policy.criterion_scan_device(c.ensembled(), thr, criterion, want_conf=True)
    assert np.array_equal(_np(exits), ex_ref)
    dump = c.fwd(dump_all=True, want_all=True)
    o = c.fwd(thresholds=thr)
    _check_rows(c, o, _np(exits), dump, (name, criterion))
    assert np.array_equal(_np(pred).astype(np.float32), _np(o.logits)) and np.array_equal(_np(conf).astype(np.float32), _np(o.confidence))
    assert c.eng.stage_counts()["docs"] == [int((ex_ref >= e).sum()) for e in range(c.E + 1)]
    c.eng.check()


@pytest.mark.parametrize("name", ["tiny_ramp", "h256_ramp"])
def test_patience_and_the_two_rules_take_the_ensemble_rows_argmax(cases, pkg, name):
    c = cases(name)
    ens = c.ensembled()
    dump = c.fwd(dump_all=True, want_all=True)
    c.eng.set_criterion("patience")
    ex = _np(pkg.policy.patience_scan_device(ens, 2)[0])
    o = c.fwd(patience=2)
    assert np.array_equal(_np(o.exit_layer), ex) and np.array_equal(_bits(_np(o.logits)), _bits(_np(dump.all_logits)[ex, np.arange(c.B)]))
    plain_ex = _np(pkg.policy.patience_scan_device(c.plain()["al"], 2)[0])
    c.eng.set_criterion("max_confidence")
    thr, table = c.thresholds("max_confidence", position=0.5)
    msp = pkg.sweep.msp_table(ens)[0]
    seen = {tuple(ex.tolist()), tuple(plain_ex.tolist())}
    for rule in ("patient_confident", "patience_or_threshold"):
        exr = _np(pkg.policy.rule_scan_device(msp, ens, thr, 2, rule)[0])
        o = c.fwd(thresholds=thr, exit_rule=rule, patience=2)
        _check_rows(c, o, exr, dump, (name, rule))
        seen.add(tuple(exr.tolist()))
    c.eng.set_exit_rule("plain")
    assert len(seen) >= 2
    c.eng.check()


@pytest.mark.parametrize("name", ["tiny_ramp", "h256_gate", "dit_tiny"])
def test_captured_and_streamed_forwards_return_the_eager_bits(cases, pkg, name):
    c = cases(name)
    thr, table = c.thresholds("max_confidence")
    ex = csf_ref.exits(table, thr, +1)
    want = {f: _np(getattr(c.fwd(thresholds=thr), f)) for f in FIELDS}
    assert np.array_equal(want["exit_layer"], ex)
    eng = c.engine()
    eng.set_ensemble((c.w, c.b))
    cap = eng.capture(**{k: v.clone() for k, v in c.inputs().items()}, thresholds=thr, temperatures=c.tm, whole_layers=True)
    for f in FIELDS:
        assert np.array_equal(_np(getattr(cap.outputs, f)), want[f]), f
    out = cap.launch(thresholds=np.full(c.E + 1, 2.0), temperatures=c.tm)
    assert np.all(_np(out.exit_layer) == c.E)
    out = cap.launch(thresholds=thr, temperatures=c.tm)
    for f in FIELDS:
        assert np.array_equal(_np(getattr(out, f)), want[f]), f
    # a graph's launch list is the one of its capture: the ensemble cannot be switched off under it; new weights are read by the replays
    with pytest.raises(pkg.capi.MMEEError, match="captured graphs"):
        eng.set_ensemble(None)
    assert eng.has_ensemble
    w2 = np.tril(np.ones((c.E + 1, c.E + 1))) / np.arange(1, c.E + 2)[:, None]   # the running geometric mean, no bias
    eng.set_ensemble((w2, None))
    keep_all = np.full(c.E + 1, 2.0)
    out = cap.launch(thresholds=keep_all, temperatures=c.tm)
    mean = _np(pkg.sweep.ensemble_logits(c.plain()["al"], w2))[c.E].astype(np.float32)
    assert np.array_equal(_bits(_np(out.logits)), _bits(mean))
    eng.check()
    cap.close()
    eng.set_ensemble((c.w, c.b))
    rs = eng.forward_stream(**c.inputs(), thresholds=thr, temperatures=c.tm, whole_layers=True)
    chunks = list(rs)
    assert [ch.exit_index for ch in chunks] == list(range(c.E + 1))
    docs = np.concatenate([ch.doc_index for ch in chunks])
    assert np.array_equal(np.sort(docs), np.arange(c.B))                        # every document once
    for ch in chunks:
        assert np.all(ex[ch.doc_index] == ch.exit_index) and np.all(ch.exit_layer == ch.exit_index)
        assert np.array_equal(ch.logits, want["logits"][ch.doc_index]) and np.array_equal(ch.confidence, want["confidence"][ch.doc_index])
    eng.check()
    eng.close()


def test_low_latency_against_its_own_flagged_dump(cases, pkg):
    c = cases("h256_ramp")
    c.eng.set_ensemble(None)
    plain = c.fwd(dump_all=True, want_all=True, low_latency=True)
    c.eng.set_ensemble((c.w, c.b))
    ens = pkg.sweep.ensemble_logits(plain.all_logits, c.w, c.b)
    dump = c.fwd(dump_all=True, want_all=True, low_latency=True)
    assert np.array_equal(_bits(_np(dump.all_logits)), _bits(_np(ens).astype(np.float32)))
    table = csf_ref.max_softmax(_np(ens))
    thr, width = csf_ref.gap_thresholds(table, 0.65, MIN_GAP)
    assert np.abs(table[:-1] - thr[:-1, None]).min() > MIN_DIST
    ex = _np(pkg.policy.criterion_scan_device(ens, thr, "max_confidence")[0])
    assert np.array_equal(ex, csf_ref.exits(table, thr, +1)) and len(np.unique(ex)) >= 3
    o = c.fwd(thresholds=thr, low_latency=True)
    _check_rows(c, o, ex, dump, "low_latency")
    c.eng.check()


def test_clearing_the_ensemble_returns_the_bits_and_the_launches_of_before(cases, pkg):
    c = cases("h256_ramp")
    eng = c.engine()
    ac = _np(eng.forward(**c.inputs(), dump_all=True, want_all=True, whole_layers=True, temperatures=c.tm).all_crit).astype(np.float64)
    call = dict(thresholds=np.median(ac, axis=1), temperatures=c.tm, whole_layers=True)

    def run():
        eng.profile(True)
        o = eng.forward(**c.inputs(), **call)
        prof = eng.profile_read()
        eng.profile(False)
        return {f: _np(getattr(o, f)) for f in FIELDS}, {role: v["launches"] for role, v in prof.items()}

    before, n_before = run()
    assert n_before["exit_ensemble"] == 0 and n_before["exit_decide"] == c.E + 1 and not eng.has_ensemble
    eng.set_ensemble((c.w, c.b))
    under, n_under = run()
    assert eng.has_ensemble and n_under["exit_ensemble"] == c.E + 1
    assert n_under["exit_decide"] == c.E + 1 and n_under["exit_head"] == n_before["exit_head"]
    assert not np.array_equal(under["logits"], before["logits"])
    assert eng.set_ensemble(None) is None
    after, n_after = run()
    for f in FIELDS:
        assert np.array_equal(before[f], after[f]), f
    assert n_after == n_before and len(np.unique(before["exit_layer"])) >= 2
    eng.close()


def test_refusals_say_why_and_change_nothing(cases, pkg):
    c = cases("h256_gate")
    eng = c.engine()
    E1, K = c.E + 1, c.K
    eng.set_ensemble((c.w, c.b))
    ref = _np(eng.forward(**c.inputs(), dump_all=True, whole_layers=True, temperatures=c.tm).logits)
    bad = c.w.copy()
    bad[1, 2] = 0.25
    with pytest.raises(pkg.capi.MMEEError, match="above the diagonal"):
        eng.set_ensemble((bad, c.b))
    for v in (np.nan, np.inf):
        bad = c.w.copy()
        bad[E1 - 1, 0] = v
        with pytest.raises(pkg.capi.MMEEError, match="not finite"):
            eng.set_ensemble((bad, c.b))
        badb = c.b.copy()
        badb[0, K - 1] = v
        with pytest.raises(pkg.capi.MMEEError, match="not finite"):
            eng.set_ensemble((c.w, badb))
    with pytest.raises(ValueError, match="weights must be"):
        eng.set_ensemble((c.w[:-1, :-1], None))
    with pytest.raises(pkg.capi.MMEEError, match="MMEE_CRIT_GATE"):             # ee_set_criterion while an ensemble is set
        eng.set_criterion("gate")
    assert str(eng.exit_config.inference_strategy) == "max_confidence" and eng.has_ensemble
    assert np.array_equal(_np(eng.forward(**c.inputs(), dump_all=True, whole_layers=True, temperatures=c.tm).logits), ref)
    eng.set_ensemble(None)
    eng.set_criterion("gate")
    with pytest.raises(pkg.capi.MMEEError, match="MMEE_CRIT_GATE"):             # ee_set_ensemble under the gate criterion
        eng.set_ensemble((c.w, c.b))
    assert not eng.has_ensemble
    eng.set_criterion("max_confidence")
    thr = np.full(E1, 0.5)
    cap = eng.capture(**{k: v.clone() for k, v in c.inputs().items()}, thresholds=thr, temperatures=c.tm, whole_layers=True)
    with pytest.raises(pkg.capi.MMEEError, match="captured graphs"):
        eng.set_ensemble((c.w, c.b))
    assert not eng.has_ensemble
    cap.close()
    eng.set_ensemble((c.w, c.b))                                                # the graph is gone: fine
    eng.close()
    lte_cfg = pkg.ModelConfig.tiny(EE_config=dict(exits=[1, 2], encoder_layer_strategy="ramp", use_lte=True), **H256_KW)
    lte = pkg.EarlyExitEngine(lte_cfg, max_docs=4, max_text_len=16)
    with pytest.raises(pkg.capi.MMEEError, match="use_lte"):
        lte.set_ensemble((np.eye(3), None))
    lte.close()


def test_tool_nan_rows_and_the_tables_behind_it(pkg):
    """A NaN input row gives NaN from that exit on; the result goes unchanged into csf_table, the sweep, the search, the refine and the report."""
    store, refs = sweep_ref_inputs(seed=21, E1=5, N=1025, K=7)
    x = store.astype(np.float32)
    w, b = ER.random_weights(5, 7, seed=2)
    x[2, 11] = np.nan
    y = _np(pkg.sweep.ensemble_logits(x, w, b))
    ok, _ = ER.ulp_close_f32(y.astype(np.float32), ER.ensemble(x, w, b))
    assert ok.all() and np.isnan(y[2:, 11]).all() and np.isfinite(y[:2, 11]).all() and np.isfinite(np.delete(y, 11, 1)).all()
    x[2, 11] = store[2, 11]
    ens = pkg.sweep.ensemble_logits(x, w, b)
    table, correct = pkg.sweep.csf_table(ens, refs, "max_confidence")
    ref = csf_ref.max_softmax(_np(ens))
    assert np.abs(_np(table) / ref - 1.0).max() <= 1e-12
    res = pkg.sweep.threshold_search(ens, refs, num_per_exit=4, mixtures="grid")
    assert len(res.front_mean_exit) >= 1
    res_c = pkg.sweep.threshold_search(ens, refs, num_per_exit=4, mixtures="grid", cost=np.arange(1, 6) * 10)
    assert len(res_c.front_thresholds) >= 1
    ref_r = pkg.sweep.threshold_refine(ens, refs, num_per_exit=4, hit_value=2)
    assert ref_r is not None
    rep = pkg.metrics.exit_report(ens, refs)
    assert rep is not None
    pol = pkg.Policy(_np(ens), {"exit_threshold": 0.5}).max_confidence_global_thresholding_policy()
    assert pol is not None
    thr = res.front_thresholds[0]
    ex = _np(pkg.policy.criterion_scan_device(ens, thr, "max_confidence")[0])
    assert np.array_equal(ex, csf_ref.exits(ref, thr, +1)) or np.abs(ref[:-1] - np.asarray(thr)[:-1, None]).min() <= MIN_DIST


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. the fit
# ---------------------------------------------------------------------------------------------------------------------------------------
L2 = 1e-2


def _fit_table(E1, N, K):
    store, refs = sweep_ref_inputs(seed=100 + E1 + N + K, E1=E1, N=N, K=K)
    return store.astype(np.float32), refs


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", [300, 1000])
@pytest.mark.parametrize("E1", [4, 7])
def test_fit_reaches_the_reference_optimum_within_the_derived_bounds(pkg, E1, N, K):
    x, refs = _fit_table(E1, N, K)
    fit = pkg.heads.fit_exit_ensemble(x, refs, l2=L2)
    w, b = _np(fit.weights), _np(fit.bias)
    assert _np(fit.status).tolist() == [0] * E1, (_np(fit.status).tolist(), _np(fit.evals).tolist(), _np(fit.grad_norm).tolist())
    assert not np.triu(w, 1).any()
    l = ER.logsoftmax64(x)
    nll = ER.plain_nll(l, refs)
    loss = _np(fit.loss)
    assert np.all(loss <= nll), (loss.tolist(), nll.tolist())
    lnorm = np.sqrt((l ** 2).sum((0, 2)) + 1.0).max()                            # max_n |(l_.,n, 1)|, over all exits and labels: an upper bound
    w_ref, b_ref = np.zeros_like(w), np.zeros_like(b)
    worst = 0.0
    for m in range(E1):
        th = ER.full_theta(w, b, m)
        f_dev, g = ER.objective(th, l, refs, m, L2)
        th_ref, f_ref, g_ref = ER.reference_optimum(l, refs, m, L2)
        assert g_ref <= 1e-12
        bound = (np.linalg.norm(g) + g_ref) / L2
        dist = float(np.linalg.norm(th - th_ref))
        assert dist <= bound, (m, dist, bound)
        assert abs(loss[m] - f_dev) <= 1e-12 * max(1.0, abs(f_dev))              # the reported loss is the objective at the returned point
        worst = max(worst, bound)
        b_ref[m], w_ref[m, :m + 1] = th_ref[:K], th_ref[K:]
    y = _np(fit.apply(x))
    y_ref = ER.combine(l, w_ref, b_ref)
    tol = worst * lnorm + np.spacing(np.abs(y_ref).astype(np.float32)).astype(np.float64) + 1e-12 * np.abs(y_ref)
    assert np.all(np.abs(y - y_ref) <= tol), float((np.abs(y - y_ref) - tol).max())
    report_measured(f"ensemble.fit[E1={E1},N={N},K={K}]", "evaluations (max over exits) + derived |theta - theta*| bound",
                    float(_np(fit.evals).max()) + worst)


def test_fit_is_deterministic_and_an_exit_alone_equals_itself_among_others(pkg):
    x, refs = _fit_table(7, 1000, 16)
    a = pkg.heads.fit_exit_ensemble(x, refs, l2=L2)
    b = pkg.heads.fit_exit_ensemble(x, refs, l2=L2)
    for f in ("weights", "bias", "loss", "grad_norm", "evals", "status"):
        assert np.array_equal(_np(getattr(a, f)), _np(getattr(b, f))), f
    for m in (0, 3, 5):                                                         # the table cut behind exit m: exit m is fitted last, or alone (m = 0)
        cut = pkg.heads.fit_exit_ensemble(x[:m + 1], refs, l2=L2)
        assert np.array_equal(_np(cut.weights)[m], _np(a.weights)[m, :m + 1]) and np.array_equal(_np(cut.bias)[m], _np(a.bias)[m]), m
        assert _np(cut.loss)[m] == _np(a.loss)[m] and _np(cut.evals)[m] == _np(a.evals)[m]
    # a warm start from the optimum stays there
    again = pkg.heads.fit_exit_ensemble(x, refs, l2=L2, init=a)
    assert _np(again.status).tolist() == [0] * 7 and np.abs(_np(again.weights) - _np(a.weights)).max() < 1e-6


def test_fit_fails_on_a_bad_label_or_a_nan_logit_and_writes_nothing(pkg):
    torch = _torch()
    x, refs = _fit_table(4, 300, 16)
    E1, N, K = x.shape
    lib = pkg.capi.load()
    need = int(lib.ee_ensemble_fit_workspace_bytes(E1, N, K, 8))
    assert need > 0

    def run(xx, yy):
        L = torch.from_numpy(xx.astype(np.float64)).cuda()
        y = torch.from_numpy(yy).cuda()
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        outs = [torch.full(s, 7.5, dtype=torch.float64, device="cuda") for s in ((E1, E1), (E1, K), (E1,), (E1,))]
        ints = [torch.full((E1,), 77, dtype=torch.int32, device="cuda") for _ in range(2)]
        rc = lib.ee_ensemble_fit(L.data_ptr(), y.data_ptr(), None, None, E1, N, K, L2, 1e-9, 50, 8, ws.data_ptr(), need,
                                 *[t.data_ptr() for t in outs + ints], _stream())
        torch.cuda.synchronize()
        return rc, pkg.capi.last_error(), all(bool((t == 7.5).all()) for t in outs) and all(bool((t == 77).all()) for t in ints)

    rc, _, untouched = run(x, refs)
    assert rc == 0 and not untouched
    for bad_label in (-1, K):
        yy = refs.copy()
        yy[123] = bad_label
        rc, msg, untouched = run(x, yy)
        assert rc != 0 and "label" in msg and "no output was written" in msg and untouched
    for v in (np.nan, np.inf):
        xx = x.copy()
        xx[2, 17, 3] = v
        rc, msg, untouched = run(xx, refs)
        assert rc != 0 and "logit is not finite" in msg and untouched
    with pytest.raises(pkg.capi.MMEEError, match="l2"):
        pkg.heads._call("ee_ensemble_fit", torch.device("cuda:0"), torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda"), None, None, E1, N, K, 0.0,
                        1e-9, 50, 8, torch.zeros(1, device="cuda"), need, *[torch.zeros(1, device="cuda")] * 6)


def test_end_to_end_dump_fit_set_forward(cases, pkg):
    """A dump-all forward, the fit on it, set_ensemble(fit): the forward's dump-all rows equal fit.apply(...) bit for bit."""
    c = cases("tiny_ramp")
    p = c.plain()
    refs = np.random.default_rng(12).integers(0, c.K, c.B)
    fit = pkg.heads.fit_exit_ensemble(p["al"], refs, l2=L2)
    assert _np(fit.status).tolist() == [0] * (c.E + 1)
    eng = c.engine()
    eng.set_ensemble(fit)
    o = eng.forward(**c.inputs(), dump_all=True, want_all=True, whole_layers=True, temperatures=c.tm)
    want = _np(fit.apply(p["al"])).astype(np.float32)
    assert np.array_equal(_bits(_np(o.all_logits)), _bits(want))
    nll = lambda a: -ER.logsoftmax64(a)[:, np.arange(c.B), refs].mean(1)
    assert np.all(nll(want) <= nll(p["al"]) + 1e-6)                              # the training loss went down at every exit (float32 rounding aside)
    eng.check()
    eng.close()
