"""The gate decision (include/mmee.h MMEE_CRIT_GATE, ``inference_strategy = "gate"``) on the MI355X against the numpy restatement of
tests/gate_ref.py: the decide kernel alone through ee_debug_exit_decide at the wave and chunk edges, the forward (eager, captured, streamed,
low-latency) on the ``tiny_gate`` and ``h256_gate`` configurations, and the dumped-array tools (``sweep.gate_table``,
``policy.gate_scan_device``, ``Policy.gate_policy``, the sweeps, the search and the report on the table).  The reference's evaluation never
lets a gate decide, so the restatement is the oracle.

The device's exp may differ from numpy's in the last place: every threshold sits at the midpoint of two adjacent sorted reference scores more
than 1e-9 apart and every test asserts, on the CPU, that no document's reference score is within 1e-12 of its threshold.  The cases with no
rounding at all (g = 0.5, 0, 1 against thr = 0.5, nextafter(0.5, 0), 0, 1) are tested at equality.

Acceptance: integer outputs, copied logits and scaled rows by equality; out_conf / out_all_crit / out_head_crit within 1 ulp of the float32 of
the reference score; float64 table entries within 1e-12 relative."""
import ctypes as C

import numpy as np
import pytest

from . import csf_ref
from . import exit_stage_ref as R
from . import gate_ref as G
from . import rule_ref
from .conftest import H256_KW, MATRIX_CASES, TINY_CASES, report_measured, sweep_ref_inputs
from .hook_util import SENTINEL, _stream, _torch

pytestmark = pytest.mark.gpu

GUARD = 4
STAGE_N = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
KS = (2, 16, 17)
RULES = (G.PLAIN, G.STREAK, G.EITHER)
RULE_IDS = {G.PLAIN: "plain", G.STREAK: "streak", G.EITHER: "either"}
EXIT, PATIENCE = 2, 2


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the decide kernel alone
# ---------------------------------------------------------------------------------------------------------------------------------------
def _i32(a, pad=1):
    torch = _torch()
    a = np.asarray(a, np.int64).reshape(-1)
    return torch.from_numpy(np.concatenate([a, np.full(pad, SENTINEL, np.int64)]).astype(np.int32)).cuda()


def _f32(a):
    torch = _torch()
    a = np.ascontiguousarray(a, np.float32)
    return torch.from_numpy(a if a.size else np.zeros(4, np.float32)).cuda()


def _sent(words):
    torch = _torch()
    return torch.full((int(words) + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")


def _counts(stage):
    sq = stage["sum_len_sq"]
    return [stage["n"], stage["n_rows"], sq & 0xFFFFFFFF, sq >> 32]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def gate_case(n, K, rule, seed, position=0.6):
    """One exit of one stage under the gate criterion: n documents in B slots, policy logits (n,K), gate logits (n,2) with a spread of scores,
    the threshold at a gap midpoint near `position` n, state that makes the rules matter (streaks of 0 .. 2, half of the argmaxes agree)."""
    rng = np.random.default_rng(9000 + 131 * n + 7 * K + rule + seed)
    B = n + 29
    stage = R.make_stage(n, B, seed)
    temp = (1.0, 3.0, 0.5)[(n + K) % 3]
    z = (rng.standard_normal((n, K)) * 2.0).astype(np.float32)
    head = (rng.standard_normal((n, 2)) * 1.5).astype(np.float32)
    g = G.gate_score(head)
    thr, _ = G.midpoint_threshold(g, position)
    G.assert_clear(g, thr, ("gate_case", n, K, rule))
    prev, run = np.full(B, R.DIRTY, np.int64), np.full(B, R.DIRTY, np.int64)
    o = stage["doc_orig"]
    am = np.argmax((z.astype(np.float64) / temp).astype(np.float32), -1)
    prev[o] = np.where(rng.random(n) < 0.5, am, (am + 1) % K)
    run[o] = rng.integers(0, 3, n)
    return dict(n=n, B=B, K=K, stage=stage, logits=z, head=head, thr=thr, temp=temp, rule=rule, patience=PATIENCE, exit_index=EXIT, state=(prev, run))


def _decide(pkg, c, by_pointer=0, is_final=0, no_exit=0, criterion=G.CRIT_GATE, mode=0, Kh=2, null_head=False):
    """One ee_debug_exit_decide call of case c; every output buffer starts as SENTINEL words and ends in GUARD entries."""
    torch = _torch()
    st, n, B, K, e = c["stage"], c["n"], c["B"], c["K"], c["exit_index"]
    dev = dict(counts=_i32(_counts(st), 0), doc_orig=_i32(st["doc_orig"]), doc_off=_i32(st["doc_off"]), x_phys=_i32(st["x_phys"]))
    b = dict(prev=_i32(c["state"][0], GUARD), run=_i32(c["state"][1], GUARD), n_counts=_sent(4), n_doc_orig=_sent(n), n_doc_off=_sent(n + 1),
             n_x_src=_sent(n), n_meta_src=_sent(n), out_logits=_sent(B * K), out_exit=_sent(B), out_conf=_sent(B),
             out_all_logits=_sent((e + 1) * B * K), out_all_crit=_sent((e + 1) * B), out_head_logits=_sent((e + 1) * B * 2),
             out_head_crit=_sent((e + 1) * B))
    keep = [_f32(c["logits"]), _f32(c["head"])]
    a = pkg.capi.DebugExitDecideArgs()
    for k, v in dict(mode=mode, rule=c["rule"], criterion=criterion, K=K, Kh=Kh, thr=c["thr"], temp=c["temp"], patience=c["patience"],
                     by_pointer=by_pointer, exit_index=e, is_final=int(is_final), no_exit=int(no_exit), B=B).items():
        setattr(a, k, v)
    a.pol_logits, a.head_logits, a.lte_score = keep[0].data_ptr(), None if null_head else keep[1].data_ptr(), None
    for k, t in list(dev.items()) + list(b.items()):
        setattr(a, k, t.data_ptr())
    pkg.capi.check(pkg.capi.load().ee_debug_exit_decide(C.byref(a), _stream()), None, "ee_debug_exit_decide")
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in b.items()}


def _ulp_f32(tag, got_words, ref64, ct):
    """Within 1 ulp of np.float32(ref64): the value itself or a float32 neighbour."""
    got = np.asarray(got_words, np.int32).view(np.float32)
    want = np.asarray(ref64, np.float64).astype(np.float32)
    same = got == want
    near = (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))
    bad = np.nonzero(~(same | near))[0]
    assert bad.size == 0, (tag, bad[:6].tolist(), got[bad[:6]].tolist(), want[bad[:6]].tolist())
    ct["near"] += int((~same).sum())
    ct["all"] += len(got)


def _slots(tag, words, rows, width, want_rows=None):
    """Rows `rows` of a [*, width] buffer: want_rows when given (bit patterns); every other word is SENTINEL.  Returns the rows' words."""
    idx = (np.asarray(rows, np.int64)[:, None] * width + np.arange(width)[None]).reshape(-1)
    got = words[idx].copy()
    if want_rows is not None:
        want = np.asarray(want_rows, np.int32).reshape(-1)
        assert np.array_equal(got, want), (tag, np.nonzero(got != want)[0][:6].tolist())
    rest = words.copy()
    rest[idx] = SENTINEL
    assert (rest == SENTINEL).all(), (tag, "a write outside the documents' slots")
    return got


def _check(tag, c, b, ct, is_final=False, no_exit=False):
    st, n, B, K, e = c["stage"], c["n"], c["B"], c["K"], c["exit_index"]
    r = G.decide(st, c["logits"], c["head"], thr=c["thr"], temp=c["temp"], rule=c["rule"], patience=c["patience"], exit_index=e, B=B,
                 state=c["state"], is_final=is_final, no_exit=no_exit)
    lv, o = r["leave"], st["doc_orig"]
    nx = R._next_stage(st, ~lv, "")
    got_counts = [int(w) & 0xFFFFFFFF for w in b["n_counts"]]
    assert got_counts == _counts(nx) + [SENTINEL] * GUARD, (tag, got_counts, _counts(nx))
    for k, extra in (("n_doc_orig", 0), ("n_doc_off", 1), ("n_x_src", 0), ("n_meta_src", 0)):
        want = nx[k][:n + extra + GUARD]
        assert np.array_equal(b[k], want), (tag, k, np.nonzero(b[k] != want)[0][:6].tolist())
    for k, want in zip(("prev", "run"), r["state"]):
        assert np.array_equal(b[k], np.concatenate([want, [SENTINEL] * GUARD])), (tag, k)
    _slots((tag, "out_exit"), b["out_exit"], o[lv], 1, np.full(int(lv.sum()), e))
    _slots((tag, "out_logits"), b["out_logits"], o[lv], K, _bits(r["scaled32"][lv]))
    _slots((tag, "out_all_logits"), b["out_all_logits"], e * B + o, K, _bits(r["scaled32"]))
    _slots((tag, "out_head_logits"), b["out_head_logits"], e * B + o, 2, _bits(c["head"]))
    _ulp_f32((tag, "out_conf"), _slots((tag, "out_conf"), b["out_conf"], o[lv], 1), r["crit"][lv], ct)
    _ulp_f32((tag, "out_all_crit"), _slots((tag, "out_all_crit"), b["out_all_crit"], e * B + o, 1), r["crit"], ct)
    _ulp_f32((tag, "out_head_crit"), _slots((tag, "out_head_crit"), b["out_head_crit"], e * B + o, 1), r["head_crit"], ct)
    return r


@pytest.mark.parametrize("n", STAGE_N)
def test_decide_gate_at_the_wave_and_chunk_edges(pkg, n):
    """Every rule at one stage size, K cycled against it; the values handed over by pointer (a replay's form) give the same bytes."""
    ct = dict(near=0, all=0)
    left = []
    for j, rule in enumerate(RULES):
        K = KS[(STAGE_N.index(n) + j) % 3]
        c = gate_case(n, K, rule, seed=j)
        tag = f"gate.decide[n={n} K={K} {RULE_IDS[rule]}]"
        b = _decide(pkg, c)
        r = _check(tag, c, b, ct)
        left.append(int(r["leave"].sum()))
        b1 = _decide(pkg, c, by_pointer=1)
        for k in b:
            assert np.array_equal(b[k], b1[k]), (tag, k, "by_pointer changes the bytes")
    assert n == 1 or (0 < max(left) and min(left) < n), left
    report_measured(f"gate.decide[n={n}]", f"scores stored as a float32 neighbour of np.float32(ref64), of {ct['all']}", float(ct["near"]))


@pytest.mark.parametrize("rule", RULES, ids=[RULE_IDS[r] for r in RULES])
def test_decide_gate_final_exit_and_no_exit(pkg, rule):
    """The final exit has no gate: the criterion written out is the max-softmax of the scaled row and everybody leaves; under no_exit nobody
    does and the scores are written all the same."""
    ct = dict(near=0, all=0)
    c = gate_case(1025, 17, rule, seed=3)
    for flags in (dict(is_final=True), dict(no_exit=True), dict(is_final=True, no_exit=True)):
        tag = f"gate.decide[{RULE_IDS[rule]} {flags}]"
        r = _check(tag, c, _decide(pkg, c, **flags), ct, **flags)
        assert r["leave"].all() == bool(flags.get("is_final")) and r["leave"].any() == bool(flags.get("is_final"))
        if flags.get("is_final"):
            assert np.array_equal(r["crit"], csf_ref.max_softmax(c["logits"].astype(np.float64) / c["temp"]))
            assert not np.array_equal(r["crit"], r["head_crit"])


def test_decide_gate_is_exact_where_the_score_has_no_rounding(pkg):
    """g = 0.5, 0 and 1 against thr = 0.5, the float64 below it, 0 and 1: strict compares at equality, no tolerance."""
    head = np.array([[1.25, 1.25], [800.0, 0.0], [0.0, 800.0], [-3.0, -3.0]], np.float32)
    g = G.gate_score(head)
    assert g.tolist() == [0.5, 0.0, 1.0, 0.5]
    seen = set()
    for thr in (0.5, float(np.nextafter(0.5, 0.0)), 0.0, 1.0):
        c = gate_case(4, 2, G.PLAIN, seed=1)
        c.update(head=head, thr=thr, exit_index=0)
        b = _decide(pkg, c)
        r = _check(f"gate.decide[exact thr={thr!r}]", c, b, dict(near=0, all=0))
        assert r["leave"].tolist() == G.fires(g, thr).tolist()
        o = c["stage"]["doc_orig"]
        assert np.array_equal(b["out_all_crit"][o], _bits(g)) and np.array_equal(b["out_head_crit"][o], _bits(g))      # 0.5, 0, 1: no ulp to give
        seen.add(tuple(r["leave"].tolist()))
    assert seen == {(False, False, True, False), (True, False, True, True), (False, False, False, False)}


def test_decide_refuses_the_gate_criterion_without_two_gate_logits(pkg):
    c = gate_case(5, 3, G.PLAIN, seed=0)
    with pytest.raises(pkg.capi.MMEEError, match="criterion 4 is none of"):
        _decide(pkg, c, null_head=True)
    with pytest.raises(pkg.capi.MMEEError, match="criterion 4 is none of"):
        _decide(pkg, c, Kh=3)
    with pytest.raises(pkg.capi.MMEEError, match="threshold criterion"):
        _decide(pkg, dict(c, rule=G.PLAIN), mode=1)
    with pytest.raises(pkg.capi.MMEEError, match="criterion 4 is none of"):
        _decide(pkg, dict(c, rule=G.PLAIN), mode=2)
    with pytest.raises(pkg.capi.MMEEError, match="criterion 5"):
        _decide(pkg, c, criterion=5)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the forward
# ---------------------------------------------------------------------------------------------------------------------------------------
# name -> (configuration of tests/conftest.py, precision, documents, text length, per-exit temperatures)
CASES = {
    "tiny_gate_fp32": ("tiny_gate", "fp32", 24, 16, False),
    "h256_gate_fp32": ("h256_gate", "fp32", 24, 48, True),
    "h256_gate_split": ("h256_gate", "split", 24, 48, True),
}
FIELDS = ("logits", "exit_layer", "confidence")
SCHEDULES = (dict(whole_layers=True), dict(probe_always=True, xprobe=False))        # the two whose rows are the dump-all rows bit for bit


class Case:
    """One configuration in one precision: the engine under the gate criterion, its dump-all rows (once) and thresholds from their scores."""

    def __init__(self, pkg, name):
        torch = _torch()
        conf, precision, B, T, temps = CASES[name]
        self.pkg, self.name, self.B, self.T, self.precision = pkg, name, B, T, precision
        if conf in TINY_CASES:
            self.ee, mk = dict(TINY_CASES[conf]), lambda ee: pkg.ModelConfig.tiny(EE_config=ee)
        else:
            self.ee, mk = dict(MATRIX_CASES[conf][1]), lambda ee: pkg.ModelConfig.tiny(EE_config=ee, **H256_KW)
        assert self.ee["inference_strategy"] == "max_confidence" and self.ee["encoder_layer_strategy"] == "gate"
        self.twin_cfg, self.cfg = mk(dict(self.ee)), mk(dict(self.ee, inference_strategy="gate"))
        self.W = pkg.synth.make_weights(self.cfg, seed=61, head_gain=4.0)
        d = pkg.synth.make_documents(self.cfg, B, seed=62, text_len=T, min_words=2)
        self.dev = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}
        self.E, self.K = self.cfg.exit_config.num_exits, self.cfg.num_labels
        self.tm = np.random.default_rng(5).uniform(0.5, 3.0, self.E + 1) if temps else None
        self.eng = self.engine(self.cfg)
        self._dump = None

    def engine(self, cfg, **kw):
        eng = self.pkg.EarlyExitEngine(cfg, max_docs=self.B, max_text_len=self.T, precision=self.precision, **kw)
        eng.load_weights(self.W)
        return eng

    def inputs(self, sl=slice(None)):
        return {k: v[sl].contiguous() for k, v in self.dev.items()}

    def fwd(self, eng=None, **kw):
        return (eng or self.eng).forward(**self.inputs(), **kw)

    def dump(self):
        """(dump-all output as numpy, reference scores (E,B), thresholds (E+1,), reference exits (B,)): whole layers."""
        if self._dump is None:
            o = self.fwd(dump_all=True, want_all=True, want_head=True, whole_layers=True, temperatures=self.tm)
            self.eng.check()
            d = dict(al=_np(o.all_logits), ac=_np(o.all_crit), hl=_np(o.head_logits), hc=_np(o.head_crit), logits=_np(o.logits), conf=_np(o.confidence))
            assert d["hl"].shape == (self.E, self.B, 2) and np.isfinite(d["hl"]).all()
            g = G.gate_score(d["hl"])
            thr, ex = G.cascade_thresholds(g)
            assert set(ex.tolist()) == set(range(self.E + 1)), np.bincount(ex, minlength=self.E + 1).tolist()
            self._dump = (d, g, thr, ex)
        return self._dump


@pytest.fixture(scope="module")
def cases(pkg):
    built = {}

    def get(name):
        if name not in built:
            built[name] = Case(pkg, name)
        return built[name]

    yield get
    for c in built.values():
        c.eng.close()


@pytest.mark.parametrize("name", list(CASES))
def test_forward_scores_and_exits_equal_the_restatement_on_the_dump(cases, name):
    """Dump-all: all_crit and head_crit below the final exit are the float32 of the reference score of the dump's own head_logits (1 ulp); the
    final row is the max-softmax a max_confidence handle reports, and every logits output is that handle's, bit for bit.  Thresholded, under
    whole layers and under the K | V probe: exits == the restatement, a document leaves at every exit and one reaches the end, every row is
    the dump-all row of its exit bit for bit, the stage populations are the survivors."""
    c = cases(name)
    d, g, thr, ex = c.dump()
    ct = dict(near=0, all=0)
    _ulp_f32((name, "all_crit"), _bits(d["ac"][:c.E]).reshape(-1), g.reshape(-1), ct)
    _ulp_f32((name, "head_crit"), _bits(d["hc"]).reshape(-1), g.reshape(-1), ct)
    assert np.array_equal(d["ac"][:c.E], d["hc"])
    report_measured(f"gate[{name}]", f"scores stored as a float32 neighbour of np.float32(ref64), of {ct['all']}", float(ct["near"]))
    twin = c.engine(c.twin_cfg)
    t = twin.forward(**c.inputs(), dump_all=True, want_all=True, want_head=True, whole_layers=True, temperatures=c.tm)
    assert np.array_equal(_np(t.all_logits), d["al"]) and np.array_equal(_np(t.head_logits), d["hl"]) and np.array_equal(_np(t.logits), d["logits"])
    assert np.array_equal(_np(t.all_crit)[c.E], d["ac"][c.E]) and not np.array_equal(_np(t.all_crit)[:c.E], d["ac"][:c.E])
    twin.close()
    # the temperature scales what is written out, never the score
    if c.tm is not None:
        plain = c.fwd(dump_all=True, want_all=True, want_head=True, whole_layers=True)
        assert np.array_equal(_np(plain.all_crit)[:c.E], d["ac"][:c.E]) and not np.array_equal(_np(plain.all_logits), d["al"])
    rows = np.arange(c.B)
    report_measured(f"gate[{name}]", "distinct exits documents leave at", float(len(np.unique(ex))))
    for sched in SCHEDULES:
        o = c.fwd(thresholds=thr, temperatures=c.tm, **sched)
        tag = (name, tuple(sched))
        assert np.array_equal(_np(o.exit_layer), ex), (tag, _np(o.exit_layer).tolist(), ex.tolist())
        assert np.array_equal(_np(o.logits), d["al"][ex, rows]), tag
        assert np.array_equal(_np(o.confidence), d["ac"][ex, rows]), tag
        assert c.eng.stage_counts()["docs"] == [int((ex >= e).sum()) for e in range(c.E + 1)], tag
    o = c.fwd(thresholds=thr, temperatures=c.tm)                       # the engine's default schedule: the same exits
    if c.precision == "fp32":
        assert np.array_equal(_np(o.exit_layer), ex)
    c.eng.check()


@pytest.mark.parametrize("name", ["h256_gate_split"])
def test_rules_take_the_gate_event(cases, name):
    """patient_confident and patience_or_threshold: exits == tests/rule_ref.py on the reference score table (sign +1) and the dump's logits."""
    c = cases(name)
    d, g, thr, plain = c.dump()
    for e in range(c.E):                                             # under a rule documents stay longer: every score clear of its threshold
        G.assert_clear(g[e], thr[e], (name, e))
    table = np.concatenate([g, d["ac"][c.E:].astype(np.float64)], 0)
    al64, rows = d["al"].astype(np.float64), np.arange(c.B)
    seen = {tuple(plain.tolist())}
    for rule in (rule_ref.STREAK, rule_ref.EITHER):
        for t in (2, [e % 2 + 1 for e in range(c.E + 1)]):
            ex = rule_ref.rule_exits(table, al64, thr, t, rule, +1)
            o = c.fwd(thresholds=thr, temperatures=c.tm, exit_rule=rule_ref.RULE_NAMES[rule], patience=t, whole_layers=True)
            assert np.array_equal(_np(o.exit_layer), ex), (rule, t, _np(o.exit_layer).tolist(), ex.tolist())
            assert np.array_equal(_np(o.logits), d["al"][ex, rows]) and np.array_equal(_np(o.confidence), d["ac"][ex, rows])
            seen.add(tuple(ex.tolist()))
    o = c.fwd(thresholds=thr, temperatures=c.tm, exit_rule="plain", whole_layers=True)
    assert np.array_equal(_np(o.exit_layer), plain) and len(seen) >= 2
    c.eng.check()


@pytest.mark.parametrize("name", ["tiny_gate_fp32", "h256_gate_split"])
def test_captured_graph_and_result_stream_return_the_eager_bits(cases, name):
    """The criterion is bound at capture: replays equal the eager call, also after the handle's criterion has moved on.  forward_stream
    delivers every document once, at its exit, with the rows of the eager call."""
    c = cases(name)
    d, g, thr, ex = c.dump()
    want = {f: _np(getattr(c.fwd(thresholds=thr, temperatures=c.tm, whole_layers=True), f)) for f in FIELDS}
    assert np.array_equal(want["exit_layer"], ex)
    eng = c.engine(c.cfg)
    cap = eng.capture(**{k: v.clone() for k, v in c.inputs().items()}, thresholds=thr, temperatures=c.tm, whole_layers=True)
    for f in FIELDS:
        assert np.array_equal(_np(getattr(cap.outputs, f)), want[f]), f
    eng.set_criterion("max_confidence")
    keep_all = np.where(np.arange(c.E + 1) < c.E, 2.0, thr)           # no score is above 2: everybody reaches the end
    out = cap.launch(thresholds=keep_all, temperatures=c.tm)
    assert np.all(_np(out.exit_layer) == c.E)
    out = cap.launch(thresholds=thr, temperatures=c.tm)
    for f in FIELDS:
        assert np.array_equal(_np(getattr(out, f)), want[f]), f
    eng.check()
    cap.close()
    eng.set_criterion("gate")
    rs = eng.forward_stream(**c.inputs(), thresholds=thr, temperatures=c.tm, whole_layers=True)
    chunks = list(rs)
    assert [ch.exit_index for ch in chunks] == list(range(c.E + 1))
    docs = np.concatenate([ch.doc_index for ch in chunks])
    assert np.array_equal(np.sort(docs), np.arange(c.B))                # every document once
    for ch in chunks:
        assert np.all(ex[ch.doc_index] == ch.exit_index) and np.all(ch.exit_layer == ch.exit_index)
        assert np.array_equal(ch.logits, want["logits"][ch.doc_index]) and np.array_equal(ch.confidence, want["confidence"][ch.doc_index])
    for f in FIELDS:
        assert np.array_equal(_np(getattr(rs.output, f)), want[f]), f
    eng.check()
    eng.close()


def test_low_latency_keeps_the_exit_indices(cases):
    """MMEE_FLAG_LOW_LATENCY re-associates the residual GEMMs: the scores move by a measured amount, the thresholds are put into gaps at least
    ten times that wide, and the flagged forward then leaves every document where the plain one does."""
    c = cases("h256_gate_split")
    d, g, _, _ = c.dump()
    o = c.fwd(dump_all=True, want_head=True, whole_layers=True, low_latency=True)
    g_ll = G.gate_score(_np(o.head_logits))
    dev = float(np.abs(g_ll - g).max())
    report_measured("gate[low_latency]", "max |score(low latency) - score| and split-K parts", dev + 0.0)
    thr, ex = G.cascade_thresholds(g, min_gap=max(20.0 * dev, G.MIN_GAP))
    assert np.array_equal(G.gate_exits(np.concatenate([g_ll, np.ones((1, c.B))]), thr), ex)
    plain = c.fwd(thresholds=thr, whole_layers=True)
    ll = c.fwd(thresholds=thr, whole_layers=True, low_latency=True)
    assert np.array_equal(_np(plain.exit_layer), ex) and np.array_equal(_np(ll.exit_layer), ex)
    assert float(np.abs(_np(ll.logits).astype(np.float64) - _np(plain.logits)).max()) < 1e-4
    c.eng.check()


def test_table_scan_and_policy_reproduce_the_forwards_exits(cases, pkg):
    """forward -> sweep.gate_table -> policy.gate_scan_device gives the forward's out_exit exactly, and so does Policy.gate_policy; the table
    is the restatement's to 1e-12 relative and its last row is msp_table's."""
    c = cases("h256_gate_split")
    d, g, thr, ex = c.dump()
    o = c.fwd(dump_all=True, want_all=True, want_head=True, whole_layers=True)
    fw = c.fwd(thresholds=thr, whole_layers=True)
    table = pkg.sweep.gate_table(o.head_logits, o.all_logits[-1])
    ref = G.gate_table(_np(o.head_logits), _np(o.all_logits[-1]).astype(np.float64))
    rel = float(np.abs(_np(table) / ref - 1.0).max())
    report_measured("gate.table", "max relative |device - restatement|", rel)
    assert tuple(table.shape) == (c.E + 1, c.B) and rel <= 1e-12
    assert np.array_equal(_np(table)[c.E], _np(pkg.sweep.msp_table(o.all_logits)[0])[c.E])
    exits, pred, conf, counts = pkg.policy.gate_scan_device(table, o.all_logits, thr, want_conf=True)
    assert np.array_equal(_np(exits), _np(fw.exit_layer)) and np.array_equal(_np(exits), ex)
    assert np.array_equal(_np(pred).astype(np.float32), _np(fw.logits)) and np.array_equal(_np(conf).astype(np.float32), _np(fw.confidence))
    assert _np(counts).tolist() == np.bincount(ex, minlength=c.E + 1).tolist()
    es, pr, dist = pkg.Policy(_np(o.all_logits).astype(np.float64),
                              {"exit_policy": "gate_policy", "gate_scores": _np(table), "exit_thresholds": thr}).gate_policy()
    assert np.array_equal(es, ex) and es.dtype == np.int32 and abs(sum(dist.values()) - 1.0) < 1e-12
    assert np.array_equal(_np(pr), _np(pred))


def test_threshold_search_on_the_gate_table_names_thresholds_the_forward_honours(cases, pkg):
    """The front of threshold_search((gate table, correct)): its thresholds, fed back to engine.forward, give the front's mean exit."""
    c = cases("h256_gate_split")
    o = c.fwd(dump_all=True, want_all=True, want_head=True, whole_layers=True)
    refs = np.random.default_rng(3).integers(0, c.K, c.B)
    table = pkg.sweep.gate_table(o.head_logits, o.all_logits[-1])
    correct = pkg.sweep.msp_table(o.all_logits, refs)[1]
    res = pkg.sweep.threshold_search((table, correct), num_per_exit=4, mixtures="grid")
    F = len(res.front_mean_exit)
    assert F >= 1 and res.num_vectors == 4 ** c.E
    for i in sorted({0, F // 2, F - 1}):
        fw = c.fwd(thresholds=res.front_thresholds[i], whole_layers=True)
        got = _np(fw.exit_layer)
        assert int(got.sum()) == int(res.front_exit_sum[i]) and got.mean() == pytest.approx(res.front_mean_exit[i], abs=1e-12), (i, got.tolist())
        assert int(_np(correct)[got, np.arange(c.B)].sum()) == int(res.front_hits[i])
    c.eng.check()


def test_a_max_confidence_handle_is_unchanged_by_a_visit_to_the_gate_criterion(cases, pkg):
    """set_criterion("gate") -> set_criterion("max_confidence") on a gate handle: the bits and the launch count it had before.  Under the
    gate criterion the launches are those of a max_confidence forward that is asked for the head outputs: the gate heads, nothing else."""
    c = cases("h256_gate_split")
    eng = c.engine(c.twin_cfg)
    ac = _np(eng.forward(**c.inputs(), dump_all=True, want_all=True, whole_layers=True, temperatures=c.tm).all_crit).astype(np.float64)
    call = dict(thresholds=np.median(ac, axis=1), temperatures=c.tm, whole_layers=True)      # about half of those that reach an exit leave

    def run(**kw):
        eng.profile(True)
        o = eng.forward(**c.inputs(), **call, **kw)
        prof = eng.profile_read()
        eng.profile(False)
        return {f: _np(getattr(o, f)) for f in FIELDS}, sum(v["launches"] for v in prof.values())

    before, n_before = run()
    _, n_heads = run(want_head=True)
    assert eng.set_criterion("gate") is pkg.EarlyExitInference.GATE
    under, n_gate = run()
    eng.set_criterion("max_confidence")
    after, n_after = run()
    for f in FIELDS:
        assert np.array_equal(before[f], after[f]), f
    assert len(np.unique(before["exit_layer"])) >= 2
    assert n_before == n_after and n_gate == n_heads and n_gate > n_before, (n_before, n_heads, n_gate, n_after)
    report_measured("gate[launches]", "max_confidence forward / the same under the gate criterion", float(n_before) + float(n_gate) * 1e-3)
    eng.check()
    eng.close()


def test_refusals(cases, pkg):
    c = cases("tiny_gate_fp32")
    ramp = pkg.ModelConfig.tiny(EE_config=dict(exits=[1, 2], encoder_layer_strategy="ramp"))
    eng = pkg.EarlyExitEngine(ramp, max_docs=4, max_text_len=16)
    with pytest.raises(pkg.capi.MMEEError, match="MMEE_CRIT_GATE scores the 2-way heads"):
        eng.set_criterion("gate")
    assert str(eng.exit_config.inference_strategy) == "max_confidence"
    eng.close()
    lte = pkg.ModelConfig.tiny(EE_config=dict(exits=[1, 2], encoder_layer_strategy="gate", use_lte=True))
    eng = pkg.EarlyExitEngine(lte, max_docs=4, max_text_len=16)
    with pytest.raises(pkg.capi.MMEEError, match="use_lte handle"):
        eng.set_criterion("gate")
    eng.close()

    # ee_create itself: configurations the Python ExitConfig would never let through
    def doctored(base_ee, **over):
        class Doctored(type(ramp)):
            @property
            def exit_config(self):
                ec = pkg.ExitConfig(**self.EE_config)
                ec.inference_strategy = pkg.EarlyExitInference.GATE
                for k, v in over.items():
                    setattr(ec, k, v)
                return ec
        return Doctored(**{**ramp.__dict__, "EE_config": base_ee})

    with pytest.raises(pkg.capi.MMEEError, match="MMEE_CRIT_GATE needs MMEE_STRATEGY_GATE"):
        pkg.EarlyExitEngine(doctored(dict(exits=[1, 2], encoder_layer_strategy="ramp")), max_docs=4, max_text_len=16)
    with pytest.raises(pkg.capi.MMEEError, match="two exit decisions"):
        pkg.EarlyExitEngine(doctored(dict(exits=[1, 2], encoder_layer_strategy="gate"), use_lte=True), max_docs=4, max_text_len=16)
    with pytest.raises(ValueError, match="gate_scores"):
        pkg.Policy(np.zeros((2, 3, 4)), {"exit_threshold": 0.5}).gate_policy()
    with pytest.raises(ValueError):
        pkg.sweep.gate_table(np.zeros((2, 3, 3), np.float32), np.zeros((3, 4)))


def test_model_surface_under_the_gate_strategy(cases, pkg):
    """EE_config["inference_strategy"] = "gate" through the model: forward's exit_states[j][1] are the gate scores, exit_criterion is their
    torch expression, early_exit decides as the engine does; a model built under max_confidence follows a later write of the strategy."""
    c = cases("tiny_gate_fp32")
    d, g, thr, ex = c.dump()
    t = c.inputs()
    built = pkg.LayoutLMv3EEForSequenceClassification(c.cfg, weights=c.W, max_docs=c.B, max_text_len=c.T)
    late = pkg.LayoutLMv3EEForSequenceClassification(c.twin_cfg, weights=c.W, max_docs=c.B, max_text_len=c.T)
    late.config.exit_config["inference_strategy"] = "gate"
    want = c.fwd(thresholds=thr, whole_layers=True)
    plain = c.fwd(dump_all=True, want_all=True, want_head=True)     # model.forward's own call
    g_plain = G.gate_score(_np(plain.head_logits))
    for m in (built, late):
        out = m.forward(**t)
        assert str(m.engine.exit_config.inference_strategy) == "gate" and m.model_config.to_hf_dict()["EE_config"]["inference_strategy"] == "gate"
        for j in range(c.E):
            assert np.array_equal(_np(out.exit_states[j][0]), _np(plain.head_logits[j])) and np.array_equal(_np(out.exit_states[j][1]), _np(plain.head_crit[j]))
            mine = _np(m.exit_criterion(plain.head_logits[j])).astype(np.float64)
            assert float(np.abs(mine - g_plain[j]).max()) <= 2.0 ** -23
        got = m.early_exit(**t, thresholds=thr, whole_layers=True)
        for f in FIELDS:
            assert np.array_equal(_np(getattr(got, f)), _np(getattr(want, f))), f
    assert np.array_equal(_np(want.exit_layer), ex)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the tools on dumped arrays take the table unchanged
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_gate_table_goes_unchanged_into_the_sweeps_the_search_and_the_report(pkg):
    """ee_gate_table's rows plus msp_table's `correct` into threshold_sweep, rule_sweep, threshold_search, threshold_search(cost=) and
    exit_report(conf=, correct=), each against the numpy restatement fed with the SAME table (read back from the device); gate_scan_device and
    rule_scan_device against theirs.  N = 1025: more than one workgroup of every kernel."""
    store, refs = sweep_ref_inputs(seed=11, E1=5, N=1025, K=7)
    E1, N, K = store.shape
    rng = np.random.default_rng(12)
    head = (rng.standard_normal((E1 - 1, N, 2)) * 1.5).astype(np.float32)
    head[0, :3] = [[1.25, 1.25], [800.0, 0.0], [0.0, 800.0]]
    table_d = pkg.sweep.gate_table(head, store[-1])
    ref = G.gate_table(head, store[-1])
    table = _np(table_d)
    assert table[0, :3].tolist() == [0.5, 0.0, 1.0]
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(ref == 0.0, np.abs(table), np.abs(table / ref - 1.0))
    report_measured("gate.table[synthetic]", "max relative |device - restatement|", float(rel.max()))
    assert rel.max() <= 1e-12
    _, correct_d = pkg.sweep.msp_table(store, refs)
    correct = _np(correct_d)
    # the scan
    thr = np.array([G.midpoint_threshold(ref[e], 0.7)[0] for e in range(E1 - 1)] + [0.5])
    for e in range(E1 - 1):
        G.assert_clear(ref[e], thr[e], e)
    ex, pred, conf, counts = G.gate_scan(table, store, thr)
    assert np.array_equal(ex, G.gate_exits(ref, thr)) and len(np.unique(ex)) == E1
    d_ex, d_pred, d_conf, d_counts = pkg.policy.gate_scan_device(table_d, store, thr, want_conf=True)
    assert np.array_equal(_np(d_ex), ex) and np.array_equal(_np(d_pred), pred) and np.array_equal(_np(d_conf), conf) and np.array_equal(_np(d_counts), counts)
    # the rules on the table (sign +1)
    for rule in (rule_ref.STREAK, rule_ref.EITHER):
        want = rule_ref.rule_policy(table, store, thr, 2, rule, +1)
        got = pkg.rule_scan_device(table_d, store, thr, 2, rule_ref.RULE_NAMES[rule], sign=1.0, want_conf=True)
        assert np.array_equal(_np(got[0]), want[0]) and np.array_equal(_np(got[2]), want[2])
    # the sweeps
    V = 33
    thr_v = np.stack([np.concatenate([[np.quantile(table[e], rng.random()) for e in range(E1 - 1)], [0.0]]) for _ in range(V)])
    acc, mex, hist = pkg.sweep.threshold_sweep(table_d, correct_d, thr_v, want_hist=True)
    hits, sums, hh = csf_ref.threshold_sweep(table, correct, thr_v)
    assert np.array_equal(np.rint(_np(acc) * N).astype(np.int64), hits) and np.array_equal(np.rint(_np(mex) * N).astype(np.int64), sums)
    assert np.array_equal(_np(hist), hh)
    pats = [1, 2, 3]
    r_acc, r_mex, _ = pkg.sweep.rule_sweep(table_d, store, refs, thr_v[:9], pats, "patient_confident", sign=1.0)
    w_hits, w_sums, _ = rule_ref.rule_sweep(table, store, refs, thr_v[:9], pats, rule_ref.STREAK, +1)
    assert np.array_equal(np.rint(_np(r_acc) * N).astype(np.int64), w_hits) and np.array_equal(np.rint(_np(r_mex) * N).astype(np.int64), w_sums)
    # the search, and the cost-weighted search
    res = pkg.sweep.threshold_search((table_d, correct_d), num_per_exit=5, mixtures=200, seed=7)
    assert len(res.front_hits) >= 1
    for i in range(len(res.front_hits)):
        e_i = G.gate_exits(table, res.front_thresholds[i])
        assert int(e_i.sum()) == int(res.front_exit_sum[i]) and int(correct[e_i, np.arange(N)].sum()) == int(res.front_hits[i])
    cost = (np.arange(1, E1 + 1) * 10).astype(np.int64)
    resc = pkg.sweep.threshold_search((table_d, correct_d), num_per_exit=5, mixtures=200, seed=7, cost=cost)
    for i in range(len(resc.front_hits)):
        e_i = G.gate_exits(table, resc.front_thresholds[i])
        assert int(cost[e_i].sum()) == int(resc.front_cost_sum[i]) and int(correct[e_i, np.arange(N)].sum()) == int(resc.front_hits[i])
    # the report
    rep = pkg.exit_report((table_d, correct_d), exits=ex)
    assert rep.policy == E1 and rep.accuracy[E1] == pytest.approx(correct[ex, np.arange(N)].mean(), abs=1e-15)
    assert np.array_equal(rep.exit_hist, counts) and rep.average_confidence[E1] == pytest.approx(table[ex, np.arange(N)].mean(), rel=1e-12)
