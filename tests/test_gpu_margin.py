"""The margin criterion (include/mmee.h MMEE_CRIT_MARGIN: top-1 minus top-2 softmax probability) and the device criterion tables on the
MI355X: the criterion and the decision inside the forward pass against the numpy restatement of tests/csf_ref.py applied to the path's own
dump-all rows, the combined rules, the captured-graph form, the low-latency flag, the launch count against the max-confidence twin, and the
table / scan / Policy / sweep entry points on dumped arrays.  The reference's own margin function is wrong and never called, so the
restatement is the oracle."""
import types

import numpy as np
import pytest

from . import csf_ref
from .conftest import DIT_EE, H256_KW, report_measured, sweep_ref_inputs
from .rule_ref import EITHER, RULE_NAMES, STREAK, rule_exits, rule_policy

pytestmark = pytest.mark.gpu

# name -> (shape, EE_config, K, per-exit temperatures, documents, text length): the cases of tests/test_gpu_lte.py (tiny f32 MFMA, H256 the
# smallest split-capable shape, base), a K = 2 case (the second largest label is the only other one), and the image-only tiny DiT.
CASES = {
    "tiny_ramp_2layer_emb_k16": ("tiny", dict(exits=["vision_avg", "text_avg", 1, 2, 3, 4], encoder_layer_strategy="ramp"), 16, False, 40, 16),
    "h256_gate_1layer_emb_k10_temps": ("h256", dict(exits=["text_visual_concat", 1, 2, 3], encoder_layer_strategy="gate", exit_head_num_layers=1),
                                       10, True, 40, 48),
    "h256_ramp_k2": ("h256", dict(exits=[1, 2, 3], encoder_layer_strategy="ramp"), 2, False, 40, 48),
    "base_ramp_2layer_k16": ("base", dict(exits=[2, 4, 6, 8, 10], encoder_layer_strategy="ramp"), 16, False, 32, 128),
    "dit_tiny": ("dit", dict(DIT_EE), 16, False, 40, 0),
}
LAYOUTLM = [n for n in CASES if n != "dit_tiny"]
POSITION = 0.65      # thresholds sit near the position 0.65 N of the sorted margins: about a third of the documents clear each exit's test
MIN_GAP = 1e-5       # >> 2^-23, the rounding of a stored float32 criterion <= 1
FIELDS = ("logits", "exit_layer", "confidence")
VECTOR = lambda E1: [e % 3 + 1 for e in range(E1)]


def _np(t):
    return t.detach().cpu().numpy()


class Case:
    """One shape: its margin configuration and the max-confidence twin, weights, documents, temperatures, ONE margin engine (the default
    schedule; the tests pass whole_layers / probe_always / xprobe per call) and its dump-all rows, computed once and shared."""

    def __init__(self, pkg, name):
        import torch
        shape, ee, K, temps, B, T = CASES[name]
        self.pkg, self.name, self.B, self.T, self.dit = pkg, name, B, T, shape == "dit"
        mk = {"tiny": lambda **kw: pkg.ModelConfig.tiny(**kw), "h256": lambda **kw: pkg.ModelConfig.tiny(**kw, **H256_KW),
              "base": lambda **kw: pkg.ModelConfig.base(**kw), "dit": lambda **kw: pkg.ModelConfig.dit_tiny(**kw)}[shape]
        self.cfg = mk(EE_config=dict(ee, inference_strategy="margin"), num_labels=K)
        self.twin = mk(EE_config=dict(ee, inference_strategy="max_confidence"), num_labels=K)
        if self.dit:
            self.W = pkg.synth.make_weights_beit(self.cfg, seed=90 + K, head_gain=4.0)
            self.docs = {"pixel_values": pkg.synth.make_documents(self.cfg, B, seed=91 + K, text_len=8)["pixel_values"]}
        else:
            self.W = pkg.synth.make_weights(self.cfg, seed=90 + K, head_gain=4.0)
            d = pkg.synth.make_documents(self.cfg, B, seed=91 + K, text_len=T, min_words=2)
            self.docs = {k: d[k] for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}
        self.E = self.cfg.exit_config.num_exits
        self.tm = np.random.default_rng(K).uniform(0.5, 3.0, self.E + 1) if temps else None
        self.dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in self.docs.items()}
        self.eng = self.engine(self.cfg)
        self._dump = None

    def engine(self, cfg, **kw):
        size = dict(max_docs=self.B) if self.dit else dict(max_docs=self.B, max_text_len=self.T)
        eng = self.pkg.EarlyExitEngine(cfg, **size, **kw)
        eng.load_weights(self.W)
        return eng

    def inputs(self, sl=slice(None)):
        return {k: v[sl].contiguous() for k, v in self.dev.items()}

    def fwd(self, eng=None, sl=slice(None), **kw):
        return (eng or self.eng).forward(**self.inputs(sl), **kw)

    def dump(self):
        """Dump-all with whole layers: al / ac (the scaled logits and margins), hl / hc (the heads' own), hidden, z (the logits of a dump
        WITHOUT temperatures: all_logits of a scaled dump are already rounded) and want = the float64 restatement on (double)z / T."""
        if self._dump is None:
            kw = dict(dump_all=True, want_all=True, want_head=True, want_hidden_cls=True, whole_layers=True)
            o = self.fwd(temperatures=self.tm, **kw)
            z = _np(o.all_logits) if self.tm is None else _np(self.fwd(dump_all=True, want_all=True, whole_layers=True).all_logits)
            self.eng.check()
            self._dump = types.SimpleNamespace(al=_np(o.all_logits), ac=_np(o.all_crit), hl=_np(o.head_logits), hc=_np(o.head_crit),
                                               hidden=_np(o.hidden_cls), logits=_np(o.logits), z=z,
                                               want=csf_ref.margin(csf_ref.scaled(z, self.tm)))
        return self._dump

    def thresholds(self, min_gap=MIN_GAP):
        """Per-exit thresholds at gap midpoints of the sorted restatement margins, and the exits the restatement gives on the dump's own
        all_crit.  Guards (failing, not skipping): every gap wide enough, at least three distinct exits, the final exit among them."""
        d = self.dump()
        thr, width = csf_ref.gap_thresholds(d.want, POSITION, min_gap)
        assert np.all(width >= min_gap), (self.name, width.tolist())
        ex = csf_ref.exits(d.ac.astype(np.float64), thr, +1)
        assert np.array_equal(ex, csf_ref.exits(d.want, thr, +1)), self.name       # the float32 rounding moved nobody across a threshold
        spread = np.bincount(ex, minlength=self.E + 1).tolist()
        assert len(np.unique(ex)) >= 3 and self.E in ex, (self.name, spread)
        return thr, ex


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


# ---- 1. criterion values, the twin's bits, launch counts ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_margins_equal_the_restatement_and_the_other_outputs_are_the_twins(cases, name):
    """Dump-all, whole layers.  all_crit == float32(csf_ref.margin((double)z / T)) within 2^-23: one float32 rounding of a value <= 1, plus
    float64 order effects << 1e-12.  head_crit (the float32 form on the head's own logits) within 5e-6 of the float64 restatement on
    head_logits: two float32 softmax terms of <= K 2^-24 each at K = 16.  Every logits output is bit-identical to the same call on a
    max-confidence handle, and so is the number of launches (dump-all; thresholded under the default schedule and under whole layers)."""
    c = cases(name)
    d = c.dump()
    assert d.ac.dtype == np.float32 and d.ac.shape == (c.E + 1, c.B) and np.isfinite(d.ac).all()
    err = float(np.abs(d.ac.astype(np.float64) - d.want.astype(np.float32).astype(np.float64)).max())
    report_measured(f"margin[{name}]", "max |all_crit - float32(restatement)|", err)
    assert err <= 2.0 ** -23
    assert np.all(d.ac >= 0.0) and np.all(d.ac <= 1.0) and float(d.want.std()) > 1e-3
    herr = float(np.abs(d.hc.astype(np.float64) - csf_ref.margin(d.hl.astype(np.float64))).max())
    report_measured(f"margin[{name}]", "max |head_crit - float64 restatement on head_logits|", herr)
    assert herr <= 5e-6
    assert np.array_equal(_np(c.fwd(dump_all=True, want_all=True, whole_layers=True, temperatures=c.tm).confidence), d.ac[c.E])
    twin = c.engine(c.twin)
    kw = dict(dump_all=True, want_all=True, want_head=True, want_hidden_cls=True, whole_layers=True, temperatures=c.tm)
    t = twin.forward(**c.inputs(), **kw)
    for f, mine in (("logits", d.logits), ("all_logits", d.al), ("head_logits", d.hl), ("hidden_cls", d.hidden)):
        assert np.array_equal(_np(getattr(t, f)), mine), (name, f)
    assert not np.array_equal(_np(t.all_crit), d.ac)
    counts = {}
    for tag, eng in (("margin", c.eng), ("twin", twin)):
        for sched, call in (("dump", kw), ("default", dict(thresholds=2.0, temperatures=c.tm)),
                            ("whole", dict(thresholds=2.0, temperatures=c.tm, whole_layers=True))):
            eng.profile(True)
            eng.forward(**c.inputs(), **call)
            prof = eng.profile_read()
            eng.profile(False)
            counts[tag, sched] = sum(v["launches"] for v in prof.values())
            assert prof["exit_decide"]["launches"] == c.E + 1
        eng.check()
    twin.close()
    for sched in ("dump", "default", "whole"):
        report_measured(f"margin[{name},{sched}]", "profiled launches (margin = twin)", float(counts["margin", sched]))
        assert 0 < counts["margin", sched] == counts["twin", sched], (sched, counts)


# ---- 2. exits ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LAYOUTLM)
def test_exits_equal_the_restatement_on_the_dump_all_margins(cases, name):
    """Whole layers and the K | V probe (probe_always, xprobe=False): exit_layer == the restatement on the dump's own all_crit, logits and
    confidence bit-identical to the dump rows at that exit, stage populations are the survivors, a permuted batch gives permuted outputs
    bit for bit.  The tiny case repeats it with dense rows."""
    c = cases(name)
    d = c.dump()
    thr, ex = c.thresholds()
    report_measured(f"margin[{name}]", "distinct exits documents leave at", float(len(np.unique(ex))))
    rows = np.arange(c.B)
    perm = np.random.default_rng(5).permutation(c.B)
    for dense in (False, True) if name.startswith("tiny") else (False,):
        if dense:                                               # the dense layout's own dump, thresholds in ITS gaps (no temperatures here)
            assert c.tm is None
            o = c.fwd(dump_all=True, want_all=True, whole_layers=True, dense_rows=True)
            al, ac = _np(o.all_logits), _np(o.all_crit)
            thr, width = csf_ref.gap_thresholds(csf_ref.margin(csf_ref.scaled(al)), POSITION, MIN_GAP)
            assert np.all(width >= MIN_GAP)
            ex_d = csf_ref.exits(ac.astype(np.float64), thr, +1)
            assert len(np.unique(ex_d)) >= 3 and c.E in ex_d
        else:
            al, ac, ex_d = d.al, d.ac, ex
        for sched in (dict(whole_layers=True), dict(probe_always=True, xprobe=False)):
            tag = (name, dense, tuple(sched))
            o = c.fwd(thresholds=thr, temperatures=c.tm, dense_rows=dense, **sched)
            assert np.array_equal(_np(o.exit_layer), ex_d), (tag, _np(o.exit_layer).tolist(), ex_d.tolist())
            assert np.array_equal(_np(o.logits), al[ex_d, rows]), tag
            assert np.array_equal(_np(o.confidence), ac[ex_d, rows]), tag
            assert c.eng.stage_counts()["docs"] == [int((ex_d >= e).sum()) for e in range(c.E + 1)], tag
            p = c.fwd(sl=perm, thresholds=thr, temperatures=c.tm, dense_rows=dense, **sched)
            for f in FIELDS:
                assert np.array_equal(_np(getattr(p, f)), _np(getattr(o, f))[perm]), (tag, f)
    c.eng.check()


@pytest.mark.parametrize("name", list(CASES))
def test_thresholds_of_one_keep_everybody_and_of_minus_one_release_everybody(cases, name):
    """A margin is never above 1 and never below 0: thresholds = 1.0 keep every document to the final exit, thresholds = -1.0 release every
    document at exit 0; the rows are the dump's."""
    c = cases(name)
    d = c.dump()
    o = c.fwd(thresholds=1.0, temperatures=c.tm, whole_layers=True)
    assert np.all(_np(o.exit_layer) == c.E) and np.array_equal(_np(o.logits), d.al[c.E]) and np.array_equal(_np(o.confidence), d.ac[c.E])
    o = c.fwd(thresholds=-1.0, temperatures=c.tm, whole_layers=True)
    assert np.all(_np(o.exit_layer) == 0) and np.array_equal(_np(o.logits), d.al[0]) and np.array_equal(_np(o.confidence), d.ac[0])
    assert c.eng.stage_counts()["docs"] == [c.B] + [0] * c.E
    c.eng.check()


# ---- 3. the default engine (X-space probe) at the base shape ---------------------------------------------------------------------------------
def test_x_space_probe_gives_the_same_exits_at_the_base_shape(cases):
    """The default schedule on split precision probes in X space, a re-association of the whole-layer arithmetic: its margins are measured
    against whole layers on the same handle first, the thresholds are then put into gaps at least 10 x that wide (they must exist).  Exits
    equal the restatement, logits within 1e-4 of the dump rows, every document compared."""
    name = "base_ramp_2layer_k16"
    c = cases(name)
    d = c.dump()
    assert c.eng.precision == "split" and c.eng.xprobe_default
    # thresholds of 1 release nobody: every exit is evaluated for every document under either schedule
    s_whole = _np(c.fwd(thresholds=1.0, want_all=True, whole_layers=True).all_crit).astype(np.float64)
    s_x = _np(c.fwd(thresholds=1.0, want_all=True).all_crit).astype(np.float64)
    assert any(c.eng.layer_plan()["docs_probe"]), "no layer was probed: the default schedule did not run"
    assert np.array_equal(s_whole, d.ac.astype(np.float64))
    dev = float(np.abs(s_x - s_whole).max())
    report_measured(f"margin[{name}]", "max |margin(X-space probe) - margin(whole layers)|", dev)
    thr, width = csf_ref.gap_thresholds(d.want, POSITION, max(10.0 * dev, MIN_GAP))
    assert np.all(width >= 10.0 * dev) and np.all(width >= MIN_GAP)
    ex = csf_ref.exits(s_whole, thr, +1)
    assert len(np.unique(ex)) >= 3 and c.E in ex, np.bincount(ex, minlength=c.E + 1).tolist()
    o = c.fwd(thresholds=thr)
    c.eng.check()
    assert any(c.eng.layer_plan()["docs_probe"])
    assert np.array_equal(_np(o.exit_layer), ex)
    err = float(np.abs(_np(o.logits).astype(np.float64) - d.al[ex, np.arange(c.B)]).max())
    report_measured(f"margin[{name}]", "max |dlogit| X-space probe vs dump-all", err)
    assert err < 1e-4
    assert c.eng.stage_counts()["docs"] == [int((ex >= e).sum()) for e in range(c.E + 1)]


# ---- 4. rules ------------------------------------------------------------------------------------------------------------------------------------
def test_rules_take_the_margin_test_as_their_event(cases):
    """patient_confident and patience_or_threshold with patience 2 and a per-exit vector: exits == tests/rule_ref.py on the margin table
    with sign +1 and the dump's logits (the agreement counter reads them), outputs are the dump rows."""
    c = cases("h256_gate_1layer_emb_k10_temps")
    d = c.dump()
    thr, plain = c.thresholds()
    ac64, al64, rows = d.ac.astype(np.float64), d.al.astype(np.float64), np.arange(c.B)
    seen = {tuple(plain.tolist())}
    for rule in (STREAK, EITHER):
        for t in (2, VECTOR(c.E + 1)):
            ex = rule_exits(ac64, al64, thr, t, rule, +1)
            for sched in (dict(whole_layers=True), dict(probe_always=True, xprobe=False)):
                o = c.fwd(thresholds=thr, temperatures=c.tm, exit_rule=RULE_NAMES[rule], patience=t, **sched)
                tag = (rule, t, tuple(sched))
                assert np.array_equal(_np(o.exit_layer), ex), (tag, _np(o.exit_layer).tolist(), ex.tolist())
                assert np.array_equal(_np(o.logits), d.al[ex, rows]) and np.array_equal(_np(o.confidence), d.ac[ex, rows]), tag
            seen.add(tuple(ex.tolist()))
    o = c.fwd(thresholds=thr, temperatures=c.tm, exit_rule="plain", whole_layers=True)
    assert np.array_equal(_np(o.exit_layer), plain)
    assert len(seen) >= 3                                       # the rules change who leaves where
    c.eng.check()


# ---- 5. captured graph ----------------------------------------------------------------------------------------------------------------------------
def test_captured_graph_replays_return_the_eager_bits(cases):
    """The criterion is bound at capture, thresholds come from the device vector of each launch: replays with two different threshold vectors
    equal eager forwards with those vectors, bit for bit."""
    c = cases("h256_ramp_k2")
    thr_a, ex_a = c.thresholds()
    thr_b = np.where(np.arange(c.E + 1) % 2 == 0, 1.0, thr_a)    # even exits release nobody
    eng = c.engine(c.cfg)
    cap = eng.capture(**{k: v.clone() for k, v in c.inputs().items()}, thresholds=thr_a)
    e0 = c.fwd(thresholds=thr_a)
    for f in FIELDS:
        assert np.array_equal(_np(getattr(cap.outputs, f)), _np(getattr(e0, f))), f
    eng.set_criterion("max_confidence")                          # the capture keeps ITS criterion
    seen = []
    for thr in (thr_b, thr_a, thr_b):
        out = cap.launch(thresholds=thr)
        want = c.fwd(thresholds=thr)
        for f in FIELDS:
            assert np.array_equal(_np(getattr(out, f)), _np(getattr(want, f))), f
        seen.append(_np(out.exit_layer).copy())
    assert np.array_equal(seen[1], ex_a) and not np.array_equal(seen[0], seen[1])
    eng.check()
    cap.close()
    eng.close()


# ---- 6. low-latency flag ------------------------------------------------------------------------------------------------------------------------
def test_low_latency_forward_decides_on_its_own_margins(cases):
    """MMEE_FLAG_LOW_LATENCY needs nothing of its own: exits == the restatement on the flagged dump's all_crit, rows those of that dump."""
    c = cases("h256_gate_1layer_emb_k10_temps")
    eng = c.engine(c.cfg, precision="split", xprobe=False)
    o = eng.forward(**c.inputs(), dump_all=True, want_all=True, whole_layers=True, temperatures=c.tm, low_latency=True)
    al, ac = _np(o.all_logits), _np(o.all_crit)
    report_measured("margin[low_latency]", "split-K parts (attention-output, FFN-down)", float(sum(eng.last_k_splits())))
    thr, width = csf_ref.gap_thresholds(ac.astype(np.float64), POSITION, MIN_GAP)
    assert np.all(width >= MIN_GAP)
    ex = csf_ref.exits(ac.astype(np.float64), thr, +1)
    assert len(np.unique(ex)) >= 3 and c.E in ex
    o = eng.forward(**c.inputs(), thresholds=thr, temperatures=c.tm, whole_layers=True, low_latency=True)
    assert np.array_equal(_np(o.exit_layer), ex)
    assert np.array_equal(_np(o.logits), al[ex, np.arange(c.B)]) and np.array_equal(_np(o.confidence), ac[ex, np.arange(c.B)])
    eng.check()
    eng.close()


# ---- the model surface ------------------------------------------------------------------------------------------------------------------------------
def test_model_forward_and_early_exit_under_the_margin_strategy(cases, pkg):
    """EE_config["inference_strategy"] = "margin" through the model: forward fills exit_states[j][1] and exit_criteria from the handle,
    exit_criterion is the float32 torch expression, early_exit decides as the engine does; a model built under max_confidence follows a
    later write of config.exit_config["inference_strategy"]; MicroBatchedEngine.set_criterion reaches every slice."""
    c = cases("tiny_ramp_2layer_emb_k16")
    n, sl = 12, slice(0, 12)
    t = c.inputs(sl)
    dump = c.fwd(sl=sl, dump_all=True, want_all=True, want_head=True)
    hc, ac, hl = _np(dump.head_crit), _np(dump.all_crit), dump.head_logits
    thr, _ = csf_ref.gap_thresholds(ac.astype(np.float64), 0.5, MIN_GAP)
    want = c.fwd(sl=sl, thresholds=thr, whole_layers=True)
    assert len(np.unique(_np(want.exit_layer))) >= 2
    built = pkg.LayoutLMv3EEForSequenceClassification(c.cfg, weights=c.W, max_docs=n, max_text_len=c.T)
    late = pkg.LayoutLMv3EEForSequenceClassification(c.twin, weights=c.W, max_docs=n, max_text_len=c.T)
    late.config.exit_config["inference_strategy"] = "margin"      # the reference's driver writes it after construction (EE/utils.py:62-78)
    for m in (built, late):
        out = m.forward(**t)
        assert str(m.engine.exit_config.inference_strategy) == "margin" and m.model_config.to_hf_dict()["EE_config"]["inference_strategy"] == "margin"
        assert len(out.exit_states) == c.E and len(out.exit_criteria) == 1 and np.array_equal(_np(out.exit_criteria[0]), ac[c.E])
        for j in range(c.E):
            assert np.array_equal(_np(out.exit_states[j][0]), _np(hl[j])) and np.array_equal(_np(out.exit_states[j][1]), hc[j])
            mine = _np(m.exit_criterion(hl[j])).astype(np.float64)
            assert float(np.abs(mine - csf_ref.margin(_np(hl[j]).astype(np.float64))).max()) <= 5e-6
        got = m.early_exit(**t, thresholds=thr)                    # B <= 16 runs whole layers
        for f in FIELDS:
            assert np.array_equal(_np(getattr(got, f)), _np(getattr(want, f))), f
        m.engine.close()
    two = pkg.MicroBatchedEngine(c.twin, max_docs=n, max_text_len=c.T, micro_batches=2)
    two.load_weights(c.W)
    assert str(two.set_criterion("margin")) == "margin"
    got = two.forward(**t, thresholds=thr, whole_layers=True)
    for f in FIELDS:
        assert np.array_equal(_np(getattr(got, f)), _np(getattr(want, f))), f
    two.check()
    two.close()
    # the refusal of unknown codes stays
    assert c.eng.lib.ee_set_criterion(c.eng._h, 4) != 0 and "unknown criterion" in pkg.capi.last_error(c.eng._h)
    assert str(c.eng.exit_config.inference_strategy) == "margin"


# ---- 7. dumped arrays ------------------------------------------------------------------------------------------------------------------------------
STORES = ["sweep_ref", (5, 1000, 1), (5, 1000, 2), (3, 257, 3), (4, 1500, 64)]
_store_cache = {}


def _store(which):
    """(logits (E1,N,K) float64, references (N,), mask (E1,N) of planted exact ties): the sweep fixture's inputs, or random logits; a tenth of
    the rows copy their maximum to another label (K > 1), so their margin is exactly 0."""
    key = str(which)
    if key not in _store_cache:
        if which == "sweep_ref":
            s, refs = sweep_ref_inputs()
            s = s.copy()
            rng = np.random.default_rng(7)
        else:
            E1, N, K = which
            rng = np.random.default_rng(E1 * 1000 + K)
            s = rng.standard_normal((E1, N, K)) * rng.uniform(0.5, 4.0, (E1, 1, 1))
            refs = rng.integers(0, K, N).astype(np.int64)
        E1, N, K = s.shape
        tie = (rng.random((E1, N)) < 0.1) & (K > 1)
        am = s.argmax(-1)
        other = (am + 1 + rng.integers(0, max(K - 1, 1), (E1, N))) % K
        ee, nn = np.nonzero(tie)
        s[ee, nn, other[ee, nn]] = s[ee, nn, am[ee, nn]]
        _store_cache[key] = (s, refs, tie, {cr: csf_ref.csf(s, cr) for cr in csf_ref.CRITERIA})
    return _store_cache[key]


def _table_tolerance(criterion, store):
    """margin: absolute 1e-13 (a difference of two probabilities: cancellation makes a relative bound meaningless); entropy: 1e-12 per unit
    of the largest |logit| (B / A is of that size); max-softmax: compared with msp_table bit for bit instead."""
    return 1e-13 if criterion == "margin" else 1e-12 * max(1.0, float(np.abs(store).max()))


def _scan_thresholds(table, sign, K):
    """Per-exit quantiles (the surest ~30 % clear each test), moved to the nearest gap midpoint; a single label has one criterion value."""
    if K == 1:
        return np.full(table.shape[0], 0.5)
    thr, width = csf_ref.gap_thresholds(table, 0.7 if sign > 0 else 0.3, 1e-9)
    assert np.all(width >= 1e-9)
    return thr


@pytest.mark.parametrize("which", STORES, ids=str)
def test_csf_table_vs_restatement(pkg, which):
    store, refs, tie, ref = _store(which)
    E1, N, K = store.shape
    correct = (store.argmax(-1) == refs[None, :]).astype(np.uint8)
    msp, msp_correct = pkg.sweep.msp_table(store, refs)
    for cr in csf_ref.CRITERIA:
        table, corr = pkg.sweep.csf_table(store, refs, criterion=cr)
        table = _np(table)
        assert table.dtype == np.float64 and table.shape == (E1, N) and np.array_equal(_np(corr), correct), cr
        if cr == "max_confidence":
            assert np.array_equal(table, _np(msp)) and np.array_equal(_np(corr), _np(msp_correct))
            np.testing.assert_allclose(table, ref[cr], rtol=1e-14, atol=0)
        else:
            err = float(np.abs(table - ref[cr]).max())
            report_measured(f"csf_table[{which},{cr}]", "max |table - restatement|", err)
            assert err <= _table_tolerance(cr, store), (cr, err)
        if cr == "margin":
            assert np.all(table >= 0.0) and np.all(table[tie] == 0.0) and (K == 1 or int(tie.sum()) > 0)
            if K == 1:
                assert np.all(table == 1.0)
        as_csf, none = pkg.sweep.csf_table(store, criterion=cr, as_csf=True)
        assert none is None and np.array_equal(_np(as_csf), -table if cr == "entropy" else table), cr


@pytest.mark.parametrize("which", STORES, ids=str)
def test_criterion_scan_and_policies_vs_restatement(pkg, which):
    import torch
    store, refs, tie, ref = _store(which)
    E1, N, K = store.shape
    dev = torch.from_numpy(store).cuda()
    for cr in csf_ref.CRITERIA:
        sign = csf_ref.SIGN[cr]
        thr = _scan_thresholds(ref[cr], sign, K)
        ex, pred, conf, counts = csf_ref.scan(store, thr, cr)
        if K > 1:
            assert len(np.unique(ex)) >= 2, (cr, counts.tolist())
        g_ex, g_pred, g_conf, g_counts = pkg.criterion_scan_device(dev, thr, cr, want_conf=True)
        assert np.array_equal(_np(g_ex), ex), (cr, int((_np(g_ex) != ex).sum()))
        assert np.array_equal(_np(g_pred), pred) and np.array_equal(_np(g_counts), counts), cr
        np.testing.assert_allclose(_np(g_conf), conf, rtol=1e-14 if cr == "max_confidence" else 0,
                                   atol=0 if cr == "max_confidence" else _table_tolerance(cr, store))
        if cr == "max_confidence":
            for a, b in zip(pkg.policy_scan_device(dev, thr, want_conf=True), (g_ex, g_pred, g_conf, g_counts)):
                assert np.array_equal(_np(a), _np(b))
        else:
            name = f"{cr}_global_thresholding_policy"
            for conf_keys, t in (({"exit_thresholds": thr}, thr), ({"exit_threshold": float(thr[0])}, float(thr[0]))):
                want = csf_ref.scan(store, t, cr)
                cfg = dict(conf_keys, exit_policy=name)
                exits_store, predictions, dist = getattr(pkg.Policy(logits=store, config=cfg), cfg["exit_policy"])()
                assert exits_store.dtype == np.int32 and np.array_equal(exits_store, want[0]), (name, sorted(cfg))
                assert predictions.dtype == torch.float64 and np.array_equal(_np(predictions), want[1])
                assert dist == {e: int(want[3][e]) / N for e in range(E1)}
        # the rule policies read config["criterion"]: table and sign from csf_table
        for rule in (STREAK, EITHER):
            name = RULE_NAMES[rule] + "_policy"
            cfg = {"exit_policy": name, "exit_thresholds": thr, "patience": 2, "criterion": cr}
            exits_store, predictions, dist = getattr(pkg.Policy(logits=store, config=cfg), cfg["exit_policy"])()
            r_ex, r_pred, _, r_counts = rule_policy(ref[cr], store, thr, 2, rule, sign)
            assert np.array_equal(exits_store, r_ex) and np.array_equal(_np(predictions), r_pred), (name, cr)
            assert dist == {e: int(r_counts[e]) / N for e in range(E1)}
            if cr == "max_confidence":                             # without the key nothing changes
                del cfg["criterion"]
                again = getattr(pkg.Policy(logits=store, config=cfg), cfg["exit_policy"])()
                assert np.array_equal(again[0], exits_store) and np.array_equal(_np(again[1]), _np(predictions))


@pytest.mark.parametrize("which", ["sweep_ref", (4, 1500, 64)], ids=str)
def test_threshold_sweep_takes_the_margin_table_directly(pkg, which):
    """threshold_sweep on csf_table(..., "margin", as_csf=True) == the numpy '>='-argmax restatement, exactly: 300 threshold vectors drawn
    from per-exit percentiles of the table (entries that ARE table values among them), both kernels behind ee_threshold_sweep (the direct
    one with the histogram, the ranked one without).  The restatement reads the device table, whose values test_csf_table_vs_restatement
    checks: a percentile may land on a table value, where '>=' must see the same double on both sides."""
    store, refs, tie, ref = _store(which)
    E1, N, K = store.shape
    V = 300
    table, corr = pkg.sweep.csf_table(store, refs, criterion="margin", as_csf=True)
    t, cor = _np(table), _np(corr)
    rng = np.random.default_rng(N)
    q = rng.uniform(30.0, 100.0, (V, E1))
    thr = np.stack([np.percentile(t[e], q[:, e]) for e in range(E1)], axis=1)
    pick = t[np.arange(E1)[None, :], rng.integers(0, N, (V, E1))]
    thr = np.where(rng.random((V, E1)) < 0.2, pick, thr)
    assert V * 8 >= N and int((t[None] == thr[:, :, None]).sum()) > 0
    hits, sums, hist = csf_ref.threshold_sweep(t, cor, thr)
    assert int((hist.sum(0) > 0).sum()) >= 3                       # the vectors spread the documents over several exits
    g_acc, g_mex, g_hist = pkg.sweep.threshold_sweep(table, corr, thr, want_hist=True)
    assert np.array_equal(_np(g_hist), hist) and np.array_equal(_np(g_acc), hits / N) and np.array_equal(_np(g_mex), sums / N)
    r_acc, r_mex, none = pkg.sweep.threshold_sweep(table, corr, thr)
    assert none is None and np.array_equal(_np(r_acc), hits / N) and np.array_equal(_np(r_mex), sums / N)
    # rule_sweep takes the same table with sign +1
    a, m, _ = pkg.sweep.rule_sweep(table, store, refs, thr[:20], [1], "patient_confident")
    for v in range(20):
        ex = csf_ref.exits(t, thr[v], +1)                          # STREAK at t = 1 is the plain strict policy
        assert float(_np(a)[v, 0]) == int(cor[ex, np.arange(N)].sum()) / N and float(_np(m)[v, 0]) == int(ex.sum()) / N
