"""The result stream (include/mmee.h MMEE_FLAG_STREAM_RESULTS / ee_stream_next) on the MI355X: every exit's chunk against the numpy
restatement of tests/stream_ref.py applied to the forward's own exit_layer, every row against the bits of the forward's own outputs, every
output against the same call without the flag, the emit kernel's wave / loop boundaries, the degenerate populations, the decision modes and
schedules it must not depend on, the overlap rule, the launch count and the refusals.  No test asserts a time."""
import numpy as np
import pytest

from . import csf_ref, lte_ref, stream_ref
from .conftest import DIT_EE, H256_KW, report_measured

pytestmark = pytest.mark.gpu

TINY_EMB = dict(exits=["vision_avg", "text_avg", 1, 2, 3, 4], encoder_layer_strategy="ramp")
H256_GATE = dict(exits=["text_visual_concat", 1, 2, 3], encoder_layer_strategy="gate", exit_head_num_layers=1)
H256_RAMP = dict(exits=[1, 2, 3], encoder_layer_strategy="ramp")
# name -> (shape, EE_config, K, per-exit temperatures, documents, text length)
CASES = {
    "tiny_ramp_emb_k16": ("tiny", TINY_EMB, 16, False, 40, 16),
    "h256_gate_k10_temps": ("h256", H256_GATE, 10, True, 40, 48),
    "dit_tiny": ("dit", dict(DIT_EE), 16, False, 40, 0),
    "tiny_t8": ("tiny", TINY_EMB, 16, False, 32, 8),                          # the base documents of the boundary cases
    "h256_patience_k2": ("h256", dict(H256_RAMP, inference_strategy="patience", patience=1), 2, False, 40, 48),
    "h256_ramp_k2": ("h256", H256_RAMP, 2, False, 40, 48),
    "h256_lte_k10_temps": ("h256", dict(H256_GATE, use_lte=True), 10, True, 40, 48),
    # the X-space probe exists at the LayoutLMv3-base / -large widths only: base with four layers
    "base4_ramp_k16": ("base4", dict(exits=[1, 2, 3], encoder_layer_strategy="ramp"), 16, False, 12, 32),
}
POSITION = 0.65      # thresholds near the position 0.65 N of the sorted criteria: about a third of the documents clear each exit's test
MIN_GAP = 1e-5       # >> 2^-23, the rounding of a stored float32 criterion <= 1
FIELDS = ("logits", "exit_layer", "confidence")


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    """Floats compared as their words: a NaN would be unequal to itself."""
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


class Case:
    """One shape: configuration, weights, documents on the device, ONE engine (the default schedule; the tests pass schedules per call) and
    its dump-all criterion, computed once and shared."""

    def __init__(self, pkg, name):
        import torch
        shape, ee, K, temps, B, T = CASES[name]
        self.pkg, self.name, self.B, self.T, self.dit = pkg, name, B, T, shape == "dit"
        mk = {"tiny": lambda **kw: pkg.ModelConfig.tiny(**kw), "h256": lambda **kw: pkg.ModelConfig.tiny(**kw, **H256_KW),
              "base4": lambda **kw: pkg.ModelConfig.base(num_hidden_layers=4, **kw), "dit": lambda **kw: pkg.ModelConfig.dit_tiny(**kw)}[shape]
        self.cfg = mk(EE_config=dict(ee), num_labels=K)
        if self.dit:
            self.W = pkg.synth.make_weights_beit(self.cfg, seed=70 + K, head_gain=4.0)
            self.docs = {"pixel_values": pkg.synth.make_documents(self.cfg, B, seed=71 + K, text_len=8)["pixel_values"]}
        else:
            self.W = pkg.synth.make_weights(self.cfg, seed=70 + K, head_gain=4.0)
            d = pkg.synth.make_documents(self.cfg, B, seed=71 + K, text_len=T, min_words=2)
            self.docs = {k: d[k] for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}
        ec = self.cfg.exit_config
        self.E, self.n_emb, self.lte = ec.num_exits, len(ec.embedding_exits), bool(ec.use_lte)
        self.tm = np.random.default_rng(K).uniform(0.5, 3.0, self.E + 1) if temps else None
        self.dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in self.docs.items()}
        self.eng = self.engine()
        self._crit = None

    def engine(self, max_docs=None, weights=None, **kw):
        n = max_docs or self.B
        size = dict(max_docs=n) if self.dit else dict(max_docs=n, max_text_len=self.T)
        eng = self.pkg.EarlyExitEngine(self.cfg, **size, **kw)
        eng.load_weights(weights or self.W)
        return eng

    def inputs(self, sl=slice(None)):
        return {k: v[sl].contiguous() for k, v in self.dev.items()}

    def crit(self):
        """(E + 1, B) float64: the dump-all criterion (whole layers), the LTE score under use_lte."""
        if self._crit is None:
            o = self.eng.forward(**self.inputs(), dump_all=True, want_all=True, whole_layers=True, temperatures=self.tm)
            self._crit = _np(o.all_crit).astype(np.float64)
            self.eng.check()
        return self._crit

    def thresholds(self, position=POSITION, sl=slice(None)):
        """Per-exit thresholds at gap midpoints of the dump-all criterion of the documents `sl` (max-softmax: '>' at position 0.65 N; LTE:
        '<' at the mirrored position, embedding exits skipped)."""
        t = self.crit()[:, sl]
        if self.lte:
            thr, width = lte_ref.gap_thresholds(t, 1.0 - position, MIN_GAP, self.n_emb)
        else:
            thr, width = csf_ref.gap_thresholds(t, position, MIN_GAP)
        assert np.all(width >= MIN_GAP), (self.name, width.tolist())
        return thr


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


def snapshot(out):
    return {f: _np(getattr(out, f)).copy() for f in FIELDS}


def guard_spread(ex, E, tag, distinct=3):
    """Failing, not skipping: the documents leave at several exits, the final one among them."""
    spread = np.bincount(ex, minlength=E + 1).tolist()
    assert len(np.unique(ex)) >= distinct and E in ex, (tag, spread)
    return spread


def verify(eng, E, B, chunks, on, off, tag):
    """The contract of include/mmee.h on one drained stream: `chunks` the ResultChunks, `on` the flagged forward's outputs (host copies taken
    after a synchronise), `off` those of the same call without the flag.  Returns the exit array."""
    assert [ch.exit_index for ch in chunks] == list(range(E + 1)), (tag, [ch.exit_index for ch in chunks])
    ex = on["exit_layer"]
    want = stream_ref.chunks(ex, E + 1)
    for ch, slots in zip(chunks, want):
        e = ch.exit_index
        assert ch.doc_index.dtype == np.int32 and np.array_equal(ch.doc_index, slots), (tag, e, ch.doc_index.tolist(), slots.tolist())
        assert ch.logits.shape == (slots.size, on["logits"].shape[1]) and ch.exit_layer.shape == ch.confidence.shape == (slots.size,)
        assert np.all(ch.exit_layer == e) and np.array_equal(ch.exit_layer, ex[slots]), (tag, e)
        assert np.array_equal(_bits(ch.logits), _bits(on["logits"][slots])), (tag, e, "logits")
        assert np.array_equal(_bits(ch.confidence), _bits(on["confidence"][slots])), (tag, e, "confidence")
    assert sorted(np.concatenate([ch.doc_index for ch in chunks]).tolist()) == list(range(B)), tag      # everybody, exactly once
    for f in FIELDS:
        assert np.array_equal(_bits(on[f]), _bits(off[f])), (tag, f)
    docs = eng.stage_counts()["docs"]                           # of the flagged forward: the last one on the handle
    assert [ch.doc_index.size for ch in chunks] == [a - b for a, b in zip(docs, docs[1:] + [0])], (tag, docs)
    return ex


def run(eng, E, inputs, tag, **kw):
    """The same call without and with the flag; the stream is drained BEFORE anything synchronises, then checked."""
    B = int(inputs["pixel_values"].shape[0])
    off = snapshot(eng.forward(**inputs, **kw))
    st = eng.forward_stream(**inputs, **kw)
    chunks = list(st)
    eng.check()
    assert list(st) == []                                       # drained: the iterator stays at its end
    return verify(eng, E, B, chunks, snapshot(st.output), off, tag), chunks


# ---- 1. the main contract --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_ramp_emb_k16", "h256_gate_k10_temps", "dit_tiny"])
def test_chunks_are_the_forwards_own_rows_in_exit_order(cases, name):
    c = cases(name)
    ex, chunks = run(c.eng, c.E, c.inputs(), name, thresholds=c.thresholds(), temperatures=c.tm)
    spread = guard_spread(ex, c.E, name)
    report_measured(f"result_stream[{name}]", "non-empty chunks", float(sum(1 for n in spread if n)))
    # a second streamed forward on the handle, other thresholds: the buffer is reused, the chunks are the new call's
    ex2, _ = run(c.eng, c.E, c.inputs(), name, thresholds=c.thresholds(0.35), temperatures=c.tm)
    assert not np.array_equal(ex, ex2)


def test_model_early_exit_stream_is_early_exit_delivered_in_chunks(cases, pkg):
    c = cases("tiny_ramp_emb_k16")
    n = 12
    m = pkg.LayoutLMv3EEForSequenceClassification(c.cfg, weights=c.W, max_docs=n, max_text_len=c.T)
    thr = c.thresholds(sl=slice(0, n))
    off = snapshot(m.early_exit(**c.inputs(slice(0, n)), thresholds=thr))
    st = m.early_exit_stream(**c.inputs(slice(0, n)), thresholds=thr)
    chunks = list(st)
    m.engine.check()
    ex = verify(m.engine, c.E, n, chunks, snapshot(st.output), off, "model")
    guard_spread(ex, c.E, "model", distinct=2)
    with pytest.raises(ValueError, match="max_docs"):
        m.early_exit_stream(**c.inputs(slice(0, n + 1)), thresholds=thr)
    m.engine.close()


# ---- 2. kernel boundaries ------------------------------------------------------------------------------------------------------------------------
BASE_DOCS = 32


@pytest.fixture(scope="module")
def boundary(cases):
    """The tiny shape at T = 8: ONE engine for 1025 documents and 32 base documents whose exits under gap-midpoint thresholds are known from
    their own dump (a quarter of them clears each exit's test, so some reach the final one); batch slot i holds base document (i + shift) % 32, with the shift chosen so that slot 0 -- and with it slots 64 and 1024 --
    leaves at exit 0.  A document's arithmetic does not depend on its batch mates, so the exit array is periodic: leavers and stayers sit on
    both sides of every wave boundary and of the 1024-document loop boundary, which the tests assert from the exit array itself."""
    c = cases("tiny_t8")
    assert c.B == BASE_DOCS
    thr = c.thresholds(0.75)
    ex = csf_ref.exits(c.crit(), thr, +1)
    guard_spread(ex, c.E, "tiny_t8 base documents")
    shift = int(np.nonzero(ex == 0)[0][0])
    eng = c.engine(max_docs=1025)
    yield c, eng, thr, np.roll(ex, -shift), shift
    eng.close()


def _positions(ex, e):
    """Positions, in the document list of the stage that reaches exit e, of the documents that leave there."""
    stage = np.nonzero(ex >= e)[0]
    return np.nonzero(ex[stage] == e)[0], stage.size


@pytest.mark.parametrize("B", [1, 63, 64, 65, 1025])
def test_wave_and_loop_boundaries(boundary, B):
    c, eng, thr, ex_base, shift = boundary
    idx = (np.arange(B) + shift) % BASE_DOCS
    inputs = {k: v[idx].contiguous() for k, v in c.dev.items()}
    ex, chunks = run(eng, c.E, inputs, f"B={B}", thresholds=thr)
    assert np.array_equal(ex, ex_base[np.arange(B) % BASE_DOCS]), B       # periodic, as the base documents' own dump says
    assert ex[0] == 0 and chunks[0].doc_index[0] == 0
    if B == 1:
        assert [ch.doc_index.size for ch in chunks] == [1] + [0] * c.E      # a single lane
        return
    pos, n = _positions(ex, 0)
    assert n == B
    if B >= 64:
        assert np.any(ex[:63] != 0) and ex[B - 1 if B > 64 else 0] == 0       # stayers in the first wave; at 65 / 1025 the LAST slot leaves at exit 0
    if B == 65:
        assert pos.min() < 64 <= pos.max() == 64                            # leavers on both sides of the wave boundary
    if B == 1025:
        assert pos.min() < 1024 == pos.max() and chunks[0].doc_index[-1] == 1024      # ... and of the loop boundary: ranked behind chunk 0's carry
        crossed = 0                                                         # later stages span several waves too, leavers in more than one
        for e in range(1, c.E + 1):
            pos, n = _positions(ex, e)
            crossed += int(pos.size > 0 and pos.min() < 64 <= pos.max())
        assert crossed >= 2, crossed
    else:
        assert sum(1 for ch in chunks if ch.doc_index.size) >= 3


# ---- 3. degenerate populations ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_ramp_emb_k16", "base4_ramp_k16"])
def test_everybody_leaves_at_the_first_exit(cases, name):
    """A max-softmax is never below 0: thresholds of -1 release every document at exit 0; the later stages are empty and their chunks too.
    The base-width case runs the default schedule, the X-space probe."""
    c = cases(name)
    if name.startswith("base4"):
        assert c.eng.precision == "split" and c.eng.xprobe_default
    ex, chunks = run(c.eng, c.E, c.inputs(), name, thresholds=-1.0)
    assert np.all(ex == 0) and [ch.doc_index.size for ch in chunks] == [c.B] + [0] * c.E
    assert c.eng.stage_counts()["docs"] == [c.B] + [0] * c.E
    if name.startswith("base4"):
        assert c.eng.layer_plan()["docs_probe"][0] == c.B              # layer 0 ends in exit 0: probed first, for every document
        ex, _ = run(c.eng, c.E, c.inputs(), name, thresholds=c.thresholds())      # and a spread population under the same schedule
        guard_spread(ex, c.E, name)
        assert any(c.eng.layer_plan()["docs_probe"][1:])


@pytest.mark.parametrize("name", ["tiny_ramp_emb_k16", "dit_tiny"])
def test_nobody_leaves_before_the_final_exit(cases, name):
    """A max-softmax is never above 1: thresholds of 2 keep every document to the final classifier; only the last chunk holds rows."""
    c = cases(name)
    ex, chunks = run(c.eng, c.E, c.inputs(), name, thresholds=2.0)
    assert np.all(ex == c.E) and [ch.doc_index.size for ch in chunks] == [0] * c.E + [c.B]


# ---- 4. independence from the decision and from the schedule ------------------------------------------------------------------------------------
INDEPENDENCE = {
    "patience": ("h256_patience_k2", dict(patience=1), 40),
    "patience_or_threshold": ("h256_ramp_k2", dict(exit_rule="patience_or_threshold", patience=2), 40),
    "use_lte": ("h256_lte_k10_temps", dict(), 40),
    "whole_layers": ("h256_gate_k10_temps", dict(whole_layers=True), 40),
    "kv_probe": ("h256_gate_k10_temps", dict(xprobe=False, probe_always=True), 40),
    "low_latency": ("h256_gate_k10_temps", dict(low_latency=True, whole_layers=True), 2),
}


def patience_weights(c):
    """PABEE has no threshold to place: under patience 1 a document leaves at the first exit whose argmax repeats the previous one's, and
    with random heads every document of a batch does so at the same exit.  What thresholds at gap midpoints do for the other criteria, the
    heads' biases do here (K = 2, one head per exit, heads do not feed back): label 1's bias of exit e is lowered by a cut c_e taken at a gap
    midpoint of the dump-all logit differences z_1 - z_0, so that argmax_e(n) = [difference > c_e].  c_0: the median; c_1: the cut at which
    the number of documents agreeing with exit 0 (they leave at exit 1) is nearest to a third; c_2: the cut that splits the others nearest to
    half between agreeing with exit 1 (they leave at exit 2) and the final exit.  Returns the weights; the test guards the population."""
    assert c.cfg.num_labels == 2 and c.E == 3 and c.n_emb == 0 and c.tm is None
    o = c.eng.forward(**c.inputs(), dump_all=True, want_all=True, whole_layers=True, patience=1)
    z = _np(o.all_logits).astype(np.float64)
    c.eng.check()
    d = z[:, :, 1] - z[:, :, 0]

    def cuts(e):
        srt = np.sort(d[e])
        ok = np.nonzero(np.diff(srt) >= 1e-4)[0]              # >> the float32 rounding of a shifted logit of order 1
        assert ok.size, e
        return 0.5 * (srt[ok] + srt[ok + 1])

    def best(e, score):
        cand = cuts(e)
        return float(cand[int(np.argmin([score(d[e] > x) for x in cand]))])

    c0 = best(0, lambda a: abs(int(a.sum()) - c.B / 2))
    a0 = d[0] > c0
    c1 = best(1, lambda a: abs(int((a == a0).sum()) - c.B / 3))
    a1 = d[1] > c1
    stay = a1 != a0
    c2 = best(2, lambda a: abs(int(((a == a1) & stay).sum()) - int(stay.sum()) / 2))
    W = dict(c.W)
    for e, cut in enumerate((c0, c1, c2)):
        (name,) = [k for k in W if k.endswith(f"encoder.early_exits.{e}.out_proj.bias")]
        W[name] = W[name].copy()
        W[name][1] -= np.float32(cut)
    return W


@pytest.mark.parametrize("mode", list(INDEPENDENCE))
def test_the_stream_does_not_look_at_how_the_exit_was_decided(cases, mode):
    name, kw, B = INDEPENDENCE[mode]
    c = cases(name)
    sl = slice(0, B)
    if mode == "patience":
        thr = None
    elif B == 2:                                                # two documents: one clears exit 0's test, nothing releases the other before the final exit
        thr = np.where(np.arange(c.E + 1) == 0, c.thresholds(0.5, sl), 2.0)
    else:
        thr = c.thresholds(POSITION, sl)
    eng = c.engine(weights=patience_weights(c) if mode == "patience" else None)      # a handle of its own: rules and patience are handle state
    ex, chunks = run(eng, c.E, c.inputs(sl), mode, thresholds=thr, temperatures=c.tm, **kw)
    spread = guard_spread(ex, c.E, mode, distinct=min(3, B))
    report_measured(f"result_stream[{mode}]", "non-empty chunks", float(sum(1 for n in spread if n)))
    if mode == "low_latency":
        assert max(eng.last_k_splits()) > 1                     # the split-K mode did run
    if mode == "kv_probe":
        assert any(eng.layer_plan()["docs_probe"])
    if mode == "whole_layers":
        assert not any(eng.layer_plan()["docs_probe"])
    eng.close()


# ---- 5. the overlap rule ------------------------------------------------------------------------------------------------------------------------
def test_a_later_streamed_forward_drops_the_unread_chunks_and_nothing_else(cases, pkg):
    c = cases("h256_gate_k10_temps")
    eng = c.eng
    a_sl, b_sl = slice(0, 24), slice(24, 40)
    thr_a, thr_b = c.thresholds(POSITION, a_sl), c.thresholds(0.8, b_sl)
    off_a = snapshot(eng.forward(**c.inputs(a_sl), thresholds=thr_a, temperatures=c.tm))
    off_b = snapshot(eng.forward(**c.inputs(b_sl), thresholds=thr_b, temperatures=c.tm))
    st_a = eng.forward_stream(**c.inputs(a_sl), thresholds=thr_a, temperatures=c.tm)
    first = next(st_a)
    assert first.exit_index == 0
    st_b = eng.forward_stream(**c.inputs(b_sl), thresholds=thr_b, temperatures=c.tm)
    chunks_b = list(st_b)
    eng.check()
    ex_b = verify(eng, c.E, 16, chunks_b, snapshot(st_b.output), off_b, "B")      # B's chunks are B's
    guard_spread(ex_b, c.E, "B", distinct=2)
    on_a = snapshot(st_a.output)                                # A's outputs are complete and equal its flag-off twin
    for f in FIELDS:
        assert np.array_equal(_bits(on_a[f]), _bits(off_a[f])), f
    guard_spread(on_a["exit_layer"], c.E, "A", distinct=2)
    assert np.array_equal(first.doc_index, stream_ref.chunks(on_a["exit_layer"], c.E + 1)[0])
    assert np.array_equal(_bits(first.logits), _bits(on_a["logits"][first.doc_index]))      # a copy: B did not touch the chunk A had read
    with pytest.raises(pkg.capi.MMEEError, match="dropped"):
        next(st_a)


# ---- 6. launch accounting ------------------------------------------------------------------------------------------------------------------------
def test_the_flag_adds_one_launch_per_exit_and_leaves_other_forwards_alone(cases):
    c = cases("h256_gate_k10_temps")
    call = dict(thresholds=c.thresholds(), temperatures=c.tm)

    def profiled(eng, stream):
        eng.profile(True)
        if stream:
            st = eng.forward_stream(**c.inputs(), **call)
            n_chunks = len(list(st))
            out = st.output
        else:
            out, n_chunks = eng.forward(**c.inputs(), **call), 0
        prof = eng.profile_read()
        eng.profile(False)
        return snapshot(out), sum(v["launches"] for v in prof.values()), prof["emit_leavers"]["launches"], n_chunks

    fresh = c.engine()
    want, n_fresh, emit_fresh, _ = profiled(fresh, False)
    fresh.close()
    eng = c.engine()
    before, n_before, emit_before, _ = profiled(eng, False)
    on1, n_on1, emit_on1, chunks1 = profiled(eng, True)
    on2, n_on2, emit_on2, chunks2 = profiled(eng, True)
    after, n_after, emit_after, _ = profiled(eng, False)
    eng.check()
    eng.close()
    report_measured("result_stream[launches]", "profiled launches without the flag", float(n_fresh))
    report_measured("result_stream[launches]", "profiled launches with the flag", float(n_on1))
    assert 0 < n_fresh == n_before == n_after and emit_fresh == emit_before == emit_after == 0
    assert n_on1 == n_on2 == n_fresh + c.E + 1 and emit_on1 == emit_on2 == chunks1 == chunks2 == c.E + 1
    for got in (before, on1, on2, after):
        for f in FIELDS:
            assert np.array_equal(_bits(got[f]), _bits(want[f])), f


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_with_a_message(cases, pkg):
    c = cases("tiny_ramp_emb_k16")
    eng = c.engine()
    with pytest.raises(ValueError, match="dump_all"):
        eng.forward_stream(**c.inputs(), dump_all=True)
    with pytest.raises(ValueError, match="_capture"):
        eng.forward_stream(**c.inputs(), thresholds=2.0, _capture=True)
    with pytest.raises(pkg.capi.MMEEError, match="no forward with MMEE_FLAG_STREAM_RESULTS"):
        next(iter(pkg.ResultStream(eng)))
    # the C-ABI's own refusals, under the Python ones
    with pytest.raises(pkg.capi.MMEEError, match="MMEE_FLAG_NO_EXIT"):
        eng.forward(**c.inputs(), dump_all=True, _stream=True)
    with pytest.raises(pkg.capi.MMEEError, match="ee_graph_capture: MMEE_FLAG_STREAM_RESULTS"):
        eng.capture(**{k: v.clone() for k, v in c.inputs().items()}, thresholds=2.0, _stream=True)
    with pytest.raises(pkg.capi.MMEEError, match="no forward with MMEE_FLAG_STREAM_RESULTS"):      # none of the refused calls armed a stream
        next(iter(pkg.ResultStream(eng)))
    # ... and the handle is as good as new
    ex, _ = run(eng, c.E, c.inputs(), "after the refusals", thresholds=c.thresholds())
    guard_spread(ex, c.E, "after the refusals")
    eng.close()
