"""GPU: the low-latency mode (include/mmee.h MMEE_FLAG_LOW_LATENCY, ``forward(low_latency=True)``): the attention-output and FFN-down GEMMs of
every LayoutLMv3 layer as split-K, the LayerNorm behind them completing the row from the parts.  A re-association: the goldens' 1e-4 bar and
exit indices hold, the call's own properties (early exit == its dump-all row, permutation, independence of batch mates, graph replay) hold bit
for bit, and without the flag nothing changes.  Shapes: H = 256 / I = 512 has 8 / 16 k-stages (S = 2 / 4 at the minimum of stages per part),
LayoutLMv3-base 24 / 96."""
import numpy as np
import pytest

from .conftest import DIT_EE, H256_KW, MATRIX_CASES, MATRIX_SEEDS, load_golden, matrix_config, report_measured
from .lte_ref import gap_thresholds

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4
MIN_GAP = 4e-4                # thresholds sit in gaps this wide: no document is within 1e-4 of one
CONFIG2_EE = dict(exits=[2, 4, 6, 8, 10], encoder_layer_strategy="ramp")
KEYS = ("input_ids", "attention_mask", "bbox", "pixel_values")


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _dev(docs):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(docs[k])).cuda() for k in KEYS}


def _split_k(eng):
    a, d = eng.last_k_splits()
    assert a > 1 and d > 1, f"the rule declined (S = {a} / {d}): this call has tested nothing"
    return a, d


@pytest.fixture(scope="module")
def base(pkg):
    """LayoutLMv3-base with config 2's exits: one set of weights and one engine for the module (no test changes either)."""
    cfg = pkg.ModelConfig.base(EE_config=CONFIG2_EE)
    W = pkg.synth.make_weights(cfg, seed=1234, head_gain=6.0)
    eng = pkg.EarlyExitEngine(cfg, max_docs=24, max_text_len=512, xprobe=False)
    eng.load_weights(W)
    yield cfg, W, eng
    eng.close()


# ---- 1. goldens ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["h256_entropy_1layer", "h256_gate", "base_gate"])
def test_goldens_hold_under_the_flag(pkg, name):
    """Dump-all and early exit, ragged and dense rows: logits and every exit's policy logits within 1e-4 of the fixture, exit indices the
    fixture's, and S > 1 for both GEMMs in every call."""
    g = load_golden(name)
    cfg, ee, n_docs, T = matrix_config(pkg, name)
    W = pkg.synth.make_weights(cfg, seed=MATRIX_SEEDS["seed_w"])
    docs = pkg.synth.make_documents(cfg, n_docs, seed=MATRIX_SEEDS["seed_docs"], text_len=T, min_words=3)
    eng = pkg.EarlyExitEngine(cfg, max_docs=8, max_text_len=T, precision="split", xprobe=False)
    eng.load_weights(W)
    args = tuple(docs[k] for k in KEYS)
    store = g["logits_store"]
    seen = set()
    for dense in (False, True):
        out = eng.forward(*args, dump_all=True, dense_rows=dense, want_all=True, want_head=True, validate=True, low_latency=True)
        seen.add(_split_k(eng))
        report_measured(f"low_latency[{name},dense={int(dense)}]", f"S = {eng.last_k_splits()}, max|dlogit| vs golden",
                        float(np.abs(_np(out.all_logits) - store).max()))
        np.testing.assert_allclose(_np(out.all_logits), store, rtol=0, atol=LOGIT_TOL)
        np.testing.assert_allclose(_np(out.head_logits), g["exit_logits"], rtol=0, atol=LOGIT_TOL)
        np.testing.assert_allclose(_np(out.logits), g["logits"], rtol=0, atol=LOGIT_TOL)
        assert (_np(out.exit_layer) == store.shape[0] - 1).all()
    if name.startswith("h256"):
        assert seen == {(2, 4)}                            # 8 and 16 k-stages: parts of 4 stages each
    cases = []
    if str(cfg.exit_config.inference_strategy) == "entropy":
        # entropy BELOW the threshold leaves (EE/models/EE_modules.py:137-144); thresholds in the widest gap of every exit's entropies
        x = store.astype(np.float64)
        ent = np.log(np.exp(x).sum(-1)) - (x * np.exp(x)).sum(-1) / np.exp(x).sum(-1)
        margin = 1e-4 * max(1.0, float(np.abs(ent).max()))
        thr = np.zeros(ent.shape[0])
        for e in range(ent.shape[0]):
            srt = np.sort(ent[e])
            k = int(np.argmax(np.diff(srt)))
            thr[e] = 0.5 * (srt[k] + srt[k + 1]) if srt[k + 1] - srt[k] > 4 * margin else -1.0
        assert np.abs(ent - thr[:, None]).min() > margin
        hit = ent < thr[:, None]
        hit[-1] = True
        ex = hit.argmax(0).astype(np.int32)
        assert len(np.unique(ex)) >= 2
        cases.append((thr, ex, store[ex, np.arange(n_docs)]))
    else:
        e_ = np.exp(store - store.max(-1, keepdims=True))
        conf = (e_ / e_.sum(-1, keepdims=True)).max(-1)
        for i in range(4):
            thr = float(g[f"pol_thr{i}"])
            if thr == 0.0 or thr > 1.0 or np.abs(conf - thr).min() > 1e-5:
                cases.append((thr, g[f"pol_exits{i}"], g[f"pol_pred{i}"]))
        assert cases
    for thr, ex, pred in cases:
        for kw in (dict(), dict(dense_rows=True), dict(whole_layers=True), dict(whole_layers=True, dense_rows=True)):
            out = eng.forward(*args, thresholds=thr, low_latency=True, validate=True, **kw)
            _split_k(eng)
            assert np.array_equal(_np(out.exit_layer), ex), (name, thr, kw)
            np.testing.assert_allclose(_np(out.logits), pred, rtol=0, atol=LOGIT_TOL)
    eng.close()


# ---- 2. the residual gather after a compaction --------------------------------------------------------------------------------------------
def _first_exit(conf, thr):
    hit = conf > thr[:, None]
    hit[-1] = True
    return hit.argmax(0).astype(np.int32)


def test_early_exit_rows_are_the_dump_rows_after_compactions(pkg, oracle, base):
    """After an exit the attention-output residual is Xs read through the row map: 8 ragged documents leave at three or more different exits,
    and every document's logits and confidence are bit-identical to its dump-all row (same flags) at the exit the policy picked; a permuted
    batch gives permuted bits; other batch mates change nothing."""
    cfg, W, eng = base
    B = 8
    docs = pkg.synth.make_documents(cfg, B, seed=311, text_len=128, min_words=14, max_words=126)
    lens = docs["attention_mask"].sum(1)
    assert lens.min() >= 16 and lens.max() <= 128 and len(np.unique(lens)) > 4
    t = _dev(docs)
    dump = eng.forward(**t, dump_all=True, want_all=True, validate=True, low_latency=True)
    _split_k(eng)
    store, crit = _np(dump.all_logits), _np(dump.all_crit)
    conf = oracle.softmax64(store.astype(np.float64)).max(-1)
    thr = ex = None
    for q in (0.6, 0.5, 0.7, 0.4, 0.8, 0.3):               # the first placement (of the DUMP's confidences) that spreads the documents
        thr_q, width = gap_thresholds(conf, q, MIN_GAP)
        thr_q[-1] = 2.0
        ex_q = _first_exit(conf, thr_q)
        if len(np.unique(ex_q)) >= 3 and (ex_q == 0).any():
            thr, ex = thr_q, ex_q
            break
    assert thr is not None, "no threshold placement spreads these documents over three exits"
    assert width[:-1].min() >= MIN_GAP
    out = eng.forward(**t, thresholds=thr, whole_layers=True, low_latency=True, validate=True)
    _split_k(eng)
    got_ex = _np(out.exit_layer)
    assert np.array_equal(got_ex, ex)
    counts = eng.stage_counts()["docs"]
    assert counts == [int((ex >= e).sum()) for e in range(len(counts))] and counts[1] < B      # the compactions really happened
    n = np.arange(B)
    assert np.array_equal(_np(out.logits), store[ex, n])
    assert np.array_equal(_np(out.confidence), crit[ex, n])
    # permutation
    perm = np.random.default_rng(5).permutation(B)
    outp = eng.forward(**{k: v[perm] for k, v in t.items()}, thresholds=thr, whole_layers=True, low_latency=True, validate=True)
    assert np.array_equal(_np(outp.exit_layer), ex[perm])
    assert np.array_equal(_np(outp.logits), _np(out.logits)[perm]) and np.array_equal(_np(outp.confidence), _np(out.confidence)[perm])
    # other batch mates (same B, T): every kept document in turn, at its own slot
    other = pkg.synth.make_documents(cfg, B, seed=312, text_len=128, min_words=14, max_words=126)
    for keep in (int(np.argmax(ex == 0)), int(np.argmax(ex == ex.max()))):
        mixed = {k: other[k].copy() for k in KEYS}
        for k in KEYS:
            mixed[k][keep] = docs[k][keep]
        outm = eng.forward(**_dev(mixed), thresholds=thr, whole_layers=True, low_latency=True, validate=True)
        assert _split_k(eng)
        assert int(_np(outm.exit_layer)[keep]) == int(ex[keep])
        assert np.array_equal(_np(outm.logits)[keep], _np(out.logits)[keep])
        assert np.array_equal(_np(outm.confidence)[keep], _np(out.confidence)[keep])


# ---- 3. tile edges ------------------------------------------------------------------------------------------------------------------------
def _one_document(pkg, cfg, T, seed):
    if T > 1:
        return pkg.synth.make_documents(cfg, 1, seed=seed, text_len=T, min_words=T - 2)
    d = pkg.synth.make_documents(cfg, 1, seed=seed, text_len=8)
    return dict(input_ids=np.zeros((1, 1), np.int64), attention_mask=np.ones((1, 1), np.int64), bbox=np.zeros((1, 1, 4), np.int64),
                pixel_values=d["pixel_values"])


@pytest.mark.parametrize("T,rows", [(1, 198), (512, 709)])
def test_one_document_against_the_flag_off_forward(pkg, oracle, base, T, rows):
    """198 rows: a full and a partial 128-row tile; 709 rows: the reference's operating point.  Flag on against flag off: logits within 1e-4
    (measured value recorded), exits equal."""
    cfg, W, eng = base
    t = _dev(_one_document(pkg, cfg, T, seed=400 + T))
    off = eng.forward(**t, dump_all=True, want_all=True, validate=True)
    assert eng.last_k_splits() == (1, 1) and eng.stage_counts()["rows"][0] == rows
    on = eng.forward(**t, dump_all=True, want_all=True, validate=True, low_latency=True)
    S = _split_k(eng)
    d = float(np.abs(_np(on.all_logits) - _np(off.all_logits)).max())
    report_measured(f"low_latency[one document, T={T}, {rows} rows]", f"S = {S}, max|dlogit| flag on vs off", d)
    assert d <= LOGIT_TOL
    conf = oracle.softmax64(_np(off.all_logits).astype(np.float64)).max(-1)[:, 0]
    for leave_at in (1, 3, 5):                              # the document leaves at the second / fourth encoder exit, or at the classifier
        thr = np.where(np.arange(conf.shape[0]) < leave_at, conf + 0.01, conf - 0.01)
        a = eng.forward(**t, thresholds=thr, whole_layers=True, validate=True)
        b = eng.forward(**t, thresholds=thr, whole_layers=True, validate=True, low_latency=True)
        _split_k(eng)
        assert int(_np(a.exit_layer)[0]) == int(_np(b.exit_layer)[0]) == leave_at
        np.testing.assert_allclose(_np(b.logits), _np(a.logits), rtol=0, atol=LOGIT_TOL)


def test_first_row_count_the_rule_declines_is_the_flag_off_forward(pkg, base):
    """The first max_rows at which ee_low_latency_k_splits returns 1 for the base shape's FFN-down GEMM (read from the rule): S = 1 / 1 is
    reported and the flagged forward is the flag-off forward bit for bit."""
    import torch
    cfg, W, eng = base
    H, I, Pv = cfg.hidden_size, cfg.intermediate_size, (cfg.input_size // cfg.patch_size) ** 2 + 1
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    rule = pkg.capi.load().ee_low_latency_k_splits
    first = next(r for r in range(1, 1 << 20) if rule(r, H, I, cus) == 1)
    assert rule(first - 1, H, I, cus) > 1
    # the smallest batch shape B x (T + Pv) with that many rows or, where `first` has no such factorisation, the next row count that has one
    B, T = next((b, r // b - Pv) for r in range(first, first + 4096) for b in range(1, eng.max_docs + 1)
                if r % b == 0 and 1 <= r // b - Pv <= 512)
    assert rule(B * (T + Pv), H, I, cus) == 1 and rule(B * (T + Pv), H, H, cus) == 1
    docs = pkg.synth.make_documents(cfg, B, seed=77, text_len=T, min_words=min(8, T - 2))
    t = _dev(docs)
    off = eng.forward(**t, dump_all=True, want_all=True, validate=True)
    on = eng.forward(**t, dump_all=True, want_all=True, validate=True, low_latency=True)
    assert eng.last_k_splits() == (1, 1)
    for a, b in ((off.all_logits, on.all_logits), (off.all_crit, on.all_crit), (off.logits, on.logits), (off.confidence, on.confidence)):
        assert np.array_equal(_np(a), _np(b))


# ---- 4. flag off is untouched -------------------------------------------------------------------------------------------------------------
def test_flag_off_after_flagged_forwards_is_a_fresh_engines_forward(pkg, base):
    cfg, W, eng = base
    t = _dev(pkg.synth.make_documents(cfg, 2, seed=21, text_len=96, min_words=20))
    thr = [0.2, 0.25, 0.3, 0.35, 0.4, 2.0]
    for kw in (dict(dump_all=True), dict(thresholds=thr), dict(thresholds=thr, whole_layers=True)):
        eng.forward(**t, low_latency=True, validate=True, **kw)
        _split_k(eng)
    fresh = pkg.EarlyExitEngine(cfg, max_docs=24, max_text_len=512, xprobe=False)
    fresh.load_weights(W)
    launches = []
    for e in (eng, fresh):
        res = []
        for kw in (dict(dump_all=True, want_all=True), dict(thresholds=thr, want_all=True), dict(thresholds=thr, whole_layers=True)):
            e.profile(True)
            o = e.forward(**t, validate=True, **kw)
            prof = e.profile_read()
            e.profile(False)
            assert e.last_k_splits() == (1, 1)
            res.append(([_np(x) for x in (o.logits, o.exit_layer, o.confidence, o.all_logits) if x is not None],
                        {r: v["launches"] for r, v in prof.items()}))
        launches.append(res)
    fresh.close()
    for (xa, la), (xb, lb) in zip(*launches):
        assert la == lb and sum(la.values()) > 0
        for a, b in zip(xa, xb):
            assert np.array_equal(a, b, equal_nan=True)


# ---- 5. captured graph --------------------------------------------------------------------------------------------------------------------
def test_captured_graph_replays_the_flagged_bits(pkg, base):
    cfg, W, eng = base
    E = eng.E
    batches = [_dev(_one_document(pkg, cfg, 512, seed=500 + i)) for i in range(3)]
    thr_sets = [np.array([0.35, 0.4, 0.45, 0.5, 0.55, 2.0]), np.array([2.0, 2.0, 0.05, 0.05, 0.05, 2.0]), np.full(E + 1, 0.02)]
    cap = eng.capture(**{k: v.clone() for k, v in batches[0].items()}, thresholds=thr_sets[0], want_all=True, whole_layers=True, low_latency=True)
    _split_k(eng)
    seen = set()
    for i in (1, 2, 0):
        eager = eng.forward(**batches[i], thresholds=thr_sets[i], want_all=True, whole_layers=True, low_latency=True, validate=True)
        S = _split_k(eng)
        ref = [_np(x).copy() for x in (eager.logits, eager.exit_layer, eager.confidence, eager.all_logits, eager.all_crit)]
        eng.forward(**batches[i], thresholds=thr_sets[i])                  # a flag-off forward in between: the graph keeps its own S
        assert eng.last_k_splits() == (1, 1)
        for k, v in batches[i].items():
            cap.inputs[k].copy_(v)
        cap.outputs.all_logits.fill_(float("nan"))
        cap.outputs.all_crit.fill_(float("nan"))
        out = cap.launch(thresholds=thr_sets[i], validate=True)
        assert eng.last_k_splits() == S
        for a, b in zip(ref, (out.logits, out.exit_layer, out.confidence, out.all_logits, out.all_crit)):
            assert np.array_equal(a, _np(b), equal_nan=True)
        seen.add(int(ref[1][0]))
    assert len(seen) >= 2                                                  # the threshold vectors really were each launch's own
    cap.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_flag_and_leave_the_handle_usable(pkg):
    import torch
    ee = dict(exits=[1, 2], encoder_layer_strategy="ramp")
    # an MMEE_PREC_F32 handle
    cfg = pkg.ModelConfig.tiny(EE_config=ee, **H256_KW)
    W = pkg.synth.make_weights(cfg, seed=3, head_gain=6.0)
    docs = pkg.synth.make_documents(cfg, 4, seed=5, text_len=32, min_words=3)
    args = tuple(docs[k] for k in KEYS)
    e32 = pkg.EarlyExitEngine(cfg, max_docs=4, max_text_len=32, precision="fp32")
    e32.load_weights(W)
    with pytest.raises(pkg.capi.MMEEError, match="MMEE_FLAG_LOW_LATENCY.*MMEE_PREC_F32 handle"):
        e32.forward(*args, thresholds=2.0, low_latency=True)
    ref32 = e32.forward(*args, thresholds=2.0, validate=True)
    assert (_np(ref32.exit_layer) == 2).all()
    e32.close()
    # the flag together with MMEE_FLAG_ONE_TERM
    esp = pkg.EarlyExitEngine(cfg, max_docs=4, max_text_len=32, precision="split")
    esp.load_weights(W)
    with pytest.raises(pkg.capi.MMEEError, match="MMEE_FLAG_LOW_LATENCY together with MMEE_FLAG_ONE_TERM"):
        esp.forward(*args, thresholds=2.0, low_latency=True, one_term=True)
    ok = esp.forward(*args, thresholds=2.0, low_latency=True, validate=True)
    _split_k(esp)
    np.testing.assert_allclose(_np(ok.logits), _np(ref32.logits), rtol=0, atol=2 * LOGIT_TOL)      # two back ends, each within 1e-4 of the reference
    esp.close()
    # an MMEE_ARCH_BEIT handle
    g = load_golden("dit_tiny")
    dcfg = pkg.ModelConfig.dit_tiny(EE_config=DIT_EE)
    dit = pkg.EarlyExitEngine(dcfg, max_docs=8, max_text_len=0)
    dit.load_weights(pkg.synth.make_weights_beit(dcfg, seed=int(g["seed_w"])))
    pix = torch.from_numpy(pkg.synth.make_documents(dcfg, 6, seed=int(g["seed_docs"]), text_len=8)["pixel_values"]).cuda()
    with pytest.raises(pkg.capi.MMEEError, match="MMEE_FLAG_LOW_LATENCY.*MMEE_ARCH_BEIT handle"):
        dit.forward(pixel_values=pix, thresholds=float(g["pol_thr1"]), low_latency=True)
    out = dit.forward(pixel_values=pix, thresholds=float(g["pol_thr1"]), validate=True)
    assert np.array_equal(_np(out.exit_layer), g["pol_exits1"])
    dit.close()


# ---- 7. overflow still surfaces -----------------------------------------------------------------------------------------------------------
def test_split_overflow_is_reported_under_the_flag(pkg):
    """The x5000 LayerNorm-gain checkpoint of tests/test_gpu_config3_and_robustness.py (built the same way): the LayerNorm launches that
    complete the rows from the split-K parts flag the overflow of their output planes like the plain ones."""
    ee = dict(exits=["text_visual_concat", 1, 2], encoder_layer_strategy="ramp")
    cfg = pkg.ModelConfig.tiny(EE_config=ee, **H256_KW)
    rng = np.random.default_rng(41)
    W = pkg.synth.make_weights(cfg, seed=41, head_gain=3.0)
    for k in list(W):
        v = W[k]
        if k.endswith("LayerNorm.weight") or k.endswith("norm.weight"):
            gain = np.exp(rng.normal(0.0, 0.5, v.shape)).astype(np.float32) * np.sign(rng.normal(size=v.shape)).astype(np.float32)
            ch = rng.choice(v.shape[0], size=1, replace=False)
            gain[ch] = np.asarray((5000.0,), np.float32) * np.sign(rng.normal(size=len(ch))).astype(np.float32)
            W[k] = gain
        elif v.ndim == 2 and ("dense" in k or "query" in k or "key" in k or "value" in k) and "early_exits" not in k and "classifier" not in k:
            m = np.exp(rng.normal(0.0, 0.0, v.shape)).astype(np.float32)
            m[rng.random(v.shape) < 1e-3] *= 20.0
            W[k] = (v * m).astype(np.float32)
    docs = pkg.synth.make_documents(cfg, 4, seed=42, text_len=40, min_words=2)
    args = tuple(docs[k] for k in KEYS)
    eng = pkg.EarlyExitEngine(cfg, max_docs=4, max_text_len=40, precision="split", xprobe=False)
    eng.load_weights(W)
    with pytest.raises(pkg.capi.MMEEError, match="overflow"):
        eng.forward(*args, dump_all=True, validate=True, low_latency=True)
    _split_k(eng)
    eng.close()


# ---- the Python surfaces ------------------------------------------------------------------------------------------------------------------
def test_model_surface_passes_the_keyword_and_micro_batches_refuse_it(pkg):
    """``model.early_exit(low_latency=True)`` is the engine's flagged forward (a small batch: whole layers), bit for bit; ``MicroBatchedEngine``
    is for large batches and says so."""
    import torch
    ee = dict(exits=[1, 2], encoder_layer_strategy="ramp")
    cfg = pkg.ModelConfig.tiny(EE_config=ee, **H256_KW)
    W = pkg.synth.make_weights(cfg, seed=9, head_gain=6.0)
    m = pkg.LayoutLMv3EEForSequenceClassification(cfg, weights=W, max_docs=8, max_text_len=48)
    docs = pkg.synth.make_documents(cfg, 8, seed=10, text_len=48, min_words=3)
    t = {k: torch.from_numpy(docs[k]).cuda() for k in KEYS}
    dump = m.engine.forward(**t, dump_all=True, want_all=True, low_latency=True, validate=True)
    conf = np.sort(_np(dump.all_crit)[0])
    k = 2 + int(np.argmax(np.diff(conf)[2:6]))             # the widest gap around the middle: about half of the documents leave at the first exit
    assert conf[k + 1] - conf[k] > MIN_GAP
    thr = [float(0.5 * (conf[k] + conf[k + 1])), 2.0, 2.0]
    a = m.early_exit(**t, thresholds=thr, low_latency=True)
    assert _split_k(m.engine) == (2, 4) and sum(m.engine.layer_plan()["docs_probe"]) == 0
    b = m.engine.forward(**t, thresholds=thr, whole_layers=True, low_latency=True, validate=True)
    ex = _np(a.exit_layer)
    assert np.array_equal(ex, _np(b.exit_layer)) and len(np.unique(ex)) == 2
    assert np.array_equal(_np(a.logits), _np(b.logits)) and np.array_equal(_np(a.logits), _np(dump.all_logits)[ex, np.arange(8)])
    m.early_exit(**t, thresholds=thr)
    assert m.engine.last_k_splits() == (1, 1)
    m.engine.close()
    mb = pkg.MicroBatchedEngine(cfg, max_docs=8, max_text_len=48, micro_batches=2)
    mb.load_weights(W)
    with pytest.raises(ValueError, match="low_latency"):
        mb.forward(**t, thresholds=thr, low_latency=True)
    ok = mb.forward(**t, thresholds=thr, validate=True)
    assert np.array_equal(_np(ok.exit_layer), ex)
    mb.close()
