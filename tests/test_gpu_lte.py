"""Learning-to-exit (LTE, include/mmee.h ``ee_config.use_lte``) on the MI355X: the score and the decision inside the forward pass against the
numpy restatement of tests/lte_ref.py applied to the path's own dump-all rows, the captured-graph form, the launch count against the twin
handle without ``use_lte``, and the policy scan / sweep on dumped arrays.  The reference's own wiring of LTE cannot run, so the restatement
is the oracle."""
import numpy as np
import pytest

from .conftest import DIT_EE, H256_KW, report_measured
from .lte_ref import gap_thresholds, lte_exits, lte_policy, lte_scores

pytestmark = pytest.mark.gpu

W_NAME, B_NAME = "layoutlmv3.encoder.lte_classifier.weight", "layoutlmv3.encoder.lte_classifier.bias"

# name -> (shape, EE_config, K, per-exit temperatures, documents, text length).  Together: the tiny (f32 MFMA), H256 (smallest split-capable)
# and base shapes, ramp and gate, 1- and 2-layer heads, embedding exits, K = 10 and 16, temperatures.
CASES = {
    "tiny_ramp_2layer_emb_k16": ("tiny", dict(exits=["vision_avg", "text_avg", 1, 2, 3, 4], encoder_layer_strategy="ramp"), 16, False, 40, 16),
    "h256_gate_1layer_emb_k10_temps": ("h256", dict(exits=["text_visual_concat", 1, 2, 3], encoder_layer_strategy="gate", exit_head_num_layers=1),
                                       10, True, 40, 48),
    "base_ramp_2layer_k16": ("base", dict(exits=[2, 4, 6, 8, 10], encoder_layer_strategy="ramp"), 16, False, 32, 128),
}
QUANTILE = 0.35      # share of the documents reaching an exit that its threshold releases
MIN_GAP = 1e-5       # >> 2^-23, the rounding of a stored score


def _np(t):
    return t.detach().cpu().numpy()


def make_case(pkg, name):
    """(config with use_lte, its twin without, weights holding the two LTE tensors, documents, temperatures)."""
    shape, ee, K, temps, B, T = CASES[name]
    mk = {"tiny": lambda **kw: pkg.ModelConfig.tiny(**kw), "h256": lambda **kw: pkg.ModelConfig.tiny(**kw, **H256_KW),
          "base": lambda **kw: pkg.ModelConfig.base(**kw)}[shape]
    cfg = mk(EE_config=dict(ee, use_lte=True), num_labels=K)
    twin = mk(EE_config=dict(ee), num_labels=K)
    W = pkg.synth.make_weights(cfg, seed=90 + K, head_gain=4.0)
    docs = pkg.synth.make_documents(cfg, B, seed=91 + K, text_len=T, min_words=2)
    E1 = cfg.exit_config.num_exits + 1
    tm = np.random.default_rng(K).uniform(0.5, 3.0, E1) if temps else None
    return cfg, twin, W, docs, tm


def _args(docs, sl=slice(None)):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(docs[k][sl])).cuda() for k in ("input_ids", "attention_mask", "bbox", "pixel_values"))


def _engine(pkg, cfg, W, docs, **kw):
    eng = pkg.EarlyExitEngine(cfg, max_docs=docs["input_ids"].shape[0], max_text_len=docs["input_ids"].shape[1], **kw)
    eng.load_weights(W)
    return eng


def _guards(ex, n_emb, E, tag):
    """The checks are vacuous unless documents really leave through several exits."""
    assert int((ex < n_emb).sum()) == 0, (tag, "a document left at an embedding exit")
    assert int((ex == n_emb).sum()) > 0, (tag, "nobody leaves at the first encoder exit")
    assert len(np.unique(ex)) >= 3 and E in ex, (tag, np.bincount(ex, minlength=E + 1).tolist())


@pytest.mark.parametrize("name", list(CASES))
def test_scores_equal_the_restatement_and_the_other_outputs_are_the_twin_handles(pkg, name):
    """Dump-all, whole layers: all_crit == float32(lte_ref on out_hidden_cls) within 2^-23 (both sides sum in float64: the summation order
    differs by << 1e-12, then one float32 rounding of a value <= 1); rows of embedding exits hold 1.0; head_crit and every logits output are
    bit-identical to the same call on a handle without use_lte built from the same remaining weights."""
    cfg, twin, W, docs, tm = make_case(pkg, name)
    ec = cfg.exit_config
    n_emb, E = len(ec.embedding_exits), ec.num_exits
    args = _args(docs)
    eng = _engine(pkg, cfg, W, docs)
    assert eng.use_lte and set(eng.expected_tensors()[-2:]) == {W_NAME, B_NAME}
    ref = _engine(pkg, twin, W, docs)                           # the two LTE tensors are extra entries there: ignored
    assert not ref.use_lte and eng.expected_tensors()[:-2] == ref.expected_tensors()
    kw = dict(dump_all=True, want_all=True, want_head=True, want_hidden_cls=True, whole_layers=True, temperatures=tm)
    a, b = eng.forward(*args, **kw), ref.forward(*args, **kw)
    eng.check()
    want = lte_scores(_np(a.hidden_cls), W[W_NAME], W[B_NAME], ec.encoder_exit_layers, n_emb)
    got = _np(a.all_crit)
    assert got.dtype == np.float32 and np.all(got[:n_emb] == 1.0)
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float32).astype(np.float64)).max())
    report_measured(f"lte[{name}]", "max |score - float32(restatement)|", err)
    assert err <= 2.0 ** -23
    assert float(want[n_emb:].std()) > 1e-3                     # the scores differ between documents by far more than their rounding
    assert np.array_equal(_np(a.confidence), got[E]) and np.all(_np(a.exit_layer) == E)
    for f in ("logits", "all_logits", "head_logits", "head_crit", "hidden_cls"):
        assert np.array_equal(_np(getattr(a, f)), _np(getattr(b, f))), (name, f)
    eng.close()
    ref.close()


@pytest.mark.parametrize("name", list(CASES))
def test_exits_equal_the_restatement_on_the_dump_all_scores(pkg, name):
    """Whole layers and the K | V probe (xprobe=False): exits == lte_ref on the dump-all scores, logits / confidence bit-identical to the
    dump-all rows at the chosen exit, a permuted batch gives permuted outputs bit for bit, stage populations are the survivors.  Per-exit
    thresholds sit at midpoints of gaps between sorted restatement scores.  The tiny case repeats it with dense rows."""
    cfg, twin, W, docs, tm = make_case(pkg, name)
    ec = cfg.exit_config
    n_emb, E = len(ec.embedding_exits), ec.num_exits
    B = docs["input_ids"].shape[0]
    args = _args(docs)
    eng = _engine(pkg, cfg, W, docs, xprobe=False)
    layouts = (False, True) if name.startswith("tiny") else (False,)
    for dense in layouts:
        dump = eng.forward(*args, dump_all=True, want_all=True, want_hidden_cls=True, whole_layers=True, temperatures=tm, dense_rows=dense)
        al, ac = _np(dump.all_logits), _np(dump.all_crit)
        want = lte_scores(_np(dump.hidden_cls), W[W_NAME], W[B_NAME], ec.encoder_exit_layers, n_emb)
        thr, width = gap_thresholds(want, QUANTILE, MIN_GAP, n_emb)
        assert np.all(width >= MIN_GAP)
        ex = lte_exits(ac, thr, n_emb)
        _guards(ex, n_emb, E, (name, dense))
        rows = np.arange(B)
        for sched in (dict(whole_layers=True), dict(probe_always=True)):
            tag = (name, dense, tuple(sched))
            o = eng.forward(*args, thresholds=thr, temperatures=tm, dense_rows=dense, **sched)
            assert np.array_equal(_np(o.exit_layer), ex), (tag, _np(o.exit_layer).tolist(), ex.tolist())
            assert np.array_equal(_np(o.logits), al[ex, rows]), tag
            assert np.array_equal(_np(o.confidence), ac[ex, rows]), tag
            assert eng.stage_counts()["docs"] == [int((ex >= e).sum()) for e in range(E + 1)], tag
            perm = np.random.default_rng(5).permutation(B)
            p = eng.forward(*_args(docs, perm), thresholds=thr, temperatures=tm, dense_rows=dense, **sched)
            for f in ("logits", "exit_layer", "confidence"):
                assert np.array_equal(_np(getattr(p, f)), _np(getattr(o, f))[perm]), (tag, f)
        # a threshold vector nobody passes: everybody at the final exit, its rows those of the dump
        o = eng.forward(*args, thresholds=0.0, temperatures=tm, dense_rows=dense)
        assert np.all(_np(o.exit_layer) == E) and np.array_equal(_np(o.logits), al[E]) and np.array_equal(_np(o.confidence), ac[E])
    eng.check()
    eng.close()


def test_x_space_probe_gives_the_same_exits_at_the_base_shape(pkg):
    """The engine's default schedule on split precision (X-space probe) is a re-association of the whole-layer arithmetic: its scores are
    measured against whole layers on the same handle first, the thresholds are then put into gaps at least 10 x that wide; exits equal the
    restatement, logits within 1e-4 of the dump-all rows."""
    name = "base_ramp_2layer_k16"
    cfg, twin, W, docs, tm = make_case(pkg, name)
    ec = cfg.exit_config
    n_emb, E = len(ec.embedding_exits), ec.num_exits
    B = docs["input_ids"].shape[0]
    args = _args(docs)
    eng = _engine(pkg, cfg, W, docs)
    assert eng.precision == "split" and eng.xprobe_default
    # thresholds of 0 release nobody (a sigmoid is never below 0): every exit is evaluated for every document under either schedule
    s_whole = _np(eng.forward(*args, thresholds=0.0, want_all=True, whole_layers=True).all_crit).astype(np.float64)
    s_x = _np(eng.forward(*args, thresholds=0.0, want_all=True).all_crit).astype(np.float64)
    assert any(eng.layer_plan()["docs_probe"]), "no layer was probed: the default schedule did not run"
    d = float(np.abs(s_x - s_whole).max())
    report_measured(f"lte[{name}]", "max |score(X-space probe) - score(whole layers)|", d)
    dump = eng.forward(*args, dump_all=True, want_all=True, want_hidden_cls=True, whole_layers=True)
    al = _np(dump.all_logits)
    assert np.array_equal(_np(dump.all_crit).astype(np.float64), s_whole)
    want = lte_scores(_np(dump.hidden_cls), W[W_NAME], W[B_NAME], ec.encoder_exit_layers, n_emb)
    thr, width = gap_thresholds(want, QUANTILE, max(10.0 * d, MIN_GAP), n_emb)
    assert np.all(width >= 10.0 * d)
    ex = lte_exits(s_whole, thr, n_emb)
    _guards(ex, n_emb, E, name)
    o = eng.forward(*args, thresholds=thr)
    eng.check()
    assert np.array_equal(_np(o.exit_layer), ex)
    err = float(np.abs(_np(o.logits).astype(np.float64) - al[ex, np.arange(B)]).max())
    report_measured(f"lte[{name}]", "max |dlogit| X-space probe vs dump-all", err)
    assert err < 1e-4
    assert eng.stage_counts()["docs"] == [int((ex >= e).sum()) for e in range(E + 1)]
    eng.close()


@pytest.mark.parametrize("B", [1, 5])
def test_captured_graph_replays_return_the_eager_bits(pkg, B):
    """use_lte is bound at ee_create, thresholds come from the device vector of each launch: replays with two different threshold vectors
    equal eager forwards with those vectors, bit for bit."""
    name = "h256_gate_1layer_emb_k10_temps"
    cfg, twin, W, docs, tm = make_case(pkg, name)
    ec = cfg.exit_config
    n_emb = len(ec.embedding_exits)
    five = {k: v[:5] for k, v in docs.items()}
    eng, ref = _engine(pkg, cfg, W, five), _engine(pkg, cfg, W, five)
    dump = ref.forward(*_args(five), dump_all=True, want_all=True, whole_layers=True, temperatures=tm)
    thr_a, _ = gap_thresholds(_np(dump.all_crit), 0.6, MIN_GAP, n_emb)      # midpoints between the five documents' scores
    thr_b = np.zeros_like(thr_a)                                            # releases nobody
    args = _args(five, slice(0, B))
    cap = eng.capture(*[x.clone() for x in args], thresholds=thr_a, temperatures=tm)
    e0 = ref.forward(*args, thresholds=thr_a, temperatures=tm)
    for f in ("logits", "exit_layer", "confidence"):
        assert np.array_equal(_np(getattr(cap.outputs, f)), _np(getattr(e0, f))), f
    seen = []
    for thr in (thr_b, thr_a, thr_b):
        out = cap.launch(thresholds=thr, temperatures=tm)
        want = ref.forward(*args, thresholds=thr, temperatures=tm)
        for f in ("logits", "exit_layer", "confidence"):
            assert np.array_equal(_np(getattr(out, f)), _np(getattr(want, f))), (B, f)
        seen.append(_np(out.exit_layer).copy())
    if B == 5:
        assert not np.array_equal(seen[0], seen[1])                         # the threshold vector of the launch matters
    eng.check()
    cap.close()
    eng.close()
    ref.close()


@pytest.mark.parametrize("name", ["h256_gate_1layer_emb_k10_temps", "base_ramp_2layer_k16"])
def test_a_thresholded_lte_forward_issues_no_more_launches_than_its_twin(pkg, name):
    """The score rides in the launch of the head's output projection: the summed launches of ee_profile_read are not more than those of the
    same call on the twin handle without use_lte (default schedule, and whole layers)."""
    cfg, twin, W, docs, tm = make_case(pkg, name)
    args = _args(docs)
    counts = {}
    for tag, c in (("lte", cfg), ("twin", twin)):
        eng = _engine(pkg, c, W, docs)
        for sched in ("default", "whole"):
            eng.profile(True)
            eng.forward(*args, thresholds=0.5, temperatures=tm, whole_layers=sched == "whole")
            prof = eng.profile_read()
            eng.profile(False)
            counts[tag, sched] = sum(v["launches"] for v in prof.values())
            if tag == "lte":
                assert prof["head_out"]["launches"] > 0
        eng.check()
        eng.close()
    for sched in ("default", "whole"):
        report_measured(f"lte[{name},{sched}]", "profiled launches (lte, twin)", float(counts["lte", sched]))
        assert 0 < counts["lte", sched] <= counts["twin", sched], (sched, counts)


# ---- dumped arrays --------------------------------------------------------------------------------------------------------------------------
STORE_CASES = [(2, 1000, 2), (7, 40000, 10), (24, 5000, 16)]


def _planted(E1, N, K, seed):
    """Scores in (0, 1), per-exit thresholds, and exact ties u == thr planted in a tenth of the entries (a tie must NOT leave)."""
    rng = np.random.default_rng(seed)
    scores = rng.random((E1, N))
    thr = rng.uniform(0.05, 0.4, E1)
    tie = rng.random((E1, N)) < 0.1
    scores[tie] = np.broadcast_to(thr[:, None], (E1, N))[tie]
    return scores, rng.standard_normal((E1, N, K)), thr


@pytest.mark.parametrize("E1,N,K", STORE_CASES)
def test_lte_scan_and_policy_vs_restatement(pkg, E1, N, K):
    import torch
    scores, logits, thr = _planted(E1, N, K, seed=E1 * 100 + K)
    ex, pred, counts = lte_policy(scores, logits, thr)
    assert int((scores[:-1] == thr[:-1, None]).sum()) > 0
    g_ex, g_pred, g_counts = pkg.lte_scan_device(torch.from_numpy(scores).cuda(), torch.from_numpy(logits).cuda(), thr)
    assert np.array_equal(_np(g_ex), ex) and np.array_equal(_np(g_pred), pred) and np.array_equal(_np(g_counts), counts)
    for conf in ({"lte_thresholds": thr}, {"exit_threshold": float(thr[0])}):
        conf = dict(conf, exit_policy="lte_policy", lte_scores=scores)
        t = conf.get("lte_thresholds", conf.get("exit_threshold"))
        ex, pred, counts = lte_policy(scores, logits, t)
        exits_store, predictions, dist = getattr(pkg.Policy(logits=logits, config=conf), conf["exit_policy"])()
        assert exits_store.dtype == np.int32 and np.array_equal(exits_store, ex)
        assert predictions.dtype == torch.float64 and np.array_equal(_np(predictions), pred)
        assert dist == {e: int(counts[e]) / N for e in range(E1)}


@pytest.mark.parametrize("E1,N,V", [(7, 4000, 50), (7, 600, 300), (24, 1500, 40)])
def test_lte_sweep_vs_numpy(pkg, E1, N, V):
    """sweep.lte_sweep evaluates u <= thr (non-strict), first exit, 0 when none: numpy with <=, planted ties included.  Both kernels behind
    ee_threshold_sweep: the direct one (histogram) and the ranked one (enough vectors)."""
    rng = np.random.default_rng(E1 + V)
    scores = rng.random((E1, N))
    correct = (rng.random((E1, N)) < 0.6).astype(np.uint8)
    thr = rng.uniform(0.0, 0.5, (V, E1))
    thr[:, ::3] = scores[::3, :V].T                               # exact ties with some document's score
    acc, mex, hist = [], [], []
    for v in range(V):
        ex = (scores <= thr[v][:, None]).argmax(0)
        acc.append(int(correct[ex, np.arange(N)].sum()) / N)
        mex.append(int(ex.sum()) / N)
        hist.append(np.bincount(ex, minlength=E1))
    g_acc, g_mex, g_hist = pkg.sweep.lte_sweep(scores, correct, thr, want_hist=True)
    assert np.array_equal(_np(g_hist), np.array(hist)) and np.array_equal(_np(g_acc), np.array(acc)) and np.array_equal(_np(g_mex), np.array(mex))
    g_acc2, g_mex2, none = pkg.sweep.lte_sweep(scores, correct, thr)
    assert none is None and np.array_equal(_np(g_acc2), np.array(acc)) and np.array_equal(_np(g_mex2), np.array(mex))


def test_model_forward_fills_lte_output_and_early_exit_takes_the_global_threshold(pkg):
    import torch
    name = "tiny_ramp_2layer_emb_k16"
    cfg, twin, W, docs, tm = make_case(pkg, name)
    ec = cfg.exit_config
    n_emb, E = len(ec.embedding_exits), ec.num_exits
    small = {k: v[:12] for k, v in docs.items() if k != "labels"}
    t = {k: torch.from_numpy(v).cuda() for k, v in small.items()}
    args = (t["input_ids"], t["attention_mask"], t["bbox"], t["pixel_values"])
    eng = _engine(pkg, cfg, W, small)
    dump = eng.forward(*args, dump_all=True, want_all=True, want_head=True)
    # a global threshold in a gap of the pooled encoder-exit scores that releases about half of the first exit's documents
    ac = _np(dump.all_crit)
    thr, _ = gap_thresholds(ac, 0.5, MIN_GAP, n_emb)
    g = float(thr[n_emb])
    assert float(np.abs(ac[n_emb:E] - g).min()) > 1e-6
    import dataclasses
    cfg_g = dataclasses.replace(cfg, EE_config=dict(cfg.EE_config, global_threshold=g))
    m = pkg.LayoutLMv3EEForSequenceClassification(cfg_g, weights=W, max_docs=12, max_text_len=small["input_ids"].shape[1])
    assert m.config.exit_config["use_lte"] is True
    out = m.forward(**t)
    assert len(out.lte_output) == len(ec.encoder_exit_layers) == E - n_emb
    for j, u in enumerate(out.lte_output):
        assert tuple(u.shape) == (12,) and np.array_equal(_np(u), ac[n_emb + j])
    assert len(out.exit_states) == E and len(out.exit_criteria) == 1
    for j in range(E):
        assert np.array_equal(_np(out.exit_states[j][0]), _np(dump.head_logits[j])) and np.array_equal(_np(out.exit_states[j][1]), _np(dump.head_crit[j]))
    got = m.early_exit(**t)                                        # thresholds default to the global threshold; B <= 16 runs whole layers
    want = eng.forward(*args, thresholds=g, whole_layers=True)
    ex = lte_exits(ac, g, n_emb)
    assert np.array_equal(_np(want.exit_layer), ex) and 0 < int((ex < E).sum())
    for f in ("logits", "exit_layer", "confidence"):
        assert np.array_equal(_np(getattr(got, f)), _np(getattr(want, f))), f
    plain = pkg.LayoutLMv3EEForSequenceClassification(twin, weights=W, max_docs=12, max_text_len=small["input_ids"].shape[1])
    assert plain.forward(**t).lte_output is None
    for e in (m.engine, plain.engine, eng):
        e.close()


def test_refusals_name_their_cause(pkg):
    name = "tiny_ramp_2layer_emb_k16"
    cfg, twin, W, docs, tm = make_case(pkg, name)
    with pytest.raises(pkg.capi.MMEEError, match="use_lte.*LAYOUTLMV3"):
        pkg.EarlyExitEngine(pkg.ModelConfig.dit_tiny(EE_config=dict(DIT_EE, use_lte=True)), max_docs=4)
    with pytest.raises(pkg.capi.MMEEError, match="use_lte.*PATIENCE"):
        pkg.EarlyExitEngine(pkg.ModelConfig.tiny(EE_config=dict(cfg.EE_config, inference_strategy="patience", patience=2), num_labels=16),
                            max_docs=4, max_text_len=16)
    eng = pkg.EarlyExitEngine(cfg, max_docs=4, max_text_len=16)
    with pytest.raises(pkg.capi.MMEEError, match="PATIENCE.*use_lte"):
        eng.set_criterion("patience")
    assert str(eng.exit_config.inference_strategy) == "max_confidence"
    eng.set_criterion("entropy")                                   # the handle's criterion only feeds out_head_crit under LTE: allowed
    without = {k: v for k, v in W.items() if "lte_classifier" not in k}
    with pytest.raises(KeyError, match="lte_classifier"):
        eng.load_weights(without, strict=True)
    with pytest.raises(pkg.capi.MMEEError, match="lte_classifier"):
        eng.load_weights(without, strict=False)                    # ee_finalize names what was never loaded
    eng.close()
