"""Patience-based early exit (PABEE, include/mmee.h MMEE_CRIT_PATIENCE) on the MI355X: the policy scan and the patience sweep on dumped
arrays, and the decision inside the forward pass, against the numpy restatement of tests/patience_ref.py (the reference declares the
strategy but implements none, so the restatement is the oracle) and against the path's own dump-all rows."""
import numpy as np
import pytest

from .conftest import DIT_EE, H256_KW, report_measured
from .patience_ref import patience_exits, patience_policy, patience_sweep

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _planted_store(E1, N, K, seed):
    """Random (E1, N, K) float64 logits with long runs of one class (a third of the documents, over random spans of exits) and exact ties
    (a tenth of the rows copy their maximum to another label, which wins when it comes first)."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((E1, N, K))
    runs = rng.random(N) < 0.35
    cls = rng.integers(0, K, N)
    lo = rng.integers(0, E1, N)
    hi = lo + rng.integers(1, E1 + 1, N)
    e = np.arange(E1)[:, None]
    boost = (e >= lo) & (e < hi) & runs
    s[np.broadcast_to(e, (E1, N)), np.broadcast_to(np.arange(N), (E1, N)), np.broadcast_to(cls, (E1, N))] += 4.0 * boost
    am = s.argmax(-1)
    tie = rng.random((E1, N)) < 0.1
    other = rng.integers(0, K, (E1, N))
    ee, nn = np.nonzero(tie)
    s[ee, nn, other[ee, nn]] = s[ee, nn, am[ee, nn]]
    return s, rng.integers(0, K, N).astype(np.int64)


STORE_CASES = [(2, 1000, 2), (7, 40000, 10), (24, 5000, 16)]


@pytest.mark.parametrize("E1,N,K", STORE_CASES)
def test_patience_scan_and_policy_vs_restatement(pkg, E1, N, K):
    import torch
    store, _ = _planted_store(E1, N, K, seed=E1 * 100 + K)
    dev = torch.from_numpy(store).cuda()
    for t in range(1, E1 + 2):
        ex, pred, conf, counts = patience_policy(store, t)
        g_ex, g_pred, g_conf, g_counts = pkg.patience_scan_device(dev, t, want_conf=True)
        assert np.array_equal(_np(g_ex), ex), t
        assert np.array_equal(_np(g_pred), pred), t
        assert np.array_equal(_np(g_counts), counts), t
        np.testing.assert_allclose(_np(g_conf), conf, rtol=1e-14, atol=0)
    # Policy, dispatched as EE/eval.py:91-98 does, at a few patience values
    for t in sorted({1, 2, E1 - 1, E1} - {0}):
        cfg = {"exit_policy": "patience_policy", "patience": t}
        exits_store, predictions, dist = getattr(pkg.Policy(logits=store, config=cfg), cfg["exit_policy"])()
        ex, pred, _, counts = patience_policy(store, t)
        assert exits_store.dtype == np.int32 and np.array_equal(exits_store, ex)
        assert predictions.dtype == torch.float64 and np.array_equal(_np(predictions), pred)
        assert dist == {e: int(counts[e]) / N for e in range(E1)}


@pytest.mark.parametrize("E1,N,K", STORE_CASES)
def test_patience_sweep_vs_restatement(pkg, E1, N, K):
    store, refs = _planted_store(E1, N, K, seed=E1 * 100 + K + 1)
    pats = list(range(1, E1 + 2)) + [1, 3 * E1]
    acc, mex, hist, hits, sums = patience_sweep(store, refs, pats)
    g_acc, g_mex, g_hist = pkg.sweep.patience_sweep(store, refs, pats, want_hist=True)
    assert np.array_equal(_np(g_hist), hist)
    assert np.array_equal(_np(g_acc), hits / N) and np.array_equal(_np(g_mex), sums / N)
    g_acc2, g_mex2, none = pkg.sweep.patience_sweep(store, refs, pats)
    assert none is None and np.array_equal(_np(g_acc2), _np(g_acc)) and np.array_equal(_np(g_mex2), _np(g_mex))


# ---- the decision inside the forward pass --------------------------------------------------------------------------------------------------
ENGINE_CASES = {
    "ramp_2layer_emb": (dict(exits=["vision_avg", "text_avg", "text_visual_concat", 1, 2, 3, 4], encoder_layer_strategy="ramp"), 16, False),
    "gate_1layer_k10_temps": (dict(exits=["text_visual_concat", 1, 2, 3], encoder_layer_strategy="gate", exit_head_num_layers=1), 10, True),
    "ramp_1layer_k10_temps": (dict(exits=["text_avg", 1, 2, 3], encoder_layer_strategy="ramp", exit_head_num_layers=1), 10, True),
}
T_TINY = 16


def _shared_heads(W):
    """Every encoder exit head takes the final classifier's parameters (a model whose exits share one classifier, as in PABEE): the
    predictions of consecutive exits then agree often enough for runs to form, which the independent random heads of synth rarely do."""
    W = dict(W)
    for k in list(W):
        if ".early_exits." in k:
            src = "classifier" + k[k.index(".", k.index(".early_exits.") + len(".early_exits.")):]
            if src in W and W[src].shape == W[k].shape:
                W[k] = W[src].copy()
    return W


def _tiny(pkg, name, patience=None, strategy="patience"):
    ee, K, temps = ENGINE_CASES[name]
    ee = dict(ee, inference_strategy=strategy)
    if patience is not None:
        ee["patience"] = patience
    cfg = pkg.ModelConfig.tiny(EE_config=ee, num_labels=K)
    W = _shared_heads(pkg.synth.make_weights(cfg, seed=70 + K, head_gain=4.0))
    E1 = cfg.exit_config.num_exits + 1
    tm = np.random.default_rng(K).uniform(0.5, 3.0, E1) if temps else None
    return cfg, W, tm


def _docs(pkg, cfg, B, seed, T=T_TINY):
    d = pkg.synth.make_documents(cfg, B, seed=seed, text_len=T, min_words=2)
    return d["input_ids"], d["attention_mask"], d["bbox"], d["pixel_values"]


def _check_against_dump(eng, args, temps, ts, tag, **kw):
    """Exits of early exit under patience t == restatement of the dump-all rows; logits / confidences bit-identical to those rows."""
    dump = eng.forward(*args, dump_all=True, want_all=True, whole_layers=True, temperatures=temps)
    al, ac = _np(dump.all_logits), _np(dump.all_crit)
    B = al.shape[1]
    outs = {}
    for t in ts:
        ex = patience_exits(al.astype(np.float64), t)
        o = eng.forward(*args, temperatures=temps, patience=t, **kw)
        got = _np(o.exit_layer)
        assert np.array_equal(got, ex), (tag, t, int((got != ex).sum()))
        assert np.array_equal(_np(o.logits), al[ex, np.arange(B)]), (tag, t)
        assert np.array_equal(_np(o.confidence), ac[ex, np.arange(B)]), (tag, t)
        outs[t] = o
    eng.check()
    return outs


@pytest.mark.parametrize("name", list(ENGINE_CASES))
def test_engine_patience_equals_dump_all_restatement(pkg, name):
    """Ramp and gate, 1- and 2-layer heads, embedding exits, temperatures, K = 10 and 16; B = 1, 17 and 1100 (the decide loop takes two
    chunks of 1024); t = 1, 2, 3 and E + 1.  Whole layers: bit-identical to the dump-all rows; probe-first: bit-identical to whole layers."""
    import torch
    cfg, W, temps = _tiny(pkg, name)
    E1 = cfg.exit_config.num_exits + 1
    eng = pkg.EarlyExitEngine(cfg, max_docs=1100, max_text_len=T_TINY, xprobe=False)
    eng.load_weights(W)
    ts = (1, 2, 3, E1)
    for B in (1, 17, 1100):
        args = tuple(torch.from_numpy(x).cuda() for x in _docs(pkg, cfg, B, seed=B))
        whole = _check_against_dump(eng, args, temps, ts, f"{name} B={B}", whole_layers=True)
        for t in ts:
            p = eng.forward(*args, temperatures=temps, patience=t, probe_always=True)
            for f in ("logits", "exit_layer", "confidence"):
                assert np.array_equal(_np(getattr(p, f)), _np(getattr(whole[t], f))), (name, B, t, f)
        if B == 1100:
            for t in ts:
                early = int((_np(whole[t].exit_layer) < E1 - 1).sum())
                report_measured(f"patience[{name},B=1100,t={t}]", "documents leaving before the final exit", float(early))
            assert int((_np(whole[1].exit_layer) < E1 - 1).sum()) > 0       # documents leave early: the compaction really ran
    eng.close()


def test_engine_patience_split_precision_and_xprobe_at_base_shape(pkg):
    """The bench configuration (LayoutLMv3-base, exits [2,4,6,8,10], ramp, 2-layer heads) at B = 256: whole layers exactly the dump-all
    restatement; the DEFAULT engine (X-space probe) within 1e-4 on logits, exits equal wherever the top-2 margin exceeds 1e-4 at every exit
    the document reaches; engine.check() clean."""
    import torch
    ee = dict(exits=[2, 4, 6, 8, 10], encoder_layer_strategy="ramp", inference_strategy="patience", patience=2)
    cfg = pkg.ModelConfig.base(EE_config=ee)
    W = _shared_heads(pkg.synth.make_weights(cfg, seed=1234, head_gain=6.0))
    B = 256
    docs = pkg.synth.make_documents(cfg, B, seed=9, text_len=512)
    args = tuple(torch.from_numpy(docs[k]).cuda() for k in ("input_ids", "attention_mask", "bbox", "pixel_values"))
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=512)
    assert eng.precision == "split" and eng.xprobe_default and eng.patience == 2
    eng.load_weights(W)
    first = eng.forward(*args)                                # the patience of EE_config, the default schedule
    _check_against_dump(eng, args, None, (1, 2, 3), "base whole layers", whole_layers=True)
    dump = eng.forward(*args, dump_all=True, want_all=True, whole_layers=True)
    al = _np(dump.all_logits).astype(np.float64)
    srt = np.sort(al, axis=-1)
    margin = srt[..., -1] - srt[..., -2]                      # (E1, B)
    for t in (1, 2, 3):
        ex = patience_exits(al, t)
        o = eng.forward(*args, patience=t)
        eng.check()
        if t == 2:
            assert np.array_equal(_np(o.exit_layer), _np(first.exit_layer)) and np.array_equal(_np(o.logits), _np(first.logits))
        got = _np(o.exit_layer)
        reached = np.arange(al.shape[0])[:, None] <= np.maximum(ex, got)[None, :]
        clear = np.all((margin > 1e-4) | ~reached, axis=0)
        report_measured(f"patience[base xprobe,B=256,t={t}]", "documents excluded by the 1e-4 top-2 margin", float((~clear).sum()))
        assert np.array_equal(got[clear], ex[clear]), (t, int((got[clear] != ex[clear]).sum()))
        same = got == ex
        err = float(np.abs(_np(o.logits)[same] - al[ex[same], np.arange(B)[same]]).max())
        report_measured(f"patience[base xprobe,B=256,t={t}]", "max|dlogit| vs dump-all", err)
        assert err < 1e-4
    eng.close()


def test_dit_patience_equals_dump_all_restatement(pkg):
    import torch
    cfg = pkg.ModelConfig.dit_tiny(EE_config=dict(DIT_EE, inference_strategy="patience"))
    W = pkg.synth.make_weights_beit(cfg, seed=5, head_gain=4.0)
    px = torch.from_numpy(pkg.synth.make_documents(cfg, 40, seed=6, text_len=8)["pixel_values"]).cuda()
    eng = pkg.EarlyExitEngine(cfg, max_docs=40)
    eng.load_weights(W)
    E1 = cfg.exit_config.num_exits + 1
    dump = eng.forward(pixel_values=px, dump_all=True, want_all=True, whole_layers=True)
    al, ac = _np(dump.all_logits), _np(dump.all_crit)
    for t in range(1, E1 + 1):
        ex = patience_exits(al.astype(np.float64), t)
        o = eng.forward(pixel_values=px, patience=t, whole_layers=True)
        assert np.array_equal(_np(o.exit_layer), ex), t
        assert np.array_equal(_np(o.logits), al[ex, np.arange(40)]) and np.array_equal(_np(o.confidence), ac[ex, np.arange(40)])
    m = pkg.DiTEEForImageClassification(cfg, W, max_docs=40)
    with pytest.raises(ValueError):
        m.early_exit(pixel_values=px)                          # no patience anywhere
    r = m.early_exit(pixel_values=px, patience=2, whole_layers=True)
    assert np.array_equal(_np(r.exit_layer), patience_exits(al.astype(np.float64), 2))
    with pytest.raises(NotImplementedError):
        m(pixel_values=px)
    m.engine.close()
    eng.close()


def test_micro_batched_engine_gives_the_single_engine_bits(pkg):
    import torch
    cfg, W, temps = _tiny(pkg, "ramp_2layer_emb", patience=2)
    one = pkg.EarlyExitEngine(cfg, max_docs=40, max_text_len=T_TINY)
    two = pkg.MicroBatchedEngine(cfg, max_docs=40, max_text_len=T_TINY, micro_batches=2)
    one.load_weights(W)
    two.load_weights(W)
    args = tuple(torch.from_numpy(x).cuda() for x in _docs(pkg, cfg, 33, seed=4))
    for t in (2, 1, 3):
        a = one.forward(*args, patience=t if t != 2 else None)
        b = two.forward(*args, patience=t if t != 2 else None)
        for f in ("logits", "exit_layer", "confidence"):
            assert np.array_equal(_np(getattr(a, f)), _np(getattr(b, f))), (t, f)
    two.check()
    one.close()
    two.close()


def test_captured_graph_reads_the_patience_of_each_launch(pkg):
    """Captured at t = 2, replayed at t = 1, 3, 2 with fresh inputs copied into the graph's buffers: each replay equals an eager forward
    at that t (the patience is not baked into the graph)."""
    import torch
    cfg, W, temps = _tiny(pkg, "gate_1layer_k10_temps")
    B = 17
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T_TINY)
    ref = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T_TINY)
    eng.load_weights(W)
    ref.load_weights(W)
    first = tuple(torch.from_numpy(x).cuda() for x in _docs(pkg, cfg, B, seed=20))
    cap = eng.capture(*[x.clone() for x in first], temperatures=temps, patience=2)
    e0 = ref.forward(*first, temperatures=temps, patience=2)
    assert np.array_equal(_np(cap.outputs.exit_layer), _np(e0.exit_layer))
    keys = ("input_ids", "attention_mask", "bbox", "pixel_values")
    differs = False
    for i, t in enumerate((1, 3, 2)):
        new = tuple(torch.from_numpy(x).cuda() for x in _docs(pkg, cfg, B, seed=21 + i))
        for k, x in zip(keys, new):
            cap.inputs[k].copy_(x)
        out = cap.launch(temperatures=temps, patience=t)
        want = ref.forward(*new, temperatures=temps, patience=t)
        for f in ("logits", "exit_layer", "confidence"):
            assert np.array_equal(_np(getattr(out, f)), _np(getattr(want, f))), (t, f)
        other = ref.forward(*new, temperatures=temps, patience=2 if t != 2 else 1)
        differs |= not np.array_equal(_np(other.exit_layer), _np(want.exit_layer))
    assert differs                                             # the patience of the launch matters for these inputs
    eng.check()
    cap.close()
    eng.close()
    ref.close()


def test_no_state_leaks_between_forwards_or_criteria(pkg):
    """max_confidence at B = 17, patience at B = 9, max_confidence at B = 17 again on ONE handle: the third forward equals the first bit for
    bit and the patience forward equals a fresh handle's.  Also the refusals: no patience set, t < 1."""
    import torch
    cfg, W, temps = _tiny(pkg, "ramp_2layer_emb", strategy="max_confidence")
    eng = pkg.EarlyExitEngine(cfg, max_docs=17, max_text_len=T_TINY)
    eng.load_weights(W)
    args = tuple(torch.from_numpy(x).cuda() for x in _docs(pkg, cfg, 17, seed=30))
    small = tuple(x[:9].contiguous() for x in args)
    dump = eng.forward(*args, dump_all=True, want_all=True)
    conf = np.sort(_np(dump.all_crit).ravel())
    thr = float(0.5 * (conf[len(conf) // 2] + conf[len(conf) // 2 + 1]))
    a = eng.forward(*args, thresholds=thr)
    eng.set_criterion("patience")
    with pytest.raises(pkg.capi.MMEEError, match="ee_set_patience"):
        eng.forward(*small)
    with pytest.raises(ValueError):
        eng.set_patience(0)
    assert eng.lib.ee_set_patience(eng._h, 0) != 0
    b = eng.forward(*small, patience=2)
    eng.set_criterion("max_confidence")
    c = eng.forward(*args, thresholds=thr)
    fresh = pkg.EarlyExitEngine(pkg.ModelConfig.tiny(EE_config=dict(cfg.EE_config, inference_strategy="patience", patience=2),
                                                     num_labels=cfg.num_labels), max_docs=17, max_text_len=T_TINY)
    fresh.load_weights(W)
    d = fresh.forward(*small)
    for f in ("logits", "exit_layer", "confidence"):
        assert np.array_equal(_np(getattr(a, f)), _np(getattr(c, f))), f
        assert np.array_equal(_np(getattr(b, f)), _np(getattr(d, f))), f
    eng.check()
    eng.close()
    fresh.close()


def test_model_wrapper_under_patience(pkg):
    import torch
    ee = dict(exits=["text_avg", 1, 2, 3], encoder_layer_strategy="ramp", inference_strategy="patience", patience=2, exit_head_num_layers=1)
    cfg = pkg.ModelConfig.tiny(EE_config=ee, **H256_KW)
    W = pkg.synth.make_weights(cfg, seed=8, head_gain=4.0)
    docs = pkg.synth.make_documents(cfg, 6, seed=9, text_len=48, min_words=3)
    t = {k: torch.from_numpy(v).cuda() for k, v in docs.items() if k != "labels"}
    m = pkg.LayoutLMv3EEForSequenceClassification(cfg, weights=W, max_docs=8, max_text_len=48)
    eng = pkg.EarlyExitEngine(cfg, max_docs=8, max_text_len=48)
    eng.load_weights(W)
    args = (t["input_ids"], t["attention_mask"], t["bbox"], t["pixel_values"])
    want = eng.forward(*args, whole_layers=True)             # B <= 16: the wrapper runs whole layers
    got = m.early_exit(**t)
    for f in ("logits", "exit_layer", "confidence"):
        assert np.array_equal(_np(getattr(got, f)), _np(getattr(want, f))), f
    got3, want3 = m.early_exit(**t, patience=3), eng.forward(*args, whole_layers=True, patience=3)
    assert np.array_equal(_np(got3.exit_layer), _np(want3.exit_layer))
    with pytest.raises(NotImplementedError):
        m.forward(**t)
    m.config.exit_config["patience"] = None
    with pytest.raises(ValueError):
        m.early_exit(**t)
    # back to max_confidence: the results of a model built that way
    m.config.exit_config["inference_strategy"] = "max_confidence"
    built = pkg.LayoutLMv3EEForSequenceClassification(pkg.ModelConfig.tiny(EE_config=dict(ee, inference_strategy="max_confidence"), **H256_KW),
                                                      weights=W, max_docs=8, max_text_len=48)
    a, b = m.early_exit(**t), built.early_exit(**t)
    for f in ("logits", "exit_layer", "confidence"):
        assert np.array_equal(_np(getattr(a, f)), _np(getattr(b, f))), f
    out = m.forward(**t)
    assert len(out.exit_states) == 4
    m.engine.close()
    built.engine.close()
    eng.close()
