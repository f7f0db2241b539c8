"""The two combined exit rules (include/mmee.h MMEE_RULE_STREAK "patient and confident", MMEE_RULE_EITHER "patience or threshold") on the
MI355X: the scan and the sweep on dumped arrays, and the decision inside the forward pass, against the numpy restatement of
tests/rule_ref.py (the reference implements neither rule, so the restatement is the oracle) and against the path's own dump-all rows.
Every comparison is exact unless it says otherwise."""
import numpy as np
import pytest

from .conftest import DIT_EE, H256_KW, report_measured
from .lte_ref import gap_thresholds, lte_scores
from .patience_ref import patience_exits
from .rule_ref import EITHER, RULE_NAMES, STREAK, msp_table, plain_exits, rule_exits, rule_policy, rule_sweep

pytestmark = pytest.mark.gpu

RULES = (STREAK, EITHER)


def _np(t):
    return t.detach().cpu().numpy()


def _planted_store(E1, N, K, seed):
    """Random (E1, N, K) float64 logits with long runs of one class (a third of the documents, over random spans of exits) and exact ties
    (a tenth of the rows copy their maximum to another label, which wins when it comes first): the store of tests/test_gpu_patience.py."""
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


def _entropy_table(store):
    """(E1,N) float64 entropy of softmax(store): a criterion that exits when it is BELOW its threshold (sign -1)."""
    z = store - store.max(-1, keepdims=True)
    p = np.exp(z)
    p /= p.sum(-1, keepdims=True)
    return -(p * np.log(np.maximum(p, 1e-300))).sum(-1)


STORE_CASES = [(2, 1000, 2), (7, 40000, 10), (24, 5000, 16)]
VECTOR = lambda E1: [e % 3 + 1 for e in range(E1)]


# ---- 1. scan and Policy against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E1,N,K", STORE_CASES)
def test_rule_scan_and_policy_vs_restatement(pkg, E1, N, K):
    import torch
    store, _ = _planted_store(E1, N, K, seed=E1 * 100 + K)
    dev = torch.from_numpy(store).cuda()
    # the max-softmax table the Policy builds on the device, against the restatement's: rtol 1e-14 (two exp implementations)
    crit = _np(pkg.sweep.msp_table(store)[0])
    np.testing.assert_allclose(crit, msp_table(store), rtol=1e-14, atol=0)
    tables = {+1: crit, -1: _entropy_table(store)}
    rows = np.arange(N)
    got = {}
    for sign, table in tables.items():
        thr = np.quantile(table, 0.9, axis=1)
        tdev = torch.from_numpy(table).cuda()
        for rule in RULES:
            for t in list(range(1, E1 + 2)) + [VECTOR(E1)]:
                ex, pred, conf, counts = rule_policy(table, store, thr, t, rule, sign)
                g_ex, g_pred, g_conf, g_counts = pkg.rule_scan_device(tdev, dev, thr, t, RULE_NAMES[rule], sign=sign, want_conf=True)
                tag = (sign, rule, t)
                assert np.array_equal(_np(g_ex), ex), (tag, int((_np(g_ex) != ex).sum()))
                assert np.array_equal(_np(g_pred), pred), tag
                assert np.array_equal(_np(g_counts), counts), tag
                np.testing.assert_allclose(_np(g_conf), conf, rtol=1e-14, atol=0)
                if sign > 0:
                    np.testing.assert_allclose(_np(g_conf), msp_table(store)[ex, rows], rtol=1e-14, atol=0)
                got[sign, rule, t if isinstance(t, int) else "vec"] = _np(g_ex)
    # identities on the DEVICE results (confidence sign)
    thr = np.quantile(crit, 0.9, axis=1)
    plain = _np(pkg.policy_scan_device(dev, thr)[0])
    assert np.array_equal(plain, plain_exits(crit, thr, +1))
    assert np.array_equal(got[+1, STREAK, 1], plain)                                            # STREAK at t = 1 is the plain policy scan
    assert np.array_equal(got[+1, EITHER, E1], plain) and np.array_equal(got[+1, EITHER, E1 + 1], plain)     # t > E: the plain scan
    tcrit = torch.from_numpy(crit).cuda()
    for t in range(1, E1 + 1):
        pab = _np(pkg.patience_scan_device(dev, t)[0])
        unreachable = _np(pkg.rule_scan_device(tcrit, dev, 2.0, t, "patience_or_threshold")[0])
        assert np.array_equal(unreachable, pab), t                                               # a threshold no confidence exceeds: PABEE
        assert np.array_equal(got[+1, EITHER, t], np.minimum(plain, pab)), t                    # the minimum of the two
    if N >= 5000:
        # non-degeneracy (checked on the CPU with the restatement at exactly these inputs)
        s2 = got[+1, STREAK, 2]
        early = float((s2 < E1 - 1).mean())
        report_measured(f"rule_scan[{E1},{N},{K}]", "STREAK t=2: share leaving before the final exit", early)
        assert early >= 0.05 and len(np.unique(s2)) >= 5, (early, np.unique(s2))
        pab1 = _np(pkg.patience_scan_device(dev, 1)[0])
        pat_first, thr_first = float((pab1 < plain).mean()), float((plain < pab1).mean())
        report_measured(f"rule_scan[{E1},{N},{K}]", "EITHER t=1: share decided by the agreement first", pat_first)
        report_measured(f"rule_scan[{E1},{N},{K}]", "EITHER t=1: share decided by the threshold first", thr_first)
        assert pat_first >= 0.10 and thr_first >= 0.10
        for rule in RULES:
            for t in (1, 2, 3):
                assert not np.array_equal(got[+1, rule, "vec"], got[+1, rule, t]), (rule, t)
    # Policy, dispatched as EE/eval.py:91-98 does: global and per-exit thresholds, scalar and per-exit patience, LTE scores with sign -1
    for rule in RULES:
        name = RULE_NAMES[rule] + "_policy"
        for cfg, table, th, t, sign in (
                ({"exit_threshold": float(thr[0]), "patience": 2}, crit, float(thr[0]), 2, +1),
                ({"exit_thresholds": thr, "patience": VECTOR(E1)}, crit, thr, VECTOR(E1), +1),
                ({"lte_scores": tables[-1], "lte_thresholds": np.quantile(tables[-1], 0.1, axis=1), "patience": 1}, tables[-1],
                 np.quantile(tables[-1], 0.1, axis=1), 1, -1)):
            cfg = dict(cfg, exit_policy=name)
            exits_store, predictions, dist = getattr(pkg.Policy(logits=store, config=cfg), cfg["exit_policy"])()
            ex, pred, _, counts = rule_policy(table, store, th, t, rule, sign)
            assert exits_store.dtype == np.int32 and np.array_equal(exits_store, ex), (name, sorted(cfg))
            assert predictions.dtype == torch.float64 and np.array_equal(_np(predictions), pred)
            assert dist == {e: int(counts[e]) / N for e in range(E1)}


def test_scans_that_need_no_logits_accept_a_null_pointer(pkg):
    """The C ABI's null paths, which the Python wrappers never take: ee_lte_scan without predictions and ee_rule_scan under MMEE_RULE_STREAK
    without predictions read no logits row, so `logits = NULL` is accepted and gives exactly the exits and counts of the call with the logits;
    MMEE_RULE_EITHER counts argmax agreement and is refused without them.  (3, 70, 4): more than one wave, less than one block, and
    E1 - 1 = 2 exits that carry a test."""
    import ctypes as C
    import torch
    E1, N, K = 3, 70, 4
    PAT = [2, 2, 1]                                  # exit 1 is left only where the test held at exit 0 AND exit 1: the streak is carried
    store, _ = _planted_store(E1, N, K, seed=5)
    crit = msp_table(store)
    thr = np.quantile(crit, 0.6, axis=1)
    lib = pkg.capi.load()
    logits, table = torch.from_numpy(store).cuda(), torch.from_numpy(crit).cuda()
    thr_c, pat_c = (C.c_double * E1)(*thr.tolist()), (C.c_int32 * E1)(*PAT)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def run(call):
        exits = torch.full((N,), -1, dtype=torch.int32, device="cuda")
        counts = torch.full((E1,), -1, dtype=torch.int32, device="cuda")
        rc = call(ptr(exits), ptr(counts))
        return rc, _np(exits), _np(counts)

    lte = lambda lg: run(lambda ex, cn: lib.ee_lte_scan(ptr(table), ptr(lg), E1, N, K, thr_c, ex, None, cn, stream))
    rule = lambda lg, r: run(lambda ex, cn: lib.ee_rule_scan(ptr(table), 1.0, ptr(lg), E1, N, K, thr_c, pat_c, r, ex, None, None, cn, stream))
    for name, with_logits, without in (("ee_lte_scan", lte(logits), lte(None)), ("ee_rule_scan STREAK", rule(logits, STREAK), rule(None, STREAK))):
        assert with_logits[0] == 0 and without[0] == 0, (name, pkg.capi.last_error())
        assert np.array_equal(without[1], with_logits[1]) and np.array_equal(without[2], with_logits[2]), name
        assert without[2].sum() == N and (without[2] > 0).sum() >= 2, (name, without[2])           # the tests decide: not one exit for all
    assert np.array_equal(lte(None)[1], plain_exits(crit, thr, -1))
    assert np.array_equal(rule(None, STREAK)[1], rule_exits(crit, store, thr, PAT, STREAK, +1))
    assert rule(logits, EITHER)[0] == 0
    rc, exits, _ = rule(None, EITHER)
    assert rc != 0 and "logits" in pkg.capi.last_error() and (exits == -1).all()


# ---- 2. sweep against the restatement ------------------------------------------------------------------------------------------------------
def _sweep_inputs(E1, N, K, V, seed):
    """Criterion table with duplicate confidences (a twentieth of the entries copy another document's), V threshold vectors at random
    quantiles of it, a fifth of their entries EXACTLY a table value (the strict compare must not fire there), NaN entries, one all-NaN vector."""
    store, refs = _planted_store(E1, N, K, seed)
    rng = np.random.default_rng(seed + 1)
    crit = msp_table(store)
    dup = rng.random((E1, N)) < 0.05
    src = rng.integers(0, N, (E1, N))
    crit = np.where(dup, np.take_along_axis(crit, src, axis=1), crit)
    q = rng.uniform(0.5, 1.0, (V, E1))
    thr = np.stack([np.quantile(crit[e], q[:, e]) for e in range(E1)], axis=1)
    exact = rng.random((V, E1)) < 0.2
    pick = crit[np.arange(E1)[None, :], rng.integers(0, N, (V, E1))]
    thr = np.where(exact, pick, thr)
    thr[rng.random((V, E1)) < 0.02] = np.nan
    thr[V // 2] = np.nan
    assert int((crit[None] == thr[:, :, None]).sum()) > 0 if V * E1 * N < 5e7 else True
    return store, refs, crit, thr


@pytest.mark.parametrize("E1,N,K", STORE_CASES)
def test_rule_sweep_vs_restatement(pkg, E1, N, K):
    V, pats = 300, list(range(1, E1 + 3))
    store, refs, crit, thr = _sweep_inputs(E1, N, K, V, seed=E1 * 100 + K + 1)
    for rule in RULES:
        hits, sums, hist = rule_sweep(crit, store, refs, thr, pats, rule)
        g_acc, g_mex, g_hist = pkg.sweep.rule_sweep(crit, store, refs, thr, pats, RULE_NAMES[rule], want_hist=True)
        assert tuple(g_acc.shape) == (V, len(pats)) and tuple(g_hist.shape) == (V, len(pats), E1)
        assert np.array_equal(_np(g_hist), hist), rule
        assert np.array_equal(_np(g_acc), hits / N) and np.array_equal(_np(g_mex), sums / N), rule
        g_acc2, g_mex2, none = pkg.sweep.rule_sweep(crit, store, refs, thr, pats, RULE_NAMES[rule])
        assert none is None and np.array_equal(_np(g_acc2), hits / N) and np.array_equal(_np(g_mex2), sums / N), rule
    if E1 > 2:                                            # (c_0 = 0: with one early exit the agreement has nothing to release)
        assert int(hist[V // 2, :, :-1].sum()) > 0        # EITHER under all-NaN thresholds still leaves on the agreement ...
    assert np.all(rule_sweep(crit, store, refs, thr[V // 2:V // 2 + 1], pats, STREAK)[2][0, :, -1] == N)   # ... STREAK never does
    # the '<' sign: negated table and thresholds give the same sums
    g = pkg.sweep.rule_sweep(-crit, store, refs, -thr, pats, "patient_confident", sign=-1.0)
    h = rule_sweep(crit, store, refs, thr, pats, STREAK)
    assert np.array_equal(_np(g[0]), h[0] / N) and np.array_equal(_np(g[1]), h[1] / N)


@pytest.mark.parametrize("N,P", [(2000, 7), (2389, 8), (500, 1)])
def test_rule_sweep_on_integer_ranks_vs_restatement(pkg, N, P):
    """The reference's search shape (E1 = 7, P <= 8, no histogram, enough vectors): the one-thread-per-vector kernel on integer ranks.  Same
    planted duplicates, exact ties and NaN thresholds; patience values out of order, repeated, and beyond E."""
    E1, K, V = 7, 10, 300
    store, refs, crit, thr = _sweep_inputs(E1, N, K, V, seed=N)
    pats = [3, 1, 2, 7, 1, 6, 4, 5][:P]
    assert V * 8 >= N
    for rule in RULES:
        hits, sums, hist = rule_sweep(crit, store, refs, thr, pats, rule)
        g_acc, g_mex, none = pkg.sweep.rule_sweep(crit, store, refs, thr, pats, RULE_NAMES[rule])
        assert none is None
        assert np.array_equal(_np(g_acc), hits / N), (rule, int((_np(g_acc) != hits / N).sum()))
        assert np.array_equal(_np(g_mex), sums / N), (rule, int((_np(g_mex) != sums / N).sum()))
        d_acc, d_mex, d_hist = pkg.sweep.rule_sweep(crit, store, refs, thr, pats, RULE_NAMES[rule], want_hist=True)     # the direct kernel
        assert np.array_equal(_np(d_acc), _np(g_acc)) and np.array_equal(_np(d_mex), _np(g_mex)) and np.array_equal(_np(d_hist), hist)


# ---- 3. inside the forward -----------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_patience.py
ENGINE_CASES = {
    "ramp_2layer_emb": (dict(exits=["vision_avg", "text_avg", "text_visual_concat", 1, 2, 3, 4], encoder_layer_strategy="ramp"), 16, False),
    "gate_1layer_k10_temps": (dict(exits=["text_visual_concat", 1, 2, 3], encoder_layer_strategy="gate", exit_head_num_layers=1), 10, True),
    "ramp_1layer_k10_temps": (dict(exits=["text_avg", 1, 2, 3], encoder_layer_strategy="ramp", exit_head_num_layers=1), 10, True),
}
T_TINY = 16
QUANTILE = 0.9       # of the dump-all criteria: where the per-exit thresholds sit
MIN_GAP = 1e-6       # >> 2^-24, the rounding of a stored float32 criterion <= 1: the float64 criterion is on the same side of the threshold
FIELDS = ("logits", "exit_layer", "confidence")


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


def _tiny(pkg, name, strategy="max_confidence", **ee_kw):
    ee, K, temps = ENGINE_CASES[name]
    ee = dict(ee, inference_strategy=strategy, **ee_kw)
    cfg = pkg.ModelConfig.tiny(EE_config=ee, num_labels=K)
    W = _shared_heads(pkg.synth.make_weights(cfg, seed=70 + K, head_gain=4.0))
    E1 = cfg.exit_config.num_exits + 1
    tm = np.random.default_rng(K).uniform(0.5, 3.0, E1) if temps else None
    return cfg, W, tm


def _docs(pkg, cfg, B, seed, T=T_TINY):
    import torch
    d = pkg.synth.make_documents(cfg, B, seed=seed, text_len=T, min_words=2)
    return tuple(torch.from_numpy(d[k]).cuda() for k in ("input_ids", "attention_mask", "bbox", "pixel_values"))


def _thresholds(ac, sign, quantile=QUANTILE):
    """Per-exit thresholds in a gap (>= MIN_GAP wide) of the sorted dump-all criteria, nearest to the quantile that releases the surest
    (1 - quantile) of the documents; one document: 0.01 to one side of its criterion, alternating, so that some exits fire."""
    E1, B = ac.shape
    if B == 1:
        return ac[:, 0].astype(np.float64) + 0.01 * np.where(np.arange(E1) % 2 == 0, 1.0, -1.0)
    thr, width = gap_thresholds(ac.astype(np.float64), quantile if sign > 0 else 1.0 - quantile, MIN_GAP)
    assert np.all(width >= MIN_GAP)
    return thr


def _check_against_dump(eng, args, temps, sign, tag, settings, **kw):
    """Early exit under (rule, patience) == the restatement on the handle's own dump-all criteria and logits; logits / confidences
    bit-identical to those rows.  Returns the dump, the thresholds and {(rule, patience): output}."""
    dump = eng.forward(*args, dump_all=True, want_all=True, whole_layers=True, temperatures=temps)
    al, ac = _np(dump.all_logits), _np(dump.all_crit)
    B = al.shape[1]
    thr = _thresholds(ac, sign)
    outs = {}
    for rule, t in settings:
        ex = rule_exits(ac.astype(np.float64), al.astype(np.float64), thr, t, rule, sign)
        o = eng.forward(*args, thresholds=thr, temperatures=temps, exit_rule=RULE_NAMES[rule], patience=t, **kw)
        got = _np(o.exit_layer)
        assert np.array_equal(got, ex), (tag, rule, t, int((got != ex).sum()))
        assert np.array_equal(_np(o.logits), al[ex, np.arange(B)]), (tag, rule, t)
        assert np.array_equal(_np(o.confidence), ac[ex, np.arange(B)]), (tag, rule, t)
        outs[rule, tuple(t) if isinstance(t, list) else t] = o
    eng.check()
    return (al, ac), thr, outs


@pytest.mark.parametrize("name", list(ENGINE_CASES))
def test_engine_rules_equal_dump_all_restatement(pkg, name):
    """Ramp and gate, 1- and 2-layer heads, embedding exits, temperatures, K = 10 and 16; B = 1, 17 and 1100 (the decide loop takes two
    chunks of 1024); scalar patience 1, 2, 3 and a per-exit vector; shared heads so that runs form.  Whole layers: exits == the restatement
    on the dump-all rows, logits / confidences those rows bit for bit; probe-first bit-identical to whole layers; STREAK at t = 1
    bit-identical to a PLAIN forward; EITHER under an unreachable threshold bit-identical to a MMEE_CRIT_PATIENCE forward."""
    cfg, W, temps = _tiny(pkg, name)
    E1 = cfg.exit_config.num_exits + 1
    eng = pkg.EarlyExitEngine(cfg, max_docs=1100, max_text_len=T_TINY, xprobe=False)
    eng.load_weights(W)
    vec = VECTOR(E1)
    settings = [(rule, t) for rule in RULES for t in (1, 2, 3, vec)]
    for B in (1, 17, 1100):
        args = _docs(pkg, cfg, B, seed=B)
        (al, ac), thr, whole = _check_against_dump(eng, args, temps, +1, f"{name} B={B}", settings, whole_layers=True)
        for rule, t in settings:
            p = eng.forward(*args, thresholds=thr, temperatures=temps, exit_rule=RULE_NAMES[rule], patience=t, probe_always=True)
            for f in FIELDS:
                assert np.array_equal(_np(getattr(p, f)), _np(getattr(whole[rule, tuple(t) if isinstance(t, list) else t], f))), (name, B, rule, t, f)
        plain = eng.forward(*args, thresholds=thr, temperatures=temps, exit_rule="plain", whole_layers=True)
        assert np.array_equal(_np(plain.exit_layer), plain_exits(ac.astype(np.float64), thr, +1))
        for f in FIELDS:
            assert np.array_equal(_np(getattr(whole[STREAK, 1], f)), _np(getattr(plain, f))), (name, B, f)
        # max_confidence never exceeds 1: under thresholds of 2.0 EITHER is PABEE
        either = {t: eng.forward(*args, thresholds=2.0, temperatures=temps, exit_rule="patience_or_threshold", patience=t, whole_layers=True)
                  for t in (1, 2)}
        eng.set_exit_rule("plain")
        eng.set_criterion("patience")
        for t in (1, 2):
            pab = eng.forward(*args, temperatures=temps, patience=t, whole_layers=True)
            assert np.array_equal(_np(pab.exit_layer), patience_exits(al.astype(np.float64), t))
            for f in FIELDS:
                assert np.array_equal(_np(getattr(either[t], f)), _np(getattr(pab, f))), (name, B, t, f)
        eng.set_criterion("max_confidence")
        if B == 1100:
            pl = _np(plain.exit_layer)
            for rule, t in ((STREAK, 2), (EITHER, 1)):
                ex = _np(whole[rule, t].exit_layer)
                differ = float((ex != pl).mean())
                report_measured(f"rule[{name},B=1100,{RULE_NAMES[rule]},t={t}]", "distinct exits documents leave at", float(len(np.unique(ex))))
                report_measured(f"rule[{name},B=1100,{RULE_NAMES[rule]},t={t}]", "share of documents whose exit differs from PLAIN", differ)
                assert len(np.unique(ex)) >= 3, (rule, t, np.bincount(ex, minlength=E1).tolist())
                assert differ >= 0.10, (rule, t, differ)
    eng.close()


def test_engine_rules_under_the_entropy_criterion(pkg):
    """The '<' sign inside the forward: entropy events, both rules, against the restatement on the dump-all entropies."""
    name = "ramp_1layer_k10_temps"
    cfg, W, temps = _tiny(pkg, name, strategy="entropy")
    E1 = cfg.exit_config.num_exits + 1
    eng = pkg.EarlyExitEngine(cfg, max_docs=64, max_text_len=T_TINY, xprobe=False)
    eng.load_weights(W)
    args = _docs(pkg, cfg, 64, seed=3)
    settings = [(rule, t) for rule in RULES for t in (1, 2, VECTOR(E1))]
    _, _, outs = _check_against_dump(eng, args, temps, -1, name, settings, whole_layers=True)
    assert len(np.unique(_np(outs[STREAK, 1].exit_layer))) >= 2
    eng.close()


# ---- 4. base shape, split precision, the default (X-space probe) engine ------------------------------------------------------------------------
def test_engine_rules_split_precision_and_xprobe_at_base_shape(pkg):
    """The bench configuration (LayoutLMv3-base, exits [2,4,6,8,10], ramp, 2-layer heads) at B = 256.  Whole layers: exactly the dump-all
    restatement.  The DEFAULT engine (X-space probe, a re-association): exits equal wherever every exit the document reaches has its
    criterion further than 1e-4 from its threshold and a top-2 margin above 1e-4; logits within 1e-4 of the dump.  At most 5 % of the
    documents may be excluded."""
    ee = dict(exits=[2, 4, 6, 8, 10], encoder_layer_strategy="ramp", inference_strategy="max_confidence")
    cfg = pkg.ModelConfig.base(EE_config=ee)
    W = _shared_heads(pkg.synth.make_weights(cfg, seed=1234, head_gain=6.0))
    B = 256
    args = _docs(pkg, cfg, B, seed=9, T=512)
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=512)
    assert eng.precision == "split" and eng.xprobe_default and str(eng.exit_rule) == "plain"
    eng.load_weights(W)
    settings = [(rule, t) for rule in RULES for t in (1, 2, VECTOR(6))]
    (al, ac), thr, _ = _check_against_dump(eng, args, None, +1, "base whole layers", settings, whole_layers=True)
    al64, ac64 = al.astype(np.float64), ac.astype(np.float64)
    srt = np.sort(al64, axis=-1)
    margin = srt[..., -1] - srt[..., -2]                      # (E1, B)
    away = np.abs(ac64 - thr[:, None])                        # (E1, B)
    for rule, t in settings:
        tag = f"rule[base xprobe,B=256,{RULE_NAMES[rule]},t={t}]"
        ex = rule_exits(ac64, al64, thr, t, rule, +1)
        o = eng.forward(*args, thresholds=thr, exit_rule=RULE_NAMES[rule], patience=t)
        eng.check()
        got = _np(o.exit_layer)
        reached = np.arange(al.shape[0])[:, None] <= np.maximum(ex, got)[None, :]
        clear = np.all(((margin > 1e-4) & (away > 1e-4)) | ~reached, axis=0)
        report_measured(tag, "documents excluded by the 1e-4 margins", float((~clear).sum()))
        assert (~clear).sum() <= 0.05 * B, int((~clear).sum())
        assert np.array_equal(got[clear], ex[clear]), (rule, t, int((got[clear] != ex[clear]).sum()))
        same = got == ex
        err = float(np.abs(_np(o.logits)[same] - al64[ex[same], np.arange(B)[same]]).max())
        report_measured(tag, "max|dlogit| vs dump-all", err)
        assert err < 1e-4
    assert any(eng.layer_plan()["docs_probe"]), "no layer was probed: the default schedule did not run"
    eng.close()


# ---- 5. LTE events ------------------------------------------------------------------------------------------------------------------------------
W_NAME, B_NAME = "layoutlmv3.encoder.lte_classifier.weight", "layoutlmv3.encoder.lte_classifier.bias"
LTE_CASES = {
    "tiny_ramp_2layer_emb_k16": ("tiny", dict(exits=["vision_avg", "text_avg", 1, 2, 3, 4], encoder_layer_strategy="ramp"), 16, False, 40, 16),
    "h256_gate_1layer_emb_k10_temps": ("h256", dict(exits=["text_visual_concat", 1, 2, 3], encoder_layer_strategy="gate", exit_head_num_layers=1),
                                       10, True, 40, 48),
}


@pytest.mark.parametrize("name", list(LTE_CASES))
def test_lte_events_under_both_rules(pkg, name):
    """use_lte handles: the event is u_e < thr_e on the score tests/lte_ref.py restates from the dump's CLS rows (thresholds in gaps of those
    scores; embedding exits never fire but still count agreement).  Whole layers and the K | V probe."""
    import torch
    shape, ee, K, temps, B, T = LTE_CASES[name]
    kw = H256_KW if shape == "h256" else {}
    cfg = pkg.ModelConfig.tiny(EE_config=dict(ee, use_lte=True), num_labels=K, **kw)
    W = _shared_heads(pkg.synth.make_weights(cfg, seed=90 + K, head_gain=4.0))
    ec = cfg.exit_config
    n_emb, E = len(ec.embedding_exits), ec.num_exits
    tm = np.random.default_rng(K).uniform(0.5, 3.0, E + 1) if temps else None
    d = pkg.synth.make_documents(cfg, B, seed=91 + K, text_len=T, min_words=2)
    args = tuple(torch.from_numpy(d[k]).cuda() for k in ("input_ids", "attention_mask", "bbox", "pixel_values"))
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, xprobe=False)
    eng.load_weights(W)
    dump = eng.forward(*args, dump_all=True, want_all=True, want_hidden_cls=True, whole_layers=True, temperatures=tm)
    al, ac = _np(dump.all_logits), _np(dump.all_crit)
    want = lte_scores(_np(dump.hidden_cls), W[W_NAME], W[B_NAME], ec.encoder_exit_layers, n_emb)
    assert float(np.abs(ac.astype(np.float64) - want.astype(np.float32).astype(np.float64)).max()) <= 2.0 ** -23
    thr, width = gap_thresholds(want, 0.35, 1e-5, n_emb)
    assert np.all(width >= 1e-5)
    rows = np.arange(B)
    seen = set()
    for rule in RULES:
        for t in (1, 2, VECTOR(E + 1)):
            ex = rule_exits(ac.astype(np.float64), al.astype(np.float64), thr, t, rule, sign=-1)
            for sched in (dict(whole_layers=True), dict(probe_always=True)):
                o = eng.forward(*args, thresholds=thr, temperatures=tm, exit_rule=RULE_NAMES[rule], patience=t, **sched)
                tag = (name, rule, t, tuple(sched))
                assert np.array_equal(_np(o.exit_layer), ex), (tag, _np(o.exit_layer).tolist(), ex.tolist())
                assert np.array_equal(_np(o.logits), al[ex, rows]) and np.array_equal(_np(o.confidence), ac[ex, rows]), tag
            seen.add(tuple(ex.tolist()))
    plain = _np(eng.forward(*args, thresholds=thr, temperatures=tm, exit_rule="plain", whole_layers=True).exit_layer)
    assert np.array_equal(plain, rule_exits(ac.astype(np.float64), al.astype(np.float64), thr, 1, STREAK, sign=-1))
    assert len(seen) >= 3 and len(np.unique(plain)) >= 3
    eng.check()
    eng.close()


# ---- 6. DiT (BEiT) ---------------------------------------------------------------------------------------------------------------------------------
def test_dit_rules_equal_dump_all_restatement(pkg):
    import torch
    cfg = pkg.ModelConfig.dit_tiny(EE_config=dict(DIT_EE))
    W = pkg.synth.make_weights_beit(cfg, seed=5, head_gain=4.0)
    px = torch.from_numpy(pkg.synth.make_documents(cfg, 40, seed=6, text_len=8)["pixel_values"]).cuda()
    eng = pkg.EarlyExitEngine(cfg, max_docs=40)
    eng.load_weights(W)
    E1 = cfg.exit_config.num_exits + 1
    dump = eng.forward(pixel_values=px, dump_all=True, want_all=True, whole_layers=True)
    al, ac = _np(dump.all_logits), _np(dump.all_crit)
    thr = _thresholds(ac, +1, quantile=0.6)
    for rule in RULES:
        for t in (1, 2, VECTOR(E1)):
            ex = rule_exits(ac.astype(np.float64), al.astype(np.float64), thr, t, rule, +1)
            o = eng.forward(pixel_values=px, thresholds=thr, exit_rule=RULE_NAMES[rule], patience=t, whole_layers=True)
            assert np.array_equal(_np(o.exit_layer), ex), (rule, t)
            assert np.array_equal(_np(o.logits), al[ex, np.arange(40)]) and np.array_equal(_np(o.confidence), ac[ex, np.arange(40)])
    # the model wrapper reads both keys of its exit_config at every call
    m = pkg.DiTEEForImageClassification(cfg, W, max_docs=40)
    m.config.exit_config["exit_rule"] = "patient_confident"
    with pytest.raises(ValueError, match="patience"):
        m.early_exit(pixel_values=px, thresholds=thr)
    m.config.exit_config["patience"] = VECTOR(E1)
    r = m.early_exit(pixel_values=px, thresholds=thr, whole_layers=True)
    assert np.array_equal(_np(r.exit_layer), rule_exits(ac.astype(np.float64), al.astype(np.float64), thr, VECTOR(E1), STREAK, +1))
    out = m(pixel_values=px)                                   # dump-all: untouched by the rule
    assert np.array_equal(_np(out.exit_states[0][0]), _np(eng.forward(pixel_values=px, dump_all=True, want_head=True).head_logits[0]))
    m.config.exit_config["exit_rule"] = "plain"
    with pytest.raises(ValueError, match="patience="):
        m.early_exit(pixel_values=px, thresholds=thr, patience=2)
    r = m.early_exit(pixel_values=px, thresholds=thr, whole_layers=True)
    assert np.array_equal(_np(r.exit_layer), plain_exits(ac.astype(np.float64), thr, +1))
    m.engine.close()
    eng.close()


# ---- 7. micro-batches ---------------------------------------------------------------------------------------------------------------------------------
def test_micro_batched_engine_gives_the_single_engine_bits(pkg):
    cfg, W, temps = _tiny(pkg, "ramp_2layer_emb", exit_rule="patient_confident", patience=2)
    E1 = cfg.exit_config.num_exits + 1
    one = pkg.EarlyExitEngine(cfg, max_docs=40, max_text_len=T_TINY)
    two = pkg.MicroBatchedEngine(cfg, max_docs=40, max_text_len=T_TINY, micro_batches=2)
    assert str(one.exit_rule) == str(two.exit_rule) == "patient_confident" and one.patience == two.patience == 2
    one.load_weights(W)
    two.load_weights(W)
    args = _docs(pkg, cfg, 33, seed=4)
    ac = _np(one.forward(*args, dump_all=True, want_all=True).all_crit)
    thr = _thresholds(ac, +1, quantile=0.7)
    seen = []
    for kw in (dict(), dict(patience=1), dict(exit_rule="patience_or_threshold", patience=VECTOR(E1)), dict(exit_rule="patient_confident", patience=3)):
        a, b = one.forward(*args, thresholds=thr, **kw), two.forward(*args, thresholds=thr, **kw)
        for f in FIELDS:
            assert np.array_equal(_np(getattr(a, f)), _np(getattr(b, f))), (kw, f)
        seen.append(tuple(_np(a.exit_layer).tolist()))
    assert len(set(seen)) >= 2
    two.check()
    one.close()
    two.close()


# ---- 8. captured graph ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_captured_graph_reads_the_patience_vector_of_each_launch(pkg, rule):
    """Captured at one per-exit patience vector, replayed at three others (a scalar among them) with fresh inputs copied into the graph's
    buffers: each replay equals an eager forward at that patience; the rule is bound at capture."""
    cfg, W, temps = _tiny(pkg, "gate_1layer_k10_temps")
    E1 = cfg.exit_config.num_exits + 1
    B = 64
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T_TINY)
    ref = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T_TINY)
    eng.load_weights(W)
    ref.load_weights(W)
    first = _docs(pkg, cfg, B, seed=20)
    thr = _thresholds(_np(ref.forward(*first, dump_all=True, want_all=True, temperatures=temps).all_crit), +1,
                      quantile=0.6 if rule == STREAK else 0.9)     # STREAK differs through documents that fire, EITHER through those that do not
    name = RULE_NAMES[rule]
    cap = eng.capture(*[x.clone() for x in first], thresholds=thr, temperatures=temps, exit_rule=name, patience=VECTOR(E1))
    e0 = ref.forward(*first, thresholds=thr, temperatures=temps, exit_rule=name, patience=VECTOR(E1))
    for f in FIELDS:
        assert np.array_equal(_np(getattr(cap.outputs, f)), _np(getattr(e0, f))), f
    eng.set_exit_rule("plain")                                 # the capture keeps ITS rule
    keys = ("input_ids", "attention_mask", "bbox", "pixel_values")
    for i, t in enumerate(([2, 1, 1, 1, 1][:E1], 3, [3, 1, 2, 1, 1][:E1])):
        new = _docs(pkg, cfg, B, seed=21 + i)
        for k, x in zip(keys, new):
            cap.inputs[k].copy_(x)
        out = cap.launch(thresholds=thr, temperatures=temps, patience=t)
        want = ref.forward(*new, thresholds=thr, temperatures=temps, patience=t)
        for f in FIELDS:
            assert np.array_equal(_np(getattr(out, f)), _np(getattr(want, f))), (t, f)
        # the patience of the launch matters on these inputs: the capture-time vector gives other exits
        baked = ref.forward(*new, thresholds=thr, temperatures=temps, patience=VECTOR(E1))
        assert not np.array_equal(_np(baked.exit_layer), _np(want.exit_layer)), t
    eng.check()
    cap.close()
    eng.close()
    ref.close()


# ---- 9. state isolation, refusals ----------------------------------------------------------------------------------------------------------------
def test_no_state_leaks_between_forwards_or_rules(pkg):
    """PLAIN at B = 17, STREAK at B = 9, PLAIN at B = 17 again on ONE handle: the third forward equals the first bit for bit and the STREAK
    forward equals a fresh handle's; the same with EITHER in the middle.  Also the refusals, each with its message."""
    cfg, W, temps = _tiny(pkg, "ramp_2layer_emb")
    E1 = cfg.exit_config.num_exits + 1
    eng = pkg.EarlyExitEngine(cfg, max_docs=17, max_text_len=T_TINY)
    eng.load_weights(W)
    args = _docs(pkg, cfg, 17, seed=30)
    small = tuple(x[:9].contiguous() for x in args)
    thr = _thresholds(_np(eng.forward(*args, dump_all=True, want_all=True).all_crit), +1, quantile=0.5)
    with pytest.raises(pkg.capi.MMEEError, match="need a patience"):
        eng.forward(*small, thresholds=thr, exit_rule="patient_confident")
    eng.set_exit_rule("plain")
    for name in ("patient_confident", "patience_or_threshold"):
        a = eng.forward(*args, thresholds=thr)
        b = eng.forward(*small, thresholds=thr, exit_rule=name, patience=2)
        c = eng.forward(*args, thresholds=thr, exit_rule="plain")
        fresh = pkg.EarlyExitEngine(pkg.ModelConfig.tiny(EE_config=dict(cfg.EE_config, exit_rule=name, patience=2), num_labels=cfg.num_labels),
                                    max_docs=17, max_text_len=T_TINY)
        fresh.load_weights(W)
        d = fresh.forward(*small, thresholds=thr)
        for f in FIELDS:
            assert np.array_equal(_np(getattr(a, f)), _np(getattr(c, f))), (name, f)
            assert np.array_equal(_np(getattr(b, f)), _np(getattr(d, f))), (name, f)
        if name == "patient_confident":
            assert not np.array_equal(_np(b.exit_layer), _np(a.exit_layer)[:9])
        fresh.close()
    # refusals
    eng.set_exit_rule("patient_confident")
    with pytest.raises(pkg.capi.MMEEError, match="MMEE_CRIT_PATIENCE.*threshold event"):
        eng.set_criterion("patience")
    eng.set_exit_rule("plain")
    eng.set_criterion("patience")
    for name in ("patient_confident", "patience_or_threshold"):
        with pytest.raises(pkg.capi.MMEEError, match="MMEE_CRIT_PATIENCE.*threshold event"):
            eng.set_exit_rule(name)
    pv = eng.forward(*args, patience=VECTOR(E1))               # per-exit patience under PABEE itself: c_e >= t_e
    al = _np(eng.forward(*args, dump_all=True, want_all=True).all_logits).astype(np.float64)
    assert np.array_equal(_np(pv.exit_layer), rule_exits(np.zeros(al.shape[:2]), al, 2.0, VECTOR(E1), EITHER, +1))
    eng.set_criterion("max_confidence")
    assert eng.lib.ee_set_exit_rule(eng._h, 3) != 0 and "unknown rule" in pkg.capi.last_error(eng._h)
    import ctypes as C
    bad = (C.c_int32 * E1)(*([1] * (E1 - 1) + [0]))
    assert eng.lib.ee_set_patience_vector(eng._h, bad, E1) != 0 and ">= 1" in pkg.capi.last_error(eng._h)
    ok = (C.c_int32 * (E1 + 1))(*([1] * (E1 + 1)))
    assert eng.lib.ee_set_patience_vector(eng._h, ok, E1 + 1) != 0 and "E + 1" in pkg.capi.last_error(eng._h)
    assert eng.lib.ee_set_patience_vector(eng._h, ok, E1 - 1) != 0
    with pytest.raises(ValueError):
        eng.set_patience([1] * (E1 - 1))
    with pytest.raises(ValueError):
        eng.set_exit_rule("both")
    eng.check()
    eng.close()


# ---- 10. launch counts ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gate_1layer_k10_temps", "ramp_2layer_emb"])
def test_a_rule_forward_issues_exactly_the_launches_of_its_plain_twin(pkg, name):
    """The rules are instantiations of the decide kernel: the summed launches of ee_profile_read of a STREAK and of an EITHER forward equal
    those of the PLAIN forward with the same thresholds (default schedule, and whole layers)."""
    cfg, W, temps = _tiny(pkg, name)
    eng = pkg.EarlyExitEngine(cfg, max_docs=40, max_text_len=T_TINY)
    eng.load_weights(W)
    args = _docs(pkg, cfg, 40, seed=12)
    counts = {}
    for rule in ("plain", "patient_confident", "patience_or_threshold"):
        for sched in ("default", "whole"):
            eng.profile(True)
            eng.forward(*args, thresholds=2.0, temperatures=temps, exit_rule=rule, patience=64, whole_layers=sched == "whole")
            prof = eng.profile_read()
            eng.profile(False)
            counts[rule, sched] = sum(v["launches"] for v in prof.values())
            assert prof["exit_decide"]["launches"] == cfg.exit_config.num_exits + 1
    eng.check()
    eng.close()
    for sched in ("default", "whole"):
        report_measured(f"rule[{name},{sched}]", "profiled launches (plain)", float(counts["plain", sched]))
        for rule in ("patient_confident", "patience_or_threshold"):
            assert 0 < counts[rule, sched] == counts["plain", sched], (sched, counts)
