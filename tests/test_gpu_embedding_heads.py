"""Embedding-level exit heads on the device: the rows ``ee_embedding_inputs`` returns against the oracle, the bit equalities the header
promises, and the pipeline collect -> fit -> state_dict -> load_weights -> forward for one- and two-layer ramps and two-layer gates with the
embedding-level heads included.  The row kernels alone are held to float64 in tests/test_gpu_rows.py; the first test here is about wiring
(which kind, which divisor, padding included), and ``test_wiring_faults_move_the_oracle_rows`` (no GPU) shows that each such fault moves the
rows by more than 1e-2 on these inputs, a hundred times the 1e-4 bar."""
import ctypes as C
import functools

import numpy as np
import pytest

from . import headfit_ref as HR
from .conftest import H256_KW
from .fit_util import _gap_thresholds, _ptr, _stream, _torch

L2, GTOL = 1e-2, 1e-9
KINDS = ("vision_avg", "text_avg", "text_visual_concat")
EXITS5 = ["vision_avg", "text_avg", "text_visual_concat", 1, 2]
KEYS = ("input_ids", "attention_mask", "bbox", "pixel_values")
CASES = {"tiny_f32": ({}, "fp32"), "h256_split": (H256_KW, "split")}


def _cfg(pkg, name, exits=EXITS5, strategy="ramp", layers=1):
    ee = dict(exits=list(exits), encoder_layer_strategy=strategy, inference_strategy="max_confidence", exit_head_num_layers=layers)
    return pkg.ModelConfig.tiny(EE_config=ee, **CASES[name][0])


@functools.lru_cache(maxsize=None)
def _inputs(name, B, T):
    """-> (synthetic weights of the five-exit one-layer ramp configuration, ragged documents); read-only, shared by the tests"""
    import importlib
    pkg = importlib.import_module("multi-modal-early-exit_amd")
    cfg = _cfg(pkg, name)
    W = pkg.synth.make_weights(cfg, seed=21)
    docs = pkg.synth.make_documents(cfg, B, seed=22, text_len=T, min_words=3)
    for a in list(W.values()) + list(docs.values()):
        a.setflags(write=False)
    return W, docs


def _cuda(docs, rows=slice(None)):
    torch = _torch()
    return {k: torch.from_numpy(np.array(docs[k][rows])).cuda() for k in KEYS}


def _engine(pkg, cfg, name, W, B, T):
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision=CASES[name][1])
    eng.load_weights(W)
    return eng


@functools.lru_cache(maxsize=None)
def _oracle_rows(name, B, T):
    """{kind: (B,H) float32}: the rows the reference's three embedding-level heads read (EE/models/LayoutLMv3.py:466, 520, 582), and the
    (B,T,H) text and (B,Pv,H) visual embeddings they are means of"""
    import importlib
    pkg, oracle = importlib.import_module("multi-modal-early-exit_amd"), importlib.import_module("oracle.ee_oracle")
    cfg = _cfg(pkg, name)
    W, docs = _inputs(name, B, T)
    vis = oracle.image_embeddings(cfg, W, docs["pixel_values"])
    txt = oracle.text_embeddings(cfg, W, docs["input_ids"], docs["bbox"])
    cat = oracle.layer_norm(np.concatenate([txt, vis], axis=1), W["layoutlmv3.LayerNorm.weight"], W["layoutlmv3.LayerNorm.bias"], cfg.layer_norm_eps)
    return {"vision_avg": vis.mean(1), "text_avg": txt.mean(1), "text_visual_concat": cat.mean(1)}, txt, vis, cat


@pytest.mark.parametrize("name", list(CASES))
def test_wiring_faults_move_the_oracle_rows(name):
    """No GPU: the three faults the row test is there to catch, applied to the oracle's rows, each move them by more than 1e-2."""
    B, T = 5, 41
    rows, txt, vis, cat = _oracle_rows(name, B, T)
    _, docs = _inputs(name, B, T)
    am = docs["attention_mask"].astype(np.float64)
    assert am.sum(1).min() < T, "no padded position: the padding fault would not show"
    Pv = vis.shape[1]
    dist = lambda a, b: float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
    faults = {
        "kind: vision for text": dist(rows["vision_avg"], rows["text_avg"]),
        "kind: text for concat": dist(rows["text_avg"], rows["text_visual_concat"]),
        "kind: concat for vision": dist(rows["text_visual_concat"], rows["vision_avg"]),
        "divisor: text over T + Pv": dist(rows["text_avg"] * (T / (T + Pv)), rows["text_avg"]),
        "divisor: vision over T": dist(rows["vision_avg"] * (Pv / T), rows["vision_avg"]),
        "divisor: concat over T": dist(rows["text_visual_concat"] * ((T + Pv) / T), rows["text_visual_concat"]),
        "divisor: text over the kept positions": dist(txt.sum(1) / am.sum(1, keepdims=True), rows["text_avg"]),
        "padding: text without the padded positions": dist((txt * am[:, :, None]).sum(1) / T, rows["text_avg"]),
        "padding: concat without the padded positions": dist((cat * np.concatenate([am, np.ones((B, Pv))], 1)[:, :, None]).sum(1) / (T + Pv),
                                                             rows["text_visual_concat"]),
    }
    print(name, {k: f"{v:.3e}" for k, v in faults.items()})
    for what, d in faults.items():
        assert d > 1e-2, (what, d)


# ---- 1. the rows ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_rows_match_the_oracle(pkg, name):
    """B = 5, T = 41: a partial 32-row chunk in the text and in the visual rows, ragged documents, so padded positions enter the means.
    The bar is the project's 1e-4 absolute parity bar."""
    B, T = 5, 41
    W, docs = _inputs(name, B, T)
    want = _oracle_rows(name, B, T)[0]
    cfg = _cfg(pkg, name)
    eng = _engine(pkg, cfg, name, W, B, T)
    got = eng.embedding_inputs(**_cuda(docs))
    assert list(got) == list(KINDS)                                     # the configuration's kinds, in the reference's order
    for kind in KINDS:
        assert tuple(got[kind].shape) == (B, cfg.hidden_size) and got[kind].dtype == _torch().float32 and got[kind].is_cuda
        err = float(np.abs(got[kind].cpu().numpy().astype(np.float64) - want[kind].astype(np.float64)).max())
        print(f"{name}: {kind}: max |row - oracle| = {err:.3e}")
        assert err <= 1e-4, (kind, err)
    with pytest.raises(ValueError, match="no kinds"):
        eng.embedding_inputs(**_cuda(docs), kinds=[])
    with pytest.raises(ValueError, match="not among"):
        eng.embedding_inputs(**_cuda(docs), kinds=["cls"])
    eng.close()


# ---- 2. bit equalities --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_bit_equalities(pkg, name):
    torch = _torch()
    B, T = 5, 41
    W, docs = _inputs(name, B, T)
    t = _cuda(docs)
    eng = _engine(pkg, _cfg(pkg, name), name, W, B, T)
    before = eng.forward(**t, dump_all=True, want_all=True, want_head=True, want_hidden_cls=True)
    counts = eng.stage_counts()
    together = eng.embedding_inputs(**t)
    # the handle's record of the last forward is untouched by a call of another batch size
    eng.embedding_inputs(**_cuda(docs, slice(0, 3)))
    assert eng.stage_counts() == counts
    # each kind asked alone is the kind asked with the others
    for kind in KINDS:
        alone = eng.embedding_inputs(**t, kinds=[kind])
        assert list(alone) == [kind] and torch.equal(alone[kind], together[kind]), kind
    # batches split [3, 2] at the same T are the batch of 5
    parts = pkg.collect_embedding_features(eng, [_cuda(docs, slice(0, 3)), _cuda(docs, slice(3, 5))])
    assert tuple(parts.shape) == (3, B, eng.cfg.hidden_size)
    assert torch.equal(parts, torch.stack([together[k] for k in KINDS]))
    # a dump-all forward after the call returns what the one before it returned
    after = eng.forward(**t, dump_all=True, want_all=True, want_head=True, want_hidden_cls=True)
    for f in ("logits", "exit_layer", "confidence", "all_logits", "all_crit", "head_logits", "head_crit", "hidden_cls"):
        assert torch.equal(getattr(before, f), getattr(after, f)), f
    # inputs_embeds armed for the next call are consumed by it: the word-embedding rows handed in are the rows looked up
    word = [v for k, v in W.items() if k.endswith("word_embeddings.weight")][0]
    emb = torch.from_numpy(np.ascontiguousarray(word[docs["input_ids"]])).cuda()
    pkg.capi.check(eng.lib.ee_set_inputs_embeds(eng._h, _ptr(emb)), eng._h, "ee_set_inputs_embeds")
    via = eng.embedding_inputs(**t)
    for kind in KINDS:
        assert torch.equal(via[kind], together[kind]), kind
    eng.close()
    # a handle whose configuration names no embedding exit returns the same bits
    plain = _engine(pkg, _cfg(pkg, name, exits=[1, 2]), name, W, B, T)
    with pytest.raises(ValueError, match="no kinds"):
        plain.embedding_inputs(**t)
    got = plain.embedding_inputs(**t, kinds=KINDS)
    for kind in KINDS:
        assert torch.equal(got[kind], together[kind]), kind
    plain.close()


# ---- 3. through the engine: one-layer ramps --------------------------------------------------------------------------------------------------
def _labels(feats, K, seed=23):
    """Labels drawn as tests/test_gpu_head_fit.py::test_dump_fit_load_forward draws them: a random teacher on the last exit's rows + Gumbel noise"""
    rng = np.random.default_rng(seed)
    last = feats[-1].cpu().numpy().astype(np.float64)
    teacher = rng.standard_normal((K, last.shape[1])) * (2.0 / np.sqrt(last.shape[1]))
    return (last @ teacher.T + rng.gumbel(size=(last.shape[0], K))).argmax(-1).astype(np.int64)


def _reference(X, y, K, l2=L2):
    """The minimiser of tests/headfit_ref.py's objective that ``HR.solve`` stands for: scipy L-BFGS-B with ``HR.solve``'s options on
    ``HR.loss_grad``, held to ``HR.solve``'s own bar, a float64 gradient norm <= 1e-8.  ``HR.solve`` itself cannot be called on these rows:
    with N = 96 rows whose common component is 40 times their spread, scipy stops on ftol at gradient norms of 2e-8 ... 2e-7 and restarting it
    from its result, as ``HR.solve`` does, moves nothing (measured on the CPU on the oracle's rows of both configurations, all five exits, ten
    restarts each), so ``HR.solve`` raises.  The objective is strongly convex, so its minimiser does not depend on the method: Newton steps
    from scipy's point, each solved by conjugate gradients on the exact Hessian-vector product of the softmax loss, reach it (one step takes
    5e-8 to 1e-11)."""
    from scipy.optimize import minimize
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[0]
    x = minimize(HR.loss_grad, np.zeros(K * X.shape[1] + K), args=(X, y, K, l2), jac=True, method="L-BFGS-B",
                 options=dict(gtol=1e-12, ftol=1e-15, maxiter=5000)).x
    for _ in range(4):
        g = HR.loss_grad(x, X, y, K, l2)[1]
        if np.linalg.norm(g) <= 1e-10:
            break
        z = HR.logits(x, X, K)
        p = np.exp(z - z.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)

        def hess_vec(v):                                                # d grad / d theta . v of HR.loss_grad
            dz = HR.logits(v, X, K)
            dp = p * dz - p * (p * dz).sum(1, keepdims=True)
            return np.concatenate([(dp.T @ X).reshape(-1), dp.sum(0)]) / N + l2 * v

        d, r = np.zeros_like(x), -g
        q, rr = r.copy(), r @ r
        for _ in range(2000):
            if np.sqrt(rr) <= 1e-3 * np.linalg.norm(g):
                break
            Hq = hess_vec(q)
            a = rr / (q @ Hq)
            d += a * q
            r = r - a * Hq
            rn = r @ r
            q, rr = r + (rn / rr) * q, rn
        x = x + d
    gn = float(np.linalg.norm(HR.loss_grad(x, X, y, K, l2)[1]))
    assert gn <= 1e-8, f"the reference stopped at a gradient norm of {gn:.3e} > 1e-8"
    return x


def _confidences(all_logits):
    z = all_logits.to(_torch().float64).cpu().numpy()
    p = np.exp(z - z.max(-1, keepdims=True))
    return (p / p.sum(-1, keepdims=True)).max(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_collect_fit_load_forward(pkg, name):
    """The evaluation counts of the five exits are printed; the budget is the project's 2000.  Measured on an MI355X, vision / text / concat /
    layer 1 / layer 2: 254 / 303 / 234 / 181 / 262 (tiny, fp32) and 270 / 368 / 307 / 368 / 356 (H = 256, split): the pooled rows are of the
    conditioning class of the CLS rows."""
    torch = _torch()
    B, T = 96, 48
    W, docs = _inputs(name, B, T)
    t = _cuda(docs)
    cfg = _cfg(pkg, name)
    K, H = cfg.num_labels, cfg.hidden_size
    eng = _engine(pkg, cfg, name, W, B, T)
    feats = pkg.collect_exit_features(eng, [t], embedding_exits=True)
    assert tuple(feats.shape) == (5, B, H) and feats.is_cuda and feats.dtype == torch.float32
    assert torch.equal(feats[:3], pkg.collect_embedding_features(eng, [t]))
    exit_names = [n for n in eng.expected_tensors() if "exit" in n]
    eng.close()
    enc = _engine(pkg, _cfg(pkg, name, exits=[1, 2]), name, W, B, T)       # the embedding exits removed: the same backbone, the same CLS rows
    assert torch.equal(feats[3:], pkg.collect_exit_features(enc, [t]))
    enc.close()

    y = _labels(feats, K)
    fit = pkg.fit_exit_heads(feats, torch.from_numpy(y).cuda(), l2=L2, gtol=GTOL, max_evals=2000, num_labels=K)
    print(f"{name}: evals {fit.evals.cpu().tolist()} status {fit.status.cpu().tolist()} grad norms {fit.grad_norm.cpu().tolist()}")
    assert (fit.status.cpu().numpy() == 0).all(), (fit.status, fit.evals, fit.grad_norm)
    X = feats.cpu().numpy()
    z_dev = fit.logits(feats).cpu().numpy()
    for e in range(5):
        dz = np.abs(z_dev[e] - HR.logits(_reference(X[e], y, K), X[e], K)).max()
        print(f"{name}: exit {e}: max |logits - reference solution's| = {dz:.3e}")
        assert dz <= 1e-4, (e, dz)
    sd = fit.state_dict(cfg, embedding_exits=True)
    assert sorted(sd) == sorted(exit_names)

    eng2 = _engine(pkg, cfg, name, {**W, **sd}, B, T)
    dump = eng2.forward(**t, dump_all=True, want_head=True, want_all=True)
    err = np.abs(dump.head_logits.cpu().numpy().astype(np.float64) - z_dev).max()
    print(f"{name}: max |head_logits - HeadFit.logits| = {err:.3e}")
    assert err <= 1e-4, err
    conf = _confidences(dump.all_logits)
    thr = _gap_thresholds(conf)
    assert np.abs(conf - thr[:, None])[:-1].min() > 1e-6, "thresholds too close to a confidence"
    want_exits = pkg.criterion_scan_device(dump.all_logits.to(torch.float64), thr, "max_confidence")[0].cpu().numpy()
    out = eng2.forward(**t, thresholds=thr, xprobe=False)
    assert np.array_equal(out.exit_layer.cpu().numpy(), want_exits)
    assert (want_exits < 3).any() and len(np.unique(want_exits)) >= 2, np.bincount(want_exits)
    eng2.close()


# ---- 4. two-layer ramp and two-layer gate (tiny) ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("strategy", ["ramp", "gate"])
def test_two_layer_heads_collect_fit_load_forward(pkg, strategy):
    """A stationary-point search with a budget of 200: the status is not asserted, the loss must be below its start."""
    torch = _torch()
    name, B, T = "tiny_f32", 96, 48
    cfg = _cfg(pkg, name, strategy=strategy, layers=2)
    W = pkg.synth.make_weights(cfg, seed=21)                          # this configuration's own heads: four tensors each
    t = _cuda(_inputs(name, B, T)[1])
    eng = _engine(pkg, cfg, name, W, B, T)
    if strategy == "gate":
        feats, gated = pkg.collect_gate_features(eng, [t], embedding_exits=True)
        dump = eng.forward(**t, dump_all=True, want_all=True)
        assert tuple(gated.shape) == (5, B, cfg.num_labels) and torch.equal(gated, dump.all_logits[:5])
        y = _labels(feats, cfg.num_labels)
        targets = pkg.gate_targets(gated, torch.from_numpy(y).cuda())
        assert tuple(targets.shape) == (5, B)
        run = lambda n: pkg.fit_mlp_gate_heads(feats, targets, l2=L2, max_evals=n)
    else:
        feats = pkg.collect_exit_features(eng, [t], head_layers=2, embedding_exits=True)
        y = torch.from_numpy(_labels(feats, cfg.num_labels)).cuda()
        run = lambda n: pkg.fit_mlp_exit_heads(feats, y, l2=L2, max_evals=n, num_labels=cfg.num_labels)
    assert tuple(feats.shape) == (5, B, cfg.hidden_size)
    assert torch.equal(feats[:3], pkg.collect_embedding_features(eng, [t]))
    exit_names = [n for n in eng.expected_tensors() if "exit" in n]
    eng.close()
    start, fit = run(1), run(200)                                      # one evaluation: the objective at the start
    print(f"{strategy}: loss {start.loss.cpu().tolist()} -> {fit.loss.cpu().tolist()}, evals {fit.evals.cpu().tolist()}, status {fit.status.cpu().tolist()}")
    assert bool((fit.loss < start.loss).all()), (start.loss, fit.loss)
    sd = fit.state_dict(cfg, embedding_exits=True)
    assert sorted(sd) == sorted(exit_names)
    eng2 = _engine(pkg, cfg, name, {**W, **sd}, B, T)
    dump = eng2.forward(**t, dump_all=True, want_head=True)
    err = np.abs(dump.head_logits.cpu().numpy().astype(np.float64) - fit.logits(feats).cpu().numpy()).max()
    print(f"{strategy}: max |head_logits - fit.logits| = {err:.3e}")
    assert err <= 1e-4, err
    eng2.close()


# ---- 5. cascade weights -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reach_weights_over_all_five_exits(pkg):
    torch = _torch()
    name, B, T = "tiny_f32", 96, 48
    W, docs = _inputs(name, B, T)
    t = _cuda(docs)
    cfg = _cfg(pkg, name)
    eng = _engine(pkg, cfg, name, W, B, T)
    feats = pkg.collect_exit_features(eng, [t], embedding_exits=True)
    logits = eng.forward(**t, dump_all=True, want_all=True).all_logits.to(torch.float64)
    eng.close()
    y = torch.from_numpy(_labels(feats, cfg.num_labels)).cuda()
    plain = pkg.fit_exit_heads(feats, y, l2=L2, gtol=GTOL, max_evals=2000, num_labels=cfg.num_labels)
    bits = lambda f: [x.cpu().numpy().tobytes() for x in (f.weight, f.bias, f.weight64, f.bias64, f.loss, f.grad_norm, f.evals, f.status)]
    # no confidence exceeds 2: every exit keeps every document, the scan's exit index is 5 everywhere and every weight is 1
    kept = pkg.criterion_scan_device(logits, np.full(6, 2.0), "max_confidence")[0]
    w = pkg.reach_weights(kept, 5)
    assert tuple(w.shape) == (5, B) and bool((w == 1).all())
    assert bits(pkg.fit_exit_heads(feats, y, l2=L2, gtol=GTOL, max_evals=2000, num_labels=cfg.num_labels, sample_weight=w)) == bits(plain)
    # at gap thresholds the rows of the table are the documents each of the five exits is asked about, embedding-level exits included
    exits = pkg.criterion_scan_device(logits, _gap_thresholds(_confidences(logits)), "max_confidence")[0]
    w = pkg.reach_weights(exits, 5)
    ex = exits.cpu().numpy()
    assert np.array_equal(w.cpu().numpy(), (ex[None, :] >= np.arange(5)[:, None]).astype(np.float32))
    assert bool((w[0] == 1).all()) and float(w[1].sum()) < B           # somebody leaves at the first embedding-level exit


# ---- 6. the C entry point's refusals -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_c_refusals_leave_the_outputs_untouched(pkg):
    torch = _torch()
    name, B, T = "tiny_f32", 5, 41
    W, docs = _inputs(name, B, T)
    t = _cuda(docs)
    cfg = _cfg(pkg, name)
    H = cfg.hidden_size
    eng = _engine(pkg, cfg, name, W, B, T)
    lib = eng.lib
    outs = [torch.full((B + 1, H), 7.0, dtype=torch.float32, device="cuda") for _ in range(3)]

    def call(h, ids, outs, B=B, px=t["pixel_values"]):
        return lib.ee_embedding_inputs(h, _ptr(ids), _ptr(t["attention_mask"]), _ptr(t["bbox"]), _ptr(px), None, None, B, T,
                                       *[_ptr(o) for o in outs], _stream())

    def untouched():
        torch.cuda.synchronize()
        return all(bool((o == 7).all()) for o in outs)

    assert call(eng._h, t["input_ids"], [None, None, None]) != 0
    assert "all NULL" in pkg.capi.last_error(eng._h) and untouched()
    assert call(eng._h, t["input_ids"], outs, B=B + 1) != 0
    assert "max_docs" in pkg.capi.last_error(eng._h) and untouched()

    dcfg = pkg.ModelConfig.dit_tiny(EE_config=dict(exits=[1, 2], encoder_layer_strategy="ramp", exit_head_num_layers=1))
    dit = pkg.EarlyExitEngine(dcfg, max_docs=B, precision="fp32")
    dit.load_weights(pkg.synth.make_weights_beit(dcfg, seed=21))
    dpx = torch.zeros((B, dcfg.num_channels, dcfg.input_size, dcfg.input_size), dtype=torch.float32, device="cuda")
    assert call(dit._h, t["input_ids"], outs, px=dpx) != 0
    assert "MMEE_ARCH_BEIT" in pkg.capi.last_error(dit._h) and untouched()
    with pytest.raises(ValueError, match="LayoutLMv3"):
        dit.embedding_inputs(pixel_values=dpx)
    dit.close()

    # an id outside the vocabulary is flagged on the device, as in ee_forward: the call that follows the faulty one reports it
    bad = t["input_ids"].clone()
    bad[2, 1] = cfg.vocab_size
    rc = call(eng._h, bad, outs)
    torch.cuda.synchronize()
    rc = rc or call(eng._h, t["input_ids"], outs)
    assert rc != 0
    msg = pkg.capi.last_error(eng._h)
    assert "input out of range" in msg and "1 = token id" in msg, msg
    # the mended inputs go through, and the rows are the usual ones
    assert call(eng._h, t["input_ids"], outs) == 0
    want = eng.embedding_inputs(**t)
    for o, kind in zip(outs, KINDS):
        assert torch.equal(o[:B], want[kind]) and bool((o[B] == 7).all()), kind
    eng.close()
