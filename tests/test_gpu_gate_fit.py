"""The fit of the 2-way gate heads on the device (include/mmee.h ee_head_fit_gate) against the float64 restatement of the gate objective in
tests/gate_ref.py: the loss / gradient kernel alone, the fit against scipy's L-BFGS-B on the restated objective (the problem is strongly
convex, so there is one optimum), the column-wise identity with ``fit_lte_classifier(loss="bce", l2=2 l2)``, determinism, the failure of a bad
target, and the loop dump rows -> targets -> fit -> load -> forward under the gate criterion.

Bars: logits within 1e-4 of the reference optimum's (the project's bar, the one the distilled one-layer fit is held to: strong convexity gives
||dtheta|| <= (||g_dev|| + ||g_ref||) / l2 ~ 1e-6, times ||x|| ~ 32 at H = 1024); the kernel alone within 1e-10 relative (float64 sums of at
most a few hundred terms of order 1 and exp / log1p at a few ulp sit orders below it)."""
import functools

import numpy as np
import pytest

from . import gate_ref as G
from .conftest import MATRIX_CASES, H256_KW, report_measured
from .fit_util import _dev, _ptr, _stream, _torch

pytestmark = pytest.mark.gpu

L2, GTOL = 1e-2, 1e-9
SHAPES = [(E, N, H) for E in (1, 3) for N in (63, 257) for H in (4, 128, 132)] + [(1, 257, 1024)]
SHAPE_IDS = [f"E{E}-N{N}-H{H}" for E, N, H in SHAPES]


@functools.lru_cache(maxsize=None)
def _problem(E, N, H):
    """Unit-variance features and targets that depend on them: exit 0 hard (0 / 1), exit 1 soft (in [0,1]), exit 2 all ones; a single exit
    is hard at N = 63 and soft at N = 257."""
    rng = np.random.default_rng(1000 * E + 10 * N + H)
    X = rng.standard_normal((E, N, H)).astype(np.float32)
    w = rng.standard_normal((E, H)) / np.sqrt(H)
    p = 1.0 / (1.0 + np.exp(-(2.0 * np.einsum("enh,eh->en", X.astype(np.float64), w) + 0.3)))
    T = np.empty((E, N))
    for e in range(E):
        kind = ("hard", "soft", "ones")[e] if E == 3 else ("hard" if N == 63 else "soft")
        T[e] = (rng.random(N) < p[e]).astype(np.float64) if kind == "hard" else p[e] if kind == "soft" else 1.0
    X.setflags(write=False)
    T.setflags(write=False)
    return X, T


@functools.lru_cache(maxsize=None)
def _reference(E, N, H):
    """Per exit the scipy optimum of the restated objective and the largest entry of its gradient there; shared by the tests."""
    X, T = _problem(E, N, H)
    out = [G.gate_fit(X[e], T[e], L2) for e in range(E)]
    return [o[0] for o in out], [o[1] for o in out]


def _lossgrad(pkg, X, T, theta, l2=L2):
    """ee_debug_head_gate_lossgrad on host arrays X (E,N,H) f32, T (E,N), theta (E, 2H + 2) -> (loss (E,), grad (E, 2H + 2)) host float64."""
    torch = _torch()
    E, N, H = X.shape
    Xd, Td, td = _dev(np.array(X), torch.float32), _dev(np.array(T), torch.float64), _dev(theta, torch.float64)
    loss = torch.full((E,), float("nan"), dtype=torch.float64, device="cuda")
    grad = torch.full((E, 2 * H + 2), float("nan"), dtype=torch.float64, device="cuda")
    rc = pkg.capi.load().ee_debug_head_gate_lossgrad(_ptr(Xd), _ptr(Td), _ptr(td), E, N, H, l2, _ptr(loss), _ptr(grad), _stream())
    pkg.capi.check(rc, None, "ee_debug_head_gate_lossgrad")
    return loss.cpu().numpy(), grad.cpu().numpy()


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,N,H", SHAPES, ids=SHAPE_IDS)
def test_lossgrad_kernel_matches_the_restatement(pkg, E, N, H):
    """At a random point and at one whose logits reach +-700 (softplus must not overflow): loss and gradient within 1e-10 relative (of the
    value; of the gradient's largest entry for its components)."""
    X, T = _problem(E, N, H)
    rng = np.random.default_rng(H + N)
    worst = 0.0
    for scale in (1.0, 400.0):
        theta = rng.standard_normal((E, 2 * H + 2)) * (scale / np.sqrt(H))
        loss, grad = _lossgrad(pkg, X, T, theta)
        assert np.isfinite(loss).all() and np.isfinite(grad).all()
        for e in range(E):
            want, g = G.gate_lossgrad(theta[e], X[e], T[e], L2)
            dl = abs(loss[e] - want) / abs(want)
            dg = float(np.abs(grad[e] - g).max() / np.abs(g).max())
            worst = max(worst, dl, dg)
            assert dl <= 1e-10 and dg <= 1e-10, (e, scale, dl, dg)
    report_measured(f"gate_fit.lossgrad[{E},{N},{H}]", "worst relative difference to the restatement", worst)


# ---- 2. the fit -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,N,H", SHAPES, ids=SHAPE_IDS)
def test_fit_reaches_the_scipy_optimum(pkg, E, N, H):
    X, T = _problem(E, N, H)
    refs, ref_g = _reference(E, N, H)
    fit = pkg.fit_gate_heads(X, T, l2=L2, gtol=GTOL, max_evals=2000)
    status, evals = fit.status.cpu().numpy(), fit.evals.cpu().numpy()
    W64, b64 = fit.weight64.cpu().numpy(), fit.bias64.cpu().numpy()
    loss, gnorm = fit.loss.cpu().numpy(), fit.grad_norm.cpu().numpy()
    assert tuple(fit.weight.shape) == (E, 2, H) and tuple(fit.bias.shape) == (E, 2)
    assert np.array_equal(fit.weight.cpu().numpy(), W64.astype(np.float32)) and np.array_equal(fit.bias.cpu().numpy(), b64.astype(np.float32))
    worst = 0.0
    for e in range(E):
        theta = np.concatenate([W64[e].reshape(-1), b64[e]])
        l_dev, g_dev = G.gate_lossgrad(theta, X[e], T[e], L2)
        n_dev, n_ref = float(np.linalg.norm(g_dev)), float(np.linalg.norm(G.gate_lossgrad(refs[e], X[e], T[e], L2)[1]))
        dist = float(np.linalg.norm(theta - refs[e]))
        dz = float(np.abs(G.gate_logits(theta, X[e]) - G.gate_logits(refs[e], X[e])).max())
        worst = max(worst, dz)
        print(f"(E,N,H) = {(E, N, H)} exit {e}: evals {evals[e]} status {status[e]} ||g_dev|| {n_dev:.3e} ||g_ref|| {n_ref:.3e} "
              f"||dtheta|| {dist:.3e} max |dz| {dz:.3e} L {l_dev:.6f}")
        assert status[e] == 0 and 1 <= evals[e] <= 2000, (e, status[e], evals[e], gnorm[e])
        assert n_dev <= 2 * GTOL, (e, n_dev)
        assert dist <= (n_dev + n_ref) / L2, (e, dist, (n_dev + n_ref) / L2)       # strong convexity: fails only for another objective
        assert dz <= 1e-4, (e, dz)
        assert l_dev < G.gate_lossgrad(np.zeros_like(theta), X[e], T[e], L2)[0]
        assert abs(loss[e] - l_dev) <= 1e-10 * abs(l_dev) and abs(gnorm[e] - n_dev) <= 1e-12 + 1e-6 * n_dev, (e, loss[e], l_dev, gnorm[e], n_dev)
    report_measured(f"gate_fit[{E},{N},{H}]", "max |logit - scipy optimum's logit|", worst)
    if E == 3:                                                   # targets all 1: the gate learns "always exit", column 1 above column 0 everywhere
        z = fit.logits(X)[2].cpu().numpy()
        assert (z[:, 1] > z[:, 0]).all()


@pytest.mark.parametrize("E,N,H", [(3, 257, 132), (1, 63, 128)], ids=["E3-N257-H132", "E1-N63-H128"])
def test_each_column_is_the_lte_bce_fit_with_twice_the_penalty(pkg, E, N, H):
    """The two columns do not interact and the objectives differ by the factor 1/2: column j of exit e is fit_lte_classifier(features[e],
    t_j, loss="bce", l2 = 2 l2) with t_1 = c, t_0 = 1 - c.  No new reference needed; logits within the same 1e-4."""
    X, T = _problem(E, N, H)
    fit = pkg.fit_gate_heads(X, T, l2=L2, gtol=GTOL)
    z = fit.logits(X).cpu().numpy()
    worst = 0.0
    for e in range(E):
        for j, t in ((0, 1.0 - T[e]), (1, T[e])):
            lte = pkg.fit_lte_classifier(X[e:e + 1], t[None], loss="bce", l2=2.0 * L2, gtol=GTOL)
            assert int(lte.status.cpu()[0]) == 0
            th = lte.theta64.cpu().numpy()
            zj = X[e].astype(np.float64) @ th[:H] + th[H]
            worst = max(worst, float(np.abs(z[e, :, j] - zj).max()))
    report_measured(f"gate_fit.columns[{E},{N},{H}]", "max |gate column logit - LTE BCE logit|", worst)
    assert worst <= 1e-4


# ---- 3. properties -------------------------------------------------------------------------------------------------------------------------------
NAMES = ("weight", "bias", "weight64", "bias64", "loss", "grad_norm", "evals", "status")


def _bytes(fit, e=None):
    return [(getattr(fit, n) if e is None else getattr(fit, n)[e]).cpu().numpy().tobytes() for n in NAMES]


def test_two_streams_and_an_exit_alone_return_the_same_bits(pkg):
    torch = _torch()
    E, N, H = 3, 257, 132
    X, T = _problem(E, N, H)
    Xd, Td = _dev(np.array(X), torch.float32), _dev(np.array(T), torch.float64)
    fits = []
    for _ in range(2):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fits.append(pkg.fit_gate_heads(Xd, Td, l2=L2, gtol=GTOL))
        s.synchronize()
    assert (fits[0].status.cpu().numpy() == 0).all() and _bytes(fits[0]) == _bytes(fits[1])
    for e in (1, 2):
        alone = pkg.fit_gate_heads(Xd[e:e + 1].contiguous(), Td[e:e + 1].contiguous(), l2=L2, gtol=GTOL)
        assert _bytes(alone, 0) == _bytes(fits[0], e), e


def test_a_bad_target_fails_the_call_and_nothing_is_written(pkg):
    torch = _torch()
    lib = pkg.capi.load()
    E, N, H = 3, 63, 128
    X, T = _problem(E, N, H)
    nan = float("nan")
    for bad in (-0.1, 1.5, nan):
        Tb = np.array(T)
        Tb[E - 1, N // 2] = bad
        with pytest.raises(pkg.capi.MMEEError, match="target is not finite or lies outside"):
            pkg.fit_gate_heads(X, Tb, l2=L2, gtol=GTOL, max_evals=50)
        Xd, Td = _dev(np.array(X), torch.float32), _dev(Tb, torch.float64)
        need = lib.ee_head_fit_workspace_bytes(E, N, H, 2, 8)
        ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
        outs = [torch.full(s, v, dtype=dt, device="cuda") for s, v, dt in (((E, 2, H), nan, torch.float32), ((E, 2), nan, torch.float32),
                ((E, 2, H), nan, torch.float64), ((E, 2), nan, torch.float64), ((E,), nan, torch.float64), ((E,), nan, torch.float64),
                ((E,), 7, torch.int32), ((E,), 7, torch.int32))]
        rc = lib.ee_head_fit_gate(_ptr(Xd), _ptr(Td), E, N, H, L2, GTOL, 50, 8, _ptr(ws), need, *[_ptr(o) for o in outs], _stream())
        assert rc != 0 and "target is not finite or lies outside" in pkg.capi.last_error(), pkg.capi.last_error()
        torch.cuda.synchronize()
        for o in outs[:6]:
            assert bool(torch.isnan(o).all())
        for o in outs[6:]:
            assert bool((o == 7).all())
        with pytest.raises(pkg.capi.MMEEError, match="target is not finite or lies outside"):
            _lossgrad(pkg, X, Tb, np.zeros((E, 2 * H + 2)))
    assert (pkg.fit_gate_heads(X, T, l2=L2, gtol=GTOL).status.cpu().numpy() == 0).all()          # the mended targets go through


def test_refusals_of_the_python_surface(pkg):
    X, T = _problem(1, 63, 4)
    with pytest.raises(ValueError, match="sample_weight"):
        pkg.fit_gate_heads(X, T, sample_weight=np.ones(63))
    two_layer = pkg.ModelConfig.tiny(EE_config=dict(exits=[1, 2], encoder_layer_strategy="gate", exit_head_num_layers=2))
    emb = pkg.ModelConfig.tiny(EE_config=dict(exits=["text_avg", 1], encoder_layer_strategy="gate", exit_head_num_layers=1))
    ramp = pkg.ModelConfig.tiny(EE_config=dict(exits=[1, 2], encoder_layer_strategy="ramp", exit_head_num_layers=1))
    ok = pkg.ModelConfig.tiny(EE_config=dict(exits=[1], encoder_layer_strategy="gate", exit_head_num_layers=1))
    fit = pkg.fit_gate_heads(np.array(X), np.array(T), max_evals=5)
    for cfg, match in ((two_layer, "exit_head_num_layers == 1"), (emb, "embedding-level exits"), (ramp, "gate strategy only")):
        with pytest.raises(ValueError, match=match):
            fit.state_dict(cfg)
    with pytest.raises(ValueError, match=r"the fit is \(E,2,H\)"):
        fit.state_dict(ok)                                        # H = 4 against the configuration's 128
    with pytest.raises(ValueError, match="fit_gate_heads"):
        pkg.heads._check_fittable(pkg.ModelConfig.tiny(EE_config=dict(exits=[1], encoder_layer_strategy="gate", exit_head_num_layers=1)))


# ---- 4. through the engine ----------------------------------------------------------------------------------------------------------------------
def test_dump_targets_fit_load_forward_under_the_gate_criterion(pkg):
    """h256_gate with one-layer heads and encoder exits only (the fit's limits): collect_gate_features -> gate_targets -> fit_gate_heads ->
    load_weights(state_dict) -> forward under inference_strategy = "gate".  out_head_logits equal GateFit's float32 heads on the collected
    rows within 1e-4, all_crit is GateFit.scores, and the forward decides on them."""
    torch = _torch()
    B, T = 96, 48
    ee = dict(MATRIX_CASES["h256_gate"][1], exits=[1, 2], exit_head_num_layers=1, inference_strategy="gate")
    cfg = pkg.ModelConfig.tiny(EE_config=ee, **H256_KW)
    E, H, K = 2, cfg.hidden_size, cfg.num_labels
    W = pkg.synth.make_weights(cfg, seed=51, head_gain=4.0)
    docs = pkg.synth.make_documents(cfg, B, seed=52, text_len=T, min_words=3)
    t = {k: torch.from_numpy(docs[k]).cuda() for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision="split")
    eng.load_weights(W)
    feats, gated = pkg.collect_gate_features(eng, [t])
    assert tuple(feats.shape) == (E, B, H) and feats.dtype == torch.float32 and tuple(gated.shape) == (E, B, K)
    # a document's label is the gated argmax at a randomly chosen exit: the classifier is right at some exits and wrong at others
    rng = np.random.default_rng(53)
    pred = gated.cpu().numpy().argmax(-1)
    y = pred[rng.integers(0, E, B), np.arange(B)].astype(np.int64)
    targets = pkg.gate_targets(gated, torch.from_numpy(y).cuda())
    Tn = targets.cpu().numpy()
    assert targets.dtype == torch.float64 and np.array_equal(Tn, (pred == y[None]).astype(np.float64))
    assert ((Tn.sum(1) > 0) & (Tn.sum(1) < B)).all(), Tn.sum(1)
    fit = pkg.fit_gate_heads(feats, targets, l2=L2, gtol=GTOL)
    print(f"evals {fit.evals.cpu().numpy().tolist()} status {fit.status.cpu().numpy().tolist()} grad norm {fit.grad_norm.cpu().numpy().tolist()}")
    sd = fit.state_dict(cfg)
    assert sorted(sd) == sorted(f"layoutlmv3.encoder.early_exits.{k}.out_proj.{n}" for k in range(E) for n in ("weight", "bias"))
    assert sd["layoutlmv3.encoder.early_exits.0.out_proj.weight"].shape == (2, H) and sd["layoutlmv3.encoder.early_exits.1.out_proj.bias"].shape == (2,)
    assert set(sd) <= set(eng.expected_tensors())
    eng.close()
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision="split")
    eng.load_weights({**W, **sd})
    dump = eng.forward(**t, dump_all=True, want_all=True, want_head=True, want_hidden_cls=True, whole_layers=True)
    want = fit.logits(feats).cpu().numpy()
    got = dump.head_logits.cpu().numpy().astype(np.float64)
    err = float(np.abs(got - want).max())
    report_measured("gate_fit[engine]", "max |head_logits - GateFit.logits|", err)
    assert err <= 1e-4
    scores = fit.scores(feats).cpu().numpy()
    assert float(np.abs(dump.all_crit.cpu().numpy()[:E].astype(np.float64) - scores).max()) <= 1e-4
    g = G.gate_score(dump.head_logits.cpu().numpy())
    thr, ex = G.cascade_thresholds(g)
    out = eng.forward(**t, thresholds=thr, whole_layers=True)
    assert np.array_equal(out.exit_layer.cpu().numpy(), ex) and set(ex.tolist()) == {0, 1, 2}
    # the fitted gates beat the synthetic ones and the zero head on their own objective
    Xn = feats.cpu().numpy()
    for e in range(E):
        theta = np.concatenate([fit.weight64[e].cpu().numpy().reshape(-1), fit.bias64[e].cpu().numpy()])
        syn = np.concatenate([W[f"layoutlmv3.encoder.early_exits.{e}.out_proj.weight"].reshape(-1),
                              W[f"layoutlmv3.encoder.early_exits.{e}.out_proj.bias"].reshape(-1)]).astype(np.float64)
        l_fit = G.gate_lossgrad(theta, Xn[e], Tn[e], L2)[0]
        assert l_fit < G.gate_lossgrad(syn, Xn[e], Tn[e], L2)[0] and l_fit < G.gate_lossgrad(np.zeros_like(theta), Xn[e], Tn[e], L2)[0]
    eng.check()
    eng.close()
