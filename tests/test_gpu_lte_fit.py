"""The LTE classifier fit on the device (include/mmee.h ee_lte_fit) against the float64 restatement and the scipy solution of
tests/lte_fit_ref.py: the loss / gradient kernel alone, the targets and scores kernels, the fit, its determinism and stopping rules, and the
loop dump rows -> targets -> fit -> load -> forward through a use_lte engine.

Tolerance of the kernel-alone comparison: rtol 1e-10, atol 1e-12 (lte_fit_ref.RTOL / ATOL) -- derived, not measured: float64 sums of at most
about 1e5 terms of order 1 and ocml exp / log1p at a few ulp sit four orders below it; tests/test_host_lte_fit.py shows that each subtle fault
of the objective moves a figure by at least ten such bars on the inputs shared with this file (lte_fit_ref.kernel_cases)."""
import ctypes as C
import functools

import numpy as np
import pytest

from . import lte_fit_ref as LR
from .conftest import H256_KW
from .fit_util import _ptr, _stream, _torch
from .lte_ref import gap_thresholds, lte_exits

pytestmark = pytest.mark.gpu

L2, GTOL = 1e-2, 1e-9
RTOL, ATOL = LR.RTOL, LR.ATOL
FIT_SHAPES = [(300, 64, 3), (257, 64, 1), (1000, 256, 2), (600, 768, 1), (96, 256, 3)]       # (N, H, E)
W_NAME, B_NAME = "layoutlmv3.encoder.lte_classifier.weight", "layoutlmv3.encoder.lte_classifier.bias"


def _dev(a, dtype=None):
    torch = _torch()
    return torch.from_numpy(np.array(a)).to(device="cuda", dtype=dtype)          # a copy: the cached problems are read-only


def _code(pkg, loss):
    return {"mse": pkg.capi.LTE_LOSS_MSE, "bce": pkg.capi.LTE_LOSS_BCE}[loss]


def _lossgrad(pkg, X, T, theta, loss, l2=L2):
    """ee_debug_lte_lossgrad on host arrays X (E,N,H) f32, T (E,N), theta (H+1,) f64 -> (loss, grad (H+1,)) host float64."""
    torch = _torch()
    lib = pkg.capi.load()
    E, N, H = X.shape
    Xd, Td, td = _dev(X, torch.float32), _dev(T, torch.float64), _dev(theta, torch.float64)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    grad = torch.full((H + 1,), float("nan"), dtype=torch.float64, device="cuda")
    rc = lib.ee_debug_lte_lossgrad(_ptr(Xd), _ptr(Td), _ptr(td), E, N, H, _code(pkg, loss), l2, _ptr(out), _ptr(grad), _stream())
    pkg.capi.check(rc, None, "ee_debug_lte_lossgrad")
    return float(out.cpu().numpy()[0]), grad.cpu().numpy()


def _assert_matches(got_loss, got_grad, X, T, theta, loss, l2, what):
    want, g = LR.loss_grad(theta, X, T, loss, l2)
    dl = abs(got_loss - want) / (ATOL + RTOL * abs(want))
    dg = (np.abs(got_grad - g) / (ATOL + RTOL * np.abs(g))).max()
    assert dl <= 1.0, (what, "loss", got_loss, want)
    assert dg <= 1.0, (what, "grad", float(np.abs(got_grad - g).max()))
    return max(dl, dg)


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [4, 64, 260, 768, 1024])
def test_lossgrad_kernel_matches_the_restatement(pkg, H):
    """Both losses, E in {1, 3} and N around the unit R of rows (the last unit short by one, full, one row over, two units and a bit) at this H;
    H = 260 has a partly idle last column group, H = 4 a single busy lane."""
    R = pkg.capi.LTE_FIT_ROWS
    rng = np.random.default_rng(H)
    worst = 0.0
    for loss in LR.LOSSES:
        for E in (1, 3):
            for N in (1, R - 1, R, R + 1, 2 * R + 3):
                X = rng.standard_normal((E, N, H)).astype(np.float32)
                T = (rng.random((E, N)) < 0.4).astype(np.float64)
                theta = np.concatenate([rng.standard_normal(H) * (2.0 / np.sqrt(H)), [rng.standard_normal()]])
                got = _lossgrad(pkg, X, T, theta, loss)
                worst = max(worst, _assert_matches(*got, X, T, theta, loss, L2, (H, loss, E, N)))
    print(f"H = {H}: worst difference / tolerance = {worst:.3e}")


@pytest.mark.parametrize("loss", LR.LOSSES)
def test_lossgrad_more_units_than_chunks(pkg, loss):
    """N = 128 R + 5: 129 units in 65 chunks, so a workgroup carries its accumulators across two units and the last chunk is short."""
    R = pkg.capi.LTE_FIT_ROWS
    rng = np.random.default_rng(1)
    N, H, E = 128 * R + 5, 64, 2
    X = rng.standard_normal((E, N, H)).astype(np.float32)
    T = (rng.random((E, N)) < 0.3).astype(np.float64)
    theta = np.concatenate([rng.standard_normal(H) * 0.2, [-0.4]])
    _assert_matches(*_lossgrad(pkg, X, T, theta, loss), X, T, theta, loss, L2, "two units a chunk")


@pytest.mark.parametrize("loss", LR.LOSSES)
@pytest.mark.parametrize("name", list(LR.kernel_cases()))
def test_lossgrad_on_the_inputs_shared_with_the_host_test(pkg, name, loss):
    """Binary, soft and constant targets, and activations near +-770: loss and gradient stay finite and match."""
    X, T, theta = LR.kernel_cases()[name]
    got = _lossgrad(pkg, X, T, theta, loss)
    assert np.isfinite(got[0]) and np.isfinite(got[1]).all()
    _assert_matches(*got, X, T, theta, loss, L2, name)


# ---- 2. targets and scores -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,N,K", [(1, 1, 1), (3, 257, 3), (2, 1000, 16)])
def test_targets_equal_the_restatement_exactly(pkg, E, N, K):
    rng = np.random.default_rng(K)
    logits = rng.integers(-2, 3, (E, N, K)).astype(np.float32)          # small integers: many ties, the first maximum must win
    y = rng.integers(0, K, N)
    got = pkg.lte_targets(logits, y)
    assert got.dtype == _torch().float64 and tuple(got.shape) == (E, N)
    want = LR.targets(logits, y)
    assert np.array_equal(got.cpu().numpy(), want)
    if K > 1:
        assert 0.0 < want.mean() < 1.0


@pytest.mark.parametrize("H", [4, 260, 768])
def test_scores_match_the_restatement(pkg, H):
    """1e-14: both sides sum H products in float64 (a reordering error of a few 1e-16 H^0.5), then one exp and one division."""
    torch = _torch()
    rng = np.random.default_rng(H)
    E, N = 3, 70
    X = rng.standard_normal((E, N, H)).astype(np.float32)
    w = (rng.standard_normal((1, H)) * (2.0 / np.sqrt(H))).astype(np.float32)
    b = np.array([0.3], dtype=np.float32)
    fit = pkg.LteFit(_dev(w), _dev(b), None, None, None, None, None, L2, "mse")
    got = fit.scores(X)
    assert got.dtype == torch.float64 and tuple(got.shape) == (E, N)
    err = float(np.abs(got.cpu().numpy() - LR.scores(X, w, b)).max())
    print(f"H = {H}: max |score - restatement| = {err:.3e}")
    assert err <= 1e-14


# ---- 3. the fit -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(N, H, E):
    X, T = LR.problem(N, H, E, seed=N + H + E)
    X.setflags(write=False)
    T.setflags(write=False)
    return X, T


@functools.lru_cache(maxsize=None)
def _reference(N, H, E, loss):
    """(the reference solution, the distance between the reference's own two starts): solve()'s two runs, shared by the tests."""
    X, T = _problem(N, H, E)
    a, b = LR.solve_starts(X, T, loss, L2, 2)
    spread = float(np.linalg.norm(a - b))
    assert spread <= 1e-6, f"two starts of the scipy reference end {spread:.3e} apart: the problem has more than one basin"
    a.setflags(write=False)
    return a, spread


def _zero_loss(X, T, loss):
    return LR.loss_grad(np.zeros(X.shape[2] + 1), X, T, loss, L2)[0]


@pytest.mark.parametrize("loss", LR.LOSSES)
@pytest.mark.parametrize("N,H,E", FIT_SHAPES)
def test_fit_reaches_the_reference_point(pkg, N, H, E, loss):
    X, T = _problem(N, H, E)
    ref, spread = _reference(N, H, E, loss)
    fit = pkg.fit_lte_classifier(X, T, loss=loss, l2=L2, gtol=GTOL, max_evals=1000)
    status, evals = int(fit.status.cpu()[0]), int(fit.evals.cpu()[0])
    theta = fit.theta64.cpu().numpy()
    l_dev, g_dev = LR.loss_grad(theta, X, T, loss, L2)
    n_dev, n_ref = np.linalg.norm(g_dev), np.linalg.norm(LR.loss_grad(ref, X, T, loss, L2)[1])
    dist = float(np.linalg.norm(theta - ref))
    print(f"(N,H,E) = {(N, H, E)} {loss}: evals {evals} status {status} ||grad(theta_dev)|| {n_dev:.3e} ||grad(theta_ref)|| {n_ref:.3e} "
          f"||theta_dev - theta_ref|| {dist:.3e} reference spread {spread:.3e}")
    assert status == 0, (status, float(fit.grad_norm.cpu()[0]))
    assert 1 <= evals <= 1000
    assert n_dev <= 2 * GTOL, n_dev
    if loss == "bce":
        assert dist <= (n_dev + n_ref) / L2, (dist, (n_dev + n_ref) / L2)           # strong convexity: fails only for another objective
    else:
        assert l_dev <= _zero_loss(X, T, loss)
        bar = max(1e-6, 10.0 * spread)                                                # from the reference alone
        assert dist <= bar, (dist, bar)
    got_loss, got_norm = float(fit.loss.cpu()[0]), float(fit.grad_norm.cpu()[0])
    assert abs(got_loss - l_dev) <= ATOL + RTOL * abs(l_dev), (got_loss, l_dev)
    assert abs(got_norm - n_dev) <= ATOL + RTOL * n_dev, (got_norm, n_dev)
    # the float32 pair is the float64 point rounded
    assert tuple(fit.weight.shape) == (1, H) and tuple(fit.bias.shape) == (1,)
    assert np.array_equal(fit.weight.cpu().numpy().reshape(-1), theta[:H].astype(np.float32))
    assert np.array_equal(fit.bias.cpu().numpy(), theta[H:].astype(np.float32))


# ---- 4. properties -------------------------------------------------------------------------------------------------------------------------------
def _bits(fit):
    return [t.cpu().numpy().tobytes() for t in (fit.weight, fit.bias, fit.theta64, fit.loss, fit.grad_norm, fit.evals, fit.status)]


@pytest.mark.parametrize("loss", LR.LOSSES)
def test_two_calls_return_identical_bits(pkg, loss):
    N, H, E = FIT_SHAPES[0]
    X, T = _problem(N, H, E)
    a = pkg.fit_lte_classifier(X, T, loss=loss, l2=L2, gtol=GTOL, max_evals=1000)
    b = pkg.fit_lte_classifier(X, T, loss=loss, l2=L2, gtol=GTOL, max_evals=1000)
    assert int(a.status.cpu()[0]) == 0 and _bits(a) == _bits(b)


@pytest.mark.parametrize("loss", LR.LOSSES)
def test_max_evals_stops_with_status_1_and_a_loss_not_above_the_start(pkg, loss):
    N, H, E = FIT_SHAPES[0]
    X, T = _problem(N, H, E)
    fit = pkg.fit_lte_classifier(X, T, loss=loss, l2=L2, gtol=GTOL, max_evals=3)
    assert int(fit.status.cpu()[0]) == 1 and int(fit.evals.cpu()[0]) == 3
    got = float(fit.loss.cpu()[0])
    assert got <= _zero_loss(X, T, loss), (got, _zero_loss(X, T, loss))
    l_dev = LR.loss_grad(fit.theta64.cpu().numpy(), X, T, loss, L2)[0]
    assert abs(got - l_dev) <= ATOL + RTOL * abs(l_dev)


@pytest.mark.parametrize("loss", LR.LOSSES)
def test_a_warm_start_from_the_solution_stops_at_once(pkg, loss):
    """From the float64 solution the first evaluation already meets gtol.  From its float32 rounding (a checkpoint's tensors: about 1e-8 away,
    a gradient norm above gtol) the fit ends at the same point; it need not be quicker than from zero, since it starts without curvature pairs."""
    N, H, E = FIT_SHAPES[0]
    X, T = _problem(N, H, E)
    cold = pkg.fit_lte_classifier(X, T, loss=loss, l2=L2, gtol=GTOL, max_evals=1000)
    warm = pkg.fit_lte_classifier(X, T, loss=loss, l2=L2, gtol=GTOL, max_evals=1000, init=cold.theta64)
    print(f"{loss}: cold evals {int(cold.evals.cpu()[0])}, warm evals {int(warm.evals.cpu()[0])}")
    assert int(warm.status.cpu()[0]) == 0 and 1 <= int(warm.evals.cpu()[0]) <= 2
    assert float(np.linalg.norm(warm.theta64.cpu().numpy() - cold.theta64.cpu().numpy())) <= 1e-6
    cfg_like = {W_NAME: cold.weight.cpu().numpy(), B_NAME: cold.bias.cpu().numpy()}
    ckpt = pkg.fit_lte_classifier(X, T, loss=loss, l2=L2, gtol=GTOL, max_evals=1000, init=cfg_like)
    assert int(ckpt.status.cpu()[0]) == 0
    assert float(np.linalg.norm(ckpt.theta64.cpu().numpy() - cold.theta64.cpu().numpy())) <= 1e-6


def test_a_bad_target_fails_the_call_and_leaves_the_outputs_untouched(pkg):
    torch = _torch()
    lib = pkg.capi.load()
    N, H, E = FIT_SHAPES[0]
    X, T = _problem(N, H, E)
    for bad in (1.5, float("nan"), -0.25):
        Tb = T.copy()
        Tb[E - 1, N // 2] = bad
        with pytest.raises(pkg.capi.MMEEError, match="target is outside"):
            pkg.fit_lte_classifier(X, Tb, l2=L2, gtol=GTOL, max_evals=50)
        Xd, Td = _dev(X, torch.float32), _dev(Tb, torch.float64)
        need = lib.ee_lte_fit_workspace_bytes(E, N, H, 8)
        ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
        outs = [torch.full(s, v, dtype=dt, device="cuda") for s, v, dt in (((1, H), 7.0, torch.float32), ((1,), 7.0, torch.float32),
                ((H + 1,), 7.0, torch.float64), ((1,), 7.0, torch.float64), ((1,), 7.0, torch.float64), ((1,), 7, torch.int32), ((1,), 7, torch.int32))]
        rc = lib.ee_lte_fit(_ptr(Xd), _ptr(Td), None, E, N, H, 0, L2, GTOL, 50, 8, _ptr(ws), need, *[_ptr(o) for o in outs], _stream())
        assert rc != 0 and "target is outside" in pkg.capi.last_error()
        torch.cuda.synchronize()
        for o in outs:
            assert bool((o == 7).all())
        with pytest.raises(pkg.capi.MMEEError, match="target is outside"):
            _lossgrad(pkg, X, Tb, np.zeros(H + 1), "mse")
    assert int(pkg.fit_lte_classifier(X, T, l2=L2, gtol=GTOL, max_evals=1000).status.cpu()[0]) == 0       # the mended targets go through


def test_a_bad_label_or_a_nan_logit_fails_lte_targets_and_nothing_is_written(pkg):
    torch = _torch()
    lib = pkg.capi.load()
    rng = np.random.default_rng(5)
    E, N, K = 3, 300, 10
    logits = rng.standard_normal((E, N, K)).astype(np.float32)
    y = rng.integers(0, K, N)
    for what in ("label K", "label -1", "nan logit"):
        lb, yb = logits.copy(), y.copy()
        if what == "nan logit":
            lb[1, N // 3, K - 1] = np.nan
        else:
            yb[N // 2] = K if what == "label K" else -1
        with pytest.raises(pkg.capi.MMEEError, match="label is outside"):
            pkg.lte_targets(lb, yb)
        out = torch.full((E, N), 7.0, dtype=torch.float64, device="cuda")
        ld, yd = _dev(lb, torch.float32), _dev(yb, torch.int64)
        rc = lib.ee_lte_targets(_ptr(ld), _ptr(yd), E, N, K, _ptr(out), _stream())
        assert rc != 0 and "label is outside" in pkg.capi.last_error(), what
        torch.cuda.synchronize()
        assert bool((out == 7).all()), what
    assert np.array_equal(pkg.lte_targets(logits, y).cpu().numpy(), LR.targets(logits, y))


# ---- 5. through the engine ----------------------------------------------------------------------------------------------------------------------
LTE_EE = dict(exits=[1, 2, 3], encoder_layer_strategy="ramp", use_lte=True)
QUANTILE, MIN_GAP = 0.35, 1e-5       # as tests/test_gpu_lte.py: the share an exit releases; >> 2^-23, the rounding of a stored score


@pytest.mark.parametrize("name", ["tiny_f32", "h256_split"])
def test_dump_fit_load_forward(pkg, name):
    torch = _torch()
    B, T = 96, 48
    if name == "h256_split":
        cfg, precision = pkg.ModelConfig.tiny(EE_config=dict(LTE_EE), **H256_KW), "split"
    else:
        cfg, precision = pkg.ModelConfig.tiny(EE_config=dict(LTE_EE)), "fp32"
    ec = cfg.exit_config
    n_emb, E, H = len(ec.embedding_exits), len(ec.encoder_exit_layers), cfg.hidden_size
    assert n_emb == 0 and E == 3
    W = pkg.synth.make_weights(cfg, seed=31, head_gain=4.0)
    docs = pkg.synth.make_documents(cfg, B, seed=32, text_len=T, min_words=3)
    t = {k: torch.from_numpy(docs[k]).cuda() for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision=precision)
    eng.load_weights(W)
    feats, logits = pkg.collect_lte_features(eng, [t])
    assert tuple(feats.shape) == (E, B, H) and feats.is_cuda and feats.dtype == torch.float32
    assert tuple(logits.shape) == (E, B, cfg.num_labels) and logits.dtype == torch.float32
    if name == "tiny_f32":                                              # several batches are concatenated in order
        pf, pl = pkg.collect_lte_features(eng, [{k: v[i:i + 32] for k, v in t.items()} for i in range(0, B, 32)])
        assert float((pf - feats).abs().max()) <= 1e-4 and float((pl - logits).abs().max()) <= 1e-4
    eng.close()

    # a document's label is the argmax at a randomly chosen exit: every exit is right on some documents and wrong on others
    rng = np.random.default_rng(33)
    pred = logits.cpu().numpy().argmax(-1)
    y = pred[rng.integers(0, E, B), np.arange(B)].astype(np.int64)
    targets = pkg.lte_targets(logits, torch.from_numpy(y).cuda())
    Tn = targets.cpu().numpy()
    assert np.array_equal(Tn, LR.targets(logits.cpu().numpy(), y))
    assert ((Tn.sum(1) > 0) & (Tn.sum(1) < B)).all(), Tn.sum(1)
    fit = pkg.fit_lte_classifier(feats, targets, loss="mse", l2=L2, gtol=GTOL)
    print(f"{name}: evals {int(fit.evals.cpu()[0])} status {int(fit.status.cpu()[0])} grad norm {float(fit.grad_norm.cpu()[0]):.3e}")
    sd = fit.state_dict(cfg)
    assert sorted(sd) == sorted([W_NAME, B_NAME])

    eng2 = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision=precision)
    assert set(eng2.expected_tensors()[-2:]) == set(sd)
    eng2.load_weights({**W, **sd})
    dump = eng2.forward(**t, dump_all=True, want_all=True, want_hidden_cls=True)
    assert torch.equal(dump.hidden_cls[ec.encoder_exit_layers], feats)                   # the same call on the same backbone: the same rows
    ac = dump.all_crit.cpu().numpy().astype(np.float64)
    want = fit.scores(feats).cpu().numpy()
    err = float(np.abs(ac[n_emb:n_emb + E] - want).max())
    print(f"{name}: max |all_crit - LteFit.scores| = {err:.3e}")
    assert err <= 2e-7, err                                                               # one float32 rounding of a value in [0, 1]
    assert float(np.abs(want - LR.scores(feats.cpu().numpy(), sd[W_NAME], sd[B_NAME])).max()) <= 1e-14

    thr, width = gap_thresholds(ac, QUANTILE, MIN_GAP, n_emb)
    assert np.all(width >= MIN_GAP)
    want_exits = lte_exits(ac, thr, n_emb)
    out = eng2.forward(**t, thresholds=thr, xprobe=False)
    assert np.array_equal(out.exit_layer.cpu().numpy(), want_exits)
    assert len(np.unique(want_exits)) >= 2, np.bincount(want_exits).tolist()
    eng2.close()

    Xn = feats.cpu().numpy()
    theta_syn = np.concatenate([W[W_NAME].reshape(-1), W[B_NAME].reshape(-1)]).astype(np.float64)
    l_fit = LR.loss_grad(fit.theta64.cpu().numpy(), Xn, Tn, "mse", L2)[0]
    l_syn, l_zero = LR.loss_grad(theta_syn, Xn, Tn, "mse", L2)[0], _zero_loss(Xn, Tn, "mse")
    print(f"{name}: objective fitted {l_fit:.6f}, synthetic classifier {l_syn:.6f}, zero {l_zero:.6f}")
    assert abs(float(fit.loss.cpu()[0]) - l_fit) <= ATOL + RTOL * abs(l_fit)
    assert l_fit < l_syn and l_fit < l_zero
