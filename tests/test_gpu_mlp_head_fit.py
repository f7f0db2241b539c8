"""The two-layer exit-head fit on the device (include/mmee.h ee_mlp_head_fit) against the float64 restatement and the controller port of
tests/mlp_headfit_ref.py: the loss / gradient launches alone, the first steps of a trajectory, the fit to a stationary point, its determinism
and stopping rules, and the loop dump rows -> fit -> load -> forward through the engine.

Tolerance of the launch-alone comparison: rtol 1e-10, atol 1e-12 on the loss and on every gradient entry -- derived, not measured: float64
sums of <= 1e3 terms plus ocml tanh / exp / log at a few ulp sit orders below it."""
import ctypes as C
import functools

import numpy as np
import pytest

from . import headfit_ref as HR
from . import mlp_headfit_ref as MR
from .conftest import H256_KW
from .fit_util import _dev, _gap_thresholds, _ptr, _stream, _torch

pytestmark = pytest.mark.gpu

L2, GTOL = 1e-2, 1e-6
RTOL, ATOL = 1e-10, 1e-12
FIT_SHAPES = [(300, 64, 10, 3), (257, 64, 2, 1), (600, 128, 16, 2)]
OUTPUTS = ("dense_weight", "dense_bias", "weight", "bias", "theta64", "loss", "grad_norm", "evals", "status")


def _lossgrad(pkg, X, y, theta, K, l2=L2):
    """ee_debug_mlp_head_lossgrad on host arrays X (E,N,H) f32, y (N,), theta (E,P) f64 -> (loss (E,), grad (E,P)) host float64."""
    torch = _torch()
    lib = pkg.capi.load()
    E, N, H = X.shape
    Xd, yd, td = _dev(X, torch.float32), _dev(y, torch.int64), _dev(theta, torch.float64)
    loss = torch.full((E,), float("nan"), dtype=torch.float64, device="cuda")
    grad = torch.full((E, MR.param_count(H, K)), float("nan"), dtype=torch.float64, device="cuda")
    rc = lib.ee_debug_mlp_head_lossgrad(_ptr(Xd), _ptr(yd), _ptr(td), E, N, H, K, l2, _ptr(loss), _ptr(grad), _stream())
    pkg.capi.check(rc, None, "ee_debug_mlp_head_lossgrad")
    return loss.cpu().numpy(), grad.cpu().numpy()


def _assert_matches(got_loss, got_grad, X, y, theta, K, l2, what):
    worst = 0.0
    for e in range(X.shape[0]):
        loss, g = MR.loss_grad(theta[e], X[e], y, K, l2)
        dl = abs(got_loss[e] - loss) / (ATOL + RTOL * abs(loss))
        dg = (np.abs(got_grad[e] - g) / (ATOL + RTOL * np.abs(g))).max()
        worst = max(worst, dl, dg)
        assert dl <= 1.0, (what, e, "loss", got_loss[e], loss)
        assert dg <= 1.0, (what, e, "grad", float(np.abs(got_grad[e] - g).max()), int(np.argmax(np.abs(got_grad[e] - g))))
    return worst


def _theta(rng, E, H, K):
    """theta ~ N(0, 1/H): pre-activations and logits of order 1."""
    return rng.standard_normal((E, MR.param_count(H, K))) / np.sqrt(H)


# ---- 1. the loss / gradient launches alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 256, 768, 1024])
def test_lossgrad_matches_the_restatement(pkg, H):
    """Every K, E and N of the grid at this H: N = 1, around a wave's 32 rows, and around the row tile R of the GEMM kernels (the last tile short
    by one, full, one row over, and two tiles and a bit); K below, at and above a 16-wide MFMA block, and K = 64, the whole column tile."""
    R = pkg.capi.MLP_HEAD_FIT_ROWS
    rng = np.random.default_rng(H)
    worst = 0.0
    for K in (2, 10, 16, 64):
        for E in (1, 3):
            theta = _theta(rng, E, H, K)
            for N in (1, 31, 32, 33, R - 1, R, R + 1, 2 * R + 3):
                X = rng.standard_normal((E, N, H)).astype(np.float32)
                y = rng.integers(0, K, N)
                loss, grad = _lossgrad(pkg, X, y, theta, K)
                worst = max(worst, _assert_matches(loss, grad, X, y, theta, K, L2, (H, K, E, N)))
    print(f"H = {H}: worst difference / tolerance = {worst:.3e}")


@pytest.mark.parametrize("H", [4, 68, 132])
def test_lossgrad_ragged_column_tiles(pkg, H):
    """H below one tile, one tile and a column group, two tiles and a column group; H is no multiple of the staged depth either."""
    rng = np.random.default_rng(H)
    N, K, E = 37, 3, 2
    X = rng.standard_normal((E, N, H)).astype(np.float32)
    y = rng.integers(0, K, N)
    theta = _theta(rng, E, H, K)
    loss, grad = _lossgrad(pkg, X, y, theta, K)
    _assert_matches(loss, grad, X, y, theta, K, L2, ("ragged", H))


def test_lossgrad_a_workgroup_walks_many_row_tiles(pkg):
    rng = np.random.default_rng(1)
    N, H, K, E = 4100, 64, 10, 2
    X = rng.standard_normal((E, N, H)).astype(np.float32)
    y = rng.integers(0, K, N)
    theta = _theta(rng, E, H, K)
    loss, grad = _lossgrad(pkg, X, y, theta, K)
    _assert_matches(loss, grad, X, y, theta, K, L2, "many row tiles")


def test_lossgrad_all_labels_equal(pkg):
    rng = np.random.default_rng(2)
    N, H, K, E = 70, 256, 10, 2
    X = rng.standard_normal((E, N, H)).astype(np.float32)
    y = np.full(N, 7)
    theta = _theta(rng, E, H, K)
    loss, grad = _lossgrad(pkg, X, y, theta, K)
    _assert_matches(loss, grad, X, y, theta, K, L2, "all labels equal")


def test_lossgrad_saturated_hidden_units(pkg):
    """Every fourth row of W1 is scaled so that its pre-activation is beyond +-40 on every row of X: tanh is exactly +-1 there and 1 - a^2
    exactly 0, so those rows of dW1 are the penalty alone."""
    rng = np.random.default_rng(4)
    N, H, K, E = 45, 256, 10, 1
    X = (np.abs(rng.standard_normal((E, N, H))) + 0.5).astype(np.float32)
    theta = _theta(rng, E, H, K)
    W1, b1, W2, b2 = MR.split(theta[0], K, H)
    sat = np.arange(0, H, 4)
    sign = np.where(sat % 8 == 0, 1.0, -1.0)
    W1 = W1.copy()
    W1[sat] = sign[:, None] * 80.0 / (H * X.mean()) * np.ones((len(sat), H))
    theta = MR.join(W1, b1, W2, b2)[None]
    pre = X[0].astype(np.float64) @ W1.T + b1
    assert np.abs(pre[:, sat]).min() > 40.0
    assert (1.0 - np.tanh(pre[:, sat]) ** 2 == 0.0).all()
    y = rng.integers(0, K, N)
    loss, grad = _lossgrad(pkg, X, y, theta, K)
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    _assert_matches(loss, grad, X, y, theta, K, L2, "saturated")
    g1 = grad[0][:H * H].reshape(H, H)
    assert np.array_equal(g1[sat], L2 * W1[sat])


def test_lossgrad_logits_that_overflow_an_unshifted_logsumexp(pkg):
    """Positive hidden rows and rows of W2 at the +-770 / (H mean a) scale: logits near +-770, exp(770) = inf in float64."""
    rng = np.random.default_rng(3)
    N, H, K, E = 45, 256, 10, 1
    X = (np.abs(rng.standard_normal((E, N, H))) + 0.5).astype(np.float32)
    W1 = np.abs(rng.standard_normal((H, H))) / (H * X.mean())                  # pre-activations near E|w| ~ 0.8, all positive
    A = np.tanh(X[0].astype(np.float64) @ W1.T)
    sign = np.where(np.arange(K) % 2 == 0, 1.0, -1.0)
    W2 = sign[:, None] * 770.0 / (H * A.mean()) * np.ones((K, H))
    theta = MR.join(W1, np.zeros(H), W2, rng.standard_normal(K))[None]
    z = MR.logits(theta[0], X[0], K)
    assert z.max() > 720.0 and z.min() < -720.0 and not np.isfinite(np.exp(z).sum())
    y = rng.integers(0, K, N)
    loss, grad = _lossgrad(pkg, X, y, theta, K)
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    _assert_matches(loss, grad, X, y, theta, K, L2, "large logits")


# ---- 2. a short trajectory against the port -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,K,E,seed", [(300, 64, 10, 3, 374), (200, 768, 16, 1, 5)])
def test_first_steps_follow_the_port(pkg, N, H, K, E, seed):
    """Twelve evaluations from the identity start: the device's iterate is the port's (the second shape runs the controller at P ~ 600 k)."""
    X, y = MR.problem(N, H, K, E, seed)
    fit = pkg.fit_mlp_exit_heads(X, y, l2=L2, gtol=0.0, max_evals=12, num_labels=K)
    assert (fit.status.cpu().numpy() == 1).all() and (fit.evals.cpu().numpy() == 12).all()
    theta, loss = fit.theta64.cpu().numpy(), fit.loss.cpu().numpy()
    for e in range(E):
        port = MR.lbfgs(lambda th: MR.loss_grad(th, X[e], y, K, L2), MR.init_identity(H, K), 0.0, 12)
        assert port[3] == 12 and port[4] == 1
        diff = np.abs(theta[e] - port[0]).max()
        l_dev = MR.loss_grad(theta[e], X[e], y, K, L2)[0]
        print(f"exit {e}: max |theta64 - port| = {diff:.3e}, loss {loss[e]:.6f} (port {port[1]:.6f})")
        assert diff <= 1e-8, (e, diff)
        assert abs(loss[e] - l_dev) <= ATOL + RTOL * abs(l_dev), (e, loss[e], l_dev)


# ---- 3. the fit to a stationary point -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(N, H, K, E):
    X, y = MR.problem(N, H, K, E, seed=N + H + K)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


@functools.lru_cache(maxsize=None)
def _one_layer_optimum(N, H, K, E):
    X, y = _problem(N, H, K, E)
    return tuple(HR.loss_grad(HR.solve(X[e], y, K, L2), X[e], y, K, L2)[0] for e in range(E))


@pytest.mark.parametrize("N,H,K,E", FIT_SHAPES)
def test_fit_reaches_a_stationary_point_below_the_one_layer_optimum(pkg, N, H, K, E):
    """First run on the device (MI355X), evaluations: two-layer loss against the one-layer optimum, per exit --
    (300,64,10,3): 1719, 641, 781 evaluations: 0.4748 / 0.4939 / 0.4868 against 0.8031 / 0.6809 / 0.6275;
    (257,64,2,1): 691: 0.1034 against 0.1781;  (600,128,16,2): 1592, 1294: 0.6056 / 0.6103 against 0.6959 / 0.6884.
    All status 0 with float64 gradient norms of 8.3e-7 ... 9.4e-7 at the returned points; the start (identity) is at 2.6226, 1.0131 and 3.4126.
    The numpy port ends at 0.4767 / 0.4939 / 0.4868, 0.1034 and 0.6054 / 0.6103 after 609 ... 2102 evaluations: beyond the first steps the
    trajectories part, and for the first exit so does the stationary point reached (the objective is not convex)."""
    X, y = _problem(N, H, K, E)
    one_layer = _one_layer_optimum(N, H, K, E)
    fit = pkg.fit_mlp_exit_heads(X, y, l2=L2, gtol=GTOL, max_evals=4000, num_labels=K)
    status, evals = fit.status.cpu().numpy(), fit.evals.cpu().numpy()
    loss, gnorm, theta = fit.loss.cpu().numpy(), fit.grad_norm.cpu().numpy(), fit.theta64.cpu().numpy()
    print(f"({N},{H},{K},{E}): evals {evals.tolist()} status {status.tolist()} loss {loss.tolist()} one-layer {list(one_layer)}")
    assert (status == 0).all(), (status, gnorm)
    assert (evals >= 1).all() and (evals <= 4000).all(), evals
    HH = H * H
    for e in range(E):
        l_dev, g_dev = MR.loss_grad(theta[e], X[e], y, K, L2)
        n_dev = np.linalg.norm(g_dev)
        l_start = MR.loss_grad(MR.init_identity(H, K), X[e], y, K, L2)[0]
        print(f"exit {e}: ||grad(theta64)|| {n_dev:.3e}  loss {l_dev:.6f}  start {l_start:.6f}  one-layer optimum {one_layer[e]:.6f}")
        assert n_dev <= 2 * GTOL, (e, n_dev)
        assert abs(loss[e] - l_dev) <= ATOL + RTOL * abs(l_dev), (e, loss[e], l_dev)
        assert abs(gnorm[e] - n_dev) <= ATOL + RTOL * n_dev, (e, gnorm[e], n_dev)
        assert loss[e] < l_start, (e, loss[e], l_start)
        assert loss[e] < one_layer[e], (e, loss[e], one_layer[e])
        # the float32 tensors are the float64 point rounded
        th32 = theta[e].astype(np.float32)
        assert np.array_equal(fit.dense_weight[e].cpu().numpy().reshape(-1), th32[:HH])
        assert np.array_equal(fit.dense_bias[e].cpu().numpy(), th32[HH:HH + H])
        assert np.array_equal(fit.weight[e].cpu().numpy().reshape(-1), th32[HH + H:HH + H + K * H])
        assert np.array_equal(fit.bias[e].cpu().numpy(), th32[HH + H + K * H:])


# ---- 4. properties ------------------------------------------------------------------------------------------------------------------------------
def _bits(fit):
    return [getattr(fit, name).cpu().numpy().tobytes() for name in OUTPUTS]


def test_two_calls_return_identical_bits_and_an_exit_fits_alone_as_among_others(pkg):
    N, H, K, E = FIT_SHAPES[0]
    X, y = _problem(N, H, K, E)
    a = pkg.fit_mlp_exit_heads(X, y, l2=L2, gtol=GTOL, num_labels=K)
    b = pkg.fit_mlp_exit_heads(X, y, l2=L2, gtol=GTOL, num_labels=K)
    assert _bits(a) == _bits(b)
    for e in range(E):
        alone = pkg.fit_mlp_exit_heads(X[e:e + 1], y, l2=L2, gtol=GTOL, num_labels=K)
        for name in OUTPUTS:
            got, want = getattr(alone, name)[0].cpu().numpy(), getattr(a, name)[e].cpu().numpy()
            assert got.tobytes() == want.tobytes(), (e, name)


def test_max_evals_stops_with_status_1_and_a_loss_not_above_the_start(pkg):
    N, H, K, E = FIT_SHAPES[0]
    X, y = _problem(N, H, K, E)
    fit = pkg.fit_mlp_exit_heads(X, y, l2=L2, gtol=GTOL, max_evals=3, num_labels=K)
    assert (fit.status.cpu().numpy() == 1).all() and (fit.evals.cpu().numpy() == 3).all()
    loss, theta = fit.loss.cpu().numpy(), fit.theta64.cpu().numpy()
    for e in range(E):
        l_start = MR.loss_grad(MR.init_identity(H, K), X[e], y, K, L2)[0]
        l_dev = MR.loss_grad(theta[e], X[e], y, K, L2)[0]
        assert loss[e] <= l_start, (e, loss[e], l_start)
        assert abs(loss[e] - l_dev) <= ATOL + RTOL * abs(l_dev)


def test_a_warm_start_from_a_stationary_point_stops_after_one_evaluation(pkg):
    N, H, K, E = FIT_SHAPES[1]
    X, y = _problem(N, H, K, E)
    cold = pkg.fit_mlp_exit_heads(X, y, l2=L2, gtol=GTOL, num_labels=K)
    assert (cold.status.cpu().numpy() == 0).all()
    warm = pkg.fit_mlp_exit_heads(X, y, l2=L2, gtol=GTOL, num_labels=K, init=cold.theta64)
    assert (warm.status.cpu().numpy() == 0).all() and (warm.evals.cpu().numpy() == 1).all()
    for name in ("dense_weight", "dense_bias", "weight", "bias", "theta64", "loss", "grad_norm"):
        assert getattr(warm, name).cpu().numpy().tobytes() == getattr(cold, name).cpu().numpy().tobytes(), name
    # the same start, named as a checkpoint names it (float64 tensors, so nothing is rounded on the way)
    HH = H * H
    th = cold.theta64[0]
    named = {"layoutlmv3.encoder.early_exits.0.dense.weight": th[:HH].view(H, H), "layoutlmv3.encoder.early_exits.0.dense.bias": th[HH:HH + H],
             "layoutlmv3.encoder.early_exits.0.out_proj.weight": th[HH + H:HH + H + K * H].view(K, H),
             "layoutlmv3.encoder.early_exits.0.out_proj.bias": th[HH + H + K * H:]}
    again = pkg.fit_mlp_exit_heads(X, y, l2=L2, gtol=GTOL, num_labels=K, init=named)
    assert (again.evals.cpu().numpy() == 1).all() and again.theta64.cpu().numpy().tobytes() == cold.theta64.cpu().numpy().tobytes()


def test_a_label_out_of_range_fails_the_call_and_leaves_the_outputs_untouched(pkg):
    torch = _torch()
    lib = pkg.capi.load()
    N, H, K, E = FIT_SHAPES[0]
    X, y = _problem(N, H, K, E)
    P = MR.param_count(H, K)
    for bad in (K, -1):
        yb = y.copy()
        yb[N // 2] = bad
        with pytest.raises(pkg.capi.MMEEError, match="label is outside"):
            pkg.fit_mlp_exit_heads(X, yb, l2=L2, gtol=GTOL, max_evals=50, num_labels=K)
        Xd, yd = _dev(X, torch.float32), _dev(yb, torch.int64)
        th0 = _dev(np.stack([MR.init_identity(H, K)] * E), torch.float64)
        need = lib.ee_mlp_head_fit_workspace_bytes(E, N, H, K, 8)
        ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
        outs = [torch.full(s, v, dtype=dt, device="cuda") for s, v, dt in (((E, H, H), 7.0, torch.float32), ((E, H), 7.0, torch.float32),
                ((E, K, H), 7.0, torch.float32), ((E, K), 7.0, torch.float32), ((E, P), 7.0, torch.float64), ((E,), 7.0, torch.float64),
                ((E,), 7.0, torch.float64), ((E,), 7, torch.int32), ((E,), 7, torch.int32))]
        rc = lib.ee_mlp_head_fit(_ptr(Xd), _ptr(yd), _ptr(th0), E, N, H, K, L2, GTOL, 50, 8, _ptr(ws), need, *[_ptr(o) for o in outs], _stream())
        assert rc != 0 and "label is outside" in pkg.capi.last_error()
        torch.cuda.synchronize()
        for o in outs:
            assert bool((o == 7).all())
    ok = pkg.fit_mlp_exit_heads(X, y, l2=L2, gtol=GTOL, max_evals=50, num_labels=K)                     # the mended labels go through
    assert (ok.status.cpu().numpy() == 1).all()


# ---- 5. through the engine ----------------------------------------------------------------------------------------------------------------------
EE_2LAYER = dict(exits=[1, 2, 3], encoder_layer_strategy="ramp", inference_strategy="max_confidence", exit_head_num_layers=2)


@pytest.mark.parametrize("name", ["tiny_f32", "h256_split", "dit_tiny"])
def test_dump_fit_load_forward(pkg, name):
    torch = _torch()
    B, T = 96, 48
    if name == "dit_tiny":
        cfg, precision, mk = pkg.ModelConfig.dit_tiny(EE_config=dict(EE_2LAYER)), "fp32", pkg.synth.make_weights_beit
    elif name == "h256_split":
        cfg, precision, mk = pkg.ModelConfig.tiny(EE_config=dict(EE_2LAYER), **H256_KW), "split", pkg.synth.make_weights
    else:
        cfg, precision, mk = pkg.ModelConfig.tiny(EE_config=dict(EE_2LAYER)), "fp32", pkg.synth.make_weights
    K, H = cfg.num_labels, cfg.hidden_size
    W = mk(cfg, seed=21)
    docs = pkg.synth.make_documents(cfg, B, seed=22, text_len=T, min_words=3)
    keys = ("pixel_values",) if cfg.arch == "beit" else ("input_ids", "attention_mask", "bbox", "pixel_values")
    t = {k: torch.from_numpy(docs[k]).cuda() for k in keys}
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision=precision)
    eng.load_weights(W)
    with pytest.raises(ValueError, match="exit_head_num_layers == 1"):
        pkg.collect_exit_features(eng, [t])
    feats = pkg.collect_exit_features(eng, [t], head_layers=2)
    assert tuple(feats.shape) == (3, B, H) and feats.is_cuda and feats.dtype == torch.float32
    head_names = [n for n in eng.expected_tensors() if "early_exits" in n]
    eng.close()

    rng = np.random.default_rng(23)
    fh = feats.cpu().numpy()
    teacher = rng.standard_normal((K, H)) * (2.0 / np.sqrt(H))
    y = (fh[-1].astype(np.float64) @ teacher.T + rng.gumbel(size=(B, K))).argmax(-1).astype(np.int64)
    fit = pkg.fit_mlp_exit_heads(feats, torch.from_numpy(y).cuda(), l2=L2, gtol=GTOL, max_evals=4000, num_labels=K)
    status, loss = fit.status.cpu().numpy(), fit.loss.cpu().numpy()
    print(f"{name}: evals {fit.evals.cpu().tolist()} status {status.tolist()} loss {loss.tolist()} grad norms {fit.grad_norm.cpu().tolist()}")
    assert np.isin(status, (0, 1)).all(), status
    for e in range(3):
        l_start = MR.loss_grad(MR.init_identity(H, K), fh[e], y, K, L2)[0]
        assert loss[e] < l_start, (e, loss[e], l_start)
    sd = fit.state_dict(cfg)
    assert sorted(sd) == sorted(head_names)

    eng2 = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision=precision)
    eng2.load_weights({**W, **sd})
    dump = eng2.forward(**t, dump_all=True, want_head=True, want_all=True, want_hidden_cls=True)
    assert torch.equal(dump.hidden_cls[cfg.exit_config.encoder_exit_layers], feats)       # the same call on the same backbone: the same rows
    want = fit.logits(feats).cpu().numpy()
    err = np.abs(dump.head_logits.cpu().numpy().astype(np.float64) - want).max()
    print(f"{name}: max |head_logits - MlpHeadFit.logits| = {err:.3e}")
    assert err <= 1e-4, err

    logits = dump.all_logits.to(torch.float64)
    z = logits.cpu().numpy()
    p = np.exp(z - z.max(-1, keepdims=True))
    conf = (p / p.sum(-1, keepdims=True)).max(-1)
    thr = _gap_thresholds(conf)
    assert np.abs(conf - thr[:, None])[:-1].min() > 1e-6, "thresholds too close to a confidence"       # the last exit takes whoever is left
    want_exits = pkg.criterion_scan_device(logits, thr, "max_confidence")[0].cpu().numpy()
    out = eng2.forward(**t, thresholds=thr, xprobe=False)
    assert np.array_equal(out.exit_layer.cpu().numpy(), want_exits)
    assert len(np.unique(want_exits)) >= 2
    eng2.close()
