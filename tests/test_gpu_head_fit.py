"""The exit-head fit on the device (include/mmee.h ee_head_fit) against the float64 restatement and the scipy solution of tests/headfit_ref.py:
the loss / gradient kernel alone, the fit, its determinism and stopping rules, and the loop dump rows -> fit -> load -> forward through the engine.

Tolerance of the kernel-alone comparison: rtol 1e-10, atol 1e-12 -- derived, not measured: float64 sums of <= 1e3 terms and ocml exp / log at a
few ulp sit four orders below it."""
import ctypes as C
import functools

import numpy as np
import pytest

from . import headfit_ref as HR
from .conftest import H256_KW
from .fit_util import _dev, _gap_thresholds, _ptr, _stream, _torch

pytestmark = pytest.mark.gpu

L2, GTOL = 1e-2, 1e-9
RTOL, ATOL = 1e-10, 1e-12
FIT_SHAPES = [(300, 64, 10, 3), (257, 64, 2, 1), (1000, 256, 16, 2), (600, 768, 16, 1)]


def _lossgrad(pkg, X, y, theta, K, l2=L2):
    """ee_debug_head_lossgrad on host arrays X (E,N,H) f32, y (N,), theta (E,P) f64 -> (loss (E,), grad (E,P)) host float64."""
    torch = _torch()
    lib = pkg.capi.load()
    E, N, H = X.shape
    Xd, yd, td = _dev(X, torch.float32), _dev(y, torch.int64), _dev(theta, torch.float64)
    loss = torch.full((E,), float("nan"), dtype=torch.float64, device="cuda")
    grad = torch.full((E, K * H + K), float("nan"), dtype=torch.float64, device="cuda")
    rc = lib.ee_debug_head_lossgrad(_ptr(Xd), _ptr(yd), _ptr(td), E, N, H, K, l2, _ptr(loss), _ptr(grad), _stream())
    pkg.capi.check(rc, None, "ee_debug_head_lossgrad")
    return loss.cpu().numpy(), grad.cpu().numpy()


def _assert_matches(got_loss, got_grad, X, y, theta, K, l2, what):
    worst = 0.0
    for e in range(X.shape[0]):
        loss, g = HR.loss_grad(theta[e], X[e], y, K, l2)
        dl = abs(got_loss[e] - loss) / (ATOL + RTOL * abs(loss))
        dg = (np.abs(got_grad[e] - g) / (ATOL + RTOL * np.abs(g))).max()
        worst = max(worst, dl, dg)
        assert dl <= 1.0, (what, e, "loss", got_loss[e], loss)
        assert dg <= 1.0, (what, e, "grad", float(np.abs(got_grad[e] - g).max()))
    return worst


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 256, 768, 1024])
def test_lossgrad_kernel_matches_the_restatement(pkg, H):
    """Every K, E and N of the issue at this H: N around the slab height S (the last slab short by one, full, one row over, and two slabs
    and a bit), K below, at and above the class tiles of the kernel."""
    S = pkg.capi.HEAD_FIT_SLAB
    rng = np.random.default_rng(H)
    worst = 0.0
    for K in (2, 10, 16, 64):
        for E in (1, 3):
            for N in (1, S - 1, S, S + 1, 2 * S + 3):
                X = rng.standard_normal((E, N, H)).astype(np.float32)
                y = rng.integers(0, K, N)
                theta = rng.standard_normal((E, K * H + K)) * (1.0 / np.sqrt(H))
                loss, grad = _lossgrad(pkg, X, y, theta, K)
                worst = max(worst, _assert_matches(loss, grad, X, y, theta, K, L2, (H, K, E, N)))
    print(f"H = {H}: worst difference / tolerance = {worst:.3e}")


def test_lossgrad_more_rows_than_one_chunk_holds_in_one_slab(pkg):
    """N = 128 S + 5: more slabs than chunks, so a workgroup carries its gradient over two slabs and the last chunk is short."""
    S = pkg.capi.HEAD_FIT_SLAB
    rng = np.random.default_rng(1)
    N, H, K, E = 128 * S + 5, 64, 10, 2
    X = rng.standard_normal((E, N, H)).astype(np.float32)
    y = rng.integers(0, K, N)
    theta = rng.standard_normal((E, K * H + K)) * 0.1
    loss, grad = _lossgrad(pkg, X, y, theta, K)
    _assert_matches(loss, grad, X, y, theta, K, L2, "two slabs a chunk")


def test_lossgrad_all_labels_equal(pkg):
    rng = np.random.default_rng(2)
    N, H, K, E = 70, 256, 10, 2
    X = rng.standard_normal((E, N, H)).astype(np.float32)
    y = np.full(N, 7)
    theta = rng.standard_normal((E, K * H + K)) * 0.05
    loss, grad = _lossgrad(pkg, X, y, theta, K)
    _assert_matches(loss, grad, X, y, theta, K, L2, "all labels equal")


def test_lossgrad_logits_that_overflow_an_unshifted_logsumexp(pkg):
    """Positive features and rows of W at the +-770 / (H mean x) scale: logits near +-770, exp(770) = inf in float64."""
    rng = np.random.default_rng(3)
    N, H, K, E = 45, 256, 10, 1
    X = (np.abs(rng.standard_normal((E, N, H))) + 0.5).astype(np.float32)
    sign = np.where(np.arange(K) % 2 == 0, 1.0, -1.0)
    W = sign[:, None] * 770.0 / (H * X.mean()) * np.ones((K, H))
    theta = np.concatenate([W.reshape(-1), rng.standard_normal(K)])[None]
    z = HR.logits(theta[0], X[0], K)
    assert z.max() > 720.0 and z.min() < -720.0 and not np.isfinite(np.exp(z).sum())
    y = rng.integers(0, K, N)
    loss, grad = _lossgrad(pkg, X, y, theta, K)
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    _assert_matches(loss, grad, X, y, theta, K, L2, "large logits")


# ---- 2. the fit -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(N, H, K, E):
    X, y = HR.teacher_problem(N, H, K, E, seed=N + H + K)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


@functools.lru_cache(maxsize=None)
def _reference(N, H, K, E):
    X, y = _problem(N, H, K, E)
    ref = np.stack([HR.solve(X[e], y, K, L2) for e in range(E)])
    ref.setflags(write=False)
    return ref


def _theta64(fit):
    E = fit.weight64.shape[0]
    return np.concatenate([fit.weight64.cpu().numpy().reshape(E, -1), fit.bias64.cpu().numpy()], axis=1)


@pytest.mark.parametrize("N,H,K,E", FIT_SHAPES)
def test_fit_reaches_the_optimum(pkg, N, H, K, E):
    X, y = _problem(N, H, K, E)
    ref = _reference(N, H, K, E)
    fit = pkg.fit_exit_heads(X, y, l2=L2, gtol=GTOL, max_evals=200, num_labels=K)
    status, evals = fit.status.cpu().numpy(), fit.evals.cpu().numpy()
    loss, gnorm = fit.loss.cpu().numpy(), fit.grad_norm.cpu().numpy()
    theta = _theta64(fit)
    z_dev = fit.logits(X).cpu().numpy()
    print("evals", evals, "status", status, "grad_norm", gnorm)
    assert (status == 0).all(), status
    assert (evals >= 1).all() and (evals <= 200).all(), evals
    for e in range(E):
        l_dev, g_dev = HR.loss_grad(theta[e], X[e], y, K, L2)
        g_ref = HR.loss_grad(ref[e], X[e], y, K, L2)[1]
        n_dev, n_ref = np.linalg.norm(g_dev), np.linalg.norm(g_ref)
        dist = np.linalg.norm(theta[e] - ref[e])
        dz = np.abs(z_dev[e] - HR.logits(ref[e], X[e], K)).max()
        print(f"exit {e}: ||grad(theta_dev)|| {n_dev:.3e}  ||grad(theta_ref)|| {n_ref:.3e}  ||theta_dev - theta_ref|| {dist:.3e}  max |dz| {dz:.3e}")
        assert n_dev <= 2 * GTOL, (e, n_dev)
        assert dist <= (n_dev + n_ref) / L2, (e, dist, (n_dev + n_ref) / L2)       # strong convexity: fails only for another objective
        assert dz <= 1e-4, (e, dz)
        assert abs(loss[e] - l_dev) <= ATOL + RTOL * abs(l_dev), (e, loss[e], l_dev)
        assert abs(gnorm[e] - n_dev) <= ATOL + RTOL * n_dev, (e, gnorm[e], n_dev)
        # the float32 pair is the float64 solution rounded
        assert np.array_equal(fit.weight[e].cpu().numpy().reshape(-1), theta[e][:K * H].astype(np.float32))
        assert np.array_equal(fit.bias[e].cpu().numpy(), theta[e][K * H:].astype(np.float32))


# ---- 3. properties -------------------------------------------------------------------------------------------------------------------------------
def _bits(fit):
    return [t.cpu().numpy().tobytes() for t in (fit.weight, fit.bias, fit.weight64, fit.bias64, fit.loss, fit.grad_norm, fit.evals, fit.status)]


def test_two_calls_return_identical_bits_and_an_exit_fits_alone_as_among_others(pkg):
    N, H, K, E = FIT_SHAPES[0]
    X, y = _problem(N, H, K, E)
    a = pkg.fit_exit_heads(X, y, l2=L2, gtol=GTOL, num_labels=K)
    b = pkg.fit_exit_heads(X, y, l2=L2, gtol=GTOL, num_labels=K)
    assert _bits(a) == _bits(b)
    for e in range(E):
        alone = pkg.fit_exit_heads(X[e:e + 1], y, l2=L2, gtol=GTOL, num_labels=K)
        for name in ("weight", "bias", "weight64", "bias64", "loss", "grad_norm", "evals", "status"):
            got, want = getattr(alone, name)[0].cpu().numpy(), getattr(a, name)[e].cpu().numpy()
            assert got.tobytes() == want.tobytes(), (e, name)


def test_max_evals_stops_with_status_1_and_a_loss_not_above_the_start(pkg):
    N, H, K, E = FIT_SHAPES[0]
    X, y = _problem(N, H, K, E)
    fit = pkg.fit_exit_heads(X, y, l2=L2, gtol=GTOL, max_evals=3, num_labels=K)
    assert (fit.status.cpu().numpy() == 1).all() and (fit.evals.cpu().numpy() == 3).all()
    at_zero = np.log(K)                                                 # L(0): uniform probabilities, no penalty
    loss = fit.loss.cpu().numpy()
    assert (loss <= at_zero).all(), (loss, at_zero)
    theta = _theta64(fit)
    for e in range(E):
        l_dev = HR.loss_grad(theta[e], X[e], y, K, L2)[0]
        assert abs(loss[e] - l_dev) <= ATOL + RTOL * abs(l_dev)


def test_a_label_out_of_range_fails_the_call_and_leaves_the_outputs_untouched(pkg):
    torch = _torch()
    lib = pkg.capi.load()
    N, H, K, E = FIT_SHAPES[0]
    X, y = _problem(N, H, K, E)
    for bad in (K, -1):
        yb = y.copy()
        yb[N // 2] = bad
        with pytest.raises(pkg.capi.MMEEError, match="label is outside"):
            pkg.fit_exit_heads(X, yb, l2=L2, gtol=GTOL, num_labels=K)
        Xd, yd = _dev(X, torch.float32), _dev(yb, torch.int64)
        need = lib.ee_head_fit_workspace_bytes(E, N, H, K, 8)
        ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
        outs = [torch.full(s, v, dtype=dt, device="cuda") for s, v, dt in (((E, K, H), 7.0, torch.float32), ((E, K), 7.0, torch.float32),
                ((E, K, H), 7.0, torch.float64), ((E, K), 7.0, torch.float64), ((E,), 7.0, torch.float64), ((E,), 7.0, torch.float64),
                ((E,), 7, torch.int32), ((E,), 7, torch.int32))]
        rc = lib.ee_head_fit(_ptr(Xd), _ptr(yd), E, N, H, K, L2, GTOL, 50, 8, _ptr(ws), need, *[_ptr(o) for o in outs], _stream())
        assert rc != 0 and "label is outside" in pkg.capi.last_error()
        torch.cuda.synchronize()
        for o in outs:
            assert bool((o == 7).all())
    assert (pkg.fit_exit_heads(X, y, l2=L2, gtol=GTOL, num_labels=K).status.cpu().numpy() == 0).all()      # the mended labels go through


# ---- 4. through the engine ----------------------------------------------------------------------------------------------------------------------
EE_1LAYER = dict(exits=[1, 2, 3], encoder_layer_strategy="ramp", inference_strategy="max_confidence", exit_head_num_layers=1)


@pytest.mark.parametrize("name", ["tiny_f32", "h256_split", "dit_tiny"])
def test_dump_fit_load_forward(pkg, name):
    torch = _torch()
    B, T = 96, 48
    if name == "dit_tiny":
        cfg, precision, mk = pkg.ModelConfig.dit_tiny(EE_config=dict(EE_1LAYER)), "fp32", pkg.synth.make_weights_beit
    elif name == "h256_split":
        cfg, precision, mk = pkg.ModelConfig.tiny(EE_config=dict(EE_1LAYER), **H256_KW), "split", pkg.synth.make_weights
    else:
        cfg, precision, mk = pkg.ModelConfig.tiny(EE_config=dict(EE_1LAYER)), "fp32", pkg.synth.make_weights
    K, H = cfg.num_labels, cfg.hidden_size
    W = mk(cfg, seed=21)
    docs = pkg.synth.make_documents(cfg, B, seed=22, text_len=T, min_words=3)
    keys = ("pixel_values",) if cfg.arch == "beit" else ("input_ids", "attention_mask", "bbox", "pixel_values")
    t = {k: torch.from_numpy(docs[k]).cuda() for k in keys}
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision=precision)
    eng.load_weights(W)
    feats = pkg.collect_exit_features(eng, [t])
    assert tuple(feats.shape) == (3, B, H) and feats.is_cuda and feats.dtype == torch.float32
    if name == "tiny_f32":                                              # several batches are concatenated in order
        parts = pkg.collect_exit_features(eng, [{k: v[i:i + 32] for k, v in t.items()} for i in range(0, B, 32)])
        assert tuple(parts.shape) == (3, B, H) and float((parts - feats).abs().max()) <= 1e-4
    head_names = [n for n in eng.expected_tensors() if "early_exits" in n]
    eng.close()

    rng = np.random.default_rng(23)
    last = feats[-1].cpu().numpy().astype(np.float64)
    teacher = rng.standard_normal((K, H)) * (2.0 / np.sqrt(H))
    y = (last @ teacher.T + rng.gumbel(size=(B, K))).argmax(-1).astype(np.int64)
    # CLS rows of one backbone share a large common component: worse conditioned than the unit-variance problems above, hence the larger budget
    fit = pkg.fit_exit_heads(feats, torch.from_numpy(y).cuda(), l2=L2, gtol=GTOL, max_evals=2000, num_labels=K)
    print(f"{name}: evals {fit.evals.cpu().tolist()} status {fit.status.cpu().tolist()} grad norms {fit.grad_norm.cpu().tolist()}")
    assert (fit.status.cpu().numpy() == 0).all(), (fit.status, fit.grad_norm)
    sd = fit.state_dict(cfg)
    assert sorted(sd) == sorted(head_names)

    eng2 = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision=precision)
    eng2.load_weights({**W, **sd})
    dump = eng2.forward(**t, dump_all=True, want_head=True, want_all=True, want_hidden_cls=True)
    assert torch.equal(dump.hidden_cls[cfg.exit_config.encoder_exit_layers], feats)       # the same call on the same backbone: the same rows
    want = fit.logits(feats).cpu().numpy()
    err = np.abs(dump.head_logits.cpu().numpy().astype(np.float64) - want).max()
    print(f"{name}: max |head_logits - HeadFit.logits| = {err:.3e}")
    assert err <= 1e-4, err

    logits = dump.all_logits.to(torch.float64)
    z = logits.cpu().numpy()
    p = np.exp(z - z.max(-1, keepdims=True))
    conf = (p / p.sum(-1, keepdims=True)).max(-1)
    thr = _gap_thresholds(conf)
    # The forward below (f32 back end, or split with the K | V probe) decides on the bits of the dumped rows, so any gap would do; 1e-6 is ten
    # float32 steps of a confidence.  The synthetic pages of the DiT case differ little: its confidences lie within 1e-4 of each other.
    assert np.abs(conf - thr[:, None])[:-1].min() > 1e-6, "thresholds too close to a confidence"       # the last exit takes whoever is left
    want_exits = pkg.criterion_scan_device(logits, thr, "max_confidence")[0].cpu().numpy()
    out = eng2.forward(**t, thresholds=thr, xprobe=False)
    assert np.array_equal(out.exit_layer.cpu().numpy(), want_exits)
    assert len(np.unique(want_exits)) >= 2
    eng2.close()
