"""The distilled exit-head fits on the device (include/mmee.h ee_head_fit_distill, ee_mlp_head_fit_distill) against the float64 restatement and
the scipy solution of tests/distill_headfit_ref.py: the loss / gradient kernels alone, extremes of teacher and student logits, the fit, that
alpha = 1 never looks at labels, determinism, failures, the two-layer head, and the loop dump rows -> fit -> load -> forward through the engine.

Tolerance of the kernel-alone comparisons: rtol 1e-10, atol 1e-12, the bar of tests/test_gpu_head_fit.py and tests/test_gpu_mlp_head_fit.py
-- derived, not measured: float64 sums of <= 1e3 terms and ocml exp / log / tanh at a few ulp sit four orders below it; the mixed row step
adds two more softmaxes of <= 64 terms and no longer sum."""
import functools

import numpy as np
import pytest

from . import distill_headfit_ref as DR
from . import headfit_ref as HR
from . import mlp_headfit_ref as MR
from .conftest import H256_KW
from .fit_util import _dev, _ptr, _stream, _torch
from .test_gpu_head_fit import FIT_SHAPES

pytestmark = pytest.mark.gpu

L2, GTOL, MLP_GTOL = 1e-2, 1e-9, 1e-6
RTOL, ATOL = 1e-10, 1e-12
PAIRS = [(1.0, 1.0), (0.5, 2.0), (0.25, 0.5), (0.0, 1.0)]
FIT_PAIRS = [(1.0, 1.0), (0.5, 2.0), (1.0, 4.0)]
HEAD_OUTPUTS = ("weight", "bias", "weight64", "bias64", "loss", "grad_norm", "evals", "status")


def _lossgrad(pkg, X, t, y, theta, K, alpha, T, l2=L2, mlp=False):
    """ee_debug_(mlp_)head_distill_lossgrad on host arrays X (E,N,H) f32, t (N,K) f32, y (N,) or None, theta (E,P) f64 -> (loss (E,),
    grad (E,P)) host float64."""
    torch = _torch()
    lib = pkg.capi.load()
    E, N, H = X.shape
    name = "ee_debug_mlp_head_distill_lossgrad" if mlp else "ee_debug_head_distill_lossgrad"
    Xd, td, thd = _dev(X, torch.float32), _dev(t, torch.float32), _dev(theta, torch.float64)
    yd = None if y is None else _dev(y, torch.int64)
    loss = torch.full((E,), float("nan"), dtype=torch.float64, device="cuda")
    grad = torch.full((E, theta.shape[1]), float("nan"), dtype=torch.float64, device="cuda")
    rc = getattr(lib, name)(_ptr(Xd), _ptr(td), _ptr(yd), _ptr(thd), E, N, H, K, alpha, T, l2, _ptr(loss), _ptr(grad), _stream())
    pkg.capi.check(rc, None, name)
    return loss.cpu().numpy(), grad.cpu().numpy()


def _assert_close(got_loss, got_grad, want_loss, want_grad, what):
    dl = abs(got_loss - want_loss) / (ATOL + RTOL * abs(want_loss))
    dg = (np.abs(got_grad - want_grad) / (ATOL + RTOL * np.abs(want_grad))).max()
    assert dl <= 1.0, (what, "loss", got_loss, want_loss)
    assert dg <= 1.0, (what, "grad", float(np.abs(got_grad - want_grad).max()), int(np.argmax(np.abs(got_grad - want_grad))))
    return max(dl, dg)


def _assert_matches(got_loss, got_grad, X, t, y, theta, K, alpha, T, what, mlp=False):
    ref = DR.mlp_loss_grad if mlp else DR.loss_grad
    worst = 0.0
    for e in range(X.shape[0]):
        loss, g = ref(theta[e], X[e], t, None if alpha == 1.0 else y, K, alpha, T, L2)
        worst = max(worst, _assert_close(got_loss[e], got_grad[e], loss, g, (what, e)))
    return worst


def _hard_lossgrad(pkg, X, y, theta, K):
    from .test_gpu_head_fit import _lossgrad as hard
    return hard(pkg, X, y, theta, K)


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 256, 768, 1024])
def test_lossgrad_kernel_matches_the_restatement(pkg, H):
    """Every K, E and N of tests/test_gpu_head_fit.py at this H.  The pair (alpha, T) moves on with every case: a K has ten cases in a row, so
    every K (and every H) meets all four pairs.  alpha = 1 passes no labels at all.  At alpha = 0 the result is ee_debug_head_lossgrad's too."""
    S = pkg.capi.HEAD_FIT_SLAB
    rng = np.random.default_rng(H)
    worst, case, met = 0.0, 0, set()
    for K in (2, 10, 16, 64):
        for E in (1, 3):
            for N in (1, S - 1, S, S + 1, 2 * S + 3):
                alpha, T = PAIRS[case % len(PAIRS)]
                case += 1
                met.add((K, alpha, T))
                X = rng.standard_normal((E, N, H)).astype(np.float32)
                t = (3.0 * rng.standard_normal((N, K))).astype(np.float32)
                y = rng.integers(0, K, N)
                theta = rng.standard_normal((E, K * H + K)) * (1.0 / np.sqrt(H))
                loss, grad = _lossgrad(pkg, X, t, None if alpha == 1.0 else y, theta, K, alpha, T)
                worst = max(worst, _assert_matches(loss, grad, X, t, y, theta, K, alpha, T, (H, K, E, N, alpha, T)))
                if alpha == 0.0:
                    hl, hg = _hard_lossgrad(pkg, X, y, theta, K)
                    for e in range(E):
                        _assert_close(loss[e], grad[e], hl[e], hg[e], ("against ee_debug_head_lossgrad", H, K, E, N, e))
    assert len(met) == 16
    print(f"H = {H}: worst difference / tolerance = {worst:.3e}")


@pytest.mark.parametrize("alpha,T", [(0.5, 2.0), (1.0, 1.0)])
def test_lossgrad_more_rows_than_one_chunk_holds_in_one_slab(pkg, alpha, T):
    """N = 128 S + 5: more slabs than chunks, so a workgroup carries its gradient over two slabs and the last chunk is short."""
    S = pkg.capi.HEAD_FIT_SLAB
    rng = np.random.default_rng(1)
    N, H, K, E = 128 * S + 5, 64, 10, 2
    X = rng.standard_normal((E, N, H)).astype(np.float32)
    t = (3.0 * rng.standard_normal((N, K))).astype(np.float32)
    y = rng.integers(0, K, N)
    theta = rng.standard_normal((E, K * H + K)) * 0.1
    loss, grad = _lossgrad(pkg, X, t, None if alpha == 1.0 else y, theta, K, alpha, T)
    _assert_matches(loss, grad, X, t, y, theta, K, alpha, T, "two slabs a chunk")


# ---- 2. extremes -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,T", PAIRS[:3])
def test_lossgrad_teacher_that_underflows_and_logits_that_overflow(pkg, alpha, T):
    """Teacher rows of +-3000: q is one 1 and exact zeros at every T used here (the shifted logit of the others is -6000 / T <= -1500).
    Student logits near +-770 as in tests/test_gpu_head_fit.py: exp(770) = inf in float64."""
    rng = np.random.default_rng(3)
    N, H, K, E = 45, 256, 10, 1
    X = (np.abs(rng.standard_normal((E, N, H))) + 0.5).astype(np.float32)
    sign = np.where(np.arange(K) % 2 == 0, 1.0, -1.0)
    W = sign[:, None] * 770.0 / (H * X.mean()) * np.ones((K, H))
    theta = np.concatenate([W.reshape(-1), rng.standard_normal(K)])[None]
    z = HR.logits(theta[0], X[0], K)
    assert z.max() > 720.0 and z.min() < -720.0 and not np.isfinite(np.exp(z).sum())
    t = np.full((N, K), -3000.0, dtype=np.float32)
    t[np.arange(N), rng.integers(0, K, N)] = 3000.0
    q = np.exp((t.astype(np.float64) - 3000.0) / T)
    assert ((q == 0.0).sum(axis=1) == K - 1).all()
    y = rng.integers(0, K, N)
    loss, grad = _lossgrad(pkg, X, t, None if alpha == 1.0 else y, theta, K, alpha, T)
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    _assert_matches(loss, grad, X, t, y, theta, K, alpha, T, "extremes")


# ---- 3. the fit -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(N, H, K, E):
    X, y, t = DR.fit_problem(N, H, K, E)
    for a in (X, y, t):
        a.setflags(write=False)
    return X, y, t


@functools.lru_cache(maxsize=None)
def _reference(N, H, K, E, alpha, T):
    X, y, t = _problem(N, H, K, E)
    ref = np.stack([DR.solve(X[e], t, None if alpha == 1.0 else y, K, alpha, T, L2) for e in range(E)])
    ref.setflags(write=False)
    return ref


def _theta64(fit):
    E = fit.weight64.shape[0]
    return np.concatenate([fit.weight64.cpu().numpy().reshape(E, -1), fit.bias64.cpu().numpy()], axis=1)


def _fit(pkg, X, t, y, alpha, T, **kw):
    return pkg.fit_distilled_exit_heads(X, t, None if alpha == 1.0 else y, alpha=alpha, temperature=T, l2=L2, gtol=GTOL, **kw)


@pytest.mark.parametrize("alpha,T", FIT_PAIRS)
@pytest.mark.parametrize("N,H,K,E", FIT_SHAPES)
def test_fit_reaches_the_optimum(pkg, N, H, K, E, alpha, T):
    """status 0 at gtol 1e-9 and max |dlogit| <= 1e-4 against the scipy optimum: the existing bar, derived from strong convexity --
    ||dtheta|| <= (1e-9 + 1e-8) / l2 = 1.1e-6, times ||x|| ~ sqrt(768) = 28, is 3e-5."""
    X, y, t = _problem(N, H, K, E)
    ref = _reference(N, H, K, E, alpha, T)
    yy = None if alpha == 1.0 else y
    fit = _fit(pkg, X, t, y, alpha, T)
    assert fit.alpha == alpha and fit.temperature == T
    status, evals = fit.status.cpu().numpy(), fit.evals.cpu().numpy()
    loss, gnorm = fit.loss.cpu().numpy(), fit.grad_norm.cpu().numpy()
    theta = _theta64(fit)
    z_dev = fit.logits(X).cpu().numpy()
    print("evals", evals, "status", status, "grad_norm", gnorm)
    assert (status == 0).all(), status
    for e in range(E):
        l_dev, g_dev = DR.loss_grad(theta[e], X[e], t, yy, K, alpha, T, L2)
        g_ref = DR.loss_grad(ref[e], X[e], t, yy, K, alpha, T, L2)[1]
        n_dev, n_ref = np.linalg.norm(g_dev), np.linalg.norm(g_ref)
        dist = np.linalg.norm(theta[e] - ref[e])
        dz = np.abs(z_dev[e] - HR.logits(ref[e], X[e], K)).max()
        at_zero = DR.loss_grad(np.zeros_like(theta[e]), X[e], t, yy, K, alpha, T, L2)[0]
        print(f"exit {e}: ||grad(theta_dev)|| {n_dev:.3e}  ||grad(theta_ref)|| {n_ref:.3e}  ||theta_dev - theta_ref|| {dist:.3e}  "
              f"max |dz| {dz:.3e}  L {l_dev:.6f}  L(0) {at_zero:.6f}")
        assert n_dev <= 2 * GTOL, (e, n_dev)
        assert dist <= (n_dev + n_ref) / L2, (e, dist, (n_dev + n_ref) / L2)       # strong convexity: fails only for another objective
        assert dz <= 1e-4, (e, dz)
        assert l_dev < at_zero, (e, l_dev, at_zero)
        assert abs(loss[e] - l_dev) <= ATOL + RTOL * abs(l_dev), (e, loss[e], l_dev)
        assert abs(gnorm[e] - n_dev) <= ATOL + RTOL * n_dev, (e, gnorm[e], n_dev)
        assert np.array_equal(fit.weight[e].cpu().numpy().reshape(-1), theta[e][:K * H].astype(np.float32))
        assert np.array_equal(fit.bias[e].cpu().numpy(), theta[e][K * H:].astype(np.float32))


# ---- 4. / 5. label-free, determinism ----------------------------------------------------------------------------------------------------------------
def _bits(fit, names=HEAD_OUTPUTS):
    return [getattr(fit, n).cpu().numpy().tobytes() for n in names]


def test_at_alpha_1_labels_are_not_looked_at(pkg):
    N, H, K, E = FIT_SHAPES[0]
    X, y, t = _problem(N, H, K, E)
    free = pkg.fit_distilled_exit_heads(X, t, l2=L2, gtol=GTOL)
    assert (free.status.cpu().numpy() == 0).all()
    wrong = np.full(N, K + 5, dtype=np.int64)
    wrong[::2] = -3
    for labels in (y, wrong):
        assert _bits(pkg.fit_distilled_exit_heads(X, t, labels, alpha=1.0, l2=L2, gtol=GTOL)) == _bits(free)
    theta = np.random.default_rng(0).standard_normal((E, K * H + K)) * 0.1
    a = _lossgrad(pkg, X, t, None, theta, K, 1.0, 2.0)
    b = _lossgrad(pkg, X, t, wrong, theta, K, 1.0, 2.0)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("alpha,T", [(0.5, 2.0), (1.0, 1.0)])
def test_two_calls_return_identical_bits_and_an_exit_fits_alone_as_among_others(pkg, alpha, T):
    N, H, K, E = FIT_SHAPES[0]
    assert E == 3
    X, y, t = _problem(N, H, K, E)
    a, b = _fit(pkg, X, t, y, alpha, T), _fit(pkg, X, t, y, alpha, T)
    assert _bits(a) == _bits(b)
    alone = _fit(pkg, X[1:2], t, y, alpha, T)
    for name in HEAD_OUTPUTS:
        assert getattr(alone, name)[0].cpu().numpy().tobytes() == getattr(a, name)[1].cpu().numpy().tobytes(), name


# ---- 6. failures -----------------------------------------------------------------------------------------------------------------------------------
def _raw_fit_leaves_outputs(pkg, X, t, y, alpha, T, needle):
    """The C entry point on NaN-prefilled outputs (7 in the integer ones): it fails with `needle` and none of them is touched."""
    torch = _torch()
    lib = pkg.capi.load()
    E, N, H = X.shape
    K = t.shape[1]
    Xd, td, yd = _dev(X, torch.float32), _dev(t, torch.float32), None if y is None else _dev(y, torch.int64)
    need = lib.ee_head_fit_workspace_bytes(E, N, H, K, 8)
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    nan = float("nan")
    outs = [torch.full(s, v, dtype=dt, device="cuda") for s, v, dt in (((E, K, H), nan, torch.float32), ((E, K), nan, torch.float32),
            ((E, K, H), nan, torch.float64), ((E, K), nan, torch.float64), ((E,), nan, torch.float64), ((E,), nan, torch.float64),
            ((E,), 7, torch.int32), ((E,), 7, torch.int32))]
    rc = lib.ee_head_fit_distill(_ptr(Xd), _ptr(td), _ptr(yd), E, N, H, K, alpha, T, L2, GTOL, 50, 8, _ptr(ws), need,
                                 *[_ptr(o) for o in outs], _stream())
    assert rc != 0 and needle in pkg.capi.last_error(), pkg.capi.last_error()
    torch.cuda.synchronize()
    for o in outs[:6]:
        assert bool(torch.isnan(o).all())
    for o in outs[6:]:
        assert bool((o == 7).all())


def test_a_teacher_logit_that_is_not_finite_fails_the_call_and_leaves_the_outputs_untouched(pkg):
    N, H, K, E = FIT_SHAPES[0]
    X, y, t = _problem(N, H, K, E)
    for bad in (float("nan"), float("inf")):
        tb = t.copy()
        tb[N // 2, K - 1] = bad
        with pytest.raises(pkg.capi.MMEEError, match="teacher logit is not finite"):
            pkg.fit_distilled_exit_heads(X, tb, l2=L2, gtol=GTOL)
        _raw_fit_leaves_outputs(pkg, X, tb, None, 1.0, 1.0, "teacher logit is not finite")
    theta = np.zeros((E, K * H + K))
    with pytest.raises(pkg.capi.MMEEError, match="teacher logit is not finite"):
        _lossgrad(pkg, X, tb, None, theta, K, 1.0, 1.0)
    assert (pkg.fit_distilled_exit_heads(X, t, l2=L2, gtol=GTOL).status.cpu().numpy() == 0).all()          # the mended teacher goes through


def test_a_label_out_of_range_fails_the_call_at_alpha_below_1(pkg):
    N, H, K, E = FIT_SHAPES[0]
    X, y, t = _problem(N, H, K, E)
    for bad in (K, -1):
        yb = y.copy()
        yb[N // 2] = bad
        with pytest.raises(pkg.capi.MMEEError, match="label is outside"):
            pkg.fit_distilled_exit_heads(X, t, yb, alpha=0.5, temperature=2.0, l2=L2, gtol=GTOL)
        _raw_fit_leaves_outputs(pkg, X, t, yb, 0.5, 2.0, "label is outside")


def test_max_evals_stops_with_status_1_and_a_loss_not_above_the_start(pkg):
    N, H, K, E = FIT_SHAPES[0]
    X, y, t = _problem(N, H, K, E)
    for alpha, T in FIT_PAIRS:
        fit = _fit(pkg, X, t, y, alpha, T, max_evals=3)
        assert (fit.status.cpu().numpy() == 1).all() and (fit.evals.cpu().numpy() == 3).all()
        loss, theta = fit.loss.cpu().numpy(), _theta64(fit)
        for e in range(E):
            yy = None if alpha == 1.0 else y
            at_zero = DR.loss_grad(np.zeros_like(theta[e]), X[e], t, yy, K, alpha, T, L2)[0]
            l_dev = DR.loss_grad(theta[e], X[e], t, yy, K, alpha, T, L2)[0]
            assert loss[e] <= at_zero, (alpha, T, e, loss[e], at_zero)
            assert abs(loss[e] - l_dev) <= ATOL + RTOL * abs(l_dev)


# ---- 7. the two-layer head --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,T", [(1.0, 1.0), (0.5, 2.0)])
def test_mlp_lossgrad_matches_the_restatement(pkg, alpha, T):
    """The K, E and N of tests/test_gpu_mlp_head_fit.py's launch-alone test at its smallest H, and its ragged H: only the softmax launch
    differs from the labelled evaluation, and it never sees H."""
    R = pkg.capi.MLP_HEAD_FIT_ROWS
    rng = np.random.default_rng(7)
    worst = 0.0
    shapes = [(64, K, E, N) for K in (2, 10, 16, 64) for E in (1, 3) for N in (1, 31, 32, 33, R - 1, R, R + 1, 2 * R + 3)]
    shapes += [(H, 3, 2, 37) for H in (4, 68, 132)]
    for H, K, E, N in shapes:
        X = rng.standard_normal((E, N, H)).astype(np.float32)
        t = (3.0 * rng.standard_normal((N, K))).astype(np.float32)
        y = rng.integers(0, K, N)
        theta = rng.standard_normal((E, MR.param_count(H, K))) / np.sqrt(H)
        loss, grad = _lossgrad(pkg, X, t, None if alpha == 1.0 else y, theta, K, alpha, T, mlp=True)
        worst = max(worst, _assert_matches(loss, grad, X, t, y, theta, K, alpha, T, (H, K, E, N), mlp=True))
    print(f"worst difference / tolerance = {worst:.3e}")


def test_mlp_fit_from_the_identity_start(pkg):
    """No reference optimum (the objective is not convex): the returned loss is the restatement's at the returned point, it is not above the
    start's, and status 0 means a restated gradient norm <= gtol."""
    N, H, K, E = 300, 64, 10, 2
    X, _ = MR.problem(N, H, K, E, seed=11)
    Wt = np.random.default_rng(N).standard_normal((K, H)) * (2.0 / np.sqrt(H))
    t = (X[-1].astype(np.float64) @ Wt.T).astype(np.float32)
    fit = pkg.fit_distilled_mlp_exit_heads(X, t, l2=L2, gtol=MLP_GTOL)
    assert fit.alpha == 1.0 and fit.temperature == 1.0
    status, evals, loss = fit.status.cpu().numpy(), fit.evals.cpu().numpy(), fit.loss.cpu().numpy()
    theta = fit.theta64.cpu().numpy()
    print("evals", evals, "status", status, "loss", loss)
    start = MR.init_identity(H, K)
    for e in range(E):
        l_dev, g_dev = DR.mlp_loss_grad(theta[e], X[e], t, None, K, 1.0, 1.0, L2)
        l_start = DR.mlp_loss_grad(start, X[e], t, None, K, 1.0, 1.0, L2)[0]
        assert abs(loss[e] - l_dev) <= 1e-10 * abs(l_dev), (e, loss[e], l_dev)
        assert loss[e] <= l_start, (e, loss[e], l_start)
        assert status[e] in (0, 1, 2)
        if status[e] == 0:
            assert np.linalg.norm(g_dev) <= MLP_GTOL * (1 + 1e-6), (e, np.linalg.norm(g_dev))
        W1, b1, W2, b2 = MR.split(theta[e], K, H)
        assert np.array_equal(fit.dense_weight[e].cpu().numpy(), W1.astype(np.float32))
        assert np.array_equal(fit.bias[e].cpu().numpy(), b2.astype(np.float32))


# ---- 8. through the engine ----------------------------------------------------------------------------------------------------------------------
EE_1LAYER = dict(exits=[1, 2, 3], encoder_layer_strategy="ramp", inference_strategy="max_confidence", exit_head_num_layers=1)


def _mean_kl(t, z):
    """mean_n KL(softmax(t_n) || softmax(z_n)) in float64"""
    def log_softmax(s):
        s = s - s.max(-1, keepdims=True)
        return s - np.log(np.exp(s).sum(-1, keepdims=True))
    lq, lp = log_softmax(np.asarray(t, np.float64)), log_softmax(np.asarray(z, np.float64))
    return float((np.exp(lq) * (lq - lp)).sum(-1).mean())


@pytest.mark.parametrize("name", ["tiny_f32", "h256_split", "dit_tiny"])
def test_dump_distill_load_forward(pkg, name):
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
    inputs = {k: torch.from_numpy(docs[k]).cuda() for k in keys}
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision=precision)
    eng.load_weights(W)
    feats, teacher = pkg.collect_distill_features(eng, [inputs])
    assert tuple(feats.shape) == (3, B, H) and feats.is_cuda and feats.dtype == torch.float32
    assert tuple(teacher.shape) == (B, K) and teacher.is_cuda and teacher.dtype == torch.float32
    if name == "tiny_f32":                                              # several batches are concatenated in order
        pf, pt = pkg.collect_distill_features(eng, [{k: v[i:i + 32] for k, v in inputs.items()} for i in range(0, B, 32)])
        assert tuple(pf.shape) == (3, B, H) and float((pf - feats).abs().max()) <= 1e-4
        assert tuple(pt.shape) == (B, K) and float((pt - teacher).abs().max()) <= 1e-4
    eng.close()

    fit = pkg.fit_distilled_exit_heads(feats, teacher, l2=L2, gtol=GTOL)
    print(f"{name}: evals {fit.evals.cpu().tolist()} status {fit.status.cpu().tolist()} grad norms {fit.grad_norm.cpu().tolist()}")
    sd = fit.state_dict(cfg)

    eng2 = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision=precision)
    eng2.load_weights({**W, **sd})
    dump = eng2.forward(**inputs, dump_all=True, want_head=True, want_all=True, want_hidden_cls=True)
    eng2.close()
    assert torch.equal(dump.all_logits[-1], teacher)                    # the final classifier does not depend on the heads: the same bits
    want = fit.logits(feats).cpu().numpy()
    got = dump.head_logits.cpu().numpy().astype(np.float64)
    err = np.abs(got - want).max()
    print(f"{name}: max |head_logits - HeadFit.logits| = {err:.3e}")
    assert err <= 1e-4, err
    t = teacher.cpu().numpy()
    uniform = _mean_kl(t, np.zeros_like(t))
    for e in range(3):
        kl = _mean_kl(t, got[e])
        print(f"{name}: exit {e}: mean KL(teacher || head) = {kl:.4e}, the zero head's {uniform:.4e}")
        assert kl < uniform, (e, kl, uniform)
