"""The weighted exit-head fits on the device (include/mmee.h ee_head_fit_weighted, ee_mlp_head_fit_weighted) against the float64 restatement
and the scipy solution of tests/weighted_headfit_ref.py: the loss / gradient kernels alone, the identities that tie the weighted form to the
unweighted one (all-ones weights, a power-of-two factor, row repetition, a 0/1 mask against the subset), rows of weight zero, the weight
errors, the weighted optimum, and the loop dump -> fit -> scan -> reach weights -> refit -> load -> forward through the engine.

Tolerance of the kernel-alone comparisons: rtol 1e-10, atol 1e-12, the bar of tests/test_gpu_head_fit.py, tests/test_gpu_mlp_head_fit.py and
tests/test_gpu_distill_head_fit.py -- derived, not measured: the weighted form takes the same float64 sums and adds one multiplication per
element (and the reference divides by W where the device multiplies by N / W and divides by N: three roundings)."""
import functools

import numpy as np
import pytest

from . import distill_headfit_ref as DR
from . import headfit_ref as HR
from . import mlp_headfit_ref as MR
from . import weighted_headfit_ref as WR
from .fit_util import _dev, _ptr, _stream, _torch

pytestmark = pytest.mark.gpu

L2, GTOL, MLP_GTOL = 1e-2, 1e-9, 1e-6
RTOL, ATOL = 1e-10, 1e-12
OBJECTIVES = [(False, 0.0, 1.0), (True, 1.0, 2.0), (True, 0.5, 2.0)]           # (a teacher?, alpha, T): labelled, pure and mixed distillation
HEAD_OUTPUTS = ("weight", "bias", "weight64", "bias64", "loss", "grad_norm", "evals", "status")
MLP_OUTPUTS = ("dense_weight", "dense_bias", "weight", "bias", "theta64", "loss", "grad_norm", "evals", "status")
BAD_WEIGHT, ZERO_SUM = "a sample weight is negative or not finite", "an exit's weights sum to zero"


def _lossgrad(pkg, X, y, t, w, theta, K, alpha, T, l2=L2, mlp=False):
    """ee_debug_(mlp_)head_weighted_lossgrad on host arrays X (E,N,H) f32, y (N,) or None, t (N,K) f32 or None, w (E,N) f32, theta (E,P) f64
    -> (loss (E,), grad (E,P)) host float64."""
    torch = _torch()
    lib = pkg.capi.load()
    E, N, H = X.shape
    name = "ee_debug_mlp_head_weighted_lossgrad" if mlp else "ee_debug_head_weighted_lossgrad"
    Xd, wd, thd = _dev(X, torch.float32), _dev(w, torch.float32), _dev(theta, torch.float64)
    yd = None if y is None else _dev(y, torch.int64)
    td = None if t is None else _dev(t, torch.float32)
    loss = torch.full((E,), float("nan"), dtype=torch.float64, device="cuda")
    grad = torch.full((E, theta.shape[1]), float("nan"), dtype=torch.float64, device="cuda")
    rc = getattr(lib, name)(_ptr(Xd), _ptr(yd), _ptr(td), _ptr(wd), _ptr(thd), E, N, H, K, alpha, T, l2, _ptr(loss), _ptr(grad), _stream())
    pkg.capi.check(rc, None, name)
    return loss.cpu().numpy(), grad.cpu().numpy()


def _close(got_loss, got_grad, want_loss, want_grad, what, scale=1.0):
    dl = abs(got_loss - want_loss) / (ATOL + RTOL * abs(want_loss))
    dg = (np.abs(got_grad - want_grad) / (ATOL + RTOL * np.abs(want_grad))).max()
    print(f"{what}: loss {dl:.3e}, grad {dg:.3e} of the tolerance")
    assert dl <= scale, (what, "loss", got_loss, want_loss)
    assert dg <= scale, (what, "grad", float(np.abs(got_grad - want_grad).max()), int(np.argmax(np.abs(got_grad - want_grad))))
    return max(dl, dg)


def _families(rng, E, N, S):
    """(name, (E,N) float32 table) for every family N allows"""
    out = [("a", WR.family_uniform(rng, E, N)), ("b", WR.family_integers(rng, E, N, S)), ("c", WR.family_one_row(rng, E, N)),
           ("e", WR.family_per_exit(rng, E, N))]
    if N > 2 * S:
        out.append(("d", WR.family_zero_slab(rng, E, N, S)))
    return out


def _kernel_alone(pkg, H, shapes, mlp):
    S = pkg.capi.HEAD_FIT_SLAB
    rng = np.random.default_rng(H + (1000 if mlp else 0))
    ref = WR.mlp_loss_grad if mlp else WR.loss_grad
    worst, seen = 0.0, set()
    for K, E, N in shapes:
        X = rng.standard_normal((E, N, H)).astype(np.float32)
        t = (3.0 * rng.standard_normal((N, K))).astype(np.float32)
        y = rng.integers(0, K, N)
        P = MR.param_count(H, K) if mlp else K * H + K
        theta = rng.standard_normal((E, P)) / np.sqrt(H)
        for fam, w in _families(rng, E, N, S):
            for soft, alpha, T in OBJECTIVES:
                tt, yy = (t if soft else None), (None if alpha == 1.0 else y)
                loss, grad = _lossgrad(pkg, X, yy, tt, w, theta, K, alpha, T, mlp=mlp)
                for e in range(E):
                    want = ref(theta[e], X[e], yy, K, L2, w[e], tt, alpha, T)
                    dl = abs(loss[e] - want[0]) / (ATOL + RTOL * abs(want[0]))
                    dg = (np.abs(grad[e] - want[1]) / (ATOL + RTOL * np.abs(want[1]))).max()
                    assert dl <= 1.0, ((H, K, E, N, fam, alpha, T, e), "loss", loss[e], want[0])
                    assert dg <= 1.0, ((H, K, E, N, fam, alpha, T, e), "grad", float(np.abs(grad[e] - want[1]).max()))
                    worst = max(worst, dl, dg)
                seen.add(fam)
    print(f"H = {H}: worst difference / tolerance = {worst:.3e}; families {sorted(seen)}")
    assert seen == {"a", "b", "c", "d", "e"}


# ---- 1. the kernels alone ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 1024])
def test_one_layer_lossgrad_matches_the_restatement(pkg, H):
    S = pkg.capi.HEAD_FIT_SLAB
    _kernel_alone(pkg, H, [(K, E, N) for K in (2, 10, 64) for E in (1, 3) for N in (1, S - 1, S, S + 1, 2 * S + 3)], mlp=False)


@pytest.mark.parametrize("H", [8, 68])
def test_two_layer_lossgrad_matches_the_restatement(pkg, H):
    _kernel_alone(pkg, H, [(K, E, N) for K in (2, 10, 64) for E in (1, 3) for N in (1, 31, 33, 63, 65, 131)], mlp=True)


# ---- problems and fits ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(N, H, K, E):
    X, y, t = DR.fit_problem(N, H, K, E)
    for a in (X, y, t):
        a.setflags(write=False)
    return X, y, t


@functools.lru_cache(maxsize=None)
def _mlp_problem(N, H, K, E):
    X, y = MR.problem(N, H, K, E, seed=11)
    Wt = np.random.default_rng(N).standard_normal((K, H)) * (2.0 / np.sqrt(H))
    t = (X[-1].astype(np.float64) @ Wt.T).astype(np.float32)
    for a in (X, y, t):
        a.setflags(write=False)
    return X, y, t


def _bits(fit, names):
    return {n: getattr(fit, n).cpu().numpy().tobytes() for n in names}


def _fit(pkg, kind, X, y, t, w, **kw):
    """kind: 'head', 'head_distill' (alpha 0.5, T 2), 'mlp', 'mlp_distill' (alpha 0.5, T 2); w None: the unweighted entry point"""
    K = t.shape[1]
    if kind == "head":
        return pkg.fit_exit_heads(X, y, l2=L2, gtol=GTOL, num_labels=K, sample_weight=w, **kw)
    if kind == "head_distill":
        return pkg.fit_distilled_exit_heads(X, t, y, alpha=0.5, temperature=2.0, l2=L2, gtol=GTOL, sample_weight=w, **kw)
    if kind == "mlp":
        return pkg.fit_mlp_exit_heads(X, y, l2=L2, gtol=MLP_GTOL, num_labels=K, sample_weight=w, **kw)
    return pkg.fit_distilled_mlp_exit_heads(X, t, y, alpha=0.5, temperature=2.0, l2=L2, gtol=MLP_GTOL, sample_weight=w, **kw)


def _outputs(kind):
    return MLP_OUTPUTS if kind.startswith("mlp") else HEAD_OUTPUTS


def _kind_problem(kind):
    return _mlp_problem(131, 68, 10, 2) if kind.startswith("mlp") else _problem(300, 64, 10, 3)


# ---- 2. all-ones weights are the unweighted fit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["head", "head_distill", "mlp", "mlp_distill"])
def test_all_ones_weights_are_the_unweighted_fit_bit_for_bit(pkg, kind):
    """W_e = N exactly, so every scale is 1.0 and the one more multiplication changes no bit: the variant is the same computation."""
    X, y, t = _kind_problem(kind)
    E, N = X.shape[:2]
    plain = _fit(pkg, kind, X, y, t, None, max_evals=50)
    assert (plain.evals.cpu().numpy() > 1).all()
    for ones in (np.ones(N, dtype=np.float32), np.ones((E, N), dtype=np.float64), _torch().ones((E, N), dtype=_torch().int32, device="cuda")):
        got = _fit(pkg, kind, X, y, t, ones, max_evals=50)
        assert _bits(got, _outputs(kind)) == _bits(plain, _outputs(kind))


# ---- 3. a power-of-two factor ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["head", "mlp_distill"])
def test_w_and_4w_return_identical_bits(pkg, kind):
    X, y, t = _kind_problem(kind)
    E, N = X.shape[:2]
    w = WR.family_per_exit(np.random.default_rng(4), E, N)
    a, b = _fit(pkg, kind, X, y, t, w, max_evals=50), _fit(pkg, kind, X, y, t, 4.0 * w, max_evals=50)
    assert _bits(a, _outputs(kind)) == _bits(b, _outputs(kind))
    again = _fit(pkg, kind, X, y, t, w, max_evals=50)                           # and two calls return the same bits
    assert _bits(a, _outputs(kind)) == _bits(again, _outputs(kind))
    alone = _fit(pkg, kind, X[1:2], y, t, w[1:2], max_evals=50)                 # an exit fitted alone gets the bits it gets among others
    for name in _outputs(kind):
        assert getattr(alone, name)[0].cpu().numpy().tobytes() == getattr(a, name)[1].cpu().numpy().tobytes(), name


# ---- 4. repetition -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mlp", [False, True])
def test_integer_weights_equal_row_repetition(pkg, mlp):
    """Family (b) on X against the UNWEIGHTED hooks on the dataset with row n repeated w_n times: the same objective, other sums -- twice the
    tolerance of the kernel-alone tests, one for either side."""
    from .test_gpu_distill_head_fit import _lossgrad as distill_hook
    from .test_gpu_head_fit import _lossgrad as head_hook
    from .test_gpu_mlp_head_fit import _lossgrad as mlp_hook
    S = pkg.capi.HEAD_FIT_SLAB
    rng = np.random.default_rng(8)
    N, H, K, E = 2 * S + 3, (68 if mlp else 64), 10, 2
    X = rng.standard_normal((E, N, H)).astype(np.float32)
    t = (3.0 * rng.standard_normal((N, K))).astype(np.float32)
    y = rng.integers(0, K, N)
    w = WR.family_integers(rng, E, N, S)
    rep = np.repeat(np.arange(N), w[0].astype(np.int64))
    assert len(rep) == int(w[0].sum()) and len(rep) != N
    theta = rng.standard_normal((E, MR.param_count(H, K) if mlp else K * H + K)) / np.sqrt(H)
    Xr = np.ascontiguousarray(X[:, rep])
    got = _lossgrad(pkg, X, y, None, w, theta, K, 0.0, 1.0, mlp=mlp)
    want = (mlp_hook if mlp else head_hook)(pkg, Xr, y[rep], theta, K)
    for e in range(E):
        _close(got[0][e], got[1][e], want[0][e], want[1][e], ("labelled", mlp, e), scale=2.0)
    got = _lossgrad(pkg, X, y, t, w, theta, K, 0.5, 2.0, mlp=mlp)
    want = distill_hook(pkg, Xr, np.ascontiguousarray(t[rep]), y[rep], theta, K, 0.5, 2.0, mlp=mlp)
    for e in range(E):
        _close(got[0][e], got[1][e], want[0][e], want[1][e], ("mixed", mlp, e), scale=2.0)


# ---- 5. rows of weight zero are not looked at ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["head_distill", "mlp_distill"])
def test_rows_of_weight_zero_are_not_looked_at(pkg, kind):
    """alpha = 0.5: labels and teacher rows both count.  Label -1 and a NaN teacher row where the weight is zero: the bits of the clean call.
    The same poison where the weight is positive: the existing messages."""
    X, y, t = _kind_problem(kind)
    E, N = X.shape[:2]
    K = t.shape[1]
    S = pkg.capi.HEAD_FIT_SLAB
    w = WR.family_integers(np.random.default_rng(6), E, N, S)
    zero = np.flatnonzero(w[0] == 0)
    assert {0, S - 1, N - 1} <= set(zero.tolist())
    yb, tb = y.copy(), t.copy()
    yb[zero] = -1
    tb[zero] = np.nan
    clean = _fit(pkg, kind, X, y, t, w, max_evals=50)
    dirty = _fit(pkg, kind, X, yb, tb, w, max_evals=50)
    assert _bits(dirty, _outputs(kind)) == _bits(clean, _outputs(kind))
    mlp = kind.startswith("mlp")
    H = X.shape[2]
    theta = np.random.default_rng(0).standard_normal((E, MR.param_count(H, K) if mlp else K * H + K)) * 0.1
    a = _lossgrad(pkg, X, y, t, w, theta, K, 0.5, 2.0, mlp=mlp)
    b = _lossgrad(pkg, X, yb, tb, w, theta, K, 0.5, 2.0, mlp=mlp)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    a = _lossgrad(pkg, X, y, None, w, theta, K, 0.0, 1.0, mlp=mlp)                 # the labelled row step
    b = _lossgrad(pkg, X, yb, None, w, theta, K, 0.0, 1.0, mlp=mlp)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    live = int(np.flatnonzero(w[0] > 0)[3])
    yl, tl = y.copy(), t.copy()
    yl[live] = -1
    tl[live] = np.nan
    with pytest.raises(pkg.capi.MMEEError, match="label is outside"):
        _fit(pkg, kind, X, yl, t, w, max_evals=50)
    with pytest.raises(pkg.capi.MMEEError, match="teacher logit is not finite"):
        _fit(pkg, kind, X, y, tl, w, max_evals=50)
    with pytest.raises(pkg.capi.MMEEError, match="label is outside"):
        _lossgrad(pkg, X, yl, None, w, theta, K, 0.0, 1.0, mlp=mlp)


# ---- 6. weight errors --------------------------------------------------------------------------------------------------------------------------
def _raw_fit_leaves_outputs(pkg, X, y, K, w, needle):
    """ee_head_fit_weighted (labelled) on NaN-prefilled outputs (7 in the integer ones): it fails with `needle` and none of them is touched."""
    torch = _torch()
    lib = pkg.capi.load()
    E, N, H = X.shape
    Xd, yd, wd = _dev(X, torch.float32), _dev(y, torch.int64), _dev(w, torch.float32)
    need = lib.ee_head_fit_weighted_workspace_bytes(E, N, H, K, 8)
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    nan = float("nan")
    outs = [torch.full(s, v, dtype=dt, device="cuda") for s, v, dt in (((E, K, H), nan, torch.float32), ((E, K), nan, torch.float32),
            ((E, K, H), nan, torch.float64), ((E, K), nan, torch.float64), ((E,), nan, torch.float64), ((E,), nan, torch.float64),
            ((E,), 7, torch.int32), ((E,), 7, torch.int32))]
    rc = lib.ee_head_fit_weighted(_ptr(Xd), _ptr(yd), None, _ptr(wd), E, N, H, K, 0.0, 1.0, L2, GTOL, 50, 8, _ptr(ws), need,
                                  *[_ptr(o) for o in outs], _stream())
    assert rc != 0 and needle in pkg.capi.last_error() and "no output was written" in pkg.capi.last_error(), pkg.capi.last_error()
    torch.cuda.synchronize()
    for o in outs[:6]:
        assert bool(torch.isnan(o).all())
    for o in outs[6:]:
        assert bool((o == 7).all())


def test_bad_weights_fail_the_call_and_leave_the_outputs_untouched(pkg):
    X, y, t = _problem(300, 64, 10, 3)
    E, N, H = X.shape
    K = t.shape[1]
    good = WR.family_uniform(np.random.default_rng(2), E, N)
    theta = np.zeros((E, K * H + K))
    mtheta = np.tile(MR.init_identity(H, K), (E, 1))
    for bad, needle in ((-0.5, BAD_WEIGHT), (float("nan"), BAD_WEIGHT), (float("inf"), BAD_WEIGHT), (None, ZERO_SUM)):
        w = good.copy()
        if bad is None:
            w[1] = 0.0                                                          # one exit's whole row
        else:
            w[E - 1, N - 1] = bad
        for kind in ("head", "head_distill", "mlp", "mlp_distill"):
            with pytest.raises(pkg.capi.MMEEError, match=needle):
                _fit(pkg, kind, X, y, t, w, max_evals=5)
        _raw_fit_leaves_outputs(pkg, X, y, K, w, needle)
        with pytest.raises(pkg.capi.MMEEError, match=needle):
            _lossgrad(pkg, X, y, None, w, theta, K, 0.0, 1.0)
        with pytest.raises(pkg.capi.MMEEError, match=needle):
            _lossgrad(pkg, X, y, t, w, mtheta, K, 0.5, 2.0, mlp=True)
    assert (_fit(pkg, "head", X, y, t, good).status.cpu().numpy() == 0).all()   # the mended table goes through


# ---- 7. the weighted optimum ---------------------------------------------------------------------------------------------------------------------
def _table(fam, N, E):
    rng = np.random.default_rng(N + (7 if fam == "e" else 0))
    w = WR.family_uniform(rng, E, N) if fam == "a" else WR.family_per_exit(rng, E, N)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _reference(N, H, K, E, fam):
    X, y, _ = _problem(N, H, K, E)
    w = _table(fam, N, E)
    ref = np.stack([WR.solve(X[e], y, K, L2, w[e]) for e in range(E)])
    ref.setflags(write=False)
    return ref


def _theta64(fit):
    E = fit.weight64.shape[0]
    return np.concatenate([fit.weight64.cpu().numpy().reshape(E, -1), fit.bias64.cpu().numpy()], axis=1)


@pytest.mark.parametrize("fam", ["a", "e"])
@pytest.mark.parametrize("N,H,K,E", [(300, 64, 10, 3), (257, 64, 2, 1)])
def test_fit_reaches_the_weighted_optimum(pkg, N, H, K, E, fam):
    """status 0 at gtol 1e-9, a restated gradient norm <= 2 gtol, the distance to the scipy optimum inside strong convexity's bound, and
    max |dlogit| <= 1e-4: the bar of tests/test_gpu_head_fit.py, derived there -- ||dtheta|| <= (1e-9 + 1e-8) / l2 = 1.1e-6, times
    ||x|| ~ sqrt(768) = 28, is 3e-5.  Against the unweighted fit: the weighted objective is not higher at the weighted solution, and the
    logits differ by more than 1e-3 somewhere."""
    X, y, _ = _problem(N, H, K, E)
    w = _table(fam, N, E)
    ref = _reference(N, H, K, E, fam)
    fit = pkg.fit_exit_heads(X, y, l2=L2, gtol=GTOL, num_labels=K, sample_weight=w)
    plain = pkg.fit_exit_heads(X, y, l2=L2, gtol=GTOL, num_labels=K)
    status, evals, loss, gnorm = (getattr(fit, n).cpu().numpy() for n in ("status", "evals", "loss", "grad_norm"))
    theta, theta_plain = _theta64(fit), _theta64(plain)
    z_dev, z_plain = fit.logits(X).cpu().numpy(), plain.logits(X).cpu().numpy()
    print("evals", evals, "status", status, "grad_norm", gnorm)
    assert (status == 0).all(), status
    for e in range(E):
        l_dev, g_dev = WR.loss_grad(theta[e], X[e], y, K, L2, w[e])
        g_ref = WR.loss_grad(ref[e], X[e], y, K, L2, w[e])[1]
        l_plain = WR.loss_grad(theta_plain[e], X[e], y, K, L2, w[e])[0]
        n_dev, n_ref = np.linalg.norm(g_dev), np.linalg.norm(g_ref)
        dist = np.linalg.norm(theta[e] - ref[e])
        dz = np.abs(z_dev[e] - HR.logits(ref[e], X[e], K)).max()
        moved = np.abs(z_dev[e] - z_plain[e]).max()
        print(f"exit {e}: ||grad(theta_dev)|| {n_dev:.3e}  ||grad(theta_ref)|| {n_ref:.3e}  ||theta_dev - theta_ref|| {dist:.3e}  "
              f"max |dz| {dz:.3e}  L_w {l_dev:.6f}  L_w(unweighted fit) {l_plain:.6f}  max |z - z_unweighted| {moved:.3e}")
        assert n_dev <= 2 * GTOL, (e, n_dev)
        assert dist <= (n_dev + n_ref) / L2, (e, dist, (n_dev + n_ref) / L2)
        assert dz <= 1e-4, (e, dz)
        assert l_dev <= l_plain, (e, l_dev, l_plain)
        assert moved > 1e-3, (e, moved)
        assert abs(loss[e] - l_dev) <= ATOL + RTOL * abs(l_dev), (e, loss[e], l_dev)
        assert abs(gnorm[e] - n_dev) <= ATOL + RTOL * n_dev, (e, gnorm[e], n_dev)


# ---- 8. a held-out mask is the subset ------------------------------------------------------------------------------------------------------------
def test_a_zero_one_mask_fits_the_kept_rows(pkg):
    """0/1 weights on X and the unweighted fit of the kept rows solve the same strongly convex problem: both stop within gtol of its one
    optimum, so their logits agree to the 1e-4 of the test above."""
    N, H, K, E = 300, 64, 10, 3
    X, y, _ = _problem(N, H, K, E)
    keep = np.random.default_rng(12).random(N) < 0.7
    keep[[0, N - 1]] = False
    masked = pkg.fit_exit_heads(X, y, l2=L2, gtol=GTOL, num_labels=K, sample_weight=keep)               # a bool mask is a real dtype too
    subset = pkg.fit_exit_heads(np.ascontiguousarray(X[:, keep]), y[keep], l2=L2, gtol=GTOL, num_labels=K)
    assert (masked.status.cpu().numpy() == 0).all() and (subset.status.cpu().numpy() == 0).all()
    dz = float((masked.logits(X) - subset.logits(X)).abs().max())
    dth = np.abs(_theta64(masked) - _theta64(subset)).max()
    print(f"kept {int(keep.sum())} of {N} rows; evals {masked.evals.cpu().tolist()} (mask) {subset.evals.cpu().tolist()} (subset); "
          f"max |dtheta64| {dth:.3e}; max |dlogit| between the masked fit and the fit of the kept rows: {dz:.3e}")
    assert dz <= 1e-4, dz


# ---- 9. through the engine -----------------------------------------------------------------------------------------------------------------------
EE_1LAYER = dict(exits=[1, 2, 3], encoder_layer_strategy="ramp", inference_strategy="max_confidence", exit_head_num_layers=1)


def test_dump_fit_scan_reach_refit_load_forward(pkg):
    torch = _torch()
    B, T = 96, 48
    cfg = pkg.ModelConfig.tiny(EE_config=dict(EE_1LAYER))
    K, H = cfg.num_labels, cfg.hidden_size
    W = pkg.synth.make_weights(cfg, seed=21)
    docs = pkg.synth.make_documents(cfg, B, seed=22, text_len=T, min_words=3)
    inputs = {k: torch.from_numpy(docs[k]).cuda() for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision="fp32")
    eng.load_weights(W)
    feats = pkg.collect_exit_features(eng, [inputs])
    rng = np.random.default_rng(23)
    teacher = rng.standard_normal((K, H)) * (2.0 / np.sqrt(H))
    y = (feats[-1].cpu().numpy().astype(np.float64) @ teacher.T + rng.gumbel(size=(B, K))).argmax(-1).astype(np.int64)
    yd = torch.from_numpy(y).cuda()
    first = pkg.fit_exit_heads(feats, yd, l2=L2, gtol=GTOL, num_labels=K)
    assert (first.status.cpu().numpy() == 0).all(), (first.status, first.grad_norm)
    eng.load_weights({**W, **first.state_dict(cfg)})
    dump = eng.forward(**inputs, dump_all=True, want_all=True)
    logits = dump.all_logits.to(torch.float64)
    z = logits.cpu().numpy()
    p = np.exp(z - z.max(-1, keepdims=True))
    conf = (p / p.sum(-1, keepdims=True)).max(-1)
    thr = np.quantile(conf, 0.6, axis=1)                                # every exit releases about 40 % of what it is shown
    exits = pkg.criterion_scan_device(logits, thr, "max_confidence")[0]
    reach = pkg.reach_weights(exits, 3)
    assert tuple(reach.shape) == (3, B) and reach.is_cuda and reach.dtype == torch.float32
    kept = reach.sum(dim=1).cpu().numpy()
    print("documents each exit is asked about:", kept)
    assert kept[0] == B and 0 < kept[1] < B and kept[2] >= 1, kept        # part of the batch leaves at exit 0, every exit keeps a document
    refit = pkg.fit_exit_heads(feats, yd, l2=L2, gtol=GTOL, num_labels=K, sample_weight=reach)
    print(f"refit: evals {refit.evals.cpu().tolist()} status {refit.status.cpu().tolist()} grad norms {refit.grad_norm.cpu().tolist()}")
    for name in HEAD_OUTPUTS:                                           # exit 0 is asked about everybody: a row of ones among the others
        assert torch.equal(getattr(refit, name)[0], getattr(first, name)[0]), name
    Xh, wh = feats.cpu().numpy(), reach.cpu().numpy()
    th_first, th_refit = _theta64(first), _theta64(refit)
    for e in range(3):
        l_first = WR.loss_grad(th_first[e], Xh[e], y, K, L2, wh[e])[0]
        l_refit = WR.loss_grad(th_refit[e], Xh[e], y, K, L2, wh[e])[0]
        print(f"exit {e}: reach-weighted objective {l_first:.6f} -> {l_refit:.6f}")
        assert l_refit <= l_first, (e, l_refit, l_first)
    eng.load_weights({**W, **refit.state_dict(cfg)})
    dump = eng.forward(**inputs, dump_all=True, want_head=True, want_all=True)
    eng.close()
    err = np.abs(dump.head_logits.cpu().numpy().astype(np.float64) - refit.logits(feats).cpu().numpy()).max()
    print(f"max |head_logits - HeadFit.logits| = {err:.3e}")
    assert err <= 1e-4, err


# ---- 10. the helpers -------------------------------------------------------------------------------------------------------------------------------
def test_helpers_match_numpy_one_liners(pkg):
    torch = _torch()
    rng = np.random.default_rng(3)
    for N, E in ((1, 1), (97, 3), (1000, 6)):
        exits = rng.integers(0, E + 1, N)
        want = (exits[None, :] >= np.arange(E)[:, None]).astype(np.float32)
        for given in (exits, torch.from_numpy(exits).cuda(), torch.from_numpy(exits.astype(np.int32)).cuda()):
            got = pkg.reach_weights(given, E)
            assert got.is_cuda and got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want)
    for N, K in ((5, 2), (97, 10), (1000, 16)):
        y = np.minimum(rng.integers(0, K, N), rng.integers(0, K, N))          # imbalanced
        y[:K] = np.arange(K)                                                     # no class is absent
        want = (N / (K * np.bincount(y, minlength=K)[y])).astype(np.float32)
        for given in (y, torch.from_numpy(y).cuda()):
            got = pkg.balanced_class_weights(given, K)
            assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (N,) and np.array_equal(got.cpu().numpy(), want)
