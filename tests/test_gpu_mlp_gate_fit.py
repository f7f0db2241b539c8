"""The two-layer gate fit on the device (include/mmee.h ee_mlp_head_fit_gate, ee_mlp_head_fit_gate_weighted) against the float64 restatement
of tests/mlp_gate_ref.py and the controller port of tests/mlp_headfit_ref.py: the loss / gradient launches alone (unweighted and weighted),
the first steps of a trajectory, the fit to a stationary point, its determinism and stopping rules, the failures of bad targets and weights,
and the loop dump rows -> targets -> fit -> load -> forward under the gate criterion.

Tolerance of the launch-alone comparison: rtol 1e-10, atol 1e-12 on the loss and on every gradient entry, the derived bars of
tests/test_gpu_mlp_head_fit.py: six of the seven launches are that fit's, and the seventh adds one exp, one log1p and one division per
logit at a few ulp."""
import functools

import numpy as np
import pytest

from . import gate_ref as G
from . import mlp_gate_ref as R
from . import mlp_headfit_ref as MR
from .conftest import H256_KW, report_measured
from .fit_util import _dev, _ptr, _stream, _torch

pytestmark = pytest.mark.gpu

L2, GTOL = 1e-2, 1e-6
RTOL, ATOL = 1e-10, 1e-12
FIT_SHAPES = [(3, 257, 64), (1, 63, 64), (2, 300, 128)]
OUTPUTS = ("dense_weight", "dense_bias", "weight", "bias", "theta64", "loss", "grad_norm", "evals", "status")
BAD_TARGET, BAD_WEIGHT, ZERO_SUM = "target is not finite or lies outside", "a sample weight is negative or not finite", "an exit's weights sum to zero"


def _lossgrad(pkg, X, T, theta, w=None, l2=L2):
    """ee_debug_mlp_head_gate_lossgrad (w None) or ee_debug_mlp_head_gate_weighted_lossgrad on host arrays X (E,N,H) f32, T (E,N), w (E,N),
    theta (E,P) f64 -> (loss (E,), grad (E,P)) host float64."""
    torch = _torch()
    lib = pkg.capi.load()
    E, N, H = X.shape
    Xd, Td, td = _dev(np.array(X), torch.float32), _dev(np.array(T), torch.float64), _dev(theta, torch.float64)
    loss = torch.full((E,), float("nan"), dtype=torch.float64, device="cuda")
    grad = torch.full((E, R.param_count(H)), float("nan"), dtype=torch.float64, device="cuda")
    if w is None:
        name = "ee_debug_mlp_head_gate_lossgrad"
        rc = lib.ee_debug_mlp_head_gate_lossgrad(_ptr(Xd), _ptr(Td), _ptr(td), E, N, H, l2, _ptr(loss), _ptr(grad), _stream())
    else:
        name = "ee_debug_mlp_head_gate_weighted_lossgrad"
        wd = _dev(np.array(w), torch.float32)
        rc = lib.ee_debug_mlp_head_gate_weighted_lossgrad(_ptr(Xd), _ptr(Td), _ptr(wd), _ptr(td), E, N, H, l2, _ptr(loss), _ptr(grad), _stream())
    pkg.capi.check(rc, None, name)
    return loss.cpu().numpy(), grad.cpu().numpy()


def _close(got_loss, got_grad, want_loss, want_grad, what):
    """-> the worst difference in units of the tolerance; asserts it is <= 1"""
    dl = abs(got_loss - want_loss) / (ATOL + RTOL * abs(want_loss))
    dg = (np.abs(got_grad - want_grad) / (ATOL + RTOL * np.abs(want_grad))).max()
    assert dl <= 1.0, (what, "loss", got_loss, want_loss)
    assert dg <= 1.0, (what, "grad", float(np.abs(got_grad - want_grad).max()), int(np.argmax(np.abs(got_grad - want_grad))))
    return max(dl, dg)


def _theta(rng, E, H):
    """theta ~ N(0, 1/H): pre-activations and logits of order 1."""
    return rng.standard_normal((E, R.param_count(H))) / np.sqrt(H)


def _weights(rng, E, N):
    """uniform in [0.25, 4), with rows at 0 (the first, the last, a few between) wherever an exit keeps a positive row"""
    w = rng.uniform(0.25, 4.0, (E, N)).astype(np.float32)
    if N > 2:
        w[:, [0, N - 1]] = 0.0
        w[rng.random((E, N)) < 0.15] = 0.0
        w[:, 1] = 1.5
    return w


# ---- 1. the loss / gradient launches alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [4, 64, 132, 256, 1024])
def test_lossgrad_matches_the_restatement(pkg, H):
    """Every E and N of the grid at this H, through both hooks: N = 1, around the row kernel's 32 rows and around the GEMMs' 64-row tile (and
    two tiles and a bit); H = 4 and 132 give ragged column tiles.  The weighted hook gets rows of weight zero whose targets are NaN."""
    rng = np.random.default_rng(H)
    worst = 0.0
    for E in (1, 3):
        theta = _theta(rng, E, H)
        for N in (1, 31, 32, 33, 63, 64, 65, 130):
            X, T = R.problem(E, N, H)
            loss, grad = _lossgrad(pkg, X, T, theta)
            for e in range(E):
                worst = max(worst, _close(loss[e], grad[e], *R.loss_grad(theta[e], X[e], T[e], L2), (H, E, N, e)))
            w = _weights(rng, E, N)
            Tw = np.where(w > 0, T, np.nan)
            loss, grad = _lossgrad(pkg, X, Tw, theta, w)
            for e in range(E):
                worst = max(worst, _close(loss[e], grad[e], *R.loss_grad(theta[e], X[e], Tw[e], L2, w[e]), (H, E, N, e, "weighted")))
    report_measured(f"mlp_gate_fit.lossgrad[H={H}]", "worst difference / tolerance (rtol 1e-10, atol 1e-12)", worst)


def test_lossgrad_logits_beyond_700_stay_finite(pkg):
    """W2 and b2 scaled until the logits pass +-700 on both sides: exp(700) is near float64's end, exp(-|z|) underflows, nothing overflows."""
    rng = np.random.default_rng(3)
    E, N, H = 2, 45, 256
    X, T = R.problem(E, N, H)
    theta = _theta(rng, E, H)
    theta[:, H * H + H:] *= 2500.0
    for e in range(E):
        z = R.logits(theta[e], X[e])
        assert z.max() > 700.0 and z.min() < -700.0, (z.min(), z.max())
    w = _weights(rng, E, N)
    worst = 0.0
    for ww in (None, w):
        loss, grad = _lossgrad(pkg, X, T, theta, ww)
        assert np.isfinite(loss).all() and np.isfinite(grad).all()
        for e in range(E):
            worst = max(worst, _close(loss[e], grad[e], *R.loss_grad(theta[e], X[e], T[e], L2, None if ww is None else ww[e]), ("large", e)))
    report_measured("mlp_gate_fit.lossgrad[logits beyond 700]", "worst difference / tolerance", worst)


def test_integer_weights_equal_row_repetition(pkg):
    """Integer weights through the weighted hook against the UNWEIGHTED hook on the rows physically repeated: the same objective, other
    sums, within the same bar."""
    rng = np.random.default_rng(8)
    E, N, H = 2, 67, 68
    X, T = R.problem(E, N, H)
    w1 = rng.integers(0, 4, N).astype(np.float32)
    w1[[0, 31, N - 1]] = 0.0
    rep = np.repeat(np.arange(N), w1.astype(np.int64))
    assert len(rep) == int(w1.sum()) and len(rep) != N
    theta = _theta(rng, E, H)
    got = _lossgrad(pkg, X, T, theta, np.tile(w1, (E, 1)))
    want = _lossgrad(pkg, np.ascontiguousarray(X[:, rep]), np.ascontiguousarray(T[:, rep]), theta)
    worst = max(_close(got[0][e], got[1][e], want[0][e], want[1][e], ("repetition", e)) for e in range(E))
    report_measured("mlp_gate_fit.lossgrad[repetition]", "worst difference / tolerance", worst)


# ---- 2. a short trajectory against the port -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,N,H", [(3, 300, 64), (1, 200, 768)])
def test_first_steps_follow_the_port(pkg, E, N, H):
    """Twelve evaluations from the identity start at gtol = 0: the device's iterate is the port's within 1e-8 (the bar and the shapes of the
    two-layer ramp's test; the second shape runs the controller at P ~ 600 k)."""
    X, T = R.problem(E, N, H)
    fit = pkg.fit_mlp_gate_heads(X, T, l2=L2, gtol=0.0, max_evals=12)
    assert (fit.status.cpu().numpy() == 1).all() and (fit.evals.cpu().numpy() == 12).all()
    theta, loss = fit.theta64.cpu().numpy(), fit.loss.cpu().numpy()
    worst = 0.0
    for e in range(E):
        port = R.port(X[e], T[e], L2, 0.0, 12)
        assert port[3] == 12 and port[4] == 1
        diff = float(np.abs(theta[e] - port[0]).max())
        worst = max(worst, diff)
        l_dev = R.loss_grad(theta[e], X[e], T[e], L2)[0]
        print(f"exit {e}: max |theta64 - port| = {diff:.3e}, loss {loss[e]:.6f} (port {port[1]:.6f})")
        assert diff <= 1e-8, (e, diff)
        assert abs(loss[e] - l_dev) <= ATOL + RTOL * abs(l_dev), (e, loss[e], l_dev)
    report_measured(f"mlp_gate_fit.first_steps[{E},{N},{H}]", "max |theta64 - port| after 12 evaluations", worst)


# ---- 3. the fit to a stationary point -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(E, N, H):
    X, T = R.problem(E, N, H)
    X.setflags(write=False)
    T.setflags(write=False)
    return X, T


@functools.lru_cache(maxsize=None)
def _one_layer_optimum(E, N, H):
    X, T = _problem(E, N, H)
    return tuple(G.gate_lossgrad(G.gate_fit(X[e], T[e], L2)[0], X[e], T[e], L2)[0] for e in range(E))


@pytest.mark.parametrize("E,N,H", FIT_SHAPES)
def test_fit_reaches_a_stationary_point_below_the_one_layer_optimum(pkg, E, N, H):
    """The numpy port (CPU) on these problems, loss against the one-layer gate optimum (gate_ref.gate_fit), per exit --
    (3,257,64): 384 / 193 / 83 evaluations: 0.2477 / 0.4425 / 0.0681 against 0.4284 / 0.4504 / 0.1284;
    (1,63,64): 190: 0.0871 against 0.1552;  (2,300,128): 1096 / 239: 0.1739 / 0.4616 against 0.3189 / 0.4665.
    The start (identity) is at log 2 + l2 H / 2 = 1.0131 (H = 64) and 1.3331 (H = 128).  "Below the one-layer optimum" is asserted for the
    hard and the all-ones exits; for the soft ones the margin is below 0.01 and both values are printed.
    First run on the device (MI355X): 378 / 187 / 83, 190 and 1014 / 257 evaluations, all status 0, to the port's losses in every printed digit
    (0.247745 / 0.442521 / 0.068082, 0.087063, 0.173869 / 0.461558) with float64 gradient norms of 3.5e-7 ... 9.6e-7; beyond the first steps
    the evaluation counts part from the port's, the stationary points reached do not."""
    X, T = _problem(E, N, H)
    one_layer = _one_layer_optimum(E, N, H)
    fit = pkg.fit_mlp_gate_heads(X, T, l2=L2, gtol=GTOL, max_evals=4000)
    status, evals = fit.status.cpu().numpy(), fit.evals.cpu().numpy()
    loss, gnorm, theta = fit.loss.cpu().numpy(), fit.grad_norm.cpu().numpy(), fit.theta64.cpu().numpy()
    print(f"({E},{N},{H}): evals {evals.tolist()} status {status.tolist()} loss {loss.tolist()} one-layer {list(one_layer)}")
    assert (status == 0).all(), (status, gnorm)
    assert (evals >= 1).all() and (evals <= 4000).all(), evals
    HH = H * H
    worst = 0.0
    for e, kind in enumerate(R.kinds(E, N)):
        l_dev, g_dev = R.loss_grad(theta[e], X[e], T[e], L2)
        n_dev = float(np.linalg.norm(g_dev))
        l_start = R.loss_grad(R.init_identity(H), X[e], T[e], L2)[0]
        print(f"exit {e} ({kind}): ||grad(theta64)|| {n_dev:.3e}  loss {l_dev:.6f}  start {l_start:.6f}  one-layer optimum {one_layer[e]:.6f}")
        assert n_dev <= 2 * GTOL, (e, n_dev)
        assert abs(loss[e] - l_dev) <= ATOL + RTOL * abs(l_dev), (e, loss[e], l_dev)
        assert abs(gnorm[e] - n_dev) <= ATOL + RTOL * n_dev, (e, gnorm[e], n_dev)
        worst = max(worst, abs(loss[e] - l_dev) / (ATOL + RTOL * abs(l_dev)), abs(gnorm[e] - n_dev) / (ATOL + RTOL * n_dev))
        assert loss[e] < l_start, (e, loss[e], l_start)
        if kind != "soft":
            assert loss[e] < one_layer[e], (e, kind, loss[e], one_layer[e])
        th32 = theta[e].astype(np.float32)
        assert np.array_equal(fit.dense_weight[e].cpu().numpy().reshape(-1), th32[:HH])
        assert np.array_equal(fit.dense_bias[e].cpu().numpy(), th32[HH:HH + H])
        assert np.array_equal(fit.weight[e].cpu().numpy().reshape(-1), th32[HH + H:HH + 3 * H])
        assert np.array_equal(fit.bias[e].cpu().numpy(), th32[HH + 3 * H:])
    assert tuple(fit.weight.shape) == (E, 2, H) and tuple(fit.bias.shape) == (E, 2)
    report_measured(f"mlp_gate_fit[{E},{N},{H}]", "reported loss and gradient norm against the restatement, worst difference / tolerance", worst)


# ---- 4. properties ------------------------------------------------------------------------------------------------------------------------------
def _bits(fit, e=None):
    return [(getattr(fit, n) if e is None else getattr(fit, n)[e]).cpu().numpy().tobytes() for n in OUTPUTS]


def test_two_streams_and_an_exit_alone_return_the_same_bits(pkg):
    torch = _torch()
    E, N, H = FIT_SHAPES[0]
    X, T = _problem(E, N, H)
    Xd, Td = _dev(np.array(X), torch.float32), _dev(np.array(T), torch.float64)
    fits = []
    for _ in range(2):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fits.append(pkg.fit_mlp_gate_heads(Xd, Td, l2=L2, gtol=GTOL, max_evals=120))
        s.synchronize()
    assert (fits[0].evals.cpu().numpy() > 12).all() and _bits(fits[0]) == _bits(fits[1])
    for e in range(E):
        alone = pkg.fit_mlp_gate_heads(Xd[e:e + 1].contiguous(), Td[e:e + 1].contiguous(), l2=L2, gtol=GTOL, max_evals=120)
        assert _bits(alone, 0) == _bits(fits[0], e), e


def test_max_evals_stops_with_status_1_and_a_loss_not_above_the_start(pkg):
    E, N, H = FIT_SHAPES[0]
    X, T = _problem(E, N, H)
    fit = pkg.fit_mlp_gate_heads(X, T, l2=L2, gtol=GTOL, max_evals=3)
    assert (fit.status.cpu().numpy() == 1).all() and (fit.evals.cpu().numpy() == 3).all()
    loss, theta = fit.loss.cpu().numpy(), fit.theta64.cpu().numpy()
    for e in range(E):
        l_dev = R.loss_grad(theta[e], X[e], T[e], L2)[0]
        assert loss[e] <= R.loss_grad(R.init_identity(H), X[e], T[e], L2)[0]
        assert abs(loss[e] - l_dev) <= ATOL + RTOL * abs(l_dev)


def test_a_warm_start_from_a_returned_point_stops_after_one_evaluation(pkg):
    E, N, H = FIT_SHAPES[1]
    X, T = _problem(E, N, H)
    cold = pkg.fit_mlp_gate_heads(X, T, l2=L2, gtol=GTOL)
    assert (cold.status.cpu().numpy() == 0).all()
    warm = pkg.fit_mlp_gate_heads(X, T, l2=L2, gtol=GTOL, init=cold.theta64)
    assert (warm.status.cpu().numpy() == 0).all() and (warm.evals.cpu().numpy() == 1).all()
    for name in OUTPUTS[:7]:
        assert getattr(warm, name).cpu().numpy().tobytes() == getattr(cold, name).cpu().numpy().tobytes(), name
    # the same start, named as a checkpoint names it (float64 tensors, so nothing is rounded on the way)
    HH, th = H * H, cold.theta64[0]
    p = "layoutlmv3.encoder.early_exits.0."
    named = {p + "dense.weight": th[:HH].view(H, H), p + "dense.bias": th[HH:HH + H], p + "out_proj.weight": th[HH + H:HH + 3 * H].view(2, H),
             p + "out_proj.bias": th[HH + 3 * H:]}
    again = pkg.fit_mlp_gate_heads(X, T, l2=L2, gtol=GTOL, init=named)
    assert (again.evals.cpu().numpy() == 1).all() and again.theta64.cpu().numpy().tobytes() == cold.theta64.cpu().numpy().tobytes()


def test_all_ones_weights_are_the_unweighted_fit_and_w_and_4w_agree_bit_for_bit(pkg):
    """W_e = N exactly, so every scale is 1.0 and the one more multiplication changes no bit; 4 w and 4 W are exact, so the scales are the same
    numbers."""
    torch = _torch()
    E, N, H = FIT_SHAPES[0]
    X, T = _problem(E, N, H)
    plain = pkg.fit_mlp_gate_heads(X, T, l2=L2, gtol=GTOL, max_evals=50)
    assert (plain.evals.cpu().numpy() > 1).all()
    for ones in (np.ones(N, dtype=np.float32), np.ones((E, N), dtype=np.float64), torch.ones((E, N), dtype=torch.int32, device="cuda")):
        assert _bits(pkg.fit_mlp_gate_heads(X, T, l2=L2, gtol=GTOL, max_evals=50, sample_weight=ones)) == _bits(plain)
    w = _weights(np.random.default_rng(4), E, N)
    a = pkg.fit_mlp_gate_heads(X, T, l2=L2, gtol=GTOL, max_evals=50, sample_weight=w)
    b = pkg.fit_mlp_gate_heads(X, T, l2=L2, gtol=GTOL, max_evals=50, sample_weight=4.0 * w)
    assert _bits(a) == _bits(b) and _bits(a) != _bits(plain)
    theta, loss = a.theta64.cpu().numpy(), a.loss.cpu().numpy()
    for e in range(E):                                            # and the weighted fit reports the weighted objective
        l_dev = R.loss_grad(theta[e], X[e], T[e], L2, w[e])[0]
        assert abs(loss[e] - l_dev) <= ATOL + RTOL * abs(l_dev), (e, loss[e], l_dev)
        assert loss[e] < R.loss_grad(R.init_identity(H), X[e], T[e], L2, w[e])[0]


# ---- 5. failures ----------------------------------------------------------------------------------------------------------------------------------
def _raw_fit_leaves_outputs(pkg, X, T, w, needle):
    """The C fit (weighted when w is given) on NaN-prefilled outputs (7 in the integer ones): it fails with `needle`, none of them is touched."""
    torch = _torch()
    lib = pkg.capi.load()
    E, N, H = X.shape
    P = R.param_count(H)
    nan = float("nan")
    Xd, Td = _dev(np.array(X), torch.float32), _dev(np.array(T), torch.float64)
    th0 = _dev(np.stack([R.init_identity(H)] * E), torch.float64)
    outs = [torch.full(s, v, dtype=dt, device="cuda") for s, v, dt in (((E, H, H), nan, torch.float32), ((E, H), nan, torch.float32),
            ((E, 2, H), nan, torch.float32), ((E, 2), nan, torch.float32), ((E, P), nan, torch.float64), ((E,), nan, torch.float64),
            ((E,), nan, torch.float64), ((E,), 7, torch.int32), ((E,), 7, torch.int32))]
    if w is None:
        need = lib.ee_mlp_head_fit_workspace_bytes(E, N, H, 2, 8)
        ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
        rc = lib.ee_mlp_head_fit_gate(_ptr(Xd), _ptr(Td), _ptr(th0), E, N, H, L2, GTOL, 50, 8, _ptr(ws), need, *[_ptr(o) for o in outs], _stream())
    else:
        wd = _dev(np.array(w), torch.float32)
        need = lib.ee_mlp_head_fit_weighted_workspace_bytes(E, N, H, 2, 8)
        ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
        rc = lib.ee_mlp_head_fit_gate_weighted(_ptr(Xd), _ptr(Td), _ptr(wd), _ptr(th0), E, N, H, L2, GTOL, 50, 8, _ptr(ws), need,
                                               *[_ptr(o) for o in outs], _stream())
    assert rc != 0 and needle in pkg.capi.last_error() and "no output was written" in pkg.capi.last_error(), pkg.capi.last_error()
    torch.cuda.synchronize()
    for o in outs[:7]:
        assert bool(torch.isnan(o).all())
    for o in outs[7:]:
        assert bool((o == 7).all())


def test_bad_targets_and_weights_fail_the_call_and_leave_the_outputs_untouched(pkg):
    E, N, H = 3, 63, 64
    X, T = _problem(E, N, H)
    good = _weights(np.random.default_rng(2), E, N)
    live = int(np.flatnonzero(good[E - 1] > 0)[3])
    theta = np.stack([R.init_identity(H)] * E)
    for bad in (-0.1, 1.5, float("nan")):
        Tb = np.array(T)
        Tb[E - 1, live] = bad
        for w in (None, good):
            with pytest.raises(pkg.capi.MMEEError, match=BAD_TARGET):
                pkg.fit_mlp_gate_heads(X, Tb, l2=L2, gtol=GTOL, max_evals=50, sample_weight=w)
            _raw_fit_leaves_outputs(pkg, X, Tb, w, BAD_TARGET)
            with pytest.raises(pkg.capi.MMEEError, match=BAD_TARGET):
                _lossgrad(pkg, X, Tb, theta, w)
        # the same bad target under a zero weight goes through, with the bits of the clean call
        w0 = good.copy()
        w0[E - 1, live] = 0.0
        clean = pkg.fit_mlp_gate_heads(X, T, l2=L2, gtol=GTOL, max_evals=50, sample_weight=w0)
        dirty = pkg.fit_mlp_gate_heads(X, Tb, l2=L2, gtol=GTOL, max_evals=50, sample_weight=w0)
        assert _bits(dirty) == _bits(clean)
        a, b = _lossgrad(pkg, X, T, theta, w0), _lossgrad(pkg, X, Tb, theta, w0)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and np.isfinite(b[1]).all()
    for bad, needle in ((-0.5, BAD_WEIGHT), (float("nan"), BAD_WEIGHT), (None, ZERO_SUM)):
        w = good.copy()
        if bad is None:
            w[1] = 0.0                                                          # one exit's whole row
        else:
            w[E - 1, N - 1] = bad
        Tb = np.array(T)
        Tb[0, live] = 1.5                                                       # weight bits are looked at first
        for TT in (T, Tb):
            with pytest.raises(pkg.capi.MMEEError, match=needle):
                pkg.fit_mlp_gate_heads(X, TT, l2=L2, gtol=GTOL, max_evals=50, sample_weight=w)
            _raw_fit_leaves_outputs(pkg, X, TT, w, needle)
            with pytest.raises(pkg.capi.MMEEError, match=needle):
                _lossgrad(pkg, X, TT, theta, w)
    ok = pkg.fit_mlp_gate_heads(X, T, l2=L2, gtol=GTOL, max_evals=50, sample_weight=good)         # the mended inputs go through
    assert np.isin(ok.status.cpu().numpy(), (0, 1)).all()


# ---- 6. through the engine ----------------------------------------------------------------------------------------------------------------------
def _restated(fit, e):
    return fit.theta64[e].cpu().numpy()


def test_dump_targets_fit_load_forward_under_the_gate_criterion(pkg):
    """A two-layer gate configuration (the default depth), encoder exits only: collect_gate_features -> gate_targets -> fit_mlp_gate_heads ->
    load_weights(state_dict) on a fresh engine -> forward under inference_strategy = "gate".  head_logits equal MlpGateFit's float32 heads on
    the collected rows within 1e-4 (the project's logit bar), all_crit is MlpGateFit.scores, and the forward decides on them.  Status 0 is not
    required: at H = 256, N = 96 the two-layer fits run out a budget of 1000.  Then once more with reach_weights of that forward."""
    torch = _torch()
    B, T = 96, 48
    ee = dict(exits=[1, 2], encoder_layer_strategy="gate", exit_head_num_layers=2, inference_strategy="gate")
    cfg = pkg.ModelConfig.tiny(EE_config=ee, **H256_KW)
    E, H, K = 2, cfg.hidden_size, cfg.num_labels
    W = pkg.synth.make_weights(cfg, seed=51, head_gain=4.0)
    docs = pkg.synth.make_documents(cfg, B, seed=52, text_len=T, min_words=3)
    t = {k: torch.from_numpy(docs[k]).cuda() for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision="split")
    eng.load_weights(W)
    feats, gated = pkg.collect_gate_features(eng, [t])
    assert tuple(feats.shape) == (E, B, H) and feats.dtype == torch.float32 and tuple(gated.shape) == (E, B, K)
    head_names = [n for n in eng.expected_tensors() if "early_exits" in n]
    eng.close()
    # a document's label is the gated argmax at a randomly chosen exit, or, for about a third of the documents, the runner-up of the last exit:
    # the classifier is right on some documents and wrong on others at every exit, also where the exits' argmaxes agree
    rng = np.random.default_rng(53)
    zg = gated.cpu().numpy()
    pred = zg.argmax(-1)
    pick = rng.integers(0, E + 1, B)
    y = np.where(pick < E, pred[np.minimum(pick, E - 1), np.arange(B)], np.argsort(zg[E - 1], axis=-1)[:, -2]).astype(np.int64)
    targets = pkg.gate_targets(gated, torch.from_numpy(y).cuda())
    Tn = targets.cpu().numpy()
    assert ((Tn.sum(1) > 0) & (Tn.sum(1) < B)).all(), Tn.sum(1)
    fit = pkg.fit_mlp_gate_heads(feats, targets, l2=L2, gtol=GTOL, max_evals=1000)
    status = fit.status.cpu().numpy()
    print(f"evals {fit.evals.cpu().tolist()} status {status.tolist()} loss {fit.loss.cpu().tolist()} grad norm {fit.grad_norm.cpu().tolist()}")
    assert np.isin(status, (0, 1)).all(), status
    sd = fit.state_dict(cfg)
    assert sorted(sd) == sorted(head_names) and len(sd) == 4 * E
    assert sd["layoutlmv3.encoder.early_exits.0.out_proj.weight"].shape == (2, H) and sd["layoutlmv3.encoder.early_exits.1.dense.weight"].shape == (H, H)

    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision="split")
    eng.load_weights({**W, **sd})
    dump = eng.forward(**t, dump_all=True, want_all=True, want_head=True, want_hidden_cls=True, whole_layers=True)
    want = fit.logits(feats).cpu().numpy()
    got = dump.head_logits.cpu().numpy().astype(np.float64)
    err = float(np.abs(got - want).max())
    report_measured("mlp_gate_fit[engine]", "max |head_logits - MlpGateFit.logits|", err)
    assert err <= 1e-4
    scores = fit.scores(feats).cpu().numpy()
    err_s = float(np.abs(dump.all_crit.cpu().numpy()[:E].astype(np.float64) - scores).max())
    report_measured("mlp_gate_fit[engine]", "max |all_crit - MlpGateFit.scores|", err_s)
    assert err_s <= 1e-4
    g = G.gate_score(dump.head_logits.cpu().numpy())
    thr, ex = G.cascade_thresholds(g)
    out = eng.forward(**t, thresholds=thr, whole_layers=True)
    exits = out.exit_layer
    assert np.array_equal(exits.cpu().numpy(), ex) and set(ex.tolist()) == {0, 1, 2}
    eng.check()
    eng.close()
    # the fitted gates beat the synthetic ones on their own objective
    Xn = feats.cpu().numpy()
    p = "layoutlmv3.encoder.early_exits."
    for e in range(E):
        syn = MR.join(*[W[f"{p}{e}.{name}"] for name in ("dense.weight", "dense.bias", "out_proj.weight", "out_proj.bias")])
        l_fit, l_syn = R.loss_grad(_restated(fit, e), Xn[e], Tn[e], L2)[0], R.loss_grad(syn, Xn[e], Tn[e], L2)[0]
        print(f"exit {e}: restated loss {l_fit:.6f}, synthetic head {l_syn:.6f}, start {R.loss_grad(R.init_identity(H), Xn[e], Tn[e], L2)[0]:.6f}")
        assert l_fit < l_syn, (e, l_fit, l_syn)

    # once more, every gate fitted on the documents that reach it under that forward
    reach = pkg.reach_weights(exits, E)
    wn = reach.cpu().numpy()
    assert wn[0].sum() == B and 0 < wn[1].sum() < B, wn.sum(1)
    refit = pkg.fit_mlp_gate_heads(feats, targets, l2=L2, gtol=GTOL, max_evals=1000, sample_weight=reach)
    print(f"refit: evals {refit.evals.cpu().tolist()} status {refit.status.cpu().tolist()} loss {refit.loss.cpu().tolist()}")
    assert np.isin(refit.status.cpu().numpy(), (0, 1)).all()
    for name in OUTPUTS:                                           # exit 0 is asked about everybody: a row of ones among the others
        assert torch.equal(getattr(refit, name)[0], getattr(fit, name)[0]), name
    l_first = R.loss_grad(_restated(fit, 1), Xn[1], Tn[1], L2, wn[1])[0]
    l_refit = R.loss_grad(_restated(refit, 1), Xn[1], Tn[1], L2, wn[1])[0]
    print(f"exit 1 on the {int(wn[1].sum())} rows that reach it: objective {l_first:.6f} (unweighted fit) -> {l_refit:.6f} (reach-weighted fit)")
    assert l_refit <= l_first, (l_refit, l_first)
    assert len(refit.state_dict(cfg)) == 4 * E
