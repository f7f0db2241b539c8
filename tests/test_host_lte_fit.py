"""The LTE classifier fit without a GPU: the float64 restatement of tests/lte_fit_ref.py against central differences, its targets, its power to
tell subtle faults of the objective apart at the tolerance the device test uses, the scipy reference's own agreement between starts, and the
host-side surface (state_dict, refusals of the Python layer and of the C entry points before any device call)."""
import ctypes as C

import numpy as np
import pytest

from . import lte_fit_ref as LR
from .fit_util import _HostTensor, _refused

L2 = 1e-2
FIT_SHAPES = [(300, 64, 3), (257, 64, 1), (1000, 256, 2), (600, 768, 1), (96, 256, 3)]       # (N, H, E)


@pytest.mark.parametrize("loss", LR.LOSSES)
@pytest.mark.parametrize("N,H,E", [(7, 8, 1), (40, 12, 3), (25, 16, 2)])
def test_restatement_gradient_agrees_with_central_differences(N, H, E, loss):
    """Central differences with h = 1e-5 on an objective whose third derivatives are of order 1: truncation h^2 ~ 1e-10, rounding
    eps |L| / h ~ 1e-11; the bar is 1e-8."""
    rng = np.random.default_rng(N)
    X = rng.standard_normal((E, N, H)).astype(np.float32)
    T = rng.random((E, N)) if N == 25 else (rng.random((E, N)) < 0.5).astype(np.float64)
    theta = 0.3 * rng.standard_normal(H + 1)
    _, g = LR.loss_grad(theta, X, T, loss, L2)
    h = 1e-5
    num = np.empty_like(g)
    for i in range(theta.size):
        d = np.zeros_like(theta)
        d[i] = h
        num[i] = (LR.loss_grad(theta + d, X, T, loss, L2)[0] - LR.loss_grad(theta - d, X, T, loss, L2)[0]) / (2 * h)
    assert np.abs(num - g).max() <= 1e-8, np.abs(num - g).max()


def test_targets_on_ties_and_with_one_class():
    logits = np.array([[[1.0, 3.0, 3.0], [2.0, 2.0, 2.0], [0.0, -1.0, 5.0]]], dtype=np.float32)       # first maximum: 1, 0, 2
    assert np.array_equal(LR.targets(logits, [1, 0, 2]), [[0.0, 0.0, 0.0]])
    assert np.array_equal(LR.targets(logits, [2, 1, 0]), [[1.0, 1.0, 1.0]])        # the later tied maximum does not count
    one = np.zeros((2, 4, 1), dtype=np.float32)
    assert np.array_equal(LR.targets(one, np.zeros(4, dtype=np.int64)), np.zeros((2, 4)))              # K = 1: always right


def _faulty(theta, X, T, loss, l2, fault):
    """The restatement with one subtle fault."""
    X = np.asarray(X, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    E, N, H = X.shape
    if fault == "t for 1 - t":
        T = 1.0 - T
    a = LR.activations(theta, X)
    s = LR._sigmoid(a)
    if loss == "mse":
        l = (s - T) ** 2
        d = 2.0 * (s - T) * s * (1.0 - s)
        if fault == "s(1-s) dropped":
            d = 2.0 * (s - T)
        if fault == "factor 2 dropped":
            d = (s - T) * s * (1.0 - s)
    else:
        with np.errstate(over="ignore"):
            l = (np.log1p(np.exp(a)) if fault == "softplus not shifted" else np.maximum(a, 0.0) + np.log1p(np.exp(-np.abs(a)))) - T * a
        d = s - T
    denom = E * N if fault == "mean over E N" else N
    pen = theta.copy()
    if fault == "bias unpenalised":
        pen[-1] = 0.0
    L = float(l.sum() / denom + 0.5 * l2 * np.dot(pen, pen))
    g = np.concatenate([np.einsum("en,enh->h", d, X), [d.sum()]]) / denom + l2 * pen
    return L, g


def _bars(got, want):
    """The largest difference in units of the device test's tolerance; inf / NaN counts as infinitely far."""
    (l0, g0), (l1, g1) = got, want
    with np.errstate(invalid="ignore"):
        dl = abs(l0 - l1) / (LR.ATOL + LR.RTOL * abs(l1))
        dg = (np.abs(g0 - g1) / (LR.ATOL + LR.RTOL * np.abs(g1))).max()
    return max(np.nan_to_num(dl, nan=np.inf), np.nan_to_num(dg, nan=np.inf))


@pytest.mark.parametrize("fault,loss", [("s(1-s) dropped", "mse"), ("factor 2 dropped", "mse"), ("mean over E N", "mse"), ("mean over E N", "bce"),
                                        ("t for 1 - t", "mse"), ("t for 1 - t", "bce"), ("bias unpenalised", "mse"), ("bias unpenalised", "bce"),
                                        ("softplus not shifted", "bce")])
def test_each_subtle_fault_moves_a_figure_by_ten_tolerances_on_the_shared_inputs(fault, loss):
    cases = LR.kernel_cases()
    seen = {}
    for name, (X, T, theta) in cases.items():
        assert _bars(_faulty(theta, X, T, loss, L2, None), LR.loss_grad(theta, X, T, loss, L2)) <= 1e-2      # no fault: the restatement, up to the order of its sums
        seen[name] = _bars(_faulty(theta, X, T, loss, L2, fault), LR.loss_grad(theta, X, T, loss, L2))
    print(fault, loss, {k: f"{v:.2e}" for k, v in seen.items()})
    assert max(seen.values()) >= 10.0, seen
    if fault == "softplus not shifted":
        assert seen["large"] > 1e300 and max(v for k, v in seen.items() if k != "large") < 1.0      # exp(770) overflows: only the large activations tell


def test_the_large_case_overflows_an_unshifted_form_and_the_restatement_stays_finite():
    X, T, theta = LR.kernel_cases()["large"]
    a = LR.activations(theta, X)
    assert a.max() > 720.0 and a.min() < -720.0
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.exp(np.abs(a))).all()
    for loss in LR.LOSSES:
        L, g = LR.loss_grad(theta, X, T, loss, L2)
        assert np.isfinite(L) and np.isfinite(g).all()


@pytest.mark.parametrize("loss", LR.LOSSES)
@pytest.mark.parametrize("N,H,E", FIT_SHAPES)
def test_the_scipy_reference_reaches_one_point_from_four_starts(N, H, E, loss):
    """solve_starts asserts a gradient norm <= 1e-8 for every start.  Measured here: the four end points lie within 4.5e-7 of each other on
    every problem and both losses, so these MSE problems have one basin; the bar is solve()'s own 1e-6."""
    X, T = LR.problem(N, H, E, seed=N + H + E)
    pts = LR.solve_starts(X, T, loss, L2, n_starts=4)
    spread = max(float(np.linalg.norm(p - pts[0])) for p in pts[1:])
    print(f"(N,H,E) = {(N, H, E)} {loss}: largest distance between four starts {spread:.3e}")
    assert spread <= 1e-6, spread
    assert LR.loss_grad(pts[0], X, T, loss, L2)[0] < LR.loss_grad(np.zeros(H + 1), X, T, loss, L2)[0]


def _host_fit(pkg, H):
    rng = np.random.default_rng(0)
    w, b = rng.standard_normal((1, H)).astype(np.float32), rng.standard_normal((1,)).astype(np.float32)
    return pkg.LteFit(_HostTensor(w), _HostTensor(b), None, None, None, None, None, 1e-2, "mse"), w, b


LTE_EE = dict(exits=[1, 2, 3], encoder_layer_strategy="ramp", use_lte=True)


def test_state_dict_names_are_the_synthetic_weights_lte_names(pkg):
    cfg = pkg.ModelConfig.tiny(EE_config=dict(LTE_EE))
    W = pkg.synth.make_weights(cfg, seed=1)
    fit, w, b = _host_fit(pkg, cfg.hidden_size)
    sd = fit.state_dict(cfg)
    assert set(sd) == {k for k in W if "lte_classifier" in k} and len(sd) == 2
    for k, v in sd.items():
        assert v.shape == W[k].shape and v.dtype == np.float32 and v.flags["C_CONTIGUOUS"], k
    assert np.array_equal(sd["layoutlmv3.encoder.lte_classifier.weight"], w) and sd["layoutlmv3.encoder.lte_classifier.weight"].shape == (1, cfg.hidden_size)
    assert np.array_equal(sd["layoutlmv3.encoder.lte_classifier.bias"], b) and sd["layoutlmv3.encoder.lte_classifier.bias"].shape == (1,)
    gate = pkg.ModelConfig.tiny(EE_config=dict(exits=["text_avg", 1, 2], encoder_layer_strategy="gate", exit_head_num_layers=1))
    assert set(fit.state_dict(gate)) == set(sd)             # gates, embedding exits and a handle without use_lte are all in scope


def test_python_surface_refuses_what_is_out_of_scope(pkg):
    fit, _, _ = _host_fit(pkg, 64)
    beit = pkg.ModelConfig.dit_tiny(EE_config=dict(exits=[1, 2], encoder_layer_strategy="ramp", exit_head_num_layers=1))
    none = pkg.ModelConfig.tiny(EE_config=dict(exits=["text_avg"], encoder_layer_strategy="ramp"))
    with pytest.raises(ValueError, match="LayoutLMv3"):
        fit.state_dict(beit)
    with pytest.raises(ValueError, match="no encoder exits"):
        fit.state_dict(none)
    with pytest.raises(ValueError, match="the configuration wants"):
        fit.state_dict(pkg.ModelConfig.tiny(EE_config=dict(LTE_EE)))           # H = 64 against the tiny shape's hidden size

    class _Engine:
        def __init__(self, cfg):
            self.cfg = cfg
    with pytest.raises(ValueError, match="LayoutLMv3"):
        pkg.collect_lte_features(_Engine(beit), [])
    with pytest.raises(ValueError, match="no encoder exits"):
        pkg.collect_lte_features(_Engine(none), [])

    X, T = np.zeros((2, 5, 8), dtype=np.float32), np.zeros((2, 5))
    with pytest.raises(ValueError, match="loss = 'hinge'"):
        pkg.fit_lte_classifier(X, T, loss="hinge")
    with pytest.raises(ValueError, match=r"init is \(8,\), need \(H\+1,\) = \(9,\)"):
        pkg.fit_lte_classifier(X, T, init=np.zeros(8))
    with pytest.raises(ValueError, match=r"lte_classifier.weight is \(8,\), need \(1, 8\)"):
        pkg.fit_lte_classifier(X, T, init={"layoutlmv3.encoder.lte_classifier.weight": np.zeros(8), "layoutlmv3.encoder.lte_classifier.bias": np.zeros(1)})
    with pytest.raises(ValueError, match="names 0 tensors"):
        pkg.fit_lte_classifier(X, T, init={})


def test_c_entry_points_refuse_bad_arguments_before_any_device_call(pkg):
    """Every refusal below is decided on the host: the message names the argument and never "no HIP device"."""
    lib = pkg.capi.load()
    assert pkg.capi.LTE_FIT_ROWS == 16 and (pkg.capi.LTE_LOSS_MSE, pkg.capi.LTE_LOSS_BCE) == (0, 1)
    E, N, H = 2, 100, 64
    need = lib.ee_lte_fit_workspace_bytes(E, N, H, 8)
    assert need > 0 and lib.ee_lte_fit_workspace_bytes(0, N, H, 8) == 0
    for args in ((3, N, H, 8), (E, 5000, H, 8), (E, N, 128, 8), (E, N, H, 9)):
        assert lib.ee_lte_fit_workspace_bytes(*args) > need, args
    p = C.c_void_p(4096)                                    # never dereferenced: every call below is refused first

    def fit(X=p, T=p, E=E, N=N, H=H, loss=0, l2=1e-2, gtol=1e-9, evals=10, hist=8, ws=p, ws_bytes=need, w=p, b=p):
        return lib.ee_lte_fit(X, T, None, E, N, H, loss, l2, gtol, evals, hist, ws, ws_bytes, w, b, None, None, None, None, None, None)

    cases = {
        "null features": (dict(X=None), "NULL"), "null targets": (dict(T=None), "NULL"), "null weight": (dict(w=None), "NULL"),
        "E = 0": (dict(E=0), "E = 0"), "E = 65": (dict(E=65), "E = 65"), "N = 0": (dict(N=0), "N = 0"),
        "H = 1028": (dict(H=1028), "H = 1028"), "H = 66": (dict(H=66), "H = 66"), "loss = 2": (dict(loss=2), "loss = 2"),
        "l2 = 0": (dict(l2=0.0), "l2 = 0"), "l2 = nan": (dict(l2=float("nan")), "l2 = nan"), "gtol < 0": (dict(gtol=-1.0), "gtol"),
        "max_evals = 0": (dict(evals=0), "max_evals = 0"), "history = 0": (dict(hist=0), "history = 0"), "history = 33": (dict(hist=33), "history = 33"),
        "unaligned features": (dict(X=C.c_void_p(4100)), "aligned"), "small workspace": (dict(ws_bytes=need - 1), f"needs {need} bytes"),
    }
    _refused(pkg, "ee_lte_fit", fit, cases)
    assert lib.ee_debug_lte_lossgrad(p, p, None, E, N, H, 0, 1e-2, p, p, None) != 0 and "NULL" in pkg.capi.last_error()
    assert lib.ee_debug_lte_lossgrad(p, p, p, E, N, H, 0, -1.0, p, p, None) != 0 and "l2 = -1" in pkg.capi.last_error()
    assert lib.ee_lte_targets(p, p, E, N, 0, p, None) != 0 and "ee_lte_targets" in pkg.capi.last_error()
    assert lib.ee_lte_scores(p, C.c_void_p(4100), p, E, N, H, p, None) != 0 and "aligned" in pkg.capi.last_error()
    assert lib.ee_lte_scores(p, p, p, E, N, 6, p, None) != 0 and "H = 6" in pkg.capi.last_error()
