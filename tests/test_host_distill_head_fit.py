"""CPU checks of the distilled exit-head fits (include/mmee.h ee_head_fit_distill, ee_mlp_head_fit_distill): the C-ABI (declarations, plain-C
compile, ABI 4, exported symbols), the entry points' refusals before they look for a device, what the Python surface refuses, and the float64
restatement of tests/distill_headfit_ref.py against central differences and against tests/headfit_ref.py at alpha = 0."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import distill_headfit_ref as DR
from . import headfit_ref as HR
from . import mlp_headfit_ref as MR
from .conftest import ROOT
from .fit_util import _refused, compiles_as_c, exported_symbols

NAMES = ("ee_head_fit_distill", "ee_debug_head_distill_lossgrad", "ee_mlp_head_fit_distill", "ee_debug_mlp_head_distill_lossgrad")
PAIRS = [(1.0, 1.0), (0.5, 2.0), (0.3, 4.0), (0.0, 1.0)]


def test_header_declares_the_four_functions():
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    assert re.search(r"#define\s+MMEE_ABI_VERSION\s+4\b", header)           # four more functions: ee_config is unchanged
    declared = set(re.findall(r"\b(ee_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert name in declared, name
    for text in ("alpha T^2 KL(q_n || pT_n)", "alpha T (pT_n - q_n)", "never the log of a probability", "may be NULL and is not range-checked",
                 "bit 1 a teacher logit that is not finite"):
        assert text in header, text


def test_capi_mirrors_the_header(pkg):
    assert pkg.capi.ABI_VERSION == 4
    assert [len(pkg.capi.SYMBOLS[n][1]) for n in NAMES] == [24, 14, 26, 14]
    # the distilled fit is the labelled one plus teacher_logits, alpha and temperature
    assert len(pkg.capi.SYMBOLS["ee_head_fit_distill"][1]) == len(pkg.capi.SYMBOLS["ee_head_fit"][1]) + 3
    assert len(pkg.capi.SYMBOLS["ee_mlp_head_fit_distill"][1]) == len(pkg.capi.SYMBOLS["ee_mlp_head_fit"][1]) + 3
    for name in ("collect_distill_features", "fit_distilled_exit_heads", "fit_distilled_mlp_exit_heads"):
        assert getattr(pkg, name) is getattr(pkg.heads, name)
    # the new fields describe the existing fits by default
    for cls, n in ((pkg.HeadFit, 9), (pkg.MlpHeadFit, 10)):
        fit = cls(*([None] * n))
        assert fit.alpha == 0.0 and fit.temperature == 1.0


def test_header_compiles_as_c_and_is_at_abi_4():
    compiles_as_c('    int (*a)(const float*, const float*, const int64_t*, int32_t, int32_t, int32_t, int32_t, double, double, double, double,'
                  ' int32_t, int32_t, void*, size_t, float*, float*, double*, double*, double*, double*, int32_t*, int32_t*, void*) ='
                  ' ee_head_fit_distill;\n'
                  '    int (*b)(const float*, const float*, const int64_t*, const double*, int32_t, int32_t, int32_t, int32_t, double, double,'
                  ' double, double*, double*, void*) = ee_debug_head_distill_lossgrad;\n'
                  '    int (*c)(const float*, const float*, const int64_t*, const double*, int32_t, int32_t, int32_t, int32_t, double, double,'
                  ' double, double, int32_t, int32_t, void*, size_t, float*, float*, float*, float*, double*, double*, double*, int32_t*,'
                  ' int32_t*, void*) = ee_mlp_head_fit_distill;\n'
                  '    int (*d)(const float*, const float*, const int64_t*, const double*, int32_t, int32_t, int32_t, int32_t, double, double,'
                  ' double, double*, double*, void*) = ee_debug_mlp_head_distill_lossgrad;\n'
                  '    (void)a; (void)b; (void)c; (void)d;\n'
                  '    return MMEE_ABI_VERSION != 4;\n')


def test_library_exports_the_four_symbols(pkg):
    """Read the built library's dynamic symbol table (no GPU, no loading)."""
    exported = exported_symbols(pkg.capi.lib_path())
    for name in NAMES:
        assert name in exported, name


def test_entry_points_refuse_bad_arguments_before_any_device_call(pkg):
    """Every refusal returns non-zero with a message that names the entry point and the reason.  The pointers are never dereferenced: plain
    integers stand in for device addresses."""
    lib = pkg.capi.load()
    p = C.c_void_p(4096)
    E, N, H, K, M = 3, 100, 64, 10, 8
    nan, inf = float("nan"), float("inf")
    objective = {
        "null teacher": (dict(t=None), "NULL"),
        "null labels at alpha 0.5": (dict(y=None, alpha=0.5), "NULL labels at alpha = 0.5"),
        "null labels at alpha 0": (dict(y=None, alpha=0.0), "NULL labels at alpha = 0"),
        "alpha < 0": (dict(alpha=-0.1), "alpha = -0.1"),
        "alpha > 1": (dict(alpha=1.5), "alpha = 1.5"),
        "alpha = nan": (dict(alpha=nan), "alpha = "),
        "T = 0": (dict(T=0.0), "temperature = 0"),
        "T < 0": (dict(T=-2.0), "temperature = -2"),
        "T = inf": (dict(T=inf), "temperature = inf"),
        "T = nan": (dict(T=nan), "temperature = "),
        "l2 = 0": (dict(l2=0.0), "l2 = 0"),
        "l2 < 0": (dict(l2=-1e-3), "l2 = -0.001"),
        "l2 = nan": (dict(l2=nan), "l2 = "),
        "null features": (dict(X=None), "NULL"),
        "K = 1": (dict(K=1), "K = 1"),
        "K = 65": (dict(K=65), "K = 65"),
        "E = 0": (dict(E=0), "E = 0"),
        "N = 0": (dict(N=0), "N = 0"),
        "H = 1028": (dict(H=1028), "H = 1028"),
        "H = 66": (dict(H=66), "H = 66"),
        "unaligned features": (dict(X=C.c_void_p(4100)), "aligned"),
    }
    need = lib.ee_head_fit_workspace_bytes(E, N, H, K, M)
    mlp_need = lib.ee_mlp_head_fit_workspace_bytes(E, N, H, K, M)

    def budget(need):
        return {
            "null workspace": (dict(ws=None), "NULL"),
            "null weight": (dict(w=None), "NULL"),
            "null bias": (dict(b=None), "NULL"),
            "gtol < 0": (dict(gtol=-1.0), "gtol = -1"),
            "max_evals = 0": (dict(evals=0), "max_evals = 0"),
            "history = 0": (dict(hist=0), "history = 0"),
            "history = 33": (dict(hist=33), "history = 33"),
            "small workspace": (dict(ws_bytes=need - 1), f"needs {need} bytes"),
        }

    def fit(X=p, t=p, y=None, E=E, N=N, H=H, K=K, alpha=1.0, T=1.0, l2=1e-2, gtol=1e-9, evals=50, hist=M, ws=p, ws_bytes=need, w=p, b=p):
        return lib.ee_head_fit_distill(X, t, y, E, N, H, K, alpha, T, l2, gtol, evals, hist, ws, ws_bytes, w, b, None, None, None, None, None,
                                       None, None)

    _refused(pkg, "ee_head_fit_distill", fit, {**objective, **budget(need)})

    def mlp_fit(X=p, t=p, y=None, th0=p, E=E, N=N, H=H, K=K, alpha=1.0, T=1.0, l2=1e-2, gtol=1e-6, evals=50, hist=M, ws=p, ws_bytes=mlp_need,
                w=p, b=p, dw=p, db=p):
        return lib.ee_mlp_head_fit_distill(X, t, y, th0, E, N, H, K, alpha, T, l2, gtol, evals, hist, ws, ws_bytes, dw, db, w, b, None, None,
                                           None, None, None, None)

    _refused(pkg, "ee_mlp_head_fit_distill", mlp_fit, {**objective, **budget(mlp_need), "null theta0": (dict(th0=None), "theta0"),
                                                     "null dense_weight": (dict(dw=None), "NULL")})

    for name in ("ee_debug_head_distill_lossgrad", "ee_debug_mlp_head_distill_lossgrad"):
        def lossgrad(X=p, t=p, y=None, th=p, E=E, N=N, H=H, K=K, alpha=1.0, T=1.0, l2=1e-2, loss=p, grad=p):
            return getattr(lib, name)(X, t, y, th, E, N, H, K, alpha, T, l2, loss, grad, None)

        _refused(pkg, name, lossgrad, {**objective, "null theta": (dict(th=None), "NULL"), "null loss": (dict(loss=None), "NULL"),
                                       "null grad": (dict(grad=None), "NULL")})


def _problem(N, H, K, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, H)).astype(np.float32)
    t = (3.0 * rng.standard_normal((N, K))).astype(np.float32)
    y = rng.integers(0, K, N)
    return rng, X, t, y


def _central(fun, theta, h=1e-5):
    num = np.empty_like(theta)
    for i in range(theta.size):
        d = np.zeros_like(theta)
        d[i] = h
        num[i] = (fun(theta + d)[0] - fun(theta - d)[0]) / (2 * h)
    return num


@pytest.mark.parametrize("alpha,T", PAIRS)
@pytest.mark.parametrize("N,H,K", [(7, 8, 3), (25, 16, 10)])
def test_restatement_gradient_agrees_with_central_differences(N, H, K, alpha, T):
    """Central differences with h = 1e-5 on an objective whose third derivatives are of order 1 (the soft term's are of order 1 / T):
    truncation h^2 ~ 1e-10, rounding eps |L| / h ~ 1e-11; the bar is 1e-8, as for tests/headfit_ref.py."""
    rng, X, t, y = _problem(N, H, K, N)
    theta = 0.3 * rng.standard_normal(K * H + K)
    yy = None if alpha == 1.0 else y
    fun = lambda th: DR.loss_grad(th, X, t, yy, K, alpha, T, 1e-2)
    g = fun(theta)[1]
    assert np.abs(_central(fun, theta) - g).max() <= 1e-8


@pytest.mark.parametrize("alpha,T", PAIRS)
def test_two_layer_restatement_gradient_agrees_with_central_differences(alpha, T):
    N, H, K = 9, 4, 3
    rng, X, t, y = _problem(N, H, K, 5)
    theta = 0.5 * rng.standard_normal(MR.param_count(H, K))
    yy = None if alpha == 1.0 else y
    fun = lambda th: DR.mlp_loss_grad(th, X, t, yy, K, alpha, T, 1e-2)
    g = fun(theta)[1]
    assert np.abs(_central(fun, theta) - g).max() <= 1e-8


def test_restatement_at_alpha_0_is_the_labelled_objective():
    N, H, K = 40, 12, 5
    rng, X, t, y = _problem(N, H, K, 3)
    theta = 0.3 * rng.standard_normal(K * H + K)
    l0, g0 = HR.loss_grad(theta, X, y, K, 1e-2)
    l1, g1 = DR.loss_grad(theta, X, t, y, K, 0.0, 1.0, 1e-2)
    assert abs(l1 - l0) <= 1e-15 and np.abs(g1 - g0).max() <= 1e-15
    th2 = 0.5 * rng.standard_normal(MR.param_count(H, K))
    l0, g0 = MR.loss_grad(th2, X, y, K, 1e-2)
    l1, g1 = DR.mlp_loss_grad(th2, X, t, y, K, 0.0, 1.0, 1e-2)
    assert abs(l1 - l0) <= 1e-15 and np.abs(g1 - g0).max() <= 1e-15


def test_restatement_soft_term_is_a_kl():
    """Zero when the head reproduces the teacher (W = 0, b = t for constant teacher rows), positive otherwise, and a q that underflows to
    exact zeros contributes nothing and no NaN."""
    N, H, K = 6, 4, 5
    rng, X, _, _ = _problem(N, H, K, 1)
    row = (3.0 * rng.standard_normal(K)).astype(np.float32)
    t = np.tile(row, (N, 1))
    theta = np.concatenate([np.zeros(K * H), row.astype(np.float64)])
    for T in (1.0, 2.0, 0.5):
        rows, D = DR.row_terms(HR.logits(theta, X, K), t, None, 1.0, T)
        assert np.abs(rows).max() <= 1e-14 and np.abs(D).max() <= 1e-14
        rows, _ = DR.row_terms(HR.logits(0.5 * theta, X, K), t, None, 1.0, T)
        assert (rows > 0).all()
    t = np.tile(np.where(np.arange(K) == 2, 3000.0, -3000.0).astype(np.float32), (N, 1))
    rows, D = DR.row_terms(rng.standard_normal((N, K)), t, None, 1.0, 1.0)
    assert np.isfinite(rows).all() and np.isfinite(D).all() and (rows > 0).all()


def test_python_surface_refuses_before_it_looks_for_a_device(pkg):
    X = np.zeros((2, 10, 8), dtype=np.float32)
    t = np.zeros((10, 4), dtype=np.float32)
    y = np.zeros(10, dtype=np.int64)
    for fit in (pkg.fit_distilled_exit_heads, pkg.fit_distilled_mlp_exit_heads):
        with pytest.raises(ValueError, match="labels are required at alpha = 0.5"):
            fit(X, t, alpha=0.5)
        with pytest.raises(ValueError, match="labels are required at alpha = 0"):
            fit(X, t, alpha=0.0)
        with pytest.raises(ValueError, match=r"teacher_logits are \(9, 4\)"):
            fit(X, t[:9])
        with pytest.raises(ValueError, match=r"teacher_logits are \(2, 10, 4\)"):
            fit(X, np.zeros((2, 10, 4), dtype=np.float32))
        with pytest.raises(ValueError, match="num_labels = 5, but teacher_logits have K = 4"):
            fit(X, t, num_labels=5)
        with pytest.raises(ValueError, match="alpha = 1.5"):
            fit(X, t, y, alpha=1.5)
        with pytest.raises(ValueError, match="temperature = 0"):
            fit(X, t, temperature=0.0)
    two = pkg.ModelConfig.tiny(EE_config=dict(exits=[1, 2], encoder_layer_strategy="ramp", exit_head_num_layers=2))
    gate = pkg.ModelConfig.tiny(EE_config=dict(exits=[1, 2], encoder_layer_strategy="gate", exit_head_num_layers=1))

    class _Engine:
        cfg = two
    with pytest.raises(ValueError, match="exit_head_num_layers == 1"):
        pkg.collect_distill_features(_Engine(), [])
    _Engine.cfg = gate
    with pytest.raises(ValueError, match="gate"):
        pkg.collect_distill_features(_Engine(), [])
