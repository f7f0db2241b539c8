"""CPU checks of the weighted exit-head fits (include/mmee.h ee_head_fit_weighted, ee_mlp_head_fit_weighted): the C-ABI (declarations, plain-C
compile, ABI 4, exported symbols), the entry points' refusals before they look for a device, what the Python surface refuses, and the
identities of the float64 restatement of tests/weighted_headfit_ref.py: integer weights are row repetition, a common factor changes nothing,
all-ones weights are the unweighted restatements."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import distill_headfit_ref as DR
from . import headfit_ref as HR
from . import mlp_headfit_ref as MR
from . import weighted_headfit_ref as WR
from .conftest import ROOT
from .fit_util import _refused, compiles_as_c, exported_symbols

NAMES = ("ee_head_fit_weighted", "ee_head_fit_weighted_workspace_bytes", "ee_debug_head_weighted_lossgrad", "ee_mlp_head_fit_weighted",
         "ee_mlp_head_fit_weighted_workspace_bytes", "ee_debug_mlp_head_weighted_lossgrad")
OBJECTIVES = [(None, 0.0, 1.0), ("t", 1.0, 2.0), ("t", 0.5, 2.0)]


def test_header_declares_the_six_functions():
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    assert re.search(r"#define\s+MMEE_ABI_VERSION\s+4\b", header)           # six more functions: ee_config is unchanged
    declared = set(re.findall(r"\b(ee_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert name in declared, name
    for text in ("(1 / W_e) sum_n w[e][n] l_n(theta)", "teacher_logits == NULL selects the labelled objective", "0 * NaN is not defended against",
                 "bit 2 a weight that is negative or not finite", "bit 3 an exit whose"):
        assert text in header, text


def test_capi_mirrors_the_header(pkg):
    assert pkg.capi.ABI_VERSION == 4
    assert [len(pkg.capi.SYMBOLS[n][1]) for n in NAMES] == [25, 5, 15, 27, 5, 15]
    # the weighted fit is the distilled one plus the weights
    assert len(pkg.capi.SYMBOLS["ee_head_fit_weighted"][1]) == len(pkg.capi.SYMBOLS["ee_head_fit_distill"][1]) + 1
    assert len(pkg.capi.SYMBOLS["ee_mlp_head_fit_weighted"][1]) == len(pkg.capi.SYMBOLS["ee_mlp_head_fit_distill"][1]) + 1
    for name in ("reach_weights", "balanced_class_weights"):
        assert getattr(pkg, name) is getattr(pkg.heads, name)
    # the fits' results keep their fields
    assert [f for f in pkg.HeadFit.__dataclass_fields__] == ["weight", "bias", "weight64", "bias64", "loss", "grad_norm", "evals", "status", "l2",
                                                              "alpha", "temperature"]
    assert [f for f in pkg.MlpHeadFit.__dataclass_fields__] == ["dense_weight", "dense_bias", "weight", "bias", "theta64", "loss", "grad_norm",
                                                                 "evals", "status", "l2", "alpha", "temperature"]


def test_header_compiles_as_c_and_is_at_abi_4():
    compiles_as_c('    int (*a)(const float*, const int64_t*, const float*, const float*, int32_t, int32_t, int32_t, int32_t, double, double, double,'
                  ' double, int32_t, int32_t, void*, size_t, float*, float*, double*, double*, double*, double*, int32_t*, int32_t*, void*) ='
                  ' ee_head_fit_weighted;\n'
                  '    int (*b)(const float*, const int64_t*, const float*, const float*, const double*, int32_t, int32_t, int32_t, int32_t, double,'
                  ' double, double, double*, double*, void*) = ee_debug_head_weighted_lossgrad;\n'
                  '    int (*c)(const float*, const int64_t*, const float*, const float*, const double*, int32_t, int32_t, int32_t, int32_t, double,'
                  ' double, double, double, int32_t, int32_t, void*, size_t, float*, float*, float*, float*, double*, double*, double*, int32_t*,'
                  ' int32_t*, void*) = ee_mlp_head_fit_weighted;\n'
                  '    int (*d)(const float*, const int64_t*, const float*, const float*, const double*, int32_t, int32_t, int32_t, int32_t, double,'
                  ' double, double, double*, double*, void*) = ee_debug_mlp_head_weighted_lossgrad;\n'
                  '    size_t (*e)(int32_t, int32_t, int32_t, int32_t, int32_t) = ee_head_fit_weighted_workspace_bytes;\n'
                  '    size_t (*g)(int32_t, int32_t, int32_t, int32_t, int32_t) = ee_mlp_head_fit_weighted_workspace_bytes;\n'
                  '    (void)a; (void)b; (void)c; (void)d; (void)e; (void)g;\n'
                  '    return MMEE_ABI_VERSION != 4;\n')


def test_library_exports_the_six_symbols(pkg):
    """Read the built library's dynamic symbol table (no GPU, no loading)."""
    exported = exported_symbols(pkg.capi.lib_path())
    for name in NAMES:
        assert name in exported, name


def test_workspace_is_the_unweighted_one_plus_the_scale_table(pkg):
    lib = pkg.capi.load()
    for E, N, H, K, M in ((3, 100, 64, 10, 8), (1, 1, 4, 2, 1), (6, 40000, 768, 16, 8)):
        assert lib.ee_head_fit_weighted_workspace_bytes(E, N, H, K, M) == lib.ee_head_fit_workspace_bytes(E, N, H, K, M) + 8 * E * N
        assert lib.ee_mlp_head_fit_weighted_workspace_bytes(E, N, H, K, M) == lib.ee_mlp_head_fit_workspace_bytes(E, N, H, K, M) + 8 * E * N
    assert lib.ee_head_fit_weighted_workspace_bytes(0, 1, 4, 2, 1) == 0 and lib.ee_mlp_head_fit_weighted_workspace_bytes(1, 1, 4, 2, 0) == 0


def test_entry_points_refuse_bad_arguments_before_any_device_call(pkg):
    """Every refusal returns non-zero with a message that names the entry point and the reason.  The pointers are never dereferenced: plain
    integers stand in for device addresses."""
    lib = pkg.capi.load()
    p = C.c_void_p(4096)
    E, N, H, K, M = 3, 100, 64, 10, 8
    nan, inf = float("nan"), float("inf")
    objective = {
        "null weights": (dict(w8=None), "weights are required"),
        "null weights, labelled": (dict(w8=None, t=None, y=p, alpha=0.0), "weights are required"),
        "null teacher at alpha 1": (dict(t=None, y=p, alpha=1.0), "alpha = 1 without teacher_logits"),
        "null teacher at alpha 0.5": (dict(t=None, y=p, alpha=0.5), "alpha = 0.5 without teacher_logits"),
        "null teacher at alpha nan": (dict(t=None, y=p, alpha=nan), "without teacher_logits"),
        "null teacher, null labels": (dict(t=None, y=None, alpha=0.0), "NULL"),
        "null labels at alpha 0.5": (dict(y=None, alpha=0.5), "NULL labels at alpha = 0.5"),
        "alpha < 0": (dict(alpha=-0.1), "alpha = -0.1"),
        "alpha > 1": (dict(alpha=1.5), "alpha = 1.5"),
        "T = 0": (dict(T=0.0), "temperature = 0"),
        "T = inf": (dict(T=inf), "temperature = inf"),
        "l2 = 0": (dict(l2=0.0), "l2 = 0"),
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
    need = lib.ee_head_fit_weighted_workspace_bytes(E, N, H, K, M)
    mlp_need = lib.ee_mlp_head_fit_weighted_workspace_bytes(E, N, H, K, M)

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
            "the unweighted workspace": (dict(ws_bytes=need - 8 * E * N), f"needs {need} bytes"),
        }

    def fit(X=p, y=None, t=p, w8=p, E=E, N=N, H=H, K=K, alpha=1.0, T=1.0, l2=1e-2, gtol=1e-9, evals=50, hist=M, ws=p, ws_bytes=need, w=p, b=p):
        return lib.ee_head_fit_weighted(X, y, t, w8, E, N, H, K, alpha, T, l2, gtol, evals, hist, ws, ws_bytes, w, b, None, None, None, None,
                                        None, None, None)

    _refused(pkg, "ee_head_fit_weighted", fit, {**objective, **budget(need)})

    def mlp_fit(X=p, y=None, t=p, w8=p, th0=p, E=E, N=N, H=H, K=K, alpha=1.0, T=1.0, l2=1e-2, gtol=1e-6, evals=50, hist=M, ws=p,
                ws_bytes=mlp_need, w=p, b=p, dw=p, db=p):
        return lib.ee_mlp_head_fit_weighted(X, y, t, w8, th0, E, N, H, K, alpha, T, l2, gtol, evals, hist, ws, ws_bytes, dw, db, w, b, None,
                                            None, None, None, None, None)

    _refused(pkg, "ee_mlp_head_fit_weighted", mlp_fit, {**objective, **budget(mlp_need), "null theta0": (dict(th0=None), "theta0"),
                                                      "null dense_weight": (dict(dw=None), "NULL")})

    for name in ("ee_debug_head_weighted_lossgrad", "ee_debug_mlp_head_weighted_lossgrad"):
        def lossgrad(X=p, y=None, t=p, w8=p, th=p, E=E, N=N, H=H, K=K, alpha=1.0, T=1.0, l2=1e-2, loss=p, grad=p):
            return getattr(lib, name)(X, y, t, w8, th, E, N, H, K, alpha, T, l2, loss, grad, None)

        _refused(pkg, name, lossgrad, {**objective, "null theta": (dict(th=None), "NULL"), "null loss": (dict(loss=None), "NULL"),
                                       "null grad": (dict(grad=None), "NULL")})


def test_python_surface_refuses_a_sample_weight_of_the_wrong_shape_before_the_library(pkg, monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(pkg.capi, "load", touched)
    X = np.zeros((2, 10, 8), dtype=np.float32)
    t = np.zeros((10, 4), dtype=np.float32)
    y = np.zeros(10, dtype=np.int64)
    fits = ((pkg.fit_exit_heads, (X, y)), (pkg.fit_mlp_exit_heads, (X, y)), (pkg.fit_distilled_exit_heads, (X, t)),
            (pkg.fit_distilled_mlp_exit_heads, (X, t)))
    for fit, args in fits:
        for bad in (np.ones(9), np.ones((2, 9)), np.ones((3, 10)), np.ones((1, 10)), np.ones((10, 2)), np.ones((2, 10, 1)), np.float32(1.0)):
            with pytest.raises(ValueError, match="sample_weight is"):
                fit(*args, sample_weight=bad)
        with pytest.raises(ValueError, match="sample_weight is"):           # (N,H) features are one exit: (1,N) or (N,)
            fit(X[0], args[1], sample_weight=np.ones((2, 10)))
    # a good shape gets as far as the library
    for fit, args in fits:
        for good in (np.ones(10), np.ones((2, 10), dtype=np.int32)):
            with pytest.raises(AssertionError, match="the library was touched"):
                fit(*args, sample_weight=good)
    # the pinned refusals of the distilled fits come first, as they did
    with pytest.raises(ValueError, match="labels are required at alpha = 0.5"):
        pkg.fit_distilled_exit_heads(X, t, alpha=0.5, sample_weight=np.ones(9))


# ---- the restatement's own identities --------------------------------------------------------------------------------------------------------
def _problem(N, H, K, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, H)).astype(np.float32)
    t = (3.0 * rng.standard_normal((N, K))).astype(np.float32)
    y = rng.integers(0, K, N)
    return rng, X, t, y


def _pick(kind, t):
    return None if kind is None else t


@pytest.mark.parametrize("kind,alpha,T", OBJECTIVES)
def test_integer_weights_are_row_repetition(kind, alpha, T):
    """Sums of w_n equal terms against w_n products: the two differ by the rounding of sums of <= 120 terms of order 1, far below 1e-13."""
    N, H, K = 40, 12, 5
    rng, X, t, y = _problem(N, H, K, 3)
    w = rng.integers(0, 4, N).astype(np.float32)
    rep = np.repeat(np.arange(N), w.astype(np.int64))
    yy = None if alpha == 1.0 else y
    th = 0.3 * rng.standard_normal(K * H + K)
    l1, g1 = WR.loss_grad(th, X, yy, K, 1e-2, w, _pick(kind, t), alpha, T)
    l0, g0 = WR.loss_grad(th, X[rep], None if yy is None else yy[rep], K, 1e-2, np.ones(len(rep)), _pick(kind, t[rep]), alpha, T)
    assert abs(l1 - l0) <= 1e-13 and np.abs(g1 - g0).max() <= 1e-13
    th2 = 0.5 * rng.standard_normal(MR.param_count(H, K))
    l1, g1 = WR.mlp_loss_grad(th2, X, yy, K, 1e-2, w, _pick(kind, t), alpha, T)
    l0, g0 = WR.mlp_loss_grad(th2, X[rep], None if yy is None else yy[rep], K, 1e-2, np.ones(len(rep)), _pick(kind, t[rep]), alpha, T)
    assert abs(l1 - l0) <= 1e-13 and np.abs(g1 - g0).max() <= 1e-13


@pytest.mark.parametrize("kind,alpha,T", OBJECTIVES)
def test_a_common_factor_of_four_changes_nothing(kind, alpha, T):
    """4 w and 4 W are exact in float64, so the quotient is the same number: equal bits."""
    N, H, K = 33, 8, 4
    rng, X, t, y = _problem(N, H, K, 5)
    w = rng.uniform(0.25, 4.0, N).astype(np.float32)
    yy = None if alpha == 1.0 else y
    th = 0.3 * rng.standard_normal(K * H + K)
    a = WR.loss_grad(th, X, yy, K, 1e-2, w, _pick(kind, t), alpha, T)
    b = WR.loss_grad(th, X, yy, K, 1e-2, 4.0 * w, _pick(kind, t), alpha, T)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    th2 = 0.5 * rng.standard_normal(MR.param_count(H, K))
    a = WR.mlp_loss_grad(th2, X, yy, K, 1e-2, w, _pick(kind, t), alpha, T)
    b = WR.mlp_loss_grad(th2, X, yy, K, 1e-2, 4.0 * w, _pick(kind, t), alpha, T)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


def test_all_ones_weights_are_the_unweighted_restatements():
    """The same terms, summed by mean() there and by sum() / N here: 1e-14 allows for the two orders."""
    N, H, K = 40, 12, 5
    rng, X, t, y = _problem(N, H, K, 7)
    ones = np.ones(N, dtype=np.float32)
    th = 0.3 * rng.standard_normal(K * H + K)
    th2 = 0.5 * rng.standard_normal(MR.param_count(H, K))
    for got, want in ((WR.loss_grad(th, X, y, K, 1e-2, ones), HR.loss_grad(th, X, y, K, 1e-2)),
                      (WR.mlp_loss_grad(th2, X, y, K, 1e-2, ones), MR.loss_grad(th2, X, y, K, 1e-2)),
                      (WR.loss_grad(th, X, y, K, 1e-2, ones, t, 0.5, 2.0), DR.loss_grad(th, X, t, y, K, 0.5, 2.0, 1e-2)),
                      (WR.mlp_loss_grad(th2, X, None, K, 1e-2, ones, t, 1.0, 2.0), DR.mlp_loss_grad(th2, X, t, None, K, 1.0, 2.0, 1e-2))):
        assert abs(got[0] - want[0]) <= 1e-14 and np.abs(got[1] - want[1]).max() <= 1e-14


def test_rows_of_weight_zero_are_not_looked_at():
    N, H, K = 20, 8, 4
    rng, X, t, y = _problem(N, H, K, 9)
    w = rng.uniform(0.25, 4.0, N).astype(np.float32)
    w[[0, 7, N - 1]] = 0.0
    yb, tb = y.copy(), t.copy()
    yb[[0, 7, N - 1]] = -1
    tb[[0, 7, N - 1]] = np.nan
    th = 0.3 * rng.standard_normal(K * H + K)
    a = WR.loss_grad(th, X, y, K, 1e-2, w, t, 0.5, 2.0)
    b = WR.loss_grad(th, X, yb, K, 1e-2, w, tb, 0.5, 2.0)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.isfinite(a[1]).all()


def test_the_weight_families_are_what_they_say():
    rng = np.random.default_rng(0)
    S = 32
    for N in (1, S - 1, S, S + 1, 2 * S + 3):
        w = WR.family_integers(rng, 2, N, S)
        assert w.shape == (2, N) and w.dtype == np.float32 and set(np.unique(w)) <= {0.0, 1.0, 2.0, 3.0} and w.sum(axis=1).min() > 0
        if N > 1:
            assert w[0, 0] == 0 and w[0, N - 1] == 0
        if N > S:
            assert w[0, S - 1] == 0
        for fam in (WR.family_uniform(rng, 2, N), WR.family_one_row(rng, 2, N), WR.family_per_exit(rng, 2, N)):
            assert fam.shape == (2, N) and fam.dtype == np.float32 and (fam >= 0).all() and fam.sum(axis=1).min() > 0
    w = WR.family_zero_slab(rng, 1, 2 * S + 3, S)
    assert (w[0, S:2 * S] == 0).all() and (w[0, :S] > 0).all() and (w[0, 2 * S:] > 0).all()
    w = WR.family_per_exit(rng, 3, 40)
    assert not np.array_equal(w[0] == 0, w[1] == 0)
