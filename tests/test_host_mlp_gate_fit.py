"""CPU checks of the two-layer gate fit (include/mmee.h ee_mlp_head_fit_gate, ee_mlp_head_fit_gate_weighted): tests/mlp_gate_ref.py's gradient
against central differences, the C-ABI (declarations, plain-C compile, ABI 4, exported symbols, the binding's types), the entry points'
refusals before they look for a device, what the Python surface refuses without one, and the names ``MlpGateFit.state_dict`` produces."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import gate_ref as G
from . import mlp_gate_ref as R
from . import mlp_headfit_ref as MR
from .conftest import ROOT
from .fit_util import _HostTensor, _refused, compiles_as_c, exported_symbols

NAMES = ("ee_mlp_head_fit_gate", "ee_mlp_head_fit_gate_weighted", "ee_debug_mlp_head_gate_lossgrad", "ee_debug_mlp_head_gate_weighted_lossgrad")
TWO_LAYER_GATE = dict(exits=[1, 2, 4], encoder_layer_strategy="gate", inference_strategy="gate", exit_head_num_layers=2)
BLOCKS = ("dense.weight", "dense.bias", "out_proj.weight", "out_proj.bias")


# ---- the restatement itself ----------------------------------------------------------------------------------------------------------------------
def _central(f, theta, h=1e-5):
    g = np.empty_like(theta)
    for i in range(theta.size):
        d = np.zeros_like(theta)
        d[i] = h
        g[i] = (f(theta + d) - f(theta - d)) / (2.0 * h)
    return g


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_gradient_matches_central_differences(weighted):
    """h = 1e-5, bar 1e-8: the project's bar for the two-layer ramp restatement (truncation h^2 f''' / 6 ~ 1e-11, rounding eps L / h ~ 1e-11)."""
    N, H = 9, 8
    rng = np.random.default_rng(0)
    X = rng.standard_normal((N, H)).astype(np.float32)
    c = rng.random(N)
    c[:3] = (0.0, 1.0, 1.0)
    w = None
    if weighted:
        w = rng.uniform(0.25, 4.0, N).astype(np.float32)
        w[4] = 0.0
        c[4] = np.nan                                                 # a row of weight zero: its target is not looked at
    theta = 0.5 * rng.standard_normal(R.param_count(H))
    loss, g = R.loss_grad(theta, X, c, 1e-2, w)
    assert np.isfinite(loss) and np.isfinite(g).all()
    num = _central(lambda th: R.loss_grad(th, X, c, 1e-2, w)[0], theta)
    err = float(np.abs(g - num).max())
    print(f"max |grad - central difference| = {err:.3e}")
    assert err <= 1e-8, err


def test_restatement_identities():
    """W2 = 0: both logits are b2, whatever W1; at theta = identity start the loss is log 2 + the penalty of I.  With a one-layer head
    written into the two-layer form on rows small enough for tanh(x) = x to double precision's square root, the one-layer gate restatement.
    Integer weights are row repetition, a common factor of four changes no bit, all-ones weights are the unweighted objective."""
    N, H = 12, 8
    rng = np.random.default_rng(1)
    X = rng.standard_normal((N, H)).astype(np.float32)
    c = rng.random(N)
    l0 = R.loss_grad(R.init_identity(H), X, c, 1e-2)[0]
    assert abs(l0 - (np.log(2.0) + 0.5e-2 * H)) <= 1e-14
    Xs = (1e-6 * X).astype(np.float32)
    th1 = rng.standard_normal(2 * H + 2)
    th2 = MR.join(np.eye(H), np.zeros(H), th1[:2 * H].reshape(2, H), th1[2 * H:])
    want = G.gate_lossgrad(th1, Xs, c, 1e-2)[0] + 0.5e-2 * H
    assert abs(R.loss_grad(th2, Xs, c, 1e-2)[0] - want) <= 1e-14
    theta = 0.5 * rng.standard_normal(R.param_count(H))
    w = rng.integers(0, 4, N).astype(np.float32)
    rep = np.repeat(np.arange(N), w.astype(np.int64))
    a, b = R.loss_grad(theta, X, c, 1e-2, w), R.loss_grad(theta, X[rep], c[rep], 1e-2)
    assert abs(a[0] - b[0]) <= 1e-13 and np.abs(a[1] - b[1]).max() <= 1e-13
    wu = rng.uniform(0.25, 4.0, N).astype(np.float32)
    a, b = R.loss_grad(theta, X, c, 1e-2, wu), R.loss_grad(theta, X, c, 1e-2, 4.0 * wu)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    a, b = R.loss_grad(theta, X, c, 1e-2, np.ones(N, np.float32)), R.loss_grad(theta, X, c, 1e-2)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


def test_problems_follow_the_one_layer_gate_tests_recipe():
    X, T = R.problem(3, 257, 64)
    assert X.dtype == np.float32 and X.shape == (3, 257, 64) and T.shape == (3, 257) and R.kinds(3, 257) == ["hard", "soft", "ones"]
    assert set(np.unique(T[0])) == {0.0, 1.0} and ((T[1] > 0) & (T[1] < 1)).all() and (T[2] == 1.0).all()
    assert abs(float(X.std()) - 1.0) < 0.02
    assert R.kinds(1, 63) == ["hard"] and R.kinds(1, 200) == ["soft"] and R.kinds(2, 300) == ["hard", "soft"]


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_four_functions_and_states_the_objective():
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    assert re.search(r"#define\s+MMEE_ABI_VERSION\s+4\b", header)           # four more functions: no struct changed
    declared = set(re.findall(r"\b(ee_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert name in declared, name
    for text in ("z_n = W2 tanh(W1 x_n + b1) + b2", "(1 / (2N)) sum_n [ bce(z_1, c) + bce(z_0, 1 - c) ] + (l2 / 2) ||theta||^2",
                 "(1 / (2 W_e)) sum_n w[e][n]", "NOT convex", "ee_mlp_head_fit_weighted_workspace_bytes(E, N, H, 2, history)"):
        assert text in header, text


def test_capi_mirrors_the_header_and_the_package_exports_the_fit(pkg):
    assert pkg.capi.ABI_VERSION == 4
    S = pkg.capi.SYMBOLS
    assert [len(S[n][1]) for n in NAMES] == [22, 23, 10, 11]
    # ee_mlp_head_fit's arguments without K; the weighted forms add the weights
    assert len(S["ee_mlp_head_fit_gate"][1]) == len(S["ee_mlp_head_fit"][1]) - 1
    assert len(S["ee_debug_mlp_head_gate_lossgrad"][1]) == len(S["ee_debug_mlp_head_lossgrad"][1]) - 1
    for n in NAMES:
        assert S[n][0] is C.c_int
    vp, i32, f64 = C.c_void_p, C.c_int32, C.c_double
    assert S["ee_mlp_head_fit_gate_weighted"][1][:13] == [vp, vp, vp, vp, i32, i32, i32, f64, f64, i32, i32, vp, C.c_size_t]
    assert S["ee_debug_mlp_head_gate_weighted_lossgrad"][1] == [vp, vp, vp, vp, i32, i32, i32, f64, vp, vp, vp]
    assert pkg.fit_mlp_gate_heads is pkg.heads.fit_mlp_gate_heads and pkg.MlpGateFit is pkg.heads.MlpGateFit
    mlp = [f for f in pkg.MlpHeadFit.__dataclass_fields__ if f not in ("alpha", "temperature")]
    assert [f for f in pkg.MlpGateFit.__dataclass_fields__] == mlp


def test_header_compiles_as_c():
    compiles_as_c('    int (*a)(const float*, const double*, const double*, int32_t, int32_t, int32_t, double, double, int32_t, int32_t, void*, size_t,'
                  ' float*, float*, float*, float*, double*, double*, double*, int32_t*, int32_t*, void*) = ee_mlp_head_fit_gate;\n'
                  '    int (*b)(const float*, const double*, const float*, const double*, int32_t, int32_t, int32_t, double, double, int32_t, int32_t,'
                  ' void*, size_t, float*, float*, float*, float*, double*, double*, double*, int32_t*, int32_t*, void*) ='
                  ' ee_mlp_head_fit_gate_weighted;\n'
                  '    int (*c)(const float*, const double*, const double*, int32_t, int32_t, int32_t, double, double*, double*, void*) ='
                  ' ee_debug_mlp_head_gate_lossgrad;\n'
                  '    int (*d)(const float*, const double*, const float*, const double*, int32_t, int32_t, int32_t, double, double*, double*, void*) ='
                  ' ee_debug_mlp_head_gate_weighted_lossgrad;\n'
                  '    (void)a; (void)b; (void)c; (void)d;\n'
                  '    return MMEE_ABI_VERSION != 4;\n')


def test_library_exports_the_four_symbols(pkg):
    exported = exported_symbols(pkg.capi.lib_path())
    for name in NAMES:
        assert name in exported, name


def test_entry_points_refuse_bad_arguments_before_any_device_call(pkg):
    """Every refusal returns non-zero with a message that names the entry point and the reason.  The pointers are never dereferenced: plain
    integers stand in for device addresses."""
    lib = pkg.capi.load()
    p = C.c_void_p(4096)
    E, N, H, M = 3, 100, 64, 8
    nan = float("nan")
    problem = {
        "null targets": (dict(T=None), "targets"),
        "null features": (dict(X=None), "NULL"),
        "l2 = 0": (dict(l2=0.0), "l2 = 0"),
        "l2 = nan": (dict(l2=nan), "l2 = "),
        "E = 0": (dict(E=0), "E = 0"),
        "N = 0": (dict(N=0), "N = 0"),
        "H = 1028": (dict(H=1028), "H = 1028"),
        "H = 66": (dict(H=66), "H = 66"),
        "unaligned features": (dict(X=C.c_void_p(4100)), "aligned"),
    }

    def budget(need):
        return {
            "null theta0": (dict(th0=None), "theta0"),
            "null workspace": (dict(ws=None), "NULL"),
            "null dense_weight": (dict(dw=None), "NULL"),
            "null bias": (dict(b=None), "NULL"),
            "gtol < 0": (dict(gtol=-1.0), "gtol = -1"),
            "max_evals = 0": (dict(evals=0), "max_evals = 0"),
            "history = 0": (dict(hist=0), "history = 0"),
            "history = 33": (dict(hist=33), "history = 33"),
            "small workspace": (dict(ws_bytes=need - 1), f"needs {need} bytes"),
        }

    need = lib.ee_mlp_head_fit_workspace_bytes(E, N, H, 2, M)
    wneed = lib.ee_mlp_head_fit_weighted_workspace_bytes(E, N, H, 2, M)
    assert wneed == need + 8 * E * N

    def fit(X=p, T=p, th0=p, E=E, N=N, H=H, l2=1e-2, gtol=1e-6, evals=50, hist=M, ws=p, ws_bytes=need, dw=p, db=p, w=p, b=p):
        return lib.ee_mlp_head_fit_gate(X, T, th0, E, N, H, l2, gtol, evals, hist, ws, ws_bytes, dw, db, w, b, None, None, None, None, None, None)

    _refused(pkg, "ee_mlp_head_fit_gate", fit, {**problem, **budget(need)})

    def wfit(X=p, T=p, w8=p, th0=p, E=E, N=N, H=H, l2=1e-2, gtol=1e-6, evals=50, hist=M, ws=p, ws_bytes=wneed, dw=p, db=p, w=p, b=p):
        return lib.ee_mlp_head_fit_gate_weighted(X, T, w8, th0, E, N, H, l2, gtol, evals, hist, ws, ws_bytes, dw, db, w, b, None, None, None, None,
                                                 None, None)

    _refused(pkg, "ee_mlp_head_fit_gate_weighted", wfit, {**problem, **budget(wneed), "null weights": (dict(w8=None), "weights are required"),
                                                          "the unweighted workspace": (dict(ws_bytes=need), f"needs {wneed} bytes")})

    def hook(X=p, T=p, th=p, E=E, N=N, H=H, l2=1e-2, loss=p, grad=p):
        return lib.ee_debug_mlp_head_gate_lossgrad(X, T, th, E, N, H, l2, loss, grad, None)

    more = {"null targets": (dict(T=None), "NULL argument"), "null theta": (dict(th=None), "NULL"), "null loss": (dict(loss=None), "NULL"), "null grad": (dict(grad=None), "NULL")}
    _refused(pkg, "ee_debug_mlp_head_gate_lossgrad", hook, {**problem, **more})

    def whook(X=p, T=p, w8=p, th=p, E=E, N=N, H=H, l2=1e-2, loss=p, grad=p):
        return lib.ee_debug_mlp_head_gate_weighted_lossgrad(X, T, w8, th, E, N, H, l2, loss, grad, None)

    _refused(pkg, "ee_debug_mlp_head_gate_weighted_lossgrad", whook, {**problem, **more, "null weights": (dict(w8=None), "weights are required")})


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------------
def test_python_surface_refuses_before_the_library_is_loaded(pkg, monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(pkg.capi, "load", touched)
    fit = pkg.fit_mlp_gate_heads
    X, T = np.zeros((2, 10, 8), np.float32), np.zeros((2, 10))
    with pytest.raises(ValueError, match=r"features are \(10,\)"):
        fit(np.zeros(10, np.float32), np.zeros(10))
    with pytest.raises(ValueError, match=r"H <= 1024"):
        fit(np.zeros((1, 4, 1028), np.float32), np.zeros((1, 4)))
    with pytest.raises(ValueError, match=r"multiple of 4"):
        fit(np.zeros((1, 4, 6), np.float32), np.zeros((1, 4)))
    for bad in (np.zeros((1, 10)), np.zeros((2, 9)), np.zeros(10), np.zeros((2, 10, 1))):
        with pytest.raises(ValueError, match=r"\(E,N\)"):
            fit(X, bad)
    for l2 in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="l2"):
            fit(X, T, l2=l2)
    for bad in (np.ones(9), np.ones((2, 9)), np.ones((3, 10)), np.ones((1, 10)), np.ones((10, 2)), np.float32(1.0)):
        with pytest.raises(ValueError, match="sample_weight is"):
            fit(X, T, sample_weight=bad)
    # good shapes get as far as the library: (N,H) features with (N,) targets are one exit
    for args, kw in (((X, T), {}), ((X[0], T[0]), {}), ((X, T), dict(sample_weight=np.ones(10))), ((X, T), dict(sample_weight=np.ones((2, 10))))):
        with pytest.raises(AssertionError, match="the library was touched"):
            fit(*args, **kw)
    # the one-layer fit's refusals stay, and point here
    with pytest.raises(ValueError, match="sample_weight"):
        pkg.fit_gate_heads(X, T, sample_weight=np.ones(10))
    with pytest.raises(ValueError, match="fit_mlp_gate_heads"):
        pkg.fit_gate_heads(X, T, sample_weight=np.ones(10))


def _host_fit(pkg, E, H, K=2):
    rng = np.random.default_rng(0)
    arrays = [rng.standard_normal(s).astype(np.float32) for s in ((E, H, H), (E, H), (E, K, H), (E, K))]
    return pkg.MlpGateFit(*[_HostTensor(a) for a in arrays], None, None, None, None, None, 1e-2), arrays


def test_state_dict_names_are_the_synthetic_weights_head_names(pkg):
    cfg = pkg.ModelConfig.tiny(EE_config=TWO_LAYER_GATE)
    W = pkg.synth.make_weights(cfg, seed=1)
    fit, arrays = _host_fit(pkg, 3, cfg.hidden_size)
    sd = fit.state_dict(cfg)
    assert set(sd) == {k for k in W if "early_exits" in k} and len(sd) == 12
    for k, v in sd.items():
        assert v.shape == W[k].shape and v.dtype == W[k].dtype == np.float32 and v.flags["C_CONTIGUOUS"], k
    H = cfg.hidden_size
    assert sd["layoutlmv3.encoder.early_exits.0.out_proj.weight"].shape == (2, H) and sd["layoutlmv3.encoder.early_exits.2.out_proj.bias"].shape == (2,)
    for j in range(3):
        for name, a in zip(BLOCKS, arrays):
            assert np.array_equal(sd[f"layoutlmv3.encoder.early_exits.{j}.{name}"], a[j])


def test_state_dict_refuses_what_is_out_of_scope(pkg):
    tiny = pkg.ModelConfig.tiny
    fit, _ = _host_fit(pkg, 2, 128)
    ok = tiny(EE_config=dict(exits=[1, 2], encoder_layer_strategy="gate", exit_head_num_layers=2))
    assert len(fit.state_dict(ok)) == 8
    for ee, match in ((dict(exits=[1, 2], encoder_layer_strategy="ramp", exit_head_num_layers=2), "gate strategy only"),
                      (dict(exits=[1, 2], encoder_layer_strategy="gate", exit_head_num_layers=1), "exit_head_num_layers == 2"),
                      (dict(exits=["text_avg", 1, 2], encoder_layer_strategy="gate", exit_head_num_layers=2), "embedding-level exits"),
                      (TWO_LAYER_GATE, r"the fit is \(E,2,H\)")):
        with pytest.raises(ValueError, match=match):
            fit.state_dict(tiny(EE_config=ee))
    with pytest.raises(ValueError, match="LayoutLMv3 configurations only"):
        fit.state_dict(pkg.ModelConfig.dit_tiny(EE_config=dict(exits=[1, 2], encoder_layer_strategy="ramp", exit_head_num_layers=2)))
    with pytest.raises(ValueError, match=r"the fit is \(E,2,H\)"):
        _host_fit(pkg, 2, 64)[0].state_dict(ok)                                  # H = 64 against the configuration's 128
    with pytest.raises(ValueError, match=r"the fit is \(E,2,H\)"):
        _host_fit(pkg, 2, 128, K=3)[0].state_dict(ok)
    # the one-layer gate's refusal of a two-layer configuration keeps its text and names the fit that takes it
    one = pkg.GateFit(_HostTensor(np.zeros((2, 2, 128), np.float32)), _HostTensor(np.zeros((2, 2), np.float32)), None, None, None, None, None, None, 1e-2)
    with pytest.raises(ValueError, match="exit_head_num_layers == 1"):
        one.state_dict(ok)
    with pytest.raises(ValueError, match="fit_mlp_gate_heads"):
        one.state_dict(ok)
