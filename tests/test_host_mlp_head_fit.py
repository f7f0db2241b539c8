"""CPU checks of the two-layer exit-head fit (include/mmee.h ee_mlp_head_fit): the C-ABI (declarations, plain-C compile, ABI 4, exported
symbols), the entry points' refusals before they look for a device, the workspace size, the names ``MlpHeadFit.state_dict`` produces, the
configurations the Python surface refuses, and tests/mlp_headfit_ref.py itself: its gradient against central differences and its port of the
controller against the scipy optimum of the convex one-layer objective."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import headfit_ref as HR
from . import mlp_headfit_ref as MR
from .conftest import ROOT
from .fit_util import _HostTensor, _refused, compiles_as_c, exported_symbols

NAMES = ("ee_mlp_head_fit", "ee_mlp_head_fit_workspace_bytes", "ee_debug_mlp_head_lossgrad")
TWO_LAYER_RAMP = dict(exits=[1, 2, 4], encoder_layer_strategy="ramp", exit_head_num_layers=2)
BLOCKS = ("dense.weight", "dense.bias", "out_proj.weight", "out_proj.bias")


def test_header_declares_the_three_functions_the_constant_and_the_objective():
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    assert re.search(r"#define\s+MMEE_ABI_VERSION\s+4\b", header)
    declared = set(re.findall(r"\b(ee_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert name in declared, name
    assert re.search(r"#define\s+MMEE_MLP_HEAD_FIT_ROWS\s+\d+", header)
    for text in ("a_n = tanh(W1 x_n + b1)", "z_n = W2 a_n + b2", "L(theta) = (1/N) sum_n [ logsumexp(z_n) - z_n[y_n] ] + (l2 / 2) ||theta||^2",
                 "theta = W1 row-major, b1, W2 row-major, b2", "P = H*H + H + K*H + K", "the biases included", "l2 <= 0 (and NaN) is refused",
                 "max-shifted", "theta = 0 is a saddle"):
        assert text in header, text


def test_capi_mirrors_the_header(pkg):
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    rows = int(re.search(r"#define\s+MMEE_MLP_HEAD_FIT_ROWS\s+(\d+)", header).group(1))
    assert pkg.capi.MLP_HEAD_FIT_ROWS == rows
    assert pkg.capi.ABI_VERSION == 4
    assert [len(pkg.capi.SYMBOLS[n][1]) for n in NAMES] == [23, 5, 11]
    assert pkg.fit_mlp_exit_heads is pkg.heads.fit_mlp_exit_heads and pkg.MlpHeadFit is pkg.heads.MlpHeadFit


def test_header_compiles_as_c_and_is_at_abi_4():
    compiles_as_c('    int (*a)(const float*, const int64_t*, const double*, int32_t, int32_t, int32_t, int32_t, double, double, int32_t, int32_t,'
                  ' void*, size_t, float*, float*, float*, float*, double*, double*, double*, int32_t*, int32_t*, void*) = ee_mlp_head_fit;\n'
                  '    size_t (*b)(int32_t, int32_t, int32_t, int32_t, int32_t) = ee_mlp_head_fit_workspace_bytes;\n'
                  '    int (*c)(const float*, const int64_t*, const double*, int32_t, int32_t, int32_t, int32_t, double, double*, double*, void*) ='
                  ' ee_debug_mlp_head_lossgrad;\n'
                  '    (void)a; (void)b; (void)c;\n'
                  '    return MMEE_ABI_VERSION != 4 || MMEE_MLP_HEAD_FIT_ROWS < 1;\n')


def test_library_exports_the_three_symbols(pkg):
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
    need = lib.ee_mlp_head_fit_workspace_bytes(E, N, H, K, M)
    assert need > 8 * E * MR.param_count(H, K) * (5 + 2 * M)           # theta, trial, two gradients, the direction, M pairs

    def fit(X=p, y=p, th0=p, E=E, N=N, H=H, K=K, l2=1e-2, gtol=1e-6, evals=50, hist=M, ws=p, ws_bytes=need, dw=p, db=p, w=p, b=p):
        return lib.ee_mlp_head_fit(X, y, th0, E, N, H, K, l2, gtol, evals, hist, ws, ws_bytes, dw, db, w, b, None, None, None, None, None, None)

    cases = {
        "null features": (dict(X=None), "NULL"),
        "null labels": (dict(y=None), "NULL"),
        "null theta0": (dict(th0=None), "NULL"),
        "null workspace": (dict(ws=None), "NULL"),
        "null dense_weight": (dict(dw=None), "NULL"),
        "null dense_bias": (dict(db=None), "NULL"),
        "null weight": (dict(w=None), "NULL"),
        "null bias": (dict(b=None), "NULL"),
        "l2 = 0": (dict(l2=0.0), "l2 = 0"),
        "l2 < 0": (dict(l2=-1e-3), "l2 = -0.001"),
        "l2 = nan": (dict(l2=float("nan")), "l2 = "),
        "K = 1": (dict(K=1), "K = 1"),
        "K = 65": (dict(K=65), "K = 65"),
        "E = 0": (dict(E=0), "E = 0"),
        "N = 0": (dict(N=0), "N = 0"),
        "H = 1028": (dict(H=1028), "H = 1028"),
        "H = 66": (dict(H=66), "H = 66"),
        "max_evals = 0": (dict(evals=0), "max_evals = 0"),
        "history = 0": (dict(hist=0), "history = 0"),
        "history = 33": (dict(hist=33), "history = 33"),
        "unaligned features": (dict(X=C.c_void_p(4100)), "aligned"),
        "small workspace": (dict(ws_bytes=need - 1), f"needs {need} bytes"),
    }
    _refused(pkg, "ee_mlp_head_fit", fit, cases)

    def lossgrad(X=p, y=p, th=p, K=K, l2=1e-2, loss=p, grad=p):
        return lib.ee_debug_mlp_head_lossgrad(X, y, th, E, N, H, K, l2, loss, grad, None)

    _refused(pkg, "ee_debug_mlp_head_lossgrad", lossgrad,
             {"null theta": (dict(th=None), "NULL"), "null grad": (dict(grad=None), "NULL"),
              "l2 = 0": (dict(l2=0.0), "l2 = 0"), "K = 1": (dict(K=1), "K = 1"), "K = 65": (dict(K=65), "K = 65")})


def test_workspace_grows_with_every_dimension_and_holds_the_controller_vectors(pkg):
    lib = pkg.capi.load()
    base = lib.ee_mlp_head_fit_workspace_bytes(2, 1000, 64, 10, 8)
    assert base > 8 * 2 * MR.param_count(64, 10) * (5 + 2 * 8)
    for args in ((3, 1000, 64, 10, 8), (2, 5000, 64, 10, 8), (2, 1000, 128, 10, 8), (2, 1000, 64, 11, 8), (2, 1000, 64, 10, 9)):
        assert lib.ee_mlp_head_fit_workspace_bytes(*args) > base, args
    # the stated formula: the controller's vectors, the hidden rows, the logits and the rows' losses, and under 2 KB of control words each
    E, N, H, K, M = 6, 40000, 768, 16, 8
    stated = 8 * E * MR.param_count(H, K) * (5 + 2 * M) + 8 * E * N * (H + K + 1)
    got = lib.ee_mlp_head_fit_workspace_bytes(E, N, H, K, M)
    assert stated <= got <= stated + 2048 * E, (got, stated)


def _host_fit(pkg, E, K, H):
    rng = np.random.default_rng(0)
    arrays = [rng.standard_normal(s).astype(np.float32) for s in ((E, H, H), (E, H), (E, K, H), (E, K))]
    return pkg.MlpHeadFit(*[_HostTensor(a) for a in arrays], None, None, None, None, None, 1e-2), arrays


@pytest.mark.parametrize("arch", ["layoutlmv3", "beit"])
def test_state_dict_names_are_the_synthetic_weights_head_names(pkg, arch):
    cfg = pkg.ModelConfig.dit_tiny(EE_config=TWO_LAYER_RAMP) if arch == "beit" else pkg.ModelConfig.tiny(EE_config=TWO_LAYER_RAMP)
    W = (pkg.synth.make_weights_beit if arch == "beit" else pkg.synth.make_weights)(cfg, seed=1)
    fit, arrays = _host_fit(pkg, 3, cfg.num_labels, cfg.hidden_size)
    sd = fit.state_dict(cfg)
    assert set(sd) == {k for k in W if "early_exits" in k}
    for k, v in sd.items():
        assert v.shape == W[k].shape and v.dtype == W[k].dtype == np.float32 and v.flags["C_CONTIGUOUS"], k
    prefix = "beit." if arch == "beit" else "layoutlmv3."
    for j in range(3):
        for name, a in zip(BLOCKS, arrays):
            assert np.array_equal(sd[f"{prefix}encoder.early_exits.{j}.{name}"], a[j]), (j, name)


def test_python_surface_refuses_what_is_out_of_scope(pkg):
    fit, _ = _host_fit(pkg, 2, 16, 128)
    one = pkg.ModelConfig.tiny(EE_config=dict(exits=[1, 2], encoder_layer_strategy="ramp", exit_head_num_layers=1))
    with pytest.raises(ValueError, match="exit_head_num_layers == 2"):
        fit.state_dict(one)
    gate = pkg.ModelConfig.tiny(EE_config=dict(exits=[1, 2], encoder_layer_strategy="gate", exit_head_num_layers=2))
    with pytest.raises(ValueError, match="gate"):
        fit.state_dict(gate)
    emb = pkg.ModelConfig.tiny(EE_config=dict(exits=["text_avg", 1, 2], encoder_layer_strategy="ramp", exit_head_num_layers=2))
    with pytest.raises(ValueError, match="embedding-level"):
        fit.state_dict(emb)
    three = pkg.ModelConfig.tiny(EE_config=TWO_LAYER_RAMP)
    with pytest.raises(ValueError, match="the configuration wants"):
        fit.state_dict(three)
    two = pkg.ModelConfig.tiny(EE_config=dict(exits=[1, 2], encoder_layer_strategy="ramp", exit_head_num_layers=2))
    assert len(fit.state_dict(two)) == 8

    class _Engine:
        cfg = one
    with pytest.raises(ValueError, match="exit_head_num_layers == 2"):
        pkg.collect_exit_features(_Engine(), [], head_layers=2)
    _Engine.cfg = gate
    with pytest.raises(ValueError, match="gate"):
        pkg.collect_exit_features(_Engine(), [], head_layers=2)
    _Engine.cfg = emb
    with pytest.raises(ValueError, match="embedding-level"):
        pkg.collect_exit_features(_Engine(), [], head_layers=2)
    _Engine.cfg = two
    with pytest.raises(ValueError, match="exit_head_num_layers == 1"):       # the default keeps the one-layer refusal
        pkg.collect_exit_features(_Engine(), [])
    with pytest.raises(ValueError, match="one or two layers"):
        pkg.collect_exit_features(_Engine(), [], head_layers=3)


@pytest.mark.parametrize("N,H,K", [(9, 8, 3), (40, 12, 2), (25, 16, 10)])
def test_restatement_gradient_agrees_with_central_differences(N, H, K):
    """Central differences with h = 1e-5 on an objective whose third derivatives are of order 1: truncation h^2 ~ 1e-10, rounding
    eps |L| / h ~ 1e-11; the bar is 1e-8."""
    rng = np.random.default_rng(N)
    X = rng.standard_normal((N, H)).astype(np.float32)
    y = rng.integers(0, K, N)
    theta = rng.standard_normal(MR.param_count(H, K)) / np.sqrt(H)
    l2 = 1e-2
    _, g = MR.loss_grad(theta, X, y, K, l2)
    h = 1e-5
    num = np.empty_like(g)
    for i in range(theta.size):
        d = np.zeros_like(theta)
        d[i] = h
        num[i] = (MR.loss_grad(theta + d, X, y, K, l2)[0] - MR.loss_grad(theta - d, X, y, K, l2)[0]) / (2 * h)
    err = np.abs(num - g).max()
    print(f"({N},{H},{K}): max |central difference - gradient| = {err:.3e}")
    assert err <= 1e-8, err
    # every block is penalised: where the data term does not see a change of theta, the gradient moves by l2 times it.  A common shift of
    # b2 leaves the softmax alone.
    shift = theta.copy()
    shift[-K:] += 0.5
    _, g2 = MR.loss_grad(shift, X, y, K, l2)
    assert np.allclose(g2[-K:] - g[-K:], l2 * 0.5, rtol=0, atol=1e-14)
    # at the identity start the objective is the one-layer objective on tanh(x) at zero
    l0, g0 = MR.loss_grad(MR.init_identity(H, K), X, y, K, l2)
    l1, g1 = HR.loss_grad(np.zeros(K * H + K), np.tanh(X.astype(np.float64)), y, K, l2)
    assert abs(l0 - (l1 + 0.5 * l2 * H)) <= 1e-14
    assert np.allclose(g0[H * H + H:], g1, rtol=0, atol=1e-15)


def test_controller_port_reaches_the_optimum_of_the_convex_one_layer_objective():
    """The port on headfit_ref.loss_grad from zero ends within (||g|| + ||g_ref||) / l2 of the scipy optimum: strong convexity."""
    N, H, K, l2 = 300, 64, 10, 1e-2
    X, y = HR.teacher_problem(N, H, K, 1, seed=N + H + K)
    theta, f, gnorm, evals, status, accepted = MR.lbfgs(lambda th: HR.loss_grad(th, X[0], y, K, l2), np.zeros(K * H + K), 1e-9, 2000)
    ref = HR.solve(X[0], y, K, l2)
    n_dev = np.linalg.norm(HR.loss_grad(theta, X[0], y, K, l2)[1])
    n_ref = np.linalg.norm(HR.loss_grad(ref, X[0], y, K, l2)[1])
    dist = np.linalg.norm(theta - ref)
    print(f"evals {evals} status {status} ||g|| {n_dev:.3e} ||g_ref|| {n_ref:.3e} distance {dist:.3e}")
    assert status == 0 and gnorm <= 1e-9 and abs(gnorm - n_dev) <= 1e-15
    assert dist <= (n_dev + n_ref) / l2, (dist, (n_dev + n_ref) / l2)
    assert all(b <= a + MR.ARMIJO_SLACK * abs(a) for a, b in zip(accepted, accepted[1:]))
