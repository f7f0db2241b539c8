"""CPU checks of the exit-head fit (include/mmee.h ee_head_fit): the C-ABI (declarations, plain-C compile, ABI 4, exported symbols), the entry
points' refusals before they look for a device, the names ``HeadFit.state_dict`` produces, the configurations the Python surface refuses, and the
float64 restatement of tests/headfit_ref.py against central differences."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import headfit_ref as HR
from .conftest import ROOT
from .fit_util import _HostTensor, _refused, compiles_as_c, exported_symbols

NAMES = ("ee_head_fit", "ee_head_fit_workspace_bytes", "ee_debug_head_lossgrad")
ONE_LAYER_RAMP = dict(exits=[1, 2, 4], encoder_layer_strategy="ramp", exit_head_num_layers=1)


def test_header_declares_the_three_functions():
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    assert re.search(r"#define\s+MMEE_ABI_VERSION\s+4\b", header)           # three more functions: ee_config is unchanged
    declared = set(re.findall(r"\b(ee_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert name in declared, name
    for text in ("logsumexp(z_n) - z_n[y_n]", "(l2 / 2) (||W||^2 + ||b||^2)", "The bias is penalised too", "l2 <= 0 is refused", "c1 = 1e-4",
                 "30 halvings"):
        assert text in header, text


def test_capi_mirrors_the_header(pkg):
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    slab = int(re.search(r"#define\s+MMEE_HEAD_FIT_SLAB\s+(\d+)", header).group(1))
    assert pkg.capi.HEAD_FIT_SLAB == slab
    assert pkg.capi.ABI_VERSION == 4
    assert [len(pkg.capi.SYMBOLS[n][1]) for n in NAMES] == [21, 5, 11]
    assert pkg.fit_exit_heads is pkg.heads.fit_exit_heads and pkg.HeadFit is pkg.heads.HeadFit


def test_header_compiles_as_c_and_is_at_abi_4():
    compiles_as_c('    int (*a)(const float*, const int64_t*, int32_t, int32_t, int32_t, int32_t, double, double, int32_t, int32_t, void*, size_t, float*,'
                  ' float*, double*, double*, double*, double*, int32_t*, int32_t*, void*) = ee_head_fit;\n'
                  '    size_t (*b)(int32_t, int32_t, int32_t, int32_t, int32_t) = ee_head_fit_workspace_bytes;\n'
                  '    int (*c)(const float*, const int64_t*, const double*, int32_t, int32_t, int32_t, int32_t, double, double*, double*, void*) ='
                  ' ee_debug_head_lossgrad;\n'
                  '    (void)a; (void)b; (void)c;\n'
                  '    return MMEE_ABI_VERSION != 4 || MMEE_HEAD_FIT_SLAB < 1;\n')


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
    need = lib.ee_head_fit_workspace_bytes(E, N, H, K, M)
    assert need > 8 * E * (K * H + K) * (5 + 2 * M)                    # theta, trial, two gradients, the direction, M pairs

    def fit(X=p, y=p, E=E, N=N, H=H, K=K, l2=1e-2, gtol=1e-9, evals=50, hist=M, ws=p, ws_bytes=need, w=p, b=p):
        return lib.ee_head_fit(X, y, E, N, H, K, l2, gtol, evals, hist, ws, ws_bytes, w, b, None, None, None, None, None, None, None)

    cases = {
        "null features": (dict(X=None), "NULL"),
        "null labels": (dict(y=None), "NULL"),
        "null workspace": (dict(ws=None), "NULL"),
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
    _refused(pkg, "ee_head_fit", fit, cases)

    def lossgrad(X=p, y=p, th=p, K=K, l2=1e-2, loss=p, grad=p):
        return lib.ee_debug_head_lossgrad(X, y, th, E, N, H, K, l2, loss, grad, None)

    _refused(pkg, "ee_debug_head_lossgrad", lossgrad,
             {"null theta": (dict(th=None), "NULL"), "null grad": (dict(grad=None), "NULL"),
              "l2 = 0": (dict(l2=0.0), "l2 = 0"), "K = 1": (dict(K=1), "K = 1"), "K = 65": (dict(K=65), "K = 65")})


def test_workspace_grows_with_every_dimension(pkg):
    lib = pkg.capi.load()
    base = lib.ee_head_fit_workspace_bytes(2, 1000, 64, 10, 8)
    for args in ((3, 1000, 64, 10, 8), (2, 5000, 64, 10, 8), (2, 1000, 128, 10, 8), (2, 1000, 64, 11, 8), (2, 1000, 64, 10, 9)):
        assert lib.ee_head_fit_workspace_bytes(*args) > base, args


def _host_fit(pkg, E, K, H):
    rng = np.random.default_rng(0)
    w, b = rng.standard_normal((E, K, H)).astype(np.float32), rng.standard_normal((E, K)).astype(np.float32)
    return pkg.HeadFit(_HostTensor(w), _HostTensor(b), None, None, None, None, None, None, 1e-2), w, b


@pytest.mark.parametrize("arch", ["layoutlmv3", "beit"])
def test_state_dict_names_are_the_synthetic_weights_head_names(pkg, arch):
    """The names equal the head names of the architecture's synthetic weights, which is what the engine's expected_tensors() lists (checked on
    the device by tests/test_gpu_head_fit.py, where a handle exists); shapes and values are the fit's."""
    cfg = pkg.ModelConfig.dit_tiny(EE_config=ONE_LAYER_RAMP) if arch == "beit" else pkg.ModelConfig.tiny(EE_config=ONE_LAYER_RAMP)
    W = (pkg.synth.make_weights_beit if arch == "beit" else pkg.synth.make_weights)(cfg, seed=1)
    fit, w, b = _host_fit(pkg, 3, cfg.num_labels, cfg.hidden_size)
    sd = fit.state_dict(cfg)
    assert set(sd) == {k for k in W if "early_exits" in k}
    for k, v in sd.items():
        assert v.shape == W[k].shape and v.dtype == np.float32 and v.flags["C_CONTIGUOUS"], k
    j = 1
    prefix = "beit." if arch == "beit" else "layoutlmv3."
    assert np.array_equal(sd[f"{prefix}encoder.early_exits.{j}.out_proj.weight"], w[j])
    assert np.array_equal(sd[f"{prefix}encoder.early_exits.{j}.out_proj.bias"], b[j])


def test_python_surface_refuses_what_is_out_of_scope(pkg):
    fit, _, _ = _host_fit(pkg, 2, 16, 128)
    two = pkg.ModelConfig.tiny(EE_config=dict(exits=[1, 2], encoder_layer_strategy="ramp", exit_head_num_layers=2))
    with pytest.raises(ValueError, match="exit_head_num_layers == 1"):
        fit.state_dict(two)
    gate = pkg.ModelConfig.tiny(EE_config=dict(exits=[1, 2], encoder_layer_strategy="gate", exit_head_num_layers=1))
    with pytest.raises(ValueError, match="gate"):
        fit.state_dict(gate)
    emb = pkg.ModelConfig.tiny(EE_config=dict(exits=["text_avg", 1, 2], encoder_layer_strategy="ramp", exit_head_num_layers=1))
    with pytest.raises(ValueError, match="embedding-level"):
        fit.state_dict(emb)
    three = pkg.ModelConfig.tiny(EE_config=ONE_LAYER_RAMP)
    with pytest.raises(ValueError, match="the configuration wants"):
        fit.state_dict(three)

    class _Engine:
        cfg = two
    with pytest.raises(ValueError, match="exit_head_num_layers == 1"):
        pkg.collect_exit_features(_Engine(), [])


@pytest.mark.parametrize("N,H,K", [(7, 8, 3), (40, 12, 2), (25, 16, 10)])
def test_restatement_gradient_agrees_with_central_differences(N, H, K):
    """Central differences with h = 1e-5 on an objective whose third derivatives are of order 1: truncation h^2 ~ 1e-10, rounding
    eps |L| / h ~ 1e-11; the bar is 1e-8."""
    rng = np.random.default_rng(N)
    X = rng.standard_normal((N, H)).astype(np.float32)
    y = rng.integers(0, K, N)
    theta = 0.3 * rng.standard_normal(K * H + K)
    l2 = 1e-2
    _, g = HR.loss_grad(theta, X, y, K, l2)
    h = 1e-5
    num = np.empty_like(g)
    for i in range(theta.size):
        d = np.zeros_like(theta)
        d[i] = h
        num[i] = (HR.loss_grad(theta + d, X, y, K, l2)[0] - HR.loss_grad(theta - d, X, y, K, l2)[0]) / (2 * h)
    assert np.abs(num - g).max() <= 1e-8, np.abs(num - g).max()
    # the penalty covers the bias: the gradient's bias block at theta moves by l2 * delta when only b moves by a common shift delta
    shift = theta.copy()
    shift[K * H:] += 0.5
    _, g2 = HR.loss_grad(shift, X, y, K, l2)
    assert np.allclose(g2[K * H:] - g[K * H:], l2 * 0.5, rtol=0, atol=1e-14)
