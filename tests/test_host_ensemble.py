"""CPU-only checks of the exit ensemble (include/mmee.h, at ee_set_ensemble): the numpy restatement tests/ensemble_ref.py against the cases with
a closed form, its gradient against central differences, its reference optimum, and the new header symbols."""
import os

import numpy as np
import pytest

from . import ensemble_ref as ER
from .conftest import ROOT, sweep_ref_inputs

NEW_SYMBOLS = ("ee_set_ensemble", "ee_has_ensemble", "ee_ensemble_logits", "ee_ensemble_fit", "ee_ensemble_fit_workspace_bytes", "ee_debug_exit_ensemble")


def _table(E1=5, N=200, K=7, seed=3):
    store, refs = sweep_ref_inputs(seed=seed, E1=E1, N=N, K=K)
    return store.astype(np.float32), refs


def test_identity_weights_give_the_float32_logsoftmax():
    x, _ = _table()
    y = ER.ensemble(x, np.eye(x.shape[0]))
    want = ER.logsoftmax64(x).astype(np.float32)
    assert y.dtype == np.float32 and np.array_equal(y, want)
    # the plain exit up to one rounding: the same argmax, the softmax of y is the softmax of x
    assert np.array_equal(y.argmax(-1), x.argmax(-1))
    assert np.abs(np.exp(ER.logsoftmax64(y)) - np.exp(ER.logsoftmax64(x))).max() < 1e-6


def test_running_mean_is_the_cumulative_sum_of_l():
    x, _ = _table(E1=6)
    E1 = x.shape[0]
    w = np.tril(np.ones((E1, E1))) / np.arange(1, E1 + 1)[:, None]
    l = ER.logsoftmax64(x)
    want = np.cumsum(l, 0) / np.arange(1, E1 + 1)[:, None, None]
    a = ER.combine(l, w)
    assert np.abs(a - want).max() <= 1e-13 * np.abs(want).max()
    ok, _ = ER.ulp_close_f32(ER.ensemble(x, w), want.astype(np.float32))
    assert ok.all()


def test_bias_temperature_and_nan_rows():
    z, _ = _table()
    E1, N, K = z.shape
    w, b = ER.random_weights(E1, K, seed=1)
    ER.check_weights(w)
    assert (w[np.tril_indices(E1, -1)] == 0).any()                              # zeros below the diagonal in places
    tm = np.array([1.0, 3.0, 0.5, 1.7, 1.0])
    x = ER.scaled(z, tm)
    assert np.array_equal(x[1], (z[1].astype(np.float64) / 3.0).astype(np.float32))
    y0, yb = ER.ensemble(x, w), ER.ensemble(x, w, b)
    assert np.abs((yb - y0) - b[:, None, :]).max() < 1e-5
    x[2, 5] = np.nan                                                            # document 5 never reached exit 2
    y = ER.ensemble(x, w, b)
    assert np.isnan(y[2:, 5]).all() and np.isfinite(y[:2, 5]).all() and np.isfinite(np.delete(y, 5, 1)).all()


@pytest.mark.parametrize("m", [0, 2, 4])
def test_gradient_matches_central_differences(m):
    x, refs = _table()
    l = ER.logsoftmax64(x)
    K = x.shape[2]
    rng = np.random.default_rng(m)
    th = ER.start(m, K) + rng.normal(0, 0.2, K + m + 1)
    _, g = ER.objective(th, l, refs, m, 1e-2)
    h = 1e-6
    num = np.array([(ER.objective(th + h * e, l, refs, m, 1e-2)[0] - ER.objective(th - h * e, l, refs, m, 1e-2)[0]) / (2 * h) for e in np.eye(th.size)])
    assert np.abs(num - g).max() <= 1e-8 * max(1.0, np.abs(g).max())
    # the penalty vanishes at the start, where the objective is the plain exit's NLL
    assert ER.objective(ER.start(m, K), l, refs, m, 1e-2)[0] == pytest.approx(ER.plain_nll(l, refs)[m], rel=1e-14)


@pytest.mark.parametrize("K", [2, 7, 16])
def test_reference_optimum_is_stationary_and_below_the_plain_exit(K):
    x, refs = _table(E1=5, N=300, K=K, seed=11)
    l = ER.logsoftmax64(x)
    nll = ER.plain_nll(l, refs)
    for m in range(x.shape[0]):
        assert K + m + 1 <= 24
        th, loss, gn = ER.reference_optimum(l, refs, m, 1e-2)
        assert gn <= 1e-12, (m, gn)
        assert loss <= nll[m], (m, loss, nll[m])
        if m > 0:
            assert loss < nll[m] - 1e-6                                         # earlier exits carry information here: the ensemble helps


def test_header_declares_and_library_exports_the_new_symbols(pkg):
    import re
    import shutil
    import subprocess
    import tempfile
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    declared = set(re.findall(r"\b(ee_[a-z_0-9]+)\s*\(", header))
    lib = pkg.capi.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg.capi.SYMBOLS and getattr(lib, name) is not None, name
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "mmee.h"\nint main(void) {\n  ee_debug_exit_ensemble_args a; (void)a;\n'
                    + "".join(f"  (void)&{n};\n" for n in NEW_SYMBOLS) + "  return 0;\n}\n")
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def test_python_surface_refuses_without_a_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    x, refs = _table()
    with pytest.raises(pkg.capi.MMEEUnavailable):
        pkg.sweep.ensemble_logits(x, np.eye(x.shape[0]))
    with pytest.raises(pkg.capi.MMEEUnavailable):
        pkg.heads.fit_exit_ensemble(x, refs)
