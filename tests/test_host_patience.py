"""CPU checks of patience-based early exit (PABEE): the numpy restatement on hand-worked cases, the configuration surface, and the C-ABI
(header declarations, plain-C compile, the symbols the built library exports)."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from .conftest import ROOT
from .patience_ref import patience_exits, patience_policy, patience_sweep, run_counters

NEW_SYMBOLS = ("ee_set_patience", "ee_patience_scan", "ee_patience_sweep")


def _store(preds, K=3, ties=()):
    """(E1, N, K) logits whose argmax at exit e of document n is preds[n][e]; ties: (e, n, k) entries set equal to the row's maximum."""
    P = np.asarray(preds).T                                   # (E1, N)
    E1, N = P.shape
    s = np.zeros((E1, N, K))
    s[np.arange(E1)[:, None], np.arange(N)[None, :], P] = 1.0
    for e, n, k in ties:
        s[e, n, k] = 1.0
    return s


def test_restatement_hand_worked_runs():
    # document 0: 1 1 1 1 -> c = 0 1 2 3;  document 1: 0 1 1 2 2 2 -> a run broken and restarted
    s = _store([[1, 1, 1, 1, 0, 0], [0, 1, 1, 2, 2, 2]])
    p, c = run_counters(s)
    assert c[:, 0].tolist() == [0, 1, 2, 3, 0, 1] and c[:, 1].tolist() == [0, 0, 1, 0, 1, 2]
    assert patience_exits(s, 1).tolist() == [1, 2]           # t = 1: the first repeat
    assert patience_exits(s, 2).tolist() == [2, 5]           # document 1: the first run (length 1) is broken, the second reaches 2 at exit 5
    assert patience_exits(s, 3).tolist() == [3, 5]           # document 1 never reaches 3: the final exit
    E = s.shape[0] - 1
    assert patience_exits(s, E).tolist() == [E, E]           # t = E: only an unbroken sequence could leave before the end
    assert patience_exits(s, E + 1).tolist() == [E, E]       # t > E: everybody runs to the final exit
    assert patience_exits(_store([[2, 2, 2, 2, 2, 2]]), E).tolist() == [E]


def test_restatement_exact_ties_take_the_first_index():
    # exit 1 of document 0 ties classes 0 and 2: argmax is 0, so the run of 2s is broken there
    s = _store([[2, 2, 2, 2]], ties=[(1, 0, 0)])
    p, c = run_counters(s)
    assert p[:, 0].tolist() == [2, 0, 2, 2] and c[:, 0].tolist() == [0, 0, 0, 1]
    assert patience_exits(s, 1).tolist() == [3]
    # a tie that resolves to the SAME index as before keeps the run going
    s = _store([[0, 0, 0]], ties=[(1, 0, 2)])
    assert patience_exits(s, 2).tolist() == [2]


def test_restatement_policy_and_sweep_agree():
    rng = np.random.default_rng(3)
    s = rng.integers(0, 3, (6, 200, 4)).astype(np.float64)     # integer logits: many exact ties
    refs = rng.integers(0, 4, 200)
    acc, mex, hist, hits, sums = patience_sweep(s, refs, [1, 2, 3, 5, 6, 9])
    for i, t in enumerate([1, 2, 3, 5, 6, 9]):
        ex, pred, conf, counts = patience_policy(s, t)
        assert np.array_equal(hist[i], counts) and sums[i] == ex.sum()
        assert hits[i] == int((pred.argmax(-1) == refs).sum())
        np.testing.assert_allclose(conf, np.exp(pred - pred.max(-1, keepdims=True)).sum(-1) ** -1, rtol=1e-14)
    assert np.all(hist[-2:] == hist[-1]) and hist[-1][-1] == 200   # t >= E1: the final exit only


def test_config_accepts_and_round_trips_patience(pkg):
    assert pkg.EarlyExitInference("patience").code == 2
    with pytest.raises(NotImplementedError):
        pkg.EarlyExitInference("patience").get_sign()       # no threshold, so no sign
    with pytest.raises(NotImplementedError):
        pkg.EarlyExitInference("lte").code
    assert pkg.ExitConfig().patience is None and pkg.ExitConfig().as_dict()["patience"] is None
    ec = pkg.ExitConfig(inference_strategy="patience", patience=3, exits=[1, 2])
    assert ec.patience == 3 and ec.as_dict()["patience"] == 3 and str(ec.inference_strategy) == "patience"
    for bad in (0, -1, 1.5, True, "2"):
        with pytest.raises(ValueError):
            pkg.ExitConfig(inference_strategy="patience", patience=bad)
    cfg = pkg.ModelConfig.tiny(EE_config=dict(exits=[1, 3], inference_strategy="patience", patience=2))
    back = pkg.ModelConfig.from_hf_dict(cfg.to_hf_dict())
    assert back.EE_config["patience"] == 2 and back.exit_config.patience == 2
    assert str(back.exit_config.inference_strategy) == "patience"


def test_policy_and_sweep_entry_points_exist(pkg):
    assert callable(getattr(pkg.Policy, "patience_policy"))
    assert callable(pkg.sweep.patience_sweep) and callable(pkg.patience_scan_device)
    with pytest.raises(ValueError):
        pkg.Policy(np.zeros((2, 3, 4)), {"exit_policy": "patience_policy"}).patience_policy()


def test_header_declares_patience():
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    assert re.search(r"MMEE_CRIT_PATIENCE\s*=\s*2", header)
    declared = set(re.findall(r"\b(ee_[a-z_0-9]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared


def test_header_with_patience_compiles_as_c():
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "mmee.h"\n'
                    'int main(void) {\n'
                    '    int (*a)(ee_handle*, int32_t) = ee_set_patience;\n'
                    '    int (*b)(const double*, int32_t, int32_t, int32_t, int32_t, int32_t*, double*, double*, int32_t*, void*) = ee_patience_scan;\n'
                    '    int (*c)(const double*, const int64_t*, int32_t, int32_t, int32_t, const int32_t*, int32_t, double*, double*, int32_t*, void*)'
                    ' = ee_patience_sweep;\n'
                    '    (void)a; (void)b; (void)c;\n'
                    '    return MMEE_CRIT_PATIENCE != 2;\n'
                    '}\n')
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def test_library_exports_patience_symbols(pkg):
    """Read the built library's dynamic symbol table (no GPU, no loading)."""
    path = pkg.capi.lib_path()
    if not os.path.exists(path):
        pytest.fail(f"{path} is missing: build() first")
    tool = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    r = subprocess.run([tool, "-D", "--defined-only", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    exported = {ln.split()[-1] for ln in r.stdout.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert name in exported, name
        assert name in pkg.capi.SYMBOLS
