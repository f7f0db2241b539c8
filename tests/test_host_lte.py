"""CPU checks of learning-to-exit (LTE, ``EE_config["use_lte"]``): the numpy restatement on hand-made arrays, the configuration surface, the
synthetic weights, and the C-ABI (header declarations, plain-C compile, the symbol the built library exports, the ABI version)."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from .conftest import ROOT
from .lte_ref import gap_thresholds, lte_exits, lte_policy, lte_score, lte_scores

W_NAME, B_NAME = "layoutlmv3.encoder.lte_classifier.weight", "layoutlmv3.encoder.lte_classifier.bias"


def test_restatement_is_strict_at_the_threshold():
    # three exits + final; document 0 sits exactly ON the threshold of exit 0 and below that of exit 2, document 1 just below at exit 0
    thr = np.array([0.25, 0.25, 0.5, 0.0])
    s = np.array([[0.25, np.nextafter(0.25, 0.0), 0.9],
                  [0.60, 0.10, 0.9],
                  [0.40, 0.10, 0.5],
                  [0.00, 0.00, 0.0]])
    assert lte_exits(s, thr).tolist() == [2, 0, 3]              # u == thr stays; document 2 ties at exit 2 too and falls back to the last
    assert lte_exits(s, 0.0).tolist() == [3, 3, 3]               # nothing is below 0: the final exit, whose own threshold is never read
    assert lte_exits(s, 1.0).tolist() == [0, 0, 0]
    s[3] = -1.0
    assert lte_exits(s, thr).tolist() == [2, 0, 3]               # the last row is the fallback, not a test


def test_restatement_embedding_exits_never_fire_and_the_last_exit_is_the_fallback():
    s = np.array([[0.0, 0.0], [0.0, 0.0], [0.3, 0.7], [0.9, 0.2], [0.5, 0.5]])      # two embedding rows that WOULD pass any threshold
    assert lte_exits(s, 0.5, n_embedding_exits=2).tolist() == [2, 3]
    assert lte_exits(s, 0.5, n_embedding_exits=0).tolist() == [0, 0]
    assert lte_exits(s, 0.1, n_embedding_exits=2).tolist() == [4, 4]
    logits = np.arange(5 * 2 * 3, dtype=np.float64).reshape(5, 2, 3)
    ex, pred, counts = lte_policy(s, logits, 0.5, n_embedding_exits=2)
    assert np.array_equal(pred, logits[[2, 3], [0, 1]]) and counts.tolist() == [0, 0, 1, 1, 0]


def test_restatement_scores_and_gap_thresholds():
    rng = np.random.default_rng(0)
    h = rng.standard_normal((5, 6, 8)).astype(np.float32)        # L = 4
    w, b = rng.standard_normal((1, 8)).astype(np.float32), np.array([0.25], np.float32)
    s = lte_scores(h, w, b, [1, 3], n_embedding_exits=1)
    assert s.shape == (4, 6) and s.dtype == np.float64 and np.all(s[0] == 1.0)
    t = (h[3].astype(np.float64) * w.astype(np.float64)).sum(-1) + 0.25
    np.testing.assert_allclose(s[2], 1.0 / (1.0 + np.exp(-t)), rtol=1e-15)
    assert np.array_equal(s[3], lte_score(h[4], w, b))           # the final classifier reads the last layer's row
    thr, width = gap_thresholds(s, 0.5, 1e-9, n_embedding_exits=1)
    for e in (1, 2):
        assert int((s[e] < thr[e]).sum()) == 3 and float(np.abs(s[e] - thr[e]).min()) == pytest.approx(width[e] / 2)
    with pytest.raises(ValueError):
        gap_thresholds(s, 0.5, 2.0, n_embedding_exits=1)


def test_use_lte_round_trips_through_the_configuration(pkg):
    assert pkg.ExitConfig().use_lte is False and pkg.ExitConfig().as_dict()["use_lte"] is False
    ec = pkg.ExitConfig(use_lte=True, exits=[1, 2])
    assert ec.use_lte is True and ec.as_dict()["use_lte"] is True and str(ec.inference_strategy) == "max_confidence"
    cfg = pkg.ModelConfig.tiny(EE_config=dict(exits=[1, 3], use_lte=True))
    assert cfg.exit_config.use_lte is True
    hf = cfg.to_hf_dict()
    assert hf["EE_config"]["use_lte"] is True
    back = pkg.ModelConfig.from_hf_dict(hf)
    assert back.EE_config["use_lte"] is True and back.exit_config.use_lte is True
    assert pkg.ModelConfig.from_hf_dict(pkg.ModelConfig.tiny(EE_config=dict(exits=[1])).to_hf_dict()).exit_config.use_lte is False
    # the reference's switch is EE_config["use_lte"]; inference_strategy = "lte" leads to a TODO there and keeps raising here
    with pytest.raises(NotImplementedError):
        pkg.EarlyExitInference("lte").code


def test_synth_emits_the_lte_classifier_only_under_use_lte(pkg):
    ee = dict(exits=["text_avg", 1, 3], encoder_layer_strategy="ramp")
    plain = pkg.synth.make_weights(pkg.ModelConfig.tiny(EE_config=ee), seed=3)
    lte = pkg.synth.make_weights(pkg.ModelConfig.tiny(EE_config=dict(ee, use_lte=True)), seed=3)
    assert W_NAME not in plain and B_NAME not in plain
    H = 128
    assert lte[W_NAME].shape == (1, H) and lte[W_NAME].dtype == np.float32
    assert lte[B_NAME].shape == (1,) and lte[B_NAME].dtype == np.float32 and float(lte[B_NAME][0]) == 0.0
    assert 0.5 * 1.5 / np.sqrt(H) < float(lte[W_NAME].std()) < 2.0 * 1.5 / np.sqrt(H)
    assert set(lte) - set(plain) == {W_NAME, B_NAME}
    for k in plain:                                              # every other tensor is the one the twin configuration gets
        assert np.array_equal(plain[k], lte[k]), k


def test_policy_and_sweep_entry_points_exist(pkg):
    assert callable(getattr(pkg.Policy, "lte_policy")) and callable(pkg.lte_scan_device) and callable(pkg.sweep.lte_sweep)
    with pytest.raises(ValueError):
        pkg.Policy(np.zeros((2, 3, 4)), {"exit_policy": "lte_policy", "exit_threshold": 0.5}).lte_policy()
    with pytest.raises(ValueError):
        pkg.Policy(np.zeros((2, 3, 4)), {"exit_policy": "lte_policy", "lte_scores": np.zeros((2, 3))}).lte_policy()
    assert "lte_output" in pkg.EESequenceClassifierOutput._fields


def test_header_declares_lte_and_the_abi_versions_agree(pkg):
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    declared = set(re.findall(r"\b(ee_[a-z_0-9]+)\s*\(", header))
    assert "ee_lte_scan" in declared
    struct = header[header.index("typedef struct ee_config {"):header.index("} ee_config;")]
    fields = re.findall(r"int32_t\s+([a-z_0-9]+)\s*;", struct)
    assert fields[-1] == "use_lte"                              # appended: every earlier field keeps its offset
    version = int(re.search(r"#define\s+MMEE_ABI_VERSION\s+(\d+)", header).group(1))
    assert version == pkg.capi.ABI_VERSION == 4
    assert pkg.capi.EEConfig._fields_[-1][0] == "use_lte"
    assert "ee_lte_scan" in pkg.capi.SYMBOLS


def test_header_with_lte_compiles_as_c():
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n'
                    '#include "mmee.h"\n'
                    'int main(void) {\n'
                    '    int (*a)(const double*, const double*, int32_t, int32_t, int32_t, const double*, int32_t*, double*, int32_t*, void*) = ee_lte_scan;\n'
                    '    ee_config c;\n'
                    '    c.use_lte = 1;\n'
                    '    (void)a;\n'
                    '    return !(c.use_lte == 1 && offsetof(ee_config, use_lte) + sizeof(int32_t) == sizeof(ee_config) && MMEE_ABI_VERSION == 4);\n'
                    '}\n')
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def test_library_exports_ee_lte_scan(pkg):
    """Read the built library's dynamic symbol table (no GPU, no loading)."""
    path = pkg.capi.lib_path()
    if not os.path.exists(path):
        pytest.fail(f"{path} is missing: build() first")
    tool = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    r = subprocess.run([tool, "-D", "--defined-only", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    exported = {ln.split()[-1] for ln in r.stdout.splitlines() if ln.strip()}
    assert "ee_lte_scan" in exported
