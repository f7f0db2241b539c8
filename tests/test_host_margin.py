"""CPU checks of the margin criterion (include/mmee.h MMEE_CRIT_MARGIN) and the criterion tables: the numpy restatement of tests/csf_ref.py
on hand-computed cases, the configuration surface, the Policy's argument errors, and the C-ABI (header declarations, plain-C compile, the
symbols the built library exports, and the host-side argument checks of the two new entry points, which come before any device call)."""
import ctypes as C
import math
import operator
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from . import csf_ref
from .conftest import ROOT

NEW_SYMBOLS = ("ee_csf_table", "ee_criterion_scan")
LN3 = math.log(3.0)


def test_restatement_hand_computed_margins():
    assert csf_ref.margin([0.0, 0.0]) == 0.0                                   # a tie: exactly 0
    assert csf_ref.margin([0.7]) == 1.0 and csf_ref.margin([[-3.0], [12.5]]).tolist() == [1.0, 1.0]       # K = 1
    assert abs(csf_ref.margin([LN3, 0.0]) - 0.5) < 1e-15                       # p = (3/4, 1/4)
    assert abs(csf_ref.margin([0.0, LN3]) - 0.5) < 1e-15
    z = np.array([[[2.0 * LN3, 0.0]]], dtype=np.float32)
    want = csf_ref.margin(np.array([np.float64(z[0, 0, 0]) / 2.0, 0.0]))        # temperature 2 on [2 ln 3, 0], from the float32 logit
    assert csf_ref.margin(csf_ref.scaled(z, [2.0]))[0, 0] == want and abs(want - 0.5) < 1e-7
    assert csf_ref.margin([1.5, 1.5, 1.5]) == 0.0                              # a three-way tie
    assert csf_ref.margin([0.25, 1.5, -2.0, 1.5]) == 0.0                       # the maximum attained twice: m2 = m1
    assert abs(csf_ref.margin([LN3, 0.0, 0.0]) - 0.4) < 1e-15                  # p = (3/5, 1/5, 1/5)
    x = np.random.default_rng(0).standard_normal((5, 40, 7)) * 3.0
    m = csf_ref.margin(x)
    p = np.exp(x - x.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    srt = np.sort(p, axis=-1)
    assert m.shape == (5, 40) and np.all(m >= 0.0) and np.all(m <= 1.0)
    np.testing.assert_allclose(m, srt[..., -1] - srt[..., -2], rtol=0, atol=1e-15)      # top-1 minus top-2 probability
    np.testing.assert_allclose(csf_ref.max_softmax(x), srt[..., -1], rtol=1e-14, atol=0)
    np.testing.assert_allclose(csf_ref.entropy(x), -(p * np.log(p)).sum(-1), rtol=0, atol=1e-12)


def test_restatement_test_is_strict_and_falls_back_to_the_last_exit():
    table = np.array([[0.5, 0.5, 0.2], [0.9, 0.1, np.nan], [0.0, 0.0, 0.0]])
    assert csf_ref.exits(table, 0.5).tolist() == [1, 2, 2]                      # 0.5 > 0.5 is false; a NaN never fires; nothing fires: the last
    assert csf_ref.exits(table, [0.4, 0.95, 9.0]).tolist() == [0, 0, 2]
    assert csf_ref.exits(table, 0.5, sign=-1).tolist() == [2, 1, 0]             # the entropy direction, strict as well
    assert csf_ref.exits(table, np.nan).tolist() == [2, 2, 2]
    logits = np.array([[[LN3, 0.0], [0.0, 0.0]], [[0.0, 2.0], [0.0, 3.0]]])
    at = float(csf_ref.margin(logits[0, 0]))                                    # 0.5 up to rounding
    ex, pred, conf, counts = csf_ref.scan(logits, at, "margin")                 # a margin AT its threshold does not fire, a margin of 0 neither
    assert ex.tolist() == [1, 1] and counts.tolist() == [0, 2] and np.array_equal(pred, logits[1])
    assert np.array_equal(conf, csf_ref.margin(logits[1]))
    ex, _, conf, _ = csf_ref.scan(logits, np.nextafter(at, 0.0), "margin")      # one ulp below: it fires
    assert ex.tolist() == [0, 1] and conf[0] == at and abs(at - 0.5) < 1e-15
    thr, width = csf_ref.gap_thresholds(np.array([[0.1, 0.2, 0.6, 0.7], [0.0, 0.0, 0.0, 0.0]]), 0.5, 1e-5)
    assert abs(thr[0] - 0.4) < 1e-15 and thr[1] == 0.5 and abs(width[0] - 0.4) < 1e-15 and width[1] == np.inf
    with pytest.raises(ValueError, match="no gap"):
        csf_ref.gap_thresholds(np.zeros((2, 4)), 0.5, 1e-5)
    t = np.array([[0.1, 0.9], [0.8, 0.2]])
    hits, sums, hist = csf_ref.threshold_sweep(t, np.array([[1, 0], [0, 1]]), [[0.9, 0.0], [2.0, 2.0], [0.1, 0.1]])
    assert sums.tolist() == [1, 0, 0] and hits.tolist() == [0, 1, 1] and hist.tolist() == [[1, 1], [2, 0], [2, 0]]      # >=, exit 0 when none


def test_config_surface_round_trip_sign_and_code(pkg):
    st = pkg.EarlyExitInference("margin")
    assert st is pkg.EarlyExitInference.MARGIN and str(st) == "margin" and st.get_sign() is operator.gt and st.code == 3
    assert pkg.capi.CRIT_MARGIN == 3 and pkg.capi.CRIT_PATIENCE == 2 and pkg.capi.ABI_VERSION == 4
    assert [pkg.EarlyExitInference(n).code for n in ("max_confidence", "entropy", "patience")] == [0, 1, 2]
    ec = pkg.ExitConfig(exits=[1, 2], inference_strategy="margin")
    assert ec.inference_strategy is pkg.EarlyExitInference.MARGIN and ec.as_dict()["inference_strategy"] == "margin"
    ec = pkg.ExitConfig(exits=[1, 2], inference_strategy="margin", exit_rule="patient_confident", patience=2)      # margin has a threshold test
    assert str(ec.exit_rule) == "patient_confident"
    cfg = pkg.ModelConfig.tiny(EE_config=dict(exits=[1, 3], inference_strategy="margin"))
    d = cfg.to_hf_dict()
    assert d["EE_config"]["inference_strategy"] == "margin"
    back = pkg.ModelConfig.from_hf_dict(d)
    assert back.exit_config.inference_strategy is pkg.EarlyExitInference.MARGIN and back.exit_config.inference_strategy.code == 3
    with pytest.raises(ValueError, match="valid EarlyExitInference"):
        pkg.ExitConfig(inference_strategy="margins")


def test_header_declares_the_margin_and_both_functions():
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    assert re.search(r"#define\s+MMEE_ABI_VERSION\s+4\b", header)
    for name, v in (("MAX_CONFIDENCE", 0), ("ENTROPY", 1), ("PATIENCE", 2), ("MARGIN", 3)):
        assert re.search(rf"MMEE_CRIT_{name}\s*=\s*{v}\b", header), name
    declared = set(re.findall(r"\b(ee_[a-z_0-9]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared
    assert "margin = (1 - exp(m2 - m1)) / S" in header


def test_header_with_the_margin_compiles_as_c():
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "mmee.h"\n'
                    'int main(void) {\n'
                    '    int (*a)(const double*, const int64_t*, int32_t, int32_t, int32_t, int32_t, double*, uint8_t*, void*) = ee_csf_table;\n'
                    '    int (*b)(const double*, int32_t, int32_t, int32_t, int32_t, const double*, int32_t*, double*, double*, int32_t*, void*)'
                    ' = ee_criterion_scan;\n'
                    '    (void)a; (void)b;\n'
                    '    return MMEE_CRIT_MARGIN != 3 || MMEE_CRIT_PATIENCE != 2 || MMEE_ABI_VERSION != 4;\n'
                    '}\n')
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def test_library_exports_both_symbols(pkg):
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


def test_entry_points_refuse_bad_arguments_before_any_device_call(pkg):
    """Null pointers, E1 / N / K out of range and criteria without a threshold test are refused on the host, with a message that names the
    entry point.  The pointers are never dereferenced: plain integers stand in for device addresses."""
    lib = pkg.capi.load()
    p = C.c_void_p(4096)
    thr = (C.c_double * 3)(0.5, 0.5, 0.5)
    table_calls = {
        "null logits": (None, None, 3, 5, 4, 3, p, None, None),
        "null table": (p, None, 3, 5, 4, 3, None, None, None),
        "E1 = 0": (p, None, 0, 5, 4, 3, p, None, None),
        "N = 0": (p, None, 3, 0, 4, 3, p, None, None),
        "K = 0": (p, None, 3, 5, 0, 3, p, None, None),
        "correct without references": (p, None, 3, 5, 4, 3, p, p, None),
        "patience": (p, None, 3, 5, 4, pkg.capi.CRIT_PATIENCE, p, None, None),
        "unknown criterion": (p, None, 3, 5, 4, 4, p, None, None),
        "negative criterion": (p, None, 3, 5, 4, -1, p, None, None),
    }
    for what, args in table_calls.items():
        assert lib.ee_csf_table(*args) != 0, what
        msg = pkg.capi.last_error()
        assert msg.startswith("ee_csf_table:") and "no HIP device" not in msg, (what, msg)
        if "criterion" in what or what == "patience":
            assert "criterion" in msg, (what, msg)
    scan_calls = {
        "null logits": (None, 3, 5, 4, 3, thr, p, None, None, None, None),
        "null thresholds": (p, 3, 5, 4, 3, None, p, None, None, None, None),
        "null exits": (p, 3, 5, 4, 3, thr, None, None, None, None, None),
        "E1 = 0": (p, 0, 5, 4, 3, thr, p, None, None, None, None),
        "E1 = 257": (p, 257, 5, 4, 3, thr, p, None, None, None, None),
        "N < 0": (p, 3, -1, 4, 3, thr, p, None, None, None, None),
        "K = 0": (p, 3, 5, 0, 3, thr, p, None, None, None, None),
        "patience": (p, 3, 5, 4, pkg.capi.CRIT_PATIENCE, thr, p, None, None, None, None),
        "unknown criterion": (p, 3, 5, 4, 7, thr, p, None, None, None, None),
    }
    for what, args in scan_calls.items():
        assert lib.ee_criterion_scan(*args) != 0, what
        msg = pkg.capi.last_error()
        assert msg.startswith("ee_criterion_scan:") and "no HIP device" not in msg, (what, msg)
        if "criterion" in what or what == "patience":
            assert "criterion" in msg, (what, msg)
    # the Python wrappers name a criterion that has no threshold test before they look for a device
    for bad in ("patience", "lte"):
        with pytest.raises(ValueError, match="threshold criterion"):
            pkg.sweep.csf_table(np.zeros((2, 3, 4)), criterion=bad)
        with pytest.raises(ValueError, match="threshold criterion"):
            pkg.criterion_scan_device(np.zeros((2, 3, 4)), 0.5, bad)
    with pytest.raises(ValueError, match="valid EarlyExitInference"):
        pkg.sweep.csf_table(np.zeros((2, 3, 4)), criterion="msp")


def test_policy_entry_points_and_key_errors(pkg):
    for name in ("entropy_global_thresholding_policy", "margin_global_thresholding_policy"):
        assert callable(getattr(pkg.Policy, name))
        with pytest.raises(ValueError, match="exit_threshold"):
            getattr(pkg.Policy(np.zeros((2, 3, 4)), {"exit_policy": name}), name)()
    for name in ("patient_confident_policy", "patience_or_threshold_policy"):
        for bad, match in (("patience", "threshold criterion"), ("msp", "valid EarlyExitInference")):
            conf = {"exit_policy": name, "exit_threshold": 0.5, "patience": 1, "criterion": bad}
            with pytest.raises(ValueError, match=match):
                getattr(pkg.Policy(np.zeros((2, 3, 4)), conf), name)()
        with pytest.raises(ValueError, match="patience"):                        # the existing key errors come first
            getattr(pkg.Policy(np.zeros((2, 3, 4)), {"exit_policy": name, "exit_threshold": 0.5, "criterion": "margin"}), name)()
    assert callable(pkg.sweep.csf_table) and callable(pkg.criterion_scan_device)
