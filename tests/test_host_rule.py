"""CPU checks of the two combined exit rules (include/mmee.h MMEE_RULE_STREAK "patient and confident", MMEE_RULE_EITHER "patience or
threshold"): the numpy restatement's identities on hand-worked and random cases, the configuration surface and its refusals, the Policy's
argument errors, and the C-ABI (header declarations, plain-C compile, the symbols the built library exports)."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from .conftest import ROOT
from .patience_ref import patience_exits
from .rule_ref import EITHER, PLAIN, STREAK, events, msp_table, plain_exits, rule_exits, rule_policy, rule_sweep, streak_counters

NEW_SYMBOLS = ("ee_set_exit_rule", "ee_set_patience_vector", "ee_rule_scan", "ee_rule_sweep")


def _random_case(seed, E1=6, N=300, K=4):
    rng = np.random.default_rng(seed)
    store = rng.integers(0, 3, (E1, N, K)).astype(np.float64)          # integer logits: many exact ties, long agreement runs
    crit = msp_table(store)
    thr = np.quantile(crit, 0.6, axis=1)
    return store, crit, thr, rng.integers(0, K, N)


def test_restatement_hand_worked_streaks():
    # one document, six exits + final; the test holds at exits 0, 2, 3, 4
    crit = np.array([[0.9], [0.1], [0.9], [0.9], [0.9], [0.1], [0.1]])
    f = events(crit, 0.5, +1)
    assert f[:, 0].tolist() == [True, False, True, True, True, False, False]
    assert streak_counters(f)[:, 0].tolist() == [1, 0, 1, 2, 3, 0, 0]
    store = np.zeros((7, 1, 2))
    assert rule_exits(crit, store, 0.5, 1, STREAK).tolist() == [0]
    assert rule_exits(crit, store, 2, 1, STREAK).tolist() == [6]       # a threshold nothing exceeds: the final exit
    assert rule_exits(crit, store, 0.5, 2, STREAK).tolist() == [3]
    assert rule_exits(crit, store, 0.5, 3, STREAK).tolist() == [4]
    assert rule_exits(crit, store, 0.5, 4, STREAK).tolist() == [6]     # never four in a row: the final exit
    assert rule_exits(crit, store, 0.5, [3, 3, 1, 3, 3, 3, 1], STREAK).tolist() == [2]      # per exit: s_2 = 1 >= t_2 = 1
    assert rule_exits(crit, store, 0.5, [2, 2, 2, 3, 9, 9, 1], STREAK).tolist() == [6]      # s_3 = 2 < 3, s_4 = 3 < 9
    # strict compares, and the entropy / LTE sign
    assert rule_exits(np.full((3, 1), 0.5), store[:3], 0.5, 1, STREAK).tolist() == [2]
    assert rule_exits(np.full((3, 1), 0.5), store[:3], 0.5, 1, STREAK, sign=-1).tolist() == [2]
    assert rule_exits(1.0 - crit, store, 0.5, 2, STREAK, sign=-1).tolist() == [3]
    assert rule_exits(crit, store, np.nan, 1, STREAK).tolist() == [6]  # a NaN threshold never fires


def test_restatement_hand_worked_either():
    # predictions 0 1 1 1 2 2 2 -> c = 0 0 1 2 0 1 2; the confidence test holds at exit 4 only
    P = [0, 1, 1, 1, 2, 2, 2]
    store = np.zeros((7, 1, 3))
    store[np.arange(7), 0, P] = 1.0
    crit = np.array([[0.1], [0.1], [0.1], [0.1], [0.9], [0.1], [0.1]])
    assert rule_exits(crit, store, 0.5, 1, EITHER).tolist() == [2]     # the agreement comes first
    assert rule_exits(crit, store, 0.5, 2, EITHER).tolist() == [3]
    assert rule_exits(crit, store, 0.5, 3, EITHER).tolist() == [4]     # the threshold comes first
    assert rule_exits(crit, store, 2.0, 3, EITHER).tolist() == [6]     # neither
    assert rule_exits(crit, store, 2.0, [9, 9, 9, 9, 9, 1, 1], EITHER).tolist() == [5]      # per exit: c_5 = 1 >= t_5 = 1


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_restatement_identities(seed):
    store, crit, thr, refs = _random_case(seed)
    E1 = store.shape[0]
    plain = plain_exits(crit, thr, +1)
    assert np.array_equal(rule_exits(crit, store, thr, 1, STREAK), plain)                       # STREAK at t = 1 is PLAIN
    assert np.array_equal(rule_exits(crit, store, thr, 1, PLAIN), plain)
    assert np.array_equal(rule_exits(crit, store, thr, E1, EITHER), plain)                      # t > E: the counter never gets there
    for t in range(1, E1 + 1):
        either = rule_exits(crit, store, thr, t, EITHER)
        assert np.array_equal(rule_exits(crit, store, 2.0, t, EITHER), patience_exits(store, t))    # unreachable threshold: PABEE
        assert np.array_equal(either, np.minimum(plain, patience_exits(store, t)))               # the minimum of the two, by construction
        streak = rule_exits(crit, store, thr, t, STREAK)
        assert np.all(streak >= plain)                                                           # waiting for a streak never leaves earlier
        if t > 1:
            assert np.all(streak >= rule_exits(crit, store, thr, t - 1, STREAK))
    assert 0 < int((rule_exits(crit, store, thr, 2, STREAK) != plain).sum())
    # entropy-like sign: the same exits on the negated table
    assert np.array_equal(rule_exits(-crit, store, -thr, 2, STREAK, sign=-1), rule_exits(crit, store, thr, 2, STREAK))


def test_restatement_policy_and_sweep_agree():
    store, crit, thr, refs = _random_case(7)
    E1, N = crit.shape
    thrs = np.stack([thr, np.full(E1, 2.0), np.full(E1, np.nan), np.quantile(crit, 0.3, axis=1)])
    pats = [1, 2, 3, E1, E1 + 1]
    for rule in (STREAK, EITHER):
        hits, sums, hist = rule_sweep(crit, store, refs, thrs, pats, rule)
        for v in range(len(thrs)):
            for j, t in enumerate(pats):
                ex, pred, conf, counts = rule_policy(crit, store, thrs[v], t, rule)
                assert np.array_equal(hist[v, j], counts) and sums[v, j] == ex.sum()
                assert hits[v, j] == int((pred.argmax(-1) == refs).sum())
                assert np.array_equal(conf, crit[ex, np.arange(N)])
        assert np.all(hist[2, :, -1] == N) if rule == STREAK else True      # NaN thresholds: nobody leaves on the test


def test_config_parses_exit_rule_and_patience(pkg):
    assert [pkg.ExitRule(n).code for n in ("plain", "patient_confident", "patience_or_threshold")] == [0, 1, 2]
    assert (pkg.capi.RULE_PLAIN, pkg.capi.RULE_STREAK, pkg.capi.RULE_EITHER) == (0, 1, 2)
    ec = pkg.ExitConfig()
    assert str(ec.exit_rule) == "plain" and ec.as_dict()["exit_rule"] == "plain"
    ec = pkg.ExitConfig(exits=[1, 2], exit_rule="patient_confident", patience=2)
    assert str(ec.exit_rule) == "patient_confident" and ec.patience == 2
    ec = pkg.ExitConfig(exits=["text_avg", 1, 2], exit_rule="patience_or_threshold", patience=[1, 2, 3, 1], inference_strategy="entropy")
    assert ec.patience == [1, 2, 3, 1] and ec.as_dict()["patience"] == [1, 2, 3, 1] and ec.as_dict()["exit_rule"] == "patience_or_threshold"
    ec = pkg.ExitConfig(exits=[1, 2], inference_strategy="patience", patience=[1, 2, 1])       # per-exit patience under PABEE itself
    assert ec.patience == [1, 2, 1]
    with pytest.raises(ValueError, match="valid ExitRule"):
        pkg.ExitConfig(exit_rule="both")
    for rule in ("patient_confident", "patience_or_threshold"):
        with pytest.raises(ValueError, match="threshold test"):
            pkg.ExitConfig(exits=[1, 2], inference_strategy="patience", patience=2, exit_rule=rule)
    for bad in ([1, 2], [1, 2, 3, 4], [1, 0, 1], [1, 1.5, 1], [1, True, 1], [], "121"):
        with pytest.raises(ValueError):
            pkg.ExitConfig(exits=[1, 2], exit_rule="patient_confident", patience=bad)
    assert pkg.ExitConfig(exits=[1, 2], patience=np.array(2)).patience == 2                     # a 0-d array is one value ...
    assert pkg.ExitConfig(exits=[1, 2], patience=np.array([1, 2, 1])).patience == [1, 2, 1]
    with pytest.raises(ValueError):
        pkg.ExitConfig(exits=[1, 2], patience=np.array(1.5))                                    # ... refused like one
    cfg = pkg.ModelConfig.tiny(EE_config=dict(exits=[1, 3], exit_rule="patient_confident", patience=[2, 1, 1]))
    back = pkg.ModelConfig.from_hf_dict(cfg.to_hf_dict())
    assert back.EE_config["patience"] == [2, 1, 1] and back.exit_config.patience == [2, 1, 1]
    assert str(back.exit_config.exit_rule) == "patient_confident"


def test_policy_and_sweep_entry_points_and_argument_errors(pkg):
    for name in ("patient_confident_policy", "patience_or_threshold_policy"):
        assert callable(getattr(pkg.Policy, name))
        with pytest.raises(ValueError, match="patience"):
            getattr(pkg.Policy(np.zeros((2, 3, 4)), {"exit_policy": name, "exit_threshold": 0.5}), name)()
        with pytest.raises(ValueError, match="exit_threshold"):
            getattr(pkg.Policy(np.zeros((2, 3, 4)), {"exit_policy": name, "patience": 1}), name)()
    assert callable(pkg.sweep.rule_sweep) and callable(pkg.rule_scan_device)
    with pytest.raises(ValueError, match="plain"):
        pkg.rule_scan_device(np.zeros((2, 3)), np.zeros((2, 3, 4)), 0.5, 1, "plain")
    with pytest.raises(ValueError):
        pkg.rule_scan_device(np.zeros((2, 3)), np.zeros((2, 3, 4)), 0.5, 1, "patient_confident", sign=0.5)
    with pytest.raises(ValueError):
        pkg.sweep.rule_sweep(np.zeros((2, 3)), np.zeros((2, 3, 4)), np.zeros(3), np.zeros((1, 2)), [1], "plain")


def test_header_declares_the_rules():
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    for name, v in (("PLAIN", 0), ("STREAK", 1), ("EITHER", 2)):
        assert re.search(rf"MMEE_RULE_{name}\s*=\s*{v}", header)
    declared = set(re.findall(r"\b(ee_[a-z_0-9]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared


def test_header_with_the_rules_compiles_as_c():
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "mmee.h"\n'
                    'int main(void) {\n'
                    '    int (*a)(ee_handle*, int32_t) = ee_set_exit_rule;\n'
                    '    int (*b)(ee_handle*, const int32_t*, int32_t) = ee_set_patience_vector;\n'
                    '    int (*c)(const double*, double, const double*, int32_t, int32_t, int32_t, const double*, const int32_t*, int32_t, int32_t*,'
                    ' double*, double*, int32_t*, void*) = ee_rule_scan;\n'
                    '    int (*d)(const double*, const double*, const int64_t*, int32_t, int32_t, int32_t, const double*, int32_t, const int32_t*,'
                    ' int32_t, int32_t, double*, double*, int32_t*, void*) = ee_rule_sweep;\n'
                    '    (void)a; (void)b; (void)c; (void)d;\n'
                    '    return MMEE_RULE_PLAIN != 0 || MMEE_RULE_STREAK != 1 || MMEE_RULE_EITHER != 2;\n'
                    '}\n')
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def test_library_exports_the_rule_symbols(pkg):
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
