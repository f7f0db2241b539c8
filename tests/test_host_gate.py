"""CPU checks of the gate decision (``EE_config["inference_strategy"] = "gate"``, include/mmee.h MMEE_CRIT_GATE): the numpy restatement of
tests/gate_ref.py on hand-computed cases, the configuration surface and its refusals, ``Policy.gate_policy``'s argument checks, and the
C-ABI (header declarations, plain-C compile, the symbols the built library exports)."""
import operator
import os
import re

import numpy as np
import pytest

from . import gate_ref as G
from .conftest import ROOT
from .fit_util import compiles_as_c, exported_symbols

GATE_EE = dict(exits=["text_avg", 1, 2], encoder_layer_strategy="gate", inference_strategy="gate")
NEW_SYMBOLS = ("ee_gate_table", "ee_gate_scan", "ee_head_fit_gate", "ee_debug_head_gate_lossgrad")


# ---- the restatement on hand-computed cases -------------------------------------------------------------------------------------------------
def test_score_is_exact_where_the_arithmetic_is():
    h = np.array([[1.25, 1.25], [-3.0, -3.0], [800.0, 0.0], [0.0, 800.0], [400.0, -400.0], [-400.0, 400.0]], np.float32)
    g = G.gate_score(h)
    assert g.dtype == np.float64
    assert g.tolist() == [0.5, 0.5, 0.0, 1.0, 0.0, 1.0]         # h0 == h1: 1 / (1 + 1); exp(800) = inf: 1 / inf; exp(-800) = 0: 1 / 1
    # column 1 is "correctly gated": raising h1 raises the score
    assert G.gate_score(np.array([0.0, 1.0], np.float32)) > 0.5 > G.gate_score(np.array([1.0, 0.0], np.float32))
    assert G.gate_score(np.array([0.0, 1.0], np.float32)) == 1.0 / (1.0 + np.exp(-1.0))
    assert np.isnan(G.gate_score(np.array([np.nan, 0.0], np.float32)))
    # the widening happens BEFORE the subtraction: two float32 whose float32 difference rounds
    a, b = np.float32(16777216.0), np.float32(1.0)
    assert G.gate_score(np.array([b, a])) == 1.0 / (1.0 + np.exp(1.0 - 16777216.0))


def test_the_test_is_strict_and_a_nan_never_fires():
    g = G.gate_score(np.array([[0.0, 0.0], [800.0, 0.0], [0.0, 800.0]], np.float32))      # 0.5, 0, 1
    below = np.nextafter(0.5, 0.0)
    assert G.fires(g, 0.5).tolist() == [False, False, True]     # g == thr stays
    assert G.fires(g, below).tolist() == [True, False, True]
    assert G.fires(g, 0.0).tolist() == [True, False, True]      # 0 > 0 is false
    assert G.fires(g, 1.0).tolist() == [False, False, False]    # 1 > 1 is false
    assert not G.fires(np.array([np.nan]), 0.0)[0] and not G.fires(np.array([0.9]), np.nan)[0]


def test_exits_take_the_first_gate_that_fires_and_the_last_row_is_the_fallback():
    head = np.zeros((3, 4, 2), np.float32)
    head[0, :, 1] = [2.0, -2.0, -2.0, 0.0]                      # g = .88, .12, .12, .5
    head[1, :, 1] = [2.0, 2.0, -2.0, 0.0]
    head[2, :, 1] = [-2.0, 2.0, -2.0, 0.0]
    final = np.array([[5.0, 0.0], [0.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    t = G.gate_table(head, final)
    assert t.shape == (4, 4) and t[3].tolist() == [1.0 / (1.0 + np.exp(-5.0)), 0.5, 1.0 / (np.exp(-1.0) + 1.0), 0.5]
    assert G.gate_exits(t, 0.5).tolist() == [0, 1, 3, 3]         # document 3 sits ON the threshold everywhere: the final exit
    assert G.gate_exits(t, [0.9, 0.5, 0.5, 2.0]).tolist() == [1, 1, 3, 3]      # the final exit's own entry is never read
    assert G.gate_exits(t, 1.0).tolist() == [3, 3, 3, 3] and G.gate_exits(t, -1.0).tolist() == [0, 0, 0, 0]
    logits = np.arange(4 * 4 * 2, dtype=np.float64).reshape(4, 4, 2)
    ex, pred, conf, counts = G.gate_scan(t, logits, 0.5)
    assert np.array_equal(pred, logits[[0, 1, 3, 3], np.arange(4)]) and counts.tolist() == [1, 1, 0, 2]
    assert conf.tolist() == [t[0, 0], t[1, 1], t[3, 2], t[3, 3]]


def test_one_stage_applies_the_rules_to_the_gate_event_and_the_final_exit_has_no_gate():
    stage = dict(n=4, doc_orig=np.array([5, 0, 3, 1]))
    z = np.array([[1.0, 3.0], [2.0, 0.0], [0.5, 0.5], [0.0, 9.0]], np.float32)
    h = np.array([[0.0, 2.0], [0.0, -2.0], [0.0, 2.0], [0.0, 0.0]], np.float32)
    r = G.decide(stage, z, h, thr=0.5, temp=2.0, B=6)
    assert r["leave"].tolist() == [True, False, True, False] and np.array_equal(r["crit"], G.gate_score(h)) and np.array_equal(r["head_crit"], r["crit"])
    assert np.array_equal(r["scaled32"], (z.astype(np.float64) / 2.0).astype(np.float32))
    # the temperature scales what leaves, never the score
    assert np.array_equal(G.decide(stage, z, h, thr=0.5, temp=0.25, B=6)["crit"], r["crit"])
    prev, run = np.zeros(6, np.int64), np.zeros(6, np.int64)
    run[[5, 3]] = (1, 0)
    s = G.decide(stage, z, h, thr=0.5, temp=1.0, rule=G.STREAK, patience=2, exit_index=1, B=6, state=(prev, run))
    assert s["leave"].tolist() == [True, False, False, False] and s["state"][1][[5, 0, 3, 1]].tolist() == [2, 0, 1, 0]
    prev[[0, 1]], run[[0, 1]] = (0, 1), (1, 0)
    e = G.decide(stage, z, h, thr=0.5, temp=1.0, rule=G.EITHER, patience=2, exit_index=1, B=6, state=(prev, run))
    assert e["leave"].tolist() == [True, True, True, False]      # document 1 by agreement (run 2), 0 and 2 by their gates
    f = G.decide(stage, z, h, thr=0.5, temp=2.0, B=6, is_final=True)
    assert f["leave"].all() and np.array_equal(f["crit"], G.max_softmax(z.astype(np.float64) / 2.0))
    assert not G.decide(stage, z, h, thr=0.5, temp=2.0, B=6, no_exit=True)["leave"].any()


def test_midpoint_thresholds_keep_their_distance():
    s = np.array([0.1, 0.1 + 1e-13, 0.4, 0.4000001, 0.9])
    thr, dist = G.midpoint_threshold(s, 0.5)
    assert 0.1 + 1e-13 < thr < 0.4 and dist > 0.1
    G.assert_clear(s, thr)
    with pytest.raises(AssertionError):
        G.assert_clear(s, 0.4 + 1e-13)


def test_objective_is_bce_with_logits_on_the_one_hot_and_its_gradient_is_right():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(0)
    N, H, l2 = 37, 5, 0.03
    X = rng.standard_normal((N, H)).astype(np.float32)
    c = np.where(rng.random(N) < 0.5, rng.random(N), (rng.random(N) < 0.6).astype(np.float64))
    theta = rng.standard_normal(2 * H + 2) * 0.7
    loss, grad = G.gate_lossgrad(theta, X, c, l2)
    W, b = torch.tensor(theta[:2 * H].reshape(2, H), requires_grad=True), torch.tensor(theta[2 * H:], requires_grad=True)
    z = torch.from_numpy(X).double() @ W.T + b
    y = torch.stack([torch.from_numpy(1.0 - c), torch.from_numpy(c)], 1)
    ref = torch.nn.BCEWithLogitsLoss()(z, y) + 0.5 * l2 * ((W ** 2).sum() + (b ** 2).sum())
    ref.backward()
    ref = float(ref.detach())
    assert abs(loss - ref) <= 1e-14 * max(1.0, abs(ref))
    np.testing.assert_allclose(grad, np.concatenate([W.grad.numpy().reshape(-1), b.grad.numpy()]), rtol=1e-12, atol=1e-15)
    assert np.isfinite(G.gate_lossgrad(theta * 1e3, X, c, l2)[0])           # softplus does not overflow
    assert G.softplus(np.array([800.0, -800.0, 0.0])).tolist() == [800.0, 0.0, np.log(2.0)]


# ---- configuration --------------------------------------------------------------------------------------------------------------------------
def test_gate_strategy_round_trips_through_the_configuration(pkg):
    st = pkg.EarlyExitInference("gate")
    assert st is pkg.EarlyExitInference.GATE and str(st) == "gate" and st.code == 4 == pkg.capi.CRIT_GATE and st.get_sign() is operator.gt
    assert [pkg.EarlyExitInference(n).code for n in ("max_confidence", "entropy", "patience", "margin")] == [0, 1, 2, 3]
    ec = pkg.ExitConfig(**GATE_EE)
    assert ec.inference_strategy is st and ec.as_dict()["inference_strategy"] == "gate" and ec.as_dict()["encoder_layer_strategy"] == "gate"
    cfg = pkg.ModelConfig.tiny(EE_config=dict(GATE_EE))
    hf = cfg.to_hf_dict()
    assert hf["EE_config"]["inference_strategy"] == "gate"
    back = pkg.ModelConfig.from_hf_dict(hf)
    assert back.exit_config.inference_strategy is st and back.exit_config.as_dict() == cfg.exit_config.as_dict()
    assert pkg.ExitConfig(**dict(GATE_EE, exit_rule="patient_confident", patience=2)).exit_rule.code == 1      # the rules take the gate event


def test_gate_strategy_is_refused_without_gate_heads_and_with_lte(pkg):
    with pytest.raises(ValueError, match='needs encoder_layer_strategy "gate"'):
        pkg.ExitConfig(exits=[1, 2], encoder_layer_strategy="ramp", inference_strategy="gate")
    with pytest.raises(ValueError, match='needs encoder_layer_strategy "gate"'):
        pkg.ExitConfig(exits=[1, 2], inference_strategy="gate")             # the default strategy is ramp
    with pytest.raises(ValueError, match="two exit decisions"):
        pkg.ExitConfig(**dict(GATE_EE, use_lte=True))
    with pytest.raises(ValueError, match='needs encoder_layer_strategy "gate"'):
        pkg.ModelConfig.tiny(EE_config=dict(exits=[1], encoder_layer_strategy="ramp", inference_strategy="gate")).exit_config
    # the gate score is no function of a policy logits row: the row-criterion tools keep refusing it
    with pytest.raises(ValueError, match="threshold criterion"):
        pkg.policy.threshold_criterion("gate")


def test_gate_policy_checks_its_arguments(pkg):
    logits = np.zeros((3, 4, 5))
    assert callable(pkg.Policy.gate_policy) and callable(pkg.policy.gate_scan_device) and callable(pkg.sweep.gate_table)
    with pytest.raises(ValueError, match="gate_scores"):
        pkg.Policy(logits, {"exit_policy": "gate_policy", "exit_threshold": 0.5}).gate_policy()
    with pytest.raises(ValueError, match="exit_thresholds"):
        pkg.Policy(logits, {"exit_policy": "gate_policy", "gate_scores": np.zeros((3, 4))}).gate_policy()
    with pytest.raises(ValueError, match=r"shape \(2, 4\)"):
        pkg.Policy(logits, {"exit_policy": "gate_policy", "gate_scores": np.zeros((2, 4)), "exit_threshold": 0.5}).gate_policy()


def test_fit_surface_exists_and_points_gates_at_their_own_fit(pkg):
    H = pkg.heads
    assert callable(H.fit_gate_heads) and callable(H.gate_targets) and callable(H.collect_gate_features)
    assert {"weight", "bias", "loss", "grad_norm", "evals", "status"} <= set(H.GateFit.__dataclass_fields__)
    with pytest.raises(ValueError, match="sample_weight"):
        H.fit_gate_heads(np.zeros((1, 4, 4), np.float32), np.zeros((1, 4)), sample_weight=np.ones((1, 4)))
    with pytest.raises(ValueError, match=r"H <= 1024"):
        H.fit_gate_heads(np.zeros((1, 4, 1028), np.float32), np.zeros((1, 4)))
    with pytest.raises(ValueError, match=r"\(E,N\)"):
        H.fit_gate_heads(np.zeros((2, 4, 8), np.float32), np.zeros((1, 4)))
    with pytest.raises(ValueError, match="l2"):
        H.fit_gate_heads(np.zeros((1, 4, 8), np.float32), np.zeros((1, 4)), l2=0.0)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_gate_entry_points(pkg):
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    declared = set(re.findall(r"\b(ee_[a-z_0-9]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg.capi.SYMBOLS, name
    assert re.search(r"MMEE_CRIT_GATE\s*=\s*4\b", header)
    assert int(re.search(r"#define\s+MMEE_ABI_VERSION\s+(\d+)", header).group(1)) == pkg.capi.ABI_VERSION      # no struct changed


def test_header_with_the_gate_compiles_as_c():
    compiles_as_c('    int (*a)(const float*, const double*, int32_t, int32_t, int32_t, double*, void*) = ee_gate_table;\n'
                  '    int (*b)(const double*, const double*, int32_t, int32_t, int32_t, const double*, int32_t*, double*, double*, int32_t*, void*) = ee_gate_scan;\n'
                  '    (void)a; (void)b;\n'
                  '    return !(MMEE_CRIT_GATE == 4 && MMEE_CRIT_MARGIN == 3);\n')


def test_library_exports_the_gate_entry_points(pkg):
    """Read the built library's dynamic symbol table (no GPU, no loading)."""
    exported = exported_symbols(pkg.capi.lib_path())
    for name in NEW_SYMBOLS:
        assert name in exported, name
