"""The vision-first call without a GPU: the numpy restatement of its two phases (tests/vision_first_ref.py) against the one-call scan on dumped
arrays, the OCR term of ``sweep.exit_costs`` and the host-side surface of the feature."""
import numpy as np
import pytest

from . import csf_ref
from . import vision_first_ref as VR
from .conftest import TINY_CASES, sweep_ref_inputs


@pytest.mark.parametrize("criterion", csf_ref.CRITERIA)
@pytest.mark.parametrize("n_leave", [0, 1, 37, 399, 400])
def test_the_two_phases_compose_to_the_one_call_scan(criterion, n_leave):
    """Exit 0's decision, the survivors' order, the merge and `stage` on a dumped (7, 400, 16) array: everything equals the one-call scan, the
    text source is asked once for exactly the survivors, and not at all when nobody survives."""
    store, _ = sweep_ref_inputs()
    table = csf_ref.csf(store, criterion)
    sign = csf_ref.SIGN[criterion]
    thr = csf_ref.gap_thresholds(table, 0.7 if sign > 0 else 0.3, 1e-9)[0]
    thr[0] = VR.threshold_for(table[0], n_leave, sign)
    ex, pred, conf, counts = csf_ref.scan(store, thr, criterion)
    assert counts[0] == n_leave
    calls = []
    got = VR.compose(store, thr, criterion, text_calls=calls)
    assert np.array_equal(got["exit_layer"], ex) and np.array_equal(got["logits"], pred) and np.array_equal(got["confidence"], conf)
    assert np.array_equal(got["stage"], (ex > 0).astype(np.int32)) and got["text_docs"] == 400 - n_leave
    if n_leave == 400:
        assert calls == []
    else:
        assert len(calls) == 1 and np.array_equal(calls[0], np.nonzero(ex > 0)[0]) and np.all(np.diff(calls[0]) > 0)


def test_phase_one_writes_the_leavers_and_nothing_else():
    store, _ = sweep_ref_inputs(N=50)
    table = csf_ref.csf(store, "max_confidence")
    thr0 = VR.threshold_for(table[0], 20)
    leave, surv, lg, ex, cf = VR.phase1(store, table, thr0)
    assert leave.sum() == 20 and np.array_equal(surv, np.nonzero(~leave)[0])
    assert np.array_equal(lg[leave], store[0, leave]) and (ex[leave] == 0).all() and np.array_equal(cf[leave], table[0, leave])
    assert np.isnan(lg[~leave]).all() and (ex[~leave] == -1).all() and np.isnan(cf[~leave]).all()
    nan_table = table.copy()
    nan_table[0, 3] = np.nan                                               # a NaN never fires: the document stays
    assert not VR.exit0_leaves(nan_table[0], -1.0)[3] and not VR.exit0_leaves(nan_table[0], 9.0, -1)[3]


def test_threshold_for_refuses_a_tie():
    with pytest.raises(AssertionError, match="closer"):
        VR.threshold_for(np.array([0.5, 0.5, 0.25]), 1)


# ---- exit_costs(ocr_cost=) ---------------------------------------------------------------------------------------------------------------
def _cfg(pkg, exits):
    return pkg.ModelConfig.tiny(EE_config=dict(exits=exits, encoder_layer_strategy="ramp", inference_strategy="max_confidence"))


ROWS = np.array([3, 17, 40, 0])


def test_exit_costs_default_is_the_old_table(pkg):
    for exits in (TINY_CASES["tiny_ramp"]["exits"], ["text_avg", 1, 3], [2]):
        cfg = _cfg(pkg, exits)
        old = pkg.sweep.exit_costs(cfg, text_rows=ROWS, unit=1e3)
        assert old.dtype == np.uint32
        assert np.array_equal(pkg.sweep.exit_costs(cfg, text_rows=ROWS, unit=1e3, ocr_cost=None), old)
        assert np.array_equal(pkg.sweep.exit_costs(cfg, text_rows=ROWS, unit=1e3, ocr_cost=0), old)


@pytest.mark.parametrize("ocr", [250, np.array([10, 0, 7000, 3])], ids=["scalar", "per_document"])
def test_exit_costs_adds_ocr_behind_vision_avg_only(pkg, ocr):
    with_vis = _cfg(pkg, TINY_CASES["tiny_ramp"]["exits"])
    old = pkg.sweep.exit_costs(with_vis, text_rows=ROWS, unit=1e3).astype(np.int64)
    new = pkg.sweep.exit_costs(with_vis, text_rows=ROWS, unit=1e3, ocr_cost=ocr)
    assert new.dtype == np.uint32 and new.shape == old.shape == (8, 4)
    assert np.array_equal(new[0], old[0])                                  # vision_avg itself needs no text
    assert np.array_equal(new[1:].astype(np.int64) - old[1:], np.broadcast_to(np.asarray(ocr), (7, 4)))
    for exits in (["text_avg", "text_visual_concat", 1], [1, 3]):         # no vision_avg: every exit needs the text, nothing to tell apart
        cfg = _cfg(pkg, exits)
        assert np.array_equal(pkg.sweep.exit_costs(cfg, text_rows=ROWS, unit=1e3, ocr_cost=ocr), pkg.sweep.exit_costs(cfg, text_rows=ROWS, unit=1e3))


def test_exit_costs_ocr_refusals_and_overflow(pkg):
    cfg = _cfg(pkg, TINY_CASES["tiny_ramp"]["exits"])
    with pytest.raises(ValueError, match="one entry per document"):
        pkg.sweep.exit_costs(cfg, text_rows=ROWS, ocr_cost=[1, 2, 3])
    with pytest.raises(ValueError, match="finite and >= 0"):
        pkg.sweep.exit_costs(cfg, text_rows=ROWS, ocr_cost=-1.0)
    with pytest.raises(ValueError, match="finite and >= 0"):
        pkg.sweep.exit_costs(cfg, text_rows=ROWS, ocr_cost=[0, np.nan, 0, 0])
    with pytest.raises(ValueError, match="32 bits"):
        pkg.sweep.exit_costs(cfg, text_rows=ROWS, unit=1e3, ocr_cost=float(1 << 32))
    with pytest.raises(ValueError, match="32 bits"):                       # the table's own overflow still raises
        pkg.sweep.exit_costs(cfg, text_rows=ROWS, unit=1e-3)


def test_the_ocr_priced_table_goes_into_the_efficiency_figures_unchanged(pkg):
    """With OCR priced, leaving at vision_avg is worth the OCR it avoids: the mean cost of a policy is the table's mean at the chosen exits."""
    cfg = _cfg(pkg, TINY_CASES["tiny_ramp"]["exits"])
    cost = pkg.sweep.exit_costs(cfg, text_rows=ROWS, unit=1e3, ocr_cost=5000).astype(np.float64)
    plain = pkg.sweep.exit_costs(cfg, text_rows=ROWS, unit=1e3).astype(np.float64)
    ex = np.array([0, 0, 3, 7])
    n = np.arange(4)
    assert cost[ex, n].mean() - plain[ex, n].mean() == 5000 * 0.5


# ---- the host-side surface ---------------------------------------------------------------------------------------------------------------
def test_the_binding_and_the_outputs_exist(pkg):
    assert "ee_forward_vision" in pkg.capi.SYMBOLS and "ee_debug_vision_pool" in pkg.capi.SYMBOLS
    assert len(pkg.capi.SYMBOLS["ee_forward_vision"][1]) == 12
    f = pkg.engine.VisionFirstOutput.__dataclass_fields__
    assert list(f) == ["logits", "exit_layer", "confidence", "stage", "text_docs"]
    assert list(pkg.engine.VisionPhase.__dataclass_fields__) == ["output", "survivors", "count"]


def test_micro_batches_and_cascades_refuse_the_call(pkg):
    with pytest.raises(NotImplementedError, match="no vision-first call"):
        pkg.MicroBatchedEngine.forward_vision_first(None, None, None)
    with pytest.raises(NotImplementedError, match="inside a cascade is not built"):
        pkg.CascadeEngine.forward_vision_first(None, None, None)
