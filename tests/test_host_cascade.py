"""Model cascades (include/mmee.h, behind MMEE_QUOTA_*), the parts that need no GPU: the threshold helpers, the cumulative cost table against
the restatement of tests/cascade_ref.py, the refusals of the three entry points, of the constructor and of ``forward`` that come before any
device call, and the restatement on a hand-worked case."""
import ctypes as C
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from . import cascade_ref as CR
from .conftest import DIT_EE, H256_KW, TINY_CASES

NEW_SYMBOLS = ("ee_cascade_select", "ee_cascade_gather", "ee_cascade_merge")


def _cfgs(pkg):
    ee = TINY_CASES["tiny_ramp"]
    return [pkg.ModelConfig.dit_tiny(EE_config=DIT_EE), pkg.ModelConfig.tiny(EE_config=ee),
            pkg.ModelConfig.tiny(EE_config=dict(exits=["text_visual_concat", 1, 2], encoder_layer_strategy="ramp"), **H256_KW)]


def _fake_engine(pkg, cfg, device="cuda:0", finalized=True):
    """An EarlyExitEngine that never saw a device: what the constructor and forward's argument checks look at."""
    eng = pkg.EarlyExitEngine.__new__(pkg.EarlyExitEngine)
    eng.cfg, eng.exit_config, eng.device = cfg, cfg.exit_config, device
    eng.E, eng.K, eng.beit, eng.use_lte = cfg.exit_config.num_exits, cfg.num_labels, cfg.arch == "beit", False
    eng.max_docs, eng._finalized, eng.lib, eng._h = 8, finalized, None, None
    return eng


def test_restatement_on_a_hand_worked_stage():
    rows = np.array([[4.0, 0.0], [0.1, 0.0], [np.nan, 0.0], [0.2, 0.0], [5.0, 0.0]], np.float32)
    c = CR.criteria(rows, "max_confidence")
    assert np.isnan(c[2]) and c[0] > 0.9 > c[1]
    # the final exit is 3: documents 0 and 4 are sure and stay, 1 is unsure, 2 is NaN (never fires), 3 is unsure but left earlier, at exit 1
    ex = np.array([3, 3, 3, 1, 3])
    assert CR.select(c, ex, 3, 0.9, "max_confidence").tolist() == [1, 2]
    assert CR.select(c, ex, 3, 0.9, "max_confidence", orig=[10, 20, 30, 40, 50]).tolist() == [20, 30]
    # entropy: lower is surer, the direction flips
    h = CR.criteria(rows, "entropy")
    assert CR.select(h, ex, 3, 0.3, "entropy").tolist() == [1, 2]
    out = (np.zeros((4, 2), np.float32), np.zeros(4, np.int32), np.zeros(4, np.float32), np.zeros(4, np.int32))
    lg, e, cf, st = CR.merge(out, (np.ones((2, 2), np.float32), np.array([0, 2]), np.array([0.5, 0.25], np.float32)), [1, 3], 5, 1)
    assert e.tolist() == [0, 5, 0, 7] and st.tolist() == [0, 1, 0, 1] and lg[:, 0].tolist() == [0, 1, 0, 1] and cf.tolist() == [0, 0.5, 0, 0.25]
    assert out[1].tolist() == [0, 0, 0, 0]
    assert CR.global_exits([0, 1, 2], [4, 0, 3], [5, 8, 4]).tolist() == [4, 5, 16]


def test_flat_and_split_thresholds_round_trip(pkg):
    cfgs = _cfgs(pkg)
    e1 = [c.exit_config.num_exits + 1 for c in cfgs]
    assert e1 == [5, 8, 4]
    per = [np.linspace(0.1 * (s + 1), 0.9, n) for s, n in enumerate(e1)]
    flat = pkg.cascade.flat_thresholds(per)
    assert flat.dtype == np.float64 and flat.shape == (17,)
    for how in (cfgs, e1):
        back = pkg.cascade.split_thresholds(flat, how)
        assert len(back) == 3 and all(np.array_equal(a, b) for a, b in zip(back, per))
    assert np.array_equal(pkg.cascade.flat_thresholds(pkg.cascade.split_thresholds(flat, e1)), flat)
    with pytest.raises(ValueError, match="17"):
        pkg.cascade.split_thresholds(flat[:-1], e1)
    with pytest.raises(ValueError):
        pkg.cascade.flat_thresholds([])


def test_exit_costs_are_the_stages_costs_plus_the_final_rows_before(pkg):
    cfgs = _cfgs(pkg)
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 49, 11)
    mask = (np.arange(48)[None, :] < rows[:, None]).astype(np.int64)
    for kw in (dict(text_rows=rows), dict(attention_mask=mask)):
        for unit in (1e3, 1e6):
            got = pkg.cascade.exit_costs(cfgs, unit=unit, **kw)
            per = [pkg.sweep.exit_costs(c, unit=unit, **kw) for c in cfgs]
            want = CR.cumulative_costs(per)
            assert got.dtype == np.uint32 and got.shape == (17, 11) and np.array_equal(got, want)
            # a stage's rows grow with the exit, and a later stage starts above the earlier one's end
            assert (np.diff(got.astype(np.int64), axis=0)[[4, 12]] > 0).all()
    assert np.array_equal(pkg.cascade.exit_costs(cfgs[:1], text_rows=rows), pkg.sweep.exit_costs(cfgs[0], text_rows=rows))
    # each stage fits 32 bits at this unit, their sum does not: the cascade's own check
    per = [pkg.sweep.exit_costs(c, text_rows=rows, unit=1.0).astype(np.int64) for c in cfgs[:2]]
    scale = float(per[1].max()) / float(2 ** 32 - 2)
    assert pkg.sweep.exit_costs(cfgs[1], text_rows=rows, unit=scale).max() < 2 ** 32
    with pytest.raises(ValueError, match="32 bits"):
        pkg.cascade.exit_costs(cfgs[:2], text_rows=rows, unit=scale)
    with pytest.raises(ValueError, match="32 bits"):
        pkg.cascade.exit_costs(cfgs, text_rows=rows, unit=1e-3)
    with pytest.raises(ValueError):
        pkg.cascade.exit_costs(cfgs)


def test_library_exports_the_three_entry_points(pkg):
    path = pkg.capi.lib_path()
    if not os.path.exists(path):
        pytest.fail(f"{path} is missing: build() first")
    tool = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    r = subprocess.run([tool, "-D", "--defined-only", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    exported = {ln.split()[-1] for ln in r.stdout.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert name in exported and name in pkg.capi.SYMBOLS, name
    assert pkg.capi.ABI_VERSION == 4


def test_entry_points_refuse_bad_arguments_before_any_device_call(pkg):
    """Plain integers stand in for device addresses: the pointers are never dereferenced."""
    lib = pkg.capi.load()
    p = C.c_void_p(4096)
    select = {
        "n < 0": (p, p, None, -1, 4, 3, 0, 0.5, p, p, None, None),
        "K = 0": (p, p, None, 5, 0, 3, 0, 0.5, p, p, None, None),
        "final_exit < 0": (p, p, None, 5, 4, -1, 0, 0.5, p, p, None, None),
        "null logits": (None, p, None, 5, 4, 3, 0, 0.5, p, p, None, None),
        "null exit_layer": (p, None, None, 5, 4, 3, 0, 0.5, p, p, None, None),
        "null next_orig": (p, p, None, 5, 4, 3, 0, 0.5, None, p, None, None),
        "null count": (p, p, None, 5, 4, 3, 0, 0.5, p, None, None, None),
        "null count at n = 0": (None, None, None, 0, 4, 3, 0, 0.5, None, None, None, None),
        "criterion patience": (p, p, None, 5, 4, 3, pkg.capi.CRIT_PATIENCE, 0.5, p, p, None, None),
        "criterion gate": (p, p, None, 5, 4, 3, 4, 0.5, p, p, None, None),
        "criterion -1": (p, p, None, 5, 4, 3, -1, 0.5, p, p, None, None),
    }
    for what, args in select.items():
        assert lib.ee_cascade_select(*args) != 0, what
        msg = pkg.capi.last_error()
        assert msg.startswith("ee_cascade_select:") and "no HIP device" not in msg, (what, msg)
        if "criterion" in what:
            assert "criterion" in msg, (what, msg)

    def descs(*rows):
        d = (pkg.capi.CascadeDesc * max(len(rows), 1))()
        for i, (src, dst, rb) in enumerate(rows):
            d[i].src, d[i].dst, d[i].row_bytes = src, dst, rb
        return d
    ok = (4096, 8192, 64)
    gather = {
        "nine arrays": (descs(*[ok] * 9), 9, p, p, 4, None),
        "n_arrays < 0": (descs(ok), -1, p, p, 4, None),
        "cap < 0": (descs(ok), 1, p, p, -1, None),
        "null descs": (None, 1, p, p, 4, None),
        "null slots": (descs(ok), 1, None, p, 4, None),
        "null count": (descs(ok), 1, p, None, 4, None),
        "row_bytes 6": (descs((4096, 8192, 6)), 1, p, p, 4, None),
        "row_bytes 0": (descs((4096, 8192, 0)), 1, p, p, 4, None),
        "row_bytes -8": (descs((4096, 8192, -8)), 1, p, p, 4, None),
        "null src": (descs((None, 8192, 64)), 1, p, p, 4, None),
        "null dst": (descs(ok, (4096, None, 64)), 2, p, p, 4, None),
        "src off by 2": (descs((4098, 8192, 64)), 1, p, p, 4, None),
    }
    for what, args in gather.items():
        assert lib.ee_cascade_gather(*args) != 0, what
        msg = pkg.capi.last_error()
        assert msg.startswith("ee_cascade_gather:") and "no HIP device" not in msg, (what, msg)
    merge = {
        "n < 0": (p, p, p, p, -1, 4, 0, 1, p, p, p, p, None),
        "K = 0": (p, p, p, p, 3, 0, 0, 1, p, p, p, p, None),
        "offset < 0": (p, p, p, p, 3, 4, -1, 1, p, p, p, p, None),
        "stage < 0": (p, p, p, p, 3, 4, 0, -1, p, p, p, p, None),
    }
    for i in (0, 1, 2, 3, 8, 9, 10, 11):
        a = [p, p, p, p, 3, 4, 0, 1, p, p, p, p, None]
        a[i] = None
        merge[f"null pointer {i}"] = tuple(a)
    for what, args in merge.items():
        assert lib.ee_cascade_merge(*args) != 0, what
        msg = pkg.capi.last_error()
        assert msg.startswith("ee_cascade_merge:") and "no HIP device" not in msg, (what, msg)


def test_constructor_refusals(pkg):
    cfgs = _cfgs(pkg)
    E = pkg.CascadeEngine
    a, b = _fake_engine(pkg, cfgs[0]), _fake_engine(pkg, cfgs[1])
    with pytest.raises(ValueError, match="two stages"):
        E([a])
    with pytest.raises(ValueError, match="two stages"):
        E([])
    with pytest.raises(pkg.capi.MMEEError, match="stage 1.*load_weights"):
        E([a, _fake_engine(pkg, cfgs[1], finalized=False)])
    with pytest.raises(ValueError, match="one device"):
        E([a, _fake_engine(pkg, cfgs[1], device="cuda:1")])
    other = pkg.ModelConfig.tiny(EE_config=TINY_CASES["tiny_ramp"], num_labels=cfgs[0].num_labels + 1)
    with pytest.raises(ValueError, match="num_labels"):
        E([a, _fake_engine(pkg, other)])
    mb = pkg.MicroBatchedEngine.__new__(pkg.MicroBatchedEngine)
    with pytest.raises(TypeError, match="MicroBatchedEngine"):
        E([a, mb])
    with pytest.raises(TypeError, match="EarlyExitEngine"):
        E([a, types.SimpleNamespace()])
    with pytest.raises(ValueError, match="threshold criterion"):
        E([a, b], defer_criterion="patience")
    with pytest.raises(ValueError, match="defer_criterion"):
        E([a, b], defer_criterion=["entropy", None, None])
    c = E([a, b, _fake_engine(pkg, cfgs[2])], defer_criterion=[None, "margin"])
    assert c.E1 == [5, 8, 4] and c.offsets == [0, 5, 13] and c.num_exits == 17
    assert [str(x.value) for x in c.defer_criterion] == ["max_confidence", "margin"]
    # an entropy handle defers on entropy; gate and patience handles on the max-softmax they report at the final exit
    ent = pkg.ModelConfig.tiny(EE_config=TINY_CASES["tiny_entropy_1layer_head"])
    gate = pkg.ModelConfig.tiny(EE_config=TINY_CASES["tiny_gate"])
    pat = pkg.ModelConfig.tiny(EE_config=dict(TINY_CASES["tiny_ramp"], inference_strategy="patience"))
    c = E([_fake_engine(pkg, ent), _fake_engine(pkg, gate), _fake_engine(pkg, pat), b])
    assert [str(x.value) for x in c.defer_criterion] == ["entropy", "max_confidence", "max_confidence"]


def test_forward_refusals_before_any_device_call(pkg):
    cfgs = _cfgs(pkg)
    c = pkg.CascadeEngine([_fake_engine(pkg, cfgs[0]), _fake_engine(pkg, cfgs[1])])
    with pytest.raises(NotImplementedError, match="streaming across stages"):
        c.forward_stream({})
    with pytest.raises(NotImplementedError, match="batch size depends on the data"):
        c.capture({})
    for flag in ("dump_all", "want_all", "want_head", "want_hidden_cls", "want_hidden_states", "want_attentions"):
        with pytest.raises(ValueError, match="CascadeEngine.dump"):
            c.forward({}, **{flag: True})
    for flag in ("out", "quotas", "_capture", "_stream", "patience"):
        with pytest.raises(ValueError, match="one handle's forward"):
            c.forward({}, **{flag: None})
    with pytest.raises(ValueError, match="one entry per stage"):
        c.forward([{}, {}, {}])
    with pytest.raises(ValueError, match="stage 0"):
        c.forward([lambda slots: {}, {}])
    with pytest.raises(ValueError, match=r"flat \(13,\)"):
        c.forward({}, thresholds=np.zeros(12))
    with pytest.raises(ValueError, match="stage 1 has 8 exits"):
        c.forward({}, thresholds=[np.zeros(5), np.zeros(7)])
    with pytest.raises(ValueError, match="temperatures"):
        c.forward({}, temperatures=np.ones(3))
