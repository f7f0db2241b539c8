"""CPU checks of the cost-weighted threshold search (include/mmee.h ee_threshold_search_cost): the numpy restatement (tests/search_cost_ref.py)
against the plain search's on the golden fixture, the front's rules on literals, the C-ABI (header declaration, plain-C compile, the exported
symbol), every refusal of the entry point before it looks for a device, the Python surface's argument errors, the new ``select`` rules and
the path's cost model ``sweep.exit_costs``."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from . import search_cost_ref as RC
from . import search_ref as R
from .conftest import ROOT, load_golden


def test_unit_cost_reproduces_the_exit_index_front_on_the_golden_fixture():
    g = load_golden("sweep_ref")
    V = int(g["n_generated"])
    conf, correct, thr = g["conf"], g["correct"], g["thresholds"][:V]
    E1, N = conf.shape
    table = R.percentile_table(conf, 10)
    dg = np.zeros((V, E1), dtype=np.int64)
    for e in range(E1 - 1):
        dg[:, e] = (thr[:, e][:, None].view(np.int64) == table[e][None, :].view(np.int64)).argmax(1)
    ref = R.search(conf, correct, 10, R.MIXTURES, R.REFERENCE, V=V, mixtures=dg)
    cost = np.broadcast_to(np.arange(E1)[:, None], (E1, N))
    got = RC.search_cost(conf, correct, cost, 10, R.MIXTURES, R.REFERENCE, V=V, mixtures=dg)
    assert got["cost_sum"] == ref["exit_sum"].tolist() and all(type(c) is int for c in got["cost_sum"])
    f_sum, f_hits, f_vec = R.pareto_front(ref["hits"], ref["exit_sum"], N * (E1 - 1) + 1)
    assert len(f_vec) == 35
    assert got["front_cost_sum"] == f_sum.tolist() and got["front_exit_sum"] == f_sum.tolist()
    assert got["front_hits"] == f_hits.tolist() and got["front_vector"] == f_vec.tolist()


def test_cost_front_on_literals():
    # a tie on (cost, hits) goes to the lower index: vectors 1 and 3
    assert RC.cost_front([5, 7, 6, 7], [10, 12, 11, 12]) == ([10, 11, 12], [5, 6, 7], [0, 2, 1])
    # at equal hits the lower cost wins, whatever the index
    assert RC.cost_front([7, 7, 7], [30, 20, 25]) == ([20], [7], [1])
    # a vector with more hits and less cost removes the other; one with more hits at EQUAL cost does too (one of the two is strict)
    assert RC.cost_front([5, 9], [10, 8]) == ([8], [9], [1])
    assert RC.cost_front([5, 9], [10, 10]) == ([10], [9], [1])
    # more hits for more cost: both stay, ascending in cost and in hits
    assert RC.cost_front([9, 5], [2 ** 40, 3]) == ([3, 2 ** 40], [5, 9], [1, 0])
    # a single vector with zero hits is a front
    assert RC.cost_front([0], [0]) == ([0], [0], [0])


def test_header_declares_the_cost_search():
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    assert re.search(r"#define\s+MMEE_ABI_VERSION\s+4\b", header)           # one more function: ee_config is unchanged
    assert "ee_threshold_search_cost" in set(re.findall(r"\b(ee_[a-z_0-9]+)\s*\(", header))
    for text in ("cost_sum(v) = sum_n cost[exit(v, n)][n]", "(cost_sum, v) compared lexicographically", "LOWEST index"):
        assert text in header, text


def test_header_with_the_cost_search_compiles_as_c():
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "mmee.h"\n'
                    'int main(void) {\n'
                    '    int (*a)(const double*, const uint8_t*, const uint32_t*, int32_t, int32_t, int32_t, int32_t, int64_t, uint64_t, const uint8_t*,'
                    ' int32_t, double*, double*, double*, uint64_t*, int32_t*, uint64_t*, int32_t*, int32_t*, uint32_t*, double*, void*)'
                    ' = ee_threshold_search_cost;\n'
                    '    (void)a;\n'
                    '    return MMEE_ABI_VERSION != 4;\n'
                    '}\n')
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def test_library_exports_the_cost_search_symbol(pkg):
    """Read the built library's dynamic symbol table (no GPU, no loading)."""
    path = pkg.capi.lib_path()
    if not os.path.exists(path):
        pytest.fail(f"{path} is missing: build() first")
    tool = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    r = subprocess.run([tool, "-D", "--defined-only", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    exported = {ln.split()[-1] for ln in r.stdout.splitlines() if ln.strip()}
    assert "ee_threshold_search_cost" in exported and "ee_threshold_search_cost" in pkg.capi.SYMBOLS
    assert len(pkg.capi.SYMBOLS["ee_threshold_search_cost"][1]) == 22


def test_entry_point_refuses_bad_arguments_before_any_device_call(pkg):
    """Every refusal returns non-zero with a message that names the entry point and the reason.  The pointers are never dereferenced: plain
    integers stand in for device addresses."""
    lib = pkg.capi.load()
    p = C.c_void_p(4096)
    GRID, SAMPLED, MIX = pkg.capi.SEARCH_GRID, pkg.capi.SEARCH_SAMPLED, pkg.capi.SEARCH_MIXTURES
    POLICY = pkg.capi.SEARCH_POLICY

    def call(conf=p, correct=p, cost=p, E1=7, N=400, P=10, source=GRID, V=0, seed=42, mix=None, sem=POLICY, table=p, acc=None, mex=None, cs=None,
             fc=p, fk=p, fs=p, fh=p, fv=p, ft=p):
        return lib.ee_threshold_search_cost(conf, correct, cost, E1, N, P, source, V, seed, mix, sem, table, acc, mex, cs, fc, fk, fs, fh, fv, ft, None)

    cases = {
        "P = 1": (dict(P=1), "P = 1"),
        "P = 65": (dict(P=65), "P = 65"),
        "grid of 10^22": (dict(E1=23), "MMEE_SEARCH_SAMPLED"),
        "N = 2^24": (dict(N=1 << 24), "2^24"),
        "N = 0": (dict(N=0), "N = 0"),
        "E1 = 1": (dict(E1=1), "E1 = 1"),
        "E1 = 65": (dict(E1=65, source=SAMPLED, V=5), "E1 = 65"),
        "null conf": (dict(conf=None), "NULL"),
        "null correct": (dict(correct=None), "NULL"),
        "null cost": (dict(cost=None), "NULL"),
        "null table": (dict(table=None), "NULL"),
        "null front_count": (dict(fc=None), "NULL"),
        "null front_cost_sum": (dict(fk=None), "NULL"),
        "null front_exit_sum": (dict(fs=None), "NULL"),
        "null front_hits": (dict(fh=None), "NULL"),
        "null front_vector": (dict(fv=None), "NULL"),
        "null front_thresholds": (dict(ft=None), "NULL"),
        "V = 0 sampled": (dict(source=SAMPLED, V=0), "V = 0"),
        "V = 0 mixtures": (dict(source=MIX, V=0, mix=p), "V = 0"),
        "V = 2^32": (dict(source=SAMPLED, V=1 << 32), "2^32"),
        "mixtures without digits": (dict(source=MIX, V=5), "mixtures"),
        "unknown source": (dict(source=3), "source 3"),
        "unknown semantics": (dict(sem=2), "semantics 2"),
    }
    for what, (kw, needle) in cases.items():
        assert call(**kw) != 0, what
        msg = pkg.capi.last_error()
        assert msg.startswith("ee_threshold_search_cost:") and "no HIP device" not in msg, (what, msg)
        assert needle in msg, (what, msg)


def test_python_surface_argument_errors(pkg):
    z = np.zeros((3, 5, 4))
    refs = np.zeros(5, dtype=np.int64)
    ts = pkg.sweep.threshold_search
    with pytest.raises(ValueError, match="integer array"):
        ts(z, refs, cost=np.ones(3))                                  # a float dtype
    with pytest.raises(ValueError, match="2\\^32"):
        ts(z, refs, cost=np.array([0, -1, 2]))
    with pytest.raises(ValueError, match="2\\^32"):
        ts(z, refs, cost=np.array([0, 1 << 32, 2]))
    for shape in ((4,), (3, 4), (5, 3), (3, 5, 1), ()):
        with pytest.raises(ValueError, match="shape"):
            ts(z, refs, cost=np.zeros(shape, dtype=np.int64))
    with pytest.raises(ValueError, match="shape"):
        ts((np.zeros((3, 5)), np.zeros((3, 5), dtype=np.uint8)), cost=np.zeros((3, 6), dtype=np.int64))       # a precomputed pair: N from the table


def _results(pkg):
    common = dict(table=np.zeros((3, 4)), front_thresholds=np.array([[0.9, 0.8, 0.0], [0.5, 0.6, 0.0], [0.1, 0.2, 0.0]]),
                  front_accuracy=np.array([0.5, 0.7, 0.9]), front_mean_exit=np.array([1.0, 0.2, 1.8]), front_vector=np.array([3, 1, 7], dtype=np.uint32),
                  front_hits=np.array([5, 7, 9], dtype=np.int32), front_exit_sum=np.array([10, 2, 18], dtype=np.int32), num_vectors=16, num_samples=10,
                  source=pkg.capi.SEARCH_GRID)
    with_cost = pkg.sweep.SearchResult(front_cost_sum=np.array([20, 100, 2 ** 40], dtype=np.uint64),
                                       front_mean_cost=np.array([2.0, 10.0, 2 ** 40 / 10.0]), **common)
    return with_cost, pkg.sweep.SearchResult(**common)


def test_select_on_a_cost_result(pkg):
    res, plain = _results(pkg)
    assert plain.front_cost_sum is None and plain.front_mean_cost is None and plain.cost_sum is None      # the new fields default to None
    assert res.select(min_accuracy=0.6) == [0.5, 0.6, 0.0] and res.select_index(min_accuracy=0.5) == 0     # the cheapest that reaches it
    assert res.select(max_mean_cost=10.0) == [0.5, 0.6, 0.0] and res.select(max_mean_cost=9.99) == [0.9, 0.8, 0.0]
    assert res.select_index(max_mean_cost=1e30) == 2                                                        # the most accurate within the budget
    assert all(type(t) is float for t in res.select(max_mean_cost=2.0))
    for kw in (dict(), dict(min_accuracy=0.5, max_mean_cost=1.0), dict(max_mean_exit=1.0, max_mean_cost=1.0),
               dict(min_accuracy=0.5, max_mean_exit=1.0, max_mean_cost=1.0)):
        with pytest.raises(ValueError, match="exactly one"):
            res.select(**kw)
    with pytest.raises(ValueError, match="no front entry"):
        res.select(max_mean_cost=1.9)
    with pytest.raises(ValueError, match="no front entry"):
        res.select(min_accuracy=0.95)
    with pytest.raises(ValueError, match="max_mean_cost"):
        res.select(max_mean_exit=1.5)                                 # not monotone along a cost front: refused, with the pointer
    with pytest.raises(ValueError, match="cost"):
        plain.select(max_mean_cost=5.0)
    assert plain.select(max_mean_exit=5) == [0.1, 0.2, 0.0]


# ---- sweep.exit_costs: SURVEY 8a / 8d by formula --------------------------------------------------------------------------------------------
def test_exit_costs_at_the_base_shape(pkg):
    cfg = pkg.ModelConfig.base(EE_config=dict(exits=[2, 4, 6, 8, 10], encoder_layer_strategy="ramp"))
    mask = np.ones((1, 512), dtype=np.int64)
    c = pkg.sweep.exit_costs(cfg, mask, unit=1e6)
    assert c.shape == (6, 1) and c.dtype == np.uint32
    assert abs(float(c[-1, 0]) / 1e3 - 139.2) <= 0.1                  # GF: 12 layers of 11.58 + 0.23 of patches
    assert abs(float(c[2, 0]) / 1e3 - 69.7) <= 0.1                    # the exit behind layer 6
    assert np.array_equal(c, pkg.sweep.exit_costs(cfg, text_rows=[512], unit=1e6))
    H, I, K, S = 768, 3072, 16, 512 + 197
    want = [2 * 196 * 768 * H + l * (2 * S * (4 * H * H + 2 * H * I) + 4 * S * S * H) + (e + 1) * (2 * H * H + 2 * H * K)
            for e, l in enumerate([2, 4, 6, 8, 10, 12])]
    assert c[:, 0].tolist() == [int(np.rint(w / 1e6)) for w in want]
    with pytest.raises(ValueError, match="unit"):
        pkg.sweep.exit_costs(cfg, mask, unit=1.0)                     # 1.4e11 FLOPs do not fit 32 bits
    with pytest.raises(ValueError, match="exactly one"):
        pkg.sweep.exit_costs(cfg)


def test_exit_costs_ragged_rows_and_embedding_exits(pkg):
    cfg = pkg.ModelConfig.base(EE_config=dict(exits=["vision_avg", "text_visual_concat", 2, 6], encoder_layer_strategy="ramp"))
    mask = np.zeros((3, 512), dtype=np.int64)
    mask[0, :16] = 1
    mask[1, :510] = 1
    mask[2, :16] = 1
    mask[2, 3:9] = 0                                                  # a hole: the packed layout keeps the prefix up to the last kept position
    c = pkg.sweep.exit_costs(cfg, mask, unit=1e3).astype(np.int64)
    assert c.shape == (5, 3)
    assert np.array_equal(c[:, 0], c[:, 2])
    assert (c[2:, 0] < c[2:, 1]).all()                                # 16 rows cost less than 510 at every encoder exit ...
    H, K = 768, 16
    head, patch = 2 * H * H + 2 * H * K, 2 * 196 * 768 * H
    for e in (0, 1):                                                  # ... and embedding-level exits cost the patch and head terms only
        assert c[e].tolist() == [int(np.rint((patch + (e + 1) * head) / 1e3))] * 3
    ratio = (c[4, 1] - c[1, 1]) / float(c[4, 0] - c[1, 0])            # six layers, 707 rows against 213: between the linear 3.3x and attention's 11x
    assert 3.3 < ratio < 11.0
    beit = pkg.ModelConfig.dit_base(EE_config=dict(exits=[2, 4], encoder_layer_strategy="ramp", inference_strategy="max_confidence"))
    b = pkg.sweep.exit_costs(beit, mask, unit=1e3)
    assert b.shape == (3, 3) and (b[:, 0] == b[:, 1]).all()           # image-only: every document has visual_len rows
