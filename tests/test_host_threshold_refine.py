"""CPU checks of the threshold refinement (include/mmee.h ee_threshold_refine): the two forms of the numpy restatement (tests/refine_ref.py:
every neighbour by a full walk against the per-document prefix / suffix argument) on the cases the GPU tests use and on ties, the C-ABI
(header declaration, plain-C compile, the exported symbol), every refusal of the entry point before it looks for a device, and the Python
surface: argument errors, the cross product of starts and hit values, ``front_hit_values``, ``RefineResult.front`` and ``select``."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from . import refine_ref as RR
from .conftest import ROOT


def _table(seed, E1, N):
    """tests/test_gpu_search_cost.py's synthetic confidence table: later exits surer and more often right."""
    rng = np.random.default_rng(seed)
    conf = rng.beta(2.0 + np.arange(E1)[:, None] * 1.5, 2.0, (E1, N))
    correct = (rng.random((E1, N)) < np.linspace(0.3, 0.9, E1)[:, None]).astype(np.uint8)
    return conf, correct


def _both(conf, correct, cost, P, start, w, budget=None, max_rounds=256):
    a = RR.refine(conf, correct, cost, P, start, w, budget, max_rounds)
    b = RR.refine(conf, correct, cost, P, start, w, budget, max_rounds, incremental=True)
    for k in ("digits", "hits", "exit_sum", "cost_sum", "rounds", "status", "start_hits", "start_cost_sum", "J", "start_J", "moves"):
        assert a[k] == b[k], k
    assert np.array_equal(a["thresholds"].view(np.int64), b["thresholds"].view(np.int64))
    return a


# ---- the restatement: brute force against the per-document argument ------------------------------------------------------------------------------
@pytest.mark.parametrize("E1,N,P,w", [(2, 1, 2, 3), (3, 17, 2, 2), (7, 300, 10, 4), (7, 300, 10, 0), (5, 120, 7, 2 ** 32 - 1), (12, 90, 5, 6)])
def test_the_two_forms_agree(E1, N, P, w):
    conf, correct = _table(5, E1, N)
    for start in ([P - 1] * E1, np.random.default_rng(8).integers(0, P, E1).tolist()):
        r = _both(conf, correct, None, P, start, w)
        assert r["J"] >= r["start_J"] and (r["J"] == r["start_J"]) == (r["rounds"] == 0)
        assert r["status"] == 0 and r["digits"][-1] == 0


def test_every_neighbour_of_one_vector_both_ways():
    """Not only the chosen move: all (E1 - 1) P neighbour scores, on a table with duplicated percentiles and confidences EQUAL to thresholds
    (two decimals), one exit row constant, and a cost that is not monotone in e."""
    conf, correct = _table(6, 6, 200)
    conf = np.round(conf, 2)
    conf[2] = 0.5
    cost = np.random.default_rng(3).integers(0, 2 ** 32, (6, 200))
    table = RR.R.percentile_table(conf, 8)
    assert any(len(set(table[e])) < 8 for e in range(5)) and (conf[:5, :, None] == table[:5, None, :]).any()
    for seed in range(4):
        d = np.random.default_rng(seed).integers(0, 8, 6).tolist()
        assert RR.neighbours_brute(conf, correct, cost, table, d, 8) == RR.neighbours_incremental(conf, correct, cost, table, d, 8)


def test_budget_statuses_and_one_round():
    conf, correct = _table(5, 7, 300)
    free = _both(conf, correct, None, 10, [9] * 7, 8)                 # from "nobody leaves early": mostly thresholds coming down
    assert free["rounds"] >= 3 and free["status"] == 0
    one = _both(conf, correct, None, 10, [9] * 7, 8, max_rounds=1)
    assert one["status"] == 1 and one["rounds"] == 1 and one["moves"] == free["moves"][:1]
    exact = _both(conf, correct, None, 10, [9] * 7, 8, max_rounds=free["rounds"])
    assert exact["status"] == 1 and exact["digits"] == free["digits"]        # moved in every round: 1, although nothing would follow
    # a start over its budget: status 2, the outputs describe the start
    over = _both(conf, correct, None, 10, [9] * 7, 8, budget=free["start_cost_sum"] - 1)
    assert over["status"] == 2 and over["rounds"] == 0 and over["cost_sum"] == free["start_cost_sum"] and over["hits"] == free["start_hits"]
    assert over["digits"] == [9] * 6 + [0]
    # a budget equal to the start's cost_sum admits the start and every neighbour that costs no more
    tight = _both(conf, correct, None, 10, [9] * 7, 8, budget=free["start_cost_sum"])
    assert tight["status"] == 0 and tight["rounds"] >= 1 and tight["cost_sum"] <= free["start_cost_sum"]
    # a budget in the way: the chain that wants to pay more for accuracy stops short of where it goes without one
    rich = _both(conf, correct, None, 10, [0] * 7, 16)
    assert rich["rounds"] >= 3 and all(p_to > p_from for _, p_from, p_to in rich["moves"])       # every move RAISES a threshold (e = x0 territory)
    mid = (rich["start_cost_sum"] + rich["cost_sum"]) // 2
    capped = _both(conf, correct, None, 10, [0] * 7, 16, budget=mid)
    assert capped["cost_sum"] <= mid < rich["cost_sum"] and capped["J"] < rich["J"] and capped["status"] == 0


def test_ties_go_to_the_lowest_exit_then_the_lowest_digit():
    """Two exits with identical rows: their neighbours score alike, and the chain must move on exit 0; duplicated thresholds on one exit: the
    lowest digit."""
    rng = np.random.default_rng(0)
    row = np.round(rng.random(60), 1)
    conf = np.stack([row, row, rng.random(60)])
    good = (rng.random(60) < 0.8).astype(np.uint8)
    correct = np.stack([good, good, np.zeros(60, dtype=np.uint8)])
    cost = np.array([[1] * 60, [1] * 60, [50] * 60])
    r = _both(conf, correct, cost, 6, [5, 5, 0], 1)
    assert r["rounds"] >= 1 and r["moves"][0][0] == 0
    table = r["table"]
    e, _, p = r["moves"][0]
    assert p == int(np.argmax(table[e] == table[e][p]))               # the first digit that carries this threshold


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_refinement():
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    assert re.search(r"#define\s+MMEE_ABI_VERSION\s+4\b", header)           # two more functions: ee_config is unchanged
    declared = set(re.findall(r"\b(ee_[a-z_0-9]+)\s*\(", header))
    assert "ee_threshold_refine" in declared and "ee_threshold_refine_workspace_bytes" in declared
    for text in ("J(d) = w hits(d) - cost_sum(d)", "ties to the lowest e, then the", "status 2, rounds 0", "MMEE_SEARCH_POLICY only"):
        assert text in header, text


def test_header_with_the_refinement_compiles_as_c():
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "mmee.h"\n'
                    'int main(void) {\n'
                    '    int (*a)(const double*, const uint8_t*, const uint32_t*, int32_t, int32_t, int32_t, int32_t, const uint8_t*, const uint64_t*,'
                    ' const uint64_t*, int32_t, uint8_t*, double*, int32_t*, int32_t*, uint64_t*, int32_t*, int32_t*, int32_t*, uint64_t*, double*, void*)'
                    ' = ee_threshold_refine;\n'
                    '    size_t (*b)(int32_t, int32_t, int32_t, int32_t) = ee_threshold_refine_workspace_bytes;\n'
                    '    (void)a; (void)b;\n'
                    '    return MMEE_ABI_VERSION != 4;\n'
                    '}\n')
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def test_library_exports_the_refinement(pkg):
    """Read the built library's dynamic symbol table (no GPU, no loading)."""
    path = pkg.capi.lib_path()
    if not os.path.exists(path):
        pytest.fail(f"{path} is missing: build() first")
    tool = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    r = subprocess.run([tool, "-D", "--defined-only", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    exported = {ln.split()[-1] for ln in r.stdout.splitlines() if ln.strip()}
    assert "ee_threshold_refine" in exported and "ee_threshold_refine_workspace_bytes" in exported
    assert len(pkg.capi.SYMBOLS["ee_threshold_refine"][1]) == 22 and len(pkg.capi.SYMBOLS["ee_threshold_refine_workspace_bytes"][1]) == 4


def test_workspace_bytes_is_a_pure_function(pkg):
    lib = pkg.capi.load()
    f = lib.ee_threshold_refine_workspace_bytes
    assert f(24, 40000, 10, 1) >= 24 * 40000 + 23 * 11 * 16
    assert f(24, 40000, 10, 64) - f(24, 40000, 10, 1) >= 63 * 23 * 11 * 16        # the difference arrays: S (E1-1) (P+1) x 16 bytes
    for bad in ((1, 10, 10, 1), (65, 10, 10, 1), (7, 0, 10, 1), (7, 1 << 24, 10, 1), (7, 10, 1, 1), (7, 10, 65, 1), (7, 10, 10, 0), (7, 10, 10, 4097)):
        assert f(*bad) == 0, bad


def test_entry_point_refuses_bad_arguments_before_any_device_call(pkg):
    """Every refusal returns non-zero with a message that names the entry point and the reason.  The pointers are never dereferenced: plain
    integers stand in for device addresses."""
    lib = pkg.capi.load()
    p = C.c_void_p(4096)

    def call(conf=p, correct=p, cost=None, E1=24, N=400, P=10, S=3, start=p, w=p, budget=None, max_rounds=16, digits=p):
        return lib.ee_threshold_refine(conf, correct, cost, E1, N, P, S, start, w, budget, max_rounds, digits, None, None, None, None, None, None,
                                       None, None, None, None)

    cases = {
        "P = 1": (dict(P=1), "P = 1"),
        "P = 65": (dict(P=65), "P = 65"),
        "N = 2^24": (dict(N=1 << 24), "2^24"),
        "N = 0": (dict(N=0), "N = 0"),
        "E1 = 1": (dict(E1=1), "E1 = 1"),
        "E1 = 65": (dict(E1=65), "E1 = 65"),
        "S = 0": (dict(S=0), "S = 0"),
        "S = 4097": (dict(S=4097), "S = 4097"),
        "max_rounds = 0": (dict(max_rounds=0), "max_rounds = 0"),
        "max_rounds = 4097": (dict(max_rounds=4097), "max_rounds = 4097"),
        "null conf": (dict(conf=None), "NULL"),
        "null correct": (dict(correct=None), "NULL"),
        "null start": (dict(start=None), "NULL"),
        "null hit_value": (dict(w=None), "NULL"),
        "null digits": (dict(digits=None), "NULL"),
    }
    for what, (kw, needle) in cases.items():
        assert call(**kw) != 0, what
        msg = pkg.capi.last_error()
        assert msg.startswith("ee_threshold_refine:") and "no HIP device" not in msg, (what, msg)
        assert needle in msg, (what, msg)


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------------------
def _search_result(pkg, **kw):
    base = dict(table=np.arange(12, dtype=np.float64).reshape(3, 4), front_thresholds=np.array([[0.0, 4.0, 0.0], [1.0, 5.0, 0.0], [3.0, 7.0, 0.0]]),
                front_accuracy=np.array([0.5, 0.7, 0.9]), front_mean_exit=np.array([0.2, 1.0, 1.8]), front_vector=np.array([0, 5, 15], dtype=np.uint32),
                front_hits=np.array([5, 7, 9], dtype=np.int32), front_exit_sum=np.array([2, 10, 18], dtype=np.int32), num_vectors=16, num_samples=10,
                source=pkg.capi.SEARCH_GRID, semantics="policy")
    base.update(kw)
    return pkg.sweep.SearchResult(**base)


def test_python_surface_argument_errors(pkg):
    z = np.zeros((3, 5, 4))
    refs = np.zeros(5, dtype=np.int64)
    tr = pkg.sweep.threshold_refine
    with pytest.raises(ValueError, match="hit_value"):
        tr(z, refs)
    with pytest.raises(ValueError, match="hit_value"):
        tr(z, refs, hit_value=-1)
    with pytest.raises(ValueError, match="hit_value"):
        tr(z, refs, hit_value=[1, 1 << 32])
    with pytest.raises(ValueError, match="integers"):
        tr(z, refs, hit_value=1.5)
    with pytest.raises(ValueError, match="references"):
        tr(z, hit_value=1)
    with pytest.raises(ValueError, match="num_per_exit"):
        tr(z, refs, hit_value=1, num_per_exit=65)
    with pytest.raises(ValueError, match="max_rounds"):
        tr(z, refs, hit_value=1, max_rounds=0)
    with pytest.raises(ValueError, match="start"):
        tr(z, refs, hit_value=1, start=np.zeros((2, 4), dtype=np.int64))      # E1 is 3
    with pytest.raises(ValueError, match="start"):
        tr(z, refs, hit_value=1, start=np.array([[0, 10, 0]]))               # a digit outside [0, P)
    with pytest.raises(ValueError, match="integers"):
        tr(z, refs, hit_value=1, start=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="4096"):
        tr(z, refs, hit_value=np.arange(70), start=np.zeros((60, 3), dtype=np.int64))
    with pytest.raises(ValueError, match="budget"):
        tr(z, refs, hit_value=[1, 2], budget=[1, 2, 3])                      # two chains
    with pytest.raises(ValueError, match="budget"):
        tr(z, refs, hit_value=1, budget=-1)
    with pytest.raises(ValueError, match="one argument"):
        tr(z, refs, hit_value=1, budget=5, budget_mean=0.5)
    with pytest.raises(ValueError, match="shape"):
        tr(z, refs, hit_value=1, cost=np.zeros((4,), dtype=np.int64))
    with pytest.raises(ValueError, match="2\\^32"):
        tr(z, refs, hit_value=1, cost=np.array([0, 1 << 32, 2]))
    # a SearchResult as the start: the table's shape and the semantics are checked before any device is looked for
    with pytest.raises(ValueError, match="table"):
        tr(z, refs, hit_value=1, num_per_exit=5, start=_search_result(pkg))
    with pytest.raises(ValueError, match="policy"):
        tr(z, refs, hit_value=1, num_per_exit=4, start=_search_result(pkg, semantics="reference"))
    with pytest.raises(ValueError, match="policy"):
        tr(z, refs, hit_value=1, num_per_exit=4, start=_search_result(pkg, semantics=None))


def test_front_hit_values(pkg):
    res = _search_result(pkg, front_cost_sum=np.array([20, 100, 2 ** 40], dtype=np.uint64), front_mean_cost=np.array([2.0, 10.0, 2 ** 40 / 10.0]))
    got = pkg.sweep.front_hit_values(res)
    assert got.dtype == np.uint64 and got.tolist() == [40, 2 ** 32 - 1]      # ceil(80 / 2); (2^40 - 100) / 2 clipped
    plain = pkg.sweep.front_hit_values(_search_result(pkg))                   # no costs: the exit sums, ceil(8 / 2), ceil(8 / 2)
    assert plain.tolist() == [4, 4]
    odd = _search_result(pkg, front_cost_sum=np.array([1, 8, 9], dtype=np.uint64), front_mean_cost=np.array([0.1, 0.8, 0.9]))
    assert pkg.sweep.front_hit_values(odd).tolist() == [4, 1]                 # ceil(7 / 2), ceil(1 / 2)
    assert pkg.sweep.front_hit_values(_search_result(pkg, front_hits=np.array([5], dtype=np.int32))).tolist() == []


def _refine_result(pkg):
    #        chain:    0    1    2    3    4    5
    hits = np.array([5, 7, 7, 9, 6, 9], dtype=np.int32)
    cost = np.array([20, 30, 30, 2 ** 40, 40, 2 ** 40], dtype=np.uint64)
    xsum = np.array([4, 9, 6, 30, 2, 30], dtype=np.int32)
    S = 6
    thr = np.arange(S * 3, dtype=np.float64).reshape(S, 3) / 100.0
    return pkg.sweep.RefineResult(table=np.zeros((3, 4)), digits=np.zeros((S, 3), dtype=np.uint8), thresholds=thr, hits=hits, exit_sum=xsum, cost_sum=cost,
                                  rounds=np.zeros(S, dtype=np.int32), status=np.zeros(S, dtype=np.int32), start_hits=hits - 1,
                                  start_cost_sum=cost, hit_value=np.array([2 ** 32 - 1] * S, dtype=np.uint64), num_samples=10)


def test_refine_result_front_select_and_j(pkg):
    r = _refine_result(pkg)
    assert r.front() == [0, 1, 3]                                     # chain 2 ties with 1, chain 4 costs more for fewer hits, chain 5 ties with 3
    assert all(type(j) is int for j in r.J + r.start_J)
    assert r.J[3] == (2 ** 32 - 1) * 9 - 2 ** 40 and r.start_J[3] == (2 ** 32 - 1) * 8 - 2 ** 40
    assert r.accuracy.tolist() == [0.5, 0.7, 0.7, 0.9, 0.6, 0.9] and r.mean_cost[1] == 3.0 and r.mean_exit[4] == 0.2
    assert r.select_index(min_accuracy=0.6) == 1 and r.select_index(min_accuracy=0.5) == 0 and r.select_index(min_accuracy=0.9) == 3
    assert r.select_index(max_mean_cost=3.0) == 1 and r.select_index(max_mean_cost=2.99) == 0 and r.select_index(max_mean_cost=1e30) == 3
    assert r.select_index(max_mean_exit=0.95) == 2                    # chains 0, 1, 2, 4 qualify: 7 hits twice, chain 2 has the lower mean exit
    thr = r.select(max_mean_cost=3.0)
    assert thr == r.thresholds[1].tolist() and all(type(t) is float for t in thr)
    for kw in (dict(), dict(min_accuracy=0.5, max_mean_cost=1.0), dict(max_mean_exit=1.0, max_mean_cost=1.0)):
        with pytest.raises(ValueError, match="exactly one"):
            r.select(**kw)
    for kw in (dict(min_accuracy=0.95), dict(max_mean_cost=1.9), dict(max_mean_exit=0.1)):
        with pytest.raises(ValueError, match="no chain"):
            r.select(**kw)
