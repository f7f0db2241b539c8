"""CPU checks of the threshold search (include/mmee.h ee_threshold_search): the numpy restatement (tests/search_ref.py) against the fixture
minted from the reference's own sweep (tests/golden/sweep_ref.npz), the digit hash on literals, the C-ABI (header declaration, plain-C
compile, the exported symbol), every refusal of the entry point before it looks for a device, and the Python surface's argument errors."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from . import search_ref as R
from .conftest import ROOT, load_golden

P_GOLDEN = 10


@pytest.fixture(scope="module")
def golden():
    g = load_golden("sweep_ref")
    V = int(g["n_generated"])
    conf, correct, thr = g["conf"], g["correct"], g["thresholds"][:V]
    E1 = conf.shape[0]
    table = R.percentile_table(conf, P_GOLDEN)
    dg = np.zeros((V, E1), dtype=np.int64)
    for e in range(E1 - 1):
        member = thr[:, e][:, None].view(np.int64) == table[e][None, :].view(np.int64)
        assert member.any(1).all(), e                                # every generated threshold IS a table value, bit for bit
        dg[:, e] = member.argmax(1)
    return dict(conf=conf, correct=correct, thr=thr, V=V, table=table, digits=dg, accuracy=g["accuracy"][:V], mean_exit=g["mean_exit"][:V])


def test_restatement_table_is_numpy_percentile_bit_for_bit(golden):
    conf, table = golden["conf"], golden["table"]
    E1 = conf.shape[0]
    want = np.stack([np.percentile(conf[e], np.linspace(0, 100, P_GOLDEN)) for e in range(E1 - 1)])
    assert np.array_equal(table[:E1 - 1].view(np.int64), want.view(np.int64))
    assert (table[E1 - 1] == 0).all()
    for N, P in ((1, 2), (2, 64), (257, 5), (400, 10), (1000, 7), (4100, 4)):       # the index arithmetic alone, at other shapes
        x = np.random.default_rng(N * 100 + P).standard_normal((2, N))
        assert np.array_equal(R.percentile_table(x, P)[0].view(np.int64), np.percentile(x[0], np.linspace(0, 100, P)).view(np.int64)), (N, P)


def test_restatement_reproduces_the_reference_sweep(golden):
    V, conf = golden["V"], golden["conf"]
    E1, N = conf.shape
    assert V == 1500
    ref = R.search(conf, golden["correct"], P_GOLDEN, R.MIXTURES, R.REFERENCE, V=V, mixtures=golden["digits"])
    assert np.array_equal(ref["thresholds"].view(np.int64), golden["thr"].view(np.int64))       # the digits rebuild the rows exactly
    assert np.array_equal(ref["hits"] / N, golden["accuracy"]) and np.array_equal(ref["exit_sum"] / N, golden["mean_exit"])
    assert np.array_equal(ref["hits"], np.rint(golden["accuracy"] * N)) and np.array_equal(ref["exit_sum"], np.rint(golden["mean_exit"] * N))
    assert len(ref["front_vector"]) == 35
    assert (np.diff(ref["front_exit_sum"]) > 0).all() and (np.diff(ref["front_hits"]) > 0).all()
    pol = R.search(conf, golden["correct"], P_GOLDEN, R.MIXTURES, R.POLICY, V=V, mixtures=golden["digits"])
    assert int(((pol["hits"] != ref["hits"]) | (pol["exit_sum"] != ref["exit_sum"])).sum()) == 835    # the two rules are really distinguished


def test_front_tie_rule_and_strictness():
    # vectors 1 and 3 tie on (exit_sum, hits): the lower index; vector 4 has more exits and no more hits: off the front
    hits, sums = np.array([5, 7, 6, 7, 7, 9]), np.array([10, 12, 12, 12, 13, 20])
    f_sum, f_hits, f_vec = R.pareto_front(hits, sums, 32)
    assert f_sum.tolist() == [10, 12, 20] and f_hits.tolist() == [5, 7, 9] and f_vec.tolist() == [0, 1, 5]
    f_sum, f_hits, f_vec = R.pareto_front(np.array([0]), np.array([0]), 1)       # zero hits at the lowest exit sum is still the front
    assert f_sum.tolist() == [0] and f_hits.tolist() == [0] and f_vec.tolist() == [0]


def test_digit_sources_on_literals(pkg):
    assert R.splitmix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF     # the first output of the published generator seeded with 0
    assert R.sampled_digit(0, 0, 0, 7, 10) == 8                       # = (0xE220A839 * 10) >> 32
    assert R.sampled_digit(42, 0, 0, 23, 10) == 7
    assert R.sampled_digit(42, 3000, 21, 23, 10) == 9
    assert R.sampled_digit(7, 123456789, 5, 23, 10) == 9
    assert R.digits(R.GRID, 125, 4, 5)[[0, 1, 5, 37, 124]].tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 1], [4, 4, 4]]
    assert R.digits(R.MIXTURES, 2, 3, 4, mixtures=np.array([[1, 9, 0], [3, 0, 7]])).tolist() == [[1, 3], [3, 0]]      # clamped to P - 1
    # the package's own digits (SearchResult.digits) follow the same rules
    for v in (0, 1, 3000, 2 ** 32 - 2):
        assert pkg.sweep.search_digits(pkg.capi.SEARCH_SAMPLED, v, 23, 10, seed=42) == [R.sampled_digit(42, v, e, 23, 10) for e in range(22)]
    assert pkg.sweep.search_digits(pkg.capi.SEARCH_GRID, 37, 4, 5) == [2, 2, 1]


def test_header_declares_the_search():
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    assert re.search(r"#define\s+MMEE_ABI_VERSION\s+4\b", header)           # one function and two enums: ee_config is unchanged
    for name, v in (("GRID", 0), ("SAMPLED", 1), ("MIXTURES", 2), ("REFERENCE", 0), ("POLICY", 1)):
        assert re.search(rf"MMEE_SEARCH_{name}\s*=\s*{v}\b", header), name
    assert "ee_threshold_search" in set(re.findall(r"\b(ee_[a-z_0-9]+)\s*\(", header))
    for text in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "hits << 32 | (0xFFFFFFFF - v)", "b - (b - a) * (1 - t)"):
        assert text in header, text


def test_header_with_the_search_compiles_as_c():
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "mmee.h"\n'
                    'int main(void) {\n'
                    '    int (*a)(const double*, const uint8_t*, int32_t, int32_t, int32_t, int32_t, int64_t, uint64_t, const uint8_t*, int32_t, double*,'
                    ' double*, double*, int32_t*, int32_t*, int32_t*, uint32_t*, double*, void*) = ee_threshold_search;\n'
                    '    (void)a;\n'
                    '    return MMEE_SEARCH_GRID != 0 || MMEE_SEARCH_SAMPLED != 1 || MMEE_SEARCH_MIXTURES != 2 || MMEE_SEARCH_REFERENCE != 0 ||'
                    ' MMEE_SEARCH_POLICY != 1 || MMEE_ABI_VERSION != 4;\n'
                    '}\n')
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def test_library_exports_the_search_symbol(pkg):
    """Read the built library's dynamic symbol table (no GPU, no loading)."""
    path = pkg.capi.lib_path()
    if not os.path.exists(path):
        pytest.fail(f"{path} is missing: build() first")
    tool = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    r = subprocess.run([tool, "-D", "--defined-only", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    exported = {ln.split()[-1] for ln in r.stdout.splitlines() if ln.strip()}
    assert "ee_threshold_search" in exported and "ee_threshold_search" in pkg.capi.SYMBOLS
    assert (pkg.capi.SEARCH_GRID, pkg.capi.SEARCH_SAMPLED, pkg.capi.SEARCH_MIXTURES) == (0, 1, 2)
    assert (pkg.capi.SEARCH_REFERENCE, pkg.capi.SEARCH_POLICY) == (0, 1)


def test_entry_point_refuses_bad_arguments_before_any_device_call(pkg):
    """Every refusal returns non-zero with a message that names the entry point and the reason.  The pointers are never dereferenced: plain
    integers stand in for device addresses."""
    lib = pkg.capi.load()
    p = C.c_void_p(4096)
    GRID, SAMPLED, MIX = pkg.capi.SEARCH_GRID, pkg.capi.SEARCH_SAMPLED, pkg.capi.SEARCH_MIXTURES
    POLICY = pkg.capi.SEARCH_POLICY

    def call(conf=p, correct=p, E1=7, N=400, P=10, source=GRID, V=0, seed=42, mix=None, sem=POLICY, table=p, acc=None, mex=None, fc=p, fs=p,
             fh=p, fv=p, ft=p):
        return lib.ee_threshold_search(conf, correct, E1, N, P, source, V, seed, mix, sem, table, acc, mex, fc, fs, fh, fv, ft, None)

    cases = {
        "P = 1": (dict(P=1), "P = 1"),
        "P = 65": (dict(P=65), "P = 65"),
        "grid of 10^22": (dict(E1=23), "MMEE_SEARCH_SAMPLED"),
        "N = 2^24": (dict(N=1 << 24), "2^24"),
        "N = 0": (dict(N=0), "N = 0"),
        "buckets": (dict(N=(1 << 24) - 1), "2^26"),
        "E1 = 1": (dict(E1=1), "E1 = 1"),
        "E1 = 65": (dict(E1=65, source=SAMPLED, V=5), "E1 = 65"),
        "null conf": (dict(conf=None), "NULL"),
        "null correct": (dict(correct=None), "NULL"),
        "null table": (dict(table=None), "NULL"),
        "null front_count": (dict(fc=None), "NULL"),
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
        assert msg.startswith("ee_threshold_search:") and "no HIP device" not in msg, (what, msg)
        assert needle in msg, (what, msg)


def test_python_surface_argument_errors(pkg):
    z = np.zeros((3, 5, 4))
    refs = np.zeros(5, dtype=np.int64)
    ts = pkg.sweep.threshold_search
    with pytest.raises(ValueError, match="threshold criterion"):
        ts(z, refs, criterion="patience")
    with pytest.raises(ValueError, match="semantics"):
        ts(z, refs, semantics="strict")
    for bad in (1, 65):
        with pytest.raises(ValueError, match="num_per_exit"):
            ts(z, refs, num_per_exit=bad)
    with pytest.raises(ValueError, match="sample it"):
        ts(np.zeros((23, 5, 4)), refs, num_per_exit=10)               # config 3's 23 exits: 10^22 vectors
    with pytest.raises(ValueError, match="2\\^32"):
        ts(z, refs, mixtures=0)
    with pytest.raises(ValueError, match="percentile index"):
        ts(z, refs, num_per_exit=4, mixtures=np.array([[0, 4, 0]]))   # a digit >= P is refused before the call
    with pytest.raises(ValueError, match="mixtures"):
        ts(z, refs, mixtures=np.zeros((2, 4), dtype=np.int64))        # (V, E1) wanted
    with pytest.raises(ValueError, match="mixtures"):
        ts(z, refs, mixtures="all")
    with pytest.raises(ValueError, match="references"):
        ts(z)
    res = pkg.sweep.SearchResult(table=np.zeros((3, 4)), front_thresholds=np.array([[0.9, 0.8, 0.0], [0.5, 0.6, 0.0], [0.1, 0.2, 0.0]]),
                                 front_accuracy=np.array([0.5, 0.7, 0.9]), front_mean_exit=np.array([0.2, 1.0, 1.8]),
                                 front_vector=np.array([3, 1, 7], dtype=np.uint32), front_hits=np.array([5, 7, 9], dtype=np.int32),
                                 front_exit_sum=np.array([2, 10, 18], dtype=np.int32), num_vectors=16, num_samples=10, source=pkg.capi.SEARCH_GRID)
    assert res.select(min_accuracy=0.6) == [0.5, 0.6, 0.0] and res.select(min_accuracy=0.7) == [0.5, 0.6, 0.0]
    assert res.select(max_mean_exit=1.5) == [0.5, 0.6, 0.0] and res.select(max_mean_exit=5) == [0.1, 0.2, 0.0]
    assert isinstance(res.select(min_accuracy=0.0), list) and all(type(t) is float for t in res.select(min_accuracy=0.0))
    assert res.digits(7) == [3, 1]
    for kw in (dict(), dict(min_accuracy=0.5, max_mean_exit=1.0)):
        with pytest.raises(ValueError, match="exactly one"):
            res.select(**kw)
    with pytest.raises(ValueError, match="no front entry"):
        res.select(min_accuracy=0.95)
    with pytest.raises(ValueError, match="no front entry"):
        res.select(max_mean_exit=0.1)
