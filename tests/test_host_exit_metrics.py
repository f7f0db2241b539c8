"""CPU checks of the evaluation report (include/mmee.h ee_exit_metrics): the numpy restatement (tests/metrics_ref.py) against the values the
reference's own metric functions gave (tests/golden/exit_metrics_ref.npz, minted by tests/golden/make_metrics_golden.py), its ECE against
``calibration.expected_calibration_error`` bit for bit, the C-ABI (header declaration, metric codes, plain-C compile, the exported symbol), the
entry point's refusals before it looks for a device, and the host side of ``metrics.ExitReport`` / ``exit_report``."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from . import metrics_ref as MR
from .conftest import ROOT, load_golden

MINTED = ("accuracy", "brier_loss", "nll", "f1_micro", "f1_macro", "aurc")
CODES = dict(ACCURACY=0, BRIER=1, NLL=2, F1_MICRO=3, F1_MACRO=4, ECE=5, AURC=6, AVG_CONF=7, COUNT=8)


@pytest.fixture(scope="module")
def golden():
    g = load_golden("exit_metrics_ref")
    g["logits"] = g["logits"].astype(np.float64)
    assert tuple(g["names"].tolist()) == MINTED and g["logits"].shape == (3, 1000, 16)
    g["report"] = MR.report(g["logits"], g["references"], exits=g["exits"])
    return g


def test_restatement_reproduces_every_minted_value(golden):
    """accuracy and f1_micro exactly; the float metrics within 1e-10 relative: float64 sums of N = 1000 non-negative terms differ by at most
    N 2^-53 ~ 1e-13 between summation orders, and three decades cover exp / log differences between libraries."""
    rep = golden["report"]
    for j, name in enumerate(MINTED):
        want = np.concatenate([golden["per_exit"][:, j], golden["point"][j:j + 1]])
        got = rep[name]
        assert got.shape == (4,)
        if name in ("accuracy", "f1_micro"):
            assert np.array_equal(got, want), (name, got, want)
        else:
            rel = np.abs(got - want) / np.abs(want)
            print(name, "max relative difference", rel.max())
            assert (rel <= 1e-10).all(), (name, got, want)
    assert np.array_equal(rep["exit_hist"], np.bincount(golden["exits"], minlength=3))


def test_fixture_exercises_the_unique_labels_rule_and_has_no_ties(golden):
    L, refs = golden["logits"], golden["references"]
    absent = set(range(16)) - set(refs.tolist()) - set(L[0].argmax(-1).tolist())
    assert absent, "a class that occurs in neither the references nor the predictions of exit 0"
    cm = golden["report"]["confusion"][0]
    per_class = [2.0 * cm[c, c] / (cm[c].sum() + cm[:, c].sum()) for c in range(16) if c not in absent]
    assert abs(np.mean(per_class) - golden["per_exit"][0, 4]) <= 1e-12           # averaged over the classes present ...
    assert abs(np.sum(per_class) / 16 - golden["per_exit"][0, 4]) > 1e-3        # ... not over all K
    for e in range(3):
        conf = MR.row_quantities(L[e], refs)["conf"]
        assert len(np.unique(conf)) == conf.shape[0]
    assert int(refs.sum()) != refs.shape[0]


def test_ece_equals_the_calibration_module_bit_for_bit(pkg, golden):
    ece = pkg.calibration.expected_calibration_error
    L, refs = golden["logits"], golden["references"]
    for e in range(3):
        q = MR.row_quantities(L[e], refs)
        assert MR.ece(q["conf"], q["correct"]) == ece(refs, L[e])
        assert golden["report"]["ece"][e] == ece(refs, L[e])
        for bins in (1, 7, 15):
            assert MR.ece(q["conf"], q["correct"], bins) == ece(refs, L[e], n_bins=bins)
    # a two-class table with many ties (confidences rounded to two decimals): probabilities [1 - c, c], the label chosen to make `correct`
    rng = np.random.default_rng(3)
    for N in (1, 2, 63, 2500):
        c = np.round(0.51 + 0.49 * rng.random(N), 2)
        correct = rng.random(N) < c
        P = np.stack([1.0 - c, c], axis=1)
        y = np.where(correct, 1, 0)
        assert np.array_equal(P.max(-1), c) and np.array_equal(P.argmax(-1) == y, correct)
        assert N < 2500 or len(np.unique(c)) <= 50                   # hundreds of ties, duplicate edges
        assert MR.ece(c, correct) == ece(y, P), N
        assert MR.ece(c, correct, 10) == ece(y, P, n_bins=10), N


def test_aurc_on_literals():
    # distinct confidences, by hand: risks [2/4, 2/3, 1/2, 0], weights 1/4 each
    got = MR.aurc(np.array([0.1, 0.2, 0.3, 0.9]), np.array([1, 0, 0, 1]))
    assert got == (2 / 4 + 2 / 3) * 0.5 * 0.25 + (2 / 3 + 1 / 2) * 0.5 * 0.25 + (1 / 2 + 0.0) * 0.5 * 0.25
    # the order inside a tie matters, and it is the document order
    c = np.array([0.5, 0.5, 0.7])
    assert MR.aurc(c, np.array([0, 1, 1])) != MR.aurc(c, np.array([1, 0, 1]))
    assert MR.aurc(c, np.array([1, 1, 1])) == 0.0
    assert MR.aurc(np.array([0.4]), np.array([0])) == 0.0            # N = 1: no weights
    # all wrong: every risk is 1 and the weights of the N - 1 steps sum to (N - 1) / N
    assert abs(MR.aurc(np.linspace(0.1, 0.9, 9), np.zeros(9)) - 8 / 9) <= 1e-15


def test_header_declares_the_report():
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    assert re.search(r"#define\s+MMEE_ABI_VERSION\s+4\b", header)           # one more function: ee_config is unchanged
    assert "ee_exit_metrics" in set(re.findall(r"\b(ee_[a-z_0-9]+)\s*\(", header))
    for name, code in CODES.items():
        assert re.search(rf"#define\s+MMEE_METRIC_{name}\s+{code}\b", header), name
    for text in ("TIES IN DOCUMENT\n *     ORDER", "unique_labels", "the FIRST maximum", "upper-edge proxy", "Deviations from the reference"):
        assert text in header, text


def test_capi_carries_the_same_codes(pkg):
    for name, code in CODES.items():
        assert getattr(pkg.capi, "METRIC_" + name) == code
    assert pkg.capi.ABI_VERSION == 4
    assert len(pkg.capi.SYMBOLS["ee_exit_metrics"][1]) == 14
    assert len(pkg.metrics.FIELDS) == pkg.capi.METRIC_COUNT
    assert pkg.exit_report is pkg.metrics.exit_report and pkg.ExitReport is pkg.metrics.ExitReport


def test_header_with_the_report_compiles_as_c():
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "mmee.h"\n'
                    'int main(void) {\n'
                    '    int (*a)(const double*, const int64_t*, const double*, const uint8_t*, const double*, const int32_t*, int32_t, int32_t, int32_t,'
                    ' int32_t, double*, int64_t*, int64_t*, void*) = ee_exit_metrics;\n'
                    '    (void)a;\n'
                    '    return MMEE_ABI_VERSION != 4 || MMEE_METRIC_COUNT != 8 || MMEE_METRIC_AVG_CONF != 7;\n'
                    '}\n')
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def test_library_exports_the_report_symbol(pkg):
    """Read the built library's dynamic symbol table (no GPU, no loading)."""
    path = pkg.capi.lib_path()
    if not os.path.exists(path):
        pytest.fail(f"{path} is missing: build() first")
    tool = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    r = subprocess.run([tool, "-D", "--defined-only", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ee_exit_metrics" in {ln.split()[-1] for ln in r.stdout.splitlines() if ln.strip()}


def test_entry_point_refuses_bad_arguments_before_any_device_call(pkg):
    """Every refusal returns non-zero with a message that names the entry point and the reason.  The pointers are never dereferenced: plain
    integers stand in for device addresses."""
    lib = pkg.capi.load()
    p = C.c_void_p(4096)

    def call(logits=p, refs=p, conf=None, correct=None, T=None, exits=None, E1=3, N=100, K=16, bins=0, out=p, cm=None, hist=None):
        return lib.ee_exit_metrics(logits, refs, conf, correct, T, exits, E1, N, K, bins, out, cm, hist, None)

    cases = {
        "null out": (dict(out=None), "out"),
        "logits without references": (dict(refs=None), "references"),
        "no input at all": (dict(logits=None, refs=None), "table form"),
        "table without correct": (dict(logits=None, refs=None, conf=p), "table form"),
        "table with confusion": (dict(logits=None, refs=None, conf=p, correct=p, cm=p), "confusion"),
        "hist without exits": (dict(hist=p), "exit_hist"),
        "E1 = 0": (dict(E1=0), "E1 = 0"),
        "E1 = 257": (dict(E1=257), "E1 = 257"),
        "N = 0": (dict(N=0), "N = 0"),
        "N above 2^20": (dict(N=(1 << 20) + 1), "2^20"),
        "K = 0": (dict(K=0), "K = 0"),
        "n_bins = 1025": (dict(bins=1025), "n_bins = 1025"),
    }
    for what, (kw, needle) in cases.items():
        assert call(**kw) != 0, what
        msg = pkg.capi.last_error()
        assert msg.startswith("ee_exit_metrics:") and "no HIP device" not in msg, (what, msg)
        assert needle in msg, (what, msg)


def test_python_surface_argument_errors(pkg):
    """All raised on the host, before the library or a device is asked for."""
    z, refs = np.zeros((3, 5, 4)), np.zeros(5, dtype=np.int64)
    er = pkg.metrics.exit_report
    with pytest.raises(ValueError, match=r"exits: every exit must be in \[0, 3\)"):
        er(z, refs, exits=np.array([0, 1, 2, 3, 0]))
    with pytest.raises(ValueError, match="exits"):
        er(z, refs, exits=np.array([0, -1, 2, 1, 0]))
    with pytest.raises(ValueError, match=r"label must be in \[0, 4\)"):
        er(z, np.array([0, 1, 2, 3, 4]))
    with pytest.raises(ValueError, match="label"):
        er(z, np.array([0, 1, 2, 3, -1]))
    with pytest.raises(ValueError, match="references"):
        er(z)
    with pytest.raises(ValueError, match="references: shape"):
        er(z, np.zeros(6, dtype=np.int64))
    with pytest.raises(ValueError, match="exits: shape"):
        er(z, refs, exits=np.zeros(4, dtype=np.int64))
    with pytest.raises(ValueError, match="logits must have shape"):
        er(np.zeros((2, 3, 5, 4)), refs)
    for T in ([1.0, 0.0, 1.0], [1.0, -2.0, 1.0], [1.0, np.inf, 1.0], [1.0, np.nan, 1.0]):
        with pytest.raises(ValueError, match="finite and positive"):
            er(z, refs, temperatures=T)
    with pytest.raises(ValueError, match="temperatures: shape"):
        er(z, refs, temperatures=[1.0, 1.0])
    for bins in (0, 1025):
        with pytest.raises(ValueError, match="n_bins"):
            er(z, refs, n_bins=bins)
    table = (np.zeros((3, 5)), np.zeros((3, 5), dtype=np.uint8))
    with pytest.raises(ValueError, match="confusion"):
        er(table, want_confusion=True)
    with pytest.raises(ValueError, match="temperatures"):
        er(table, temperatures=[1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="table"):
        er((np.zeros((3, 5)), np.zeros((3, 6), dtype=np.uint8)))


def _hand_made(pkg, policy=True):
    R = 3 if policy else 2
    cols = {name: np.arange(R, dtype=np.float64) + 10.0 * j for j, name in enumerate(pkg.metrics.FIELDS)}
    return pkg.ExitReport(num_samples=10, exit_hist=np.array([6, 4], dtype=np.int64) if policy else None, policy=2 if policy else None, **cols)


def test_as_reference_dict_keys(pkg):
    rep = _hand_made(pkg)
    d = rep.as_reference_dict()
    names = ["accuracy", "brier_loss", "nll", "f1_micro", "f1_macro", "ece", "aurc"]
    assert list(d) == [f"exit_{e} _{n}" for e in range(2) for n in names] + names         # with that space; the operating point under plain names
    assert d["exit_1 _nll"] == 21.0 and d["exit_0 _aurc"] == 60.0 and d["aurc"] == 62.0 and d["accuracy"] == 2.0
    assert all(type(v) is float for v in d.values()) and "average_confidence" not in d
    plain = _hand_made(pkg, policy=False)
    assert plain.num_exits == 2 and rep.num_exits == 2
    assert list(plain.as_reference_dict()) == [f"exit_{e} _{n}" for e in range(2) for n in names]


def test_efficiency(pkg):
    rep = _hand_made(pkg)
    assert rep.efficiency() == {"exit_distribution": {0: 0.6, 1: 0.4}}
    got = rep.efficiency(cost=np.array([25, 100]))
    assert got["exit_distribution"] == {0: 0.6, 1: 0.4}
    assert abs(got["GFLOPs reduction"] - (1.0 - (0.6 * 25 + 0.4 * 100) / 100)) <= 1e-15
    assert rep.efficiency(cost=[100.0, 100.0])["GFLOPs reduction"] == 0.0
    with pytest.raises(NotImplementedError):
        rep.efficiency(cost=np.ones((2, 10)))
    with pytest.raises(ValueError, match="shape"):
        rep.efficiency(cost=np.ones(3))
    with pytest.raises(ValueError, match="operating point"):
        _hand_made(pkg, policy=False).efficiency()
