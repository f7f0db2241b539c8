"""CPU checks of the low-latency mode (include/mmee.h MMEE_FLAG_LOW_LATENCY): the flag and the two entry points are declared, exported and
bound, and the split-K rule ``ee_low_latency_k_splits`` -- a pure function that needs neither a handle nor a GPU -- has the properties the
forward schedule relies on."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

from .conftest import ROOT

NEW_SYMBOLS = ("ee_low_latency_k_splits", "ee_last_k_splits")
ROWS = (1, 128, 129, 213, 709, 1418, 5672, 45376)
SHAPES = ((256, 256), (256, 512), (768, 768), (768, 3072), (1024, 1024), (1024, 4096))      # (N, K): attention output / FFN down at H = 256, base, large
CUS = (256, 64)


def test_header_declares_the_flag_and_both_functions(pkg):
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    assert re.search(r"MMEE_FLAG_LOW_LATENCY\s*=\s*64\b", header)
    assert re.search(r"#define\s+MMEE_ABI_VERSION\s+4\b", header)           # a flag bit and two functions: ee_config is unchanged
    declared = set(re.findall(r"\b(ee_[a-z_0-9]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared
    assert re.search(r"int32_t\s+ee_low_latency_k_splits\s*\(\s*int32_t\s+max_rows\s*,\s*int32_t\s+N\s*,\s*int32_t\s+K\s*,\s*int32_t\s+num_cus\s*\)", header)
    assert re.search(r"int\s+ee_last_k_splits\s*\(\s*ee_handle\s*\*\s*h\s*,\s*int32_t\s*\*\s*attn_out\s*,\s*int32_t\s*\*\s*ffn_down\s*\)", header)
    assert pkg.capi.FLAG_LOW_LATENCY == 64
    flags = [getattr(pkg.capi, n) for n in dir(pkg.capi) if n.startswith("FLAG_")]
    assert len(set(flags)) == len(flags) and all(f & (f - 1) == 0 for f in flags)      # one bit each, none shared
    for name in NEW_SYMBOLS:
        assert name in pkg.capi.SYMBOLS


def test_library_exports_both_functions(pkg):
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


def test_python_surface_takes_the_keyword(pkg):
    import inspect
    assert inspect.signature(pkg.EarlyExitEngine.forward).parameters["low_latency"].default is False
    assert inspect.signature(pkg.LayoutLMv3EEForSequenceClassification.early_exit).parameters["low_latency"].default is False
    assert callable(pkg.EarlyExitEngine.last_k_splits)
    assert "low_latency" not in inspect.signature(pkg.MicroBatchedEngine.forward).parameters      # large batches: not its mode


@pytest.fixture(scope="module")
def rule(pkg):
    fn = pkg.capi.load().ee_low_latency_k_splits
    return lambda rows, N, K, cus: int(fn(rows, N, K, cus))


def test_rule_properties(rule):
    for (N, K), cus in itertools.product(SHAPES, CUS):
        prev = None
        for rows in ROWS:
            S = rule(rows, N, K, cus)
            assert S in (1, 2, 4, 8), (rows, N, K, cus, S)
            stages = K // 32
            assert stages % S == 0, (rows, N, K, cus, S)
            assert S == 1 or stages // S >= 3, (rows, N, K, cus, S)                 # every part fills the three-deep stage ring
            tiles = -(-rows // 128) * (N // 128)
            assert S == 1 or tiles * S <= 2 * cus, (rows, N, K, cus, S)             # the parts buffer: 2 * num_cus tiles of 128 x 128
            assert prev is None or S <= prev, (rows, N, K, cus, S, prev)            # non-increasing in max_rows
            prev = S
        assert rule(45376, N, K, cus) == 1                                         # a bench-sized batch fills the chip without it
    assert rule(709, 768, 3072, 256) > 1                                            # one base-shape document at T = 512, FFN down
    assert rule(709, 768, 768, 256) > 1                                             # ... and its attention output


def test_rule_is_a_pure_function_of_its_arguments(rule):
    seen = {a: rule(*a) for a in itertools.product(ROWS, (256, 768), (768, 3072), CUS)}
    for a in reversed(list(seen)):                                                  # another order, the same answers
        assert rule(*a) == seen[a]
    # the smallest shapes: 8 k-stages cannot be divided further than 2 x 4, 16 not further than 4 x 4
    assert rule(390, 256, 256, 256) == 2 and rule(390, 256, 512, 256) == 4
    # arguments outside the kernel's shapes decline instead of failing
    for bad in ((0, 768, 768, 256), (-5, 768, 768, 256), (709, 100, 768, 256), (709, 768, 40, 256), (709, 768, 768, 0), (709, 0, 0, 0)):
        assert rule(*bad) == 1
