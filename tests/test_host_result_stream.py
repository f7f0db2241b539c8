"""CPU checks of the result stream (include/mmee.h MMEE_FLAG_STREAM_RESULTS / ee_stream_next): the flag and the entry point are declared,
exported and bound, the Python surfaces exist and refuse what does not go with a stream before anything reaches a GPU, and
``unpack_stream_rows`` -- a pure function -- splits the K + 3-word rows back without touching a bit."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from . import stream_ref
from .conftest import ROOT


def test_header_declares_the_flag_and_the_function(pkg):
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    assert re.search(r"MMEE_FLAG_STREAM_RESULTS\s*=\s*128\b", header)
    assert re.search(r"#define\s+MMEE_ABI_VERSION\s+4\b", header)           # a flag bit and one function: ee_config is unchanged
    assert re.search(r"int\s+ee_stream_next\s*\(\s*ee_handle\s*\*\s*h\s*,\s*int32_t\s*\*\s*exit_index\s*,\s*const\s+int32_t\s*\*\*\s*rows\s*,"
                     r"\s*int32_t\s*\*\s*n_rows\s*\)", header)
    assert pkg.capi.FLAG_STREAM_RESULTS == 128
    flags = [getattr(pkg.capi, n) for n in dir(pkg.capi) if n.startswith("FLAG_")]
    assert len(set(flags)) == len(flags) and all(f & (f - 1) == 0 for f in flags)      # one bit each, none shared
    assert "ee_stream_next" in pkg.capi.SYMBOLS and pkg.capi.ABI_VERSION == 4


def test_library_exports_the_function(pkg):
    """Read the built library's dynamic symbol table (no GPU, no loading)."""
    path = pkg.capi.lib_path()
    if not os.path.exists(path):
        pytest.fail(f"{path} is missing: build() first")
    tool = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    r = subprocess.run([tool, "-D", "--defined-only", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ee_stream_next" in {ln.split()[-1] for ln in r.stdout.splitlines() if ln.strip()}


def test_python_surfaces_exist(pkg):
    assert callable(pkg.EarlyExitEngine.forward_stream) and callable(pkg.unpack_stream_rows)
    for model in (pkg.LayoutLMv3EEForSequenceClassification, pkg.DiTEEForImageClassification):
        sig = inspect.signature(model.early_exit_stream).parameters
        assert {"pixel_values", "thresholds", "temperatures", "patience", "low_latency"} <= set(sig)
    assert [f for f in pkg.ResultChunk.__dataclass_fields__] == ["exit_index", "doc_index", "logits", "exit_layer", "confidence"]
    # interleaving several handles' streams is out of scope, and says so
    with pytest.raises(NotImplementedError, match="result stream"):
        pkg.MicroBatchedEngine.forward_stream(None)
    assert "forward_stream" in inspect.getmodule(pkg.MicroBatchedEngine).__doc__


@pytest.mark.parametrize("kw", [dict(dump_all=True), dict(want_hidden_states=True), dict(want_attentions=True), dict(_capture=True),
                                dict(head_mask=np.ones(4, dtype=np.float32))], ids=lambda kw: next(iter(kw)))
def test_forward_stream_refuses_what_belongs_to_other_calls(pkg, kw):
    """The refusals come before the engine is looked at: no handle, no GPU."""
    with pytest.raises(ValueError, match="forward_stream"):
        pkg.EarlyExitEngine.forward_stream(None, **kw)


def _rows(pkg, K, n, seed):
    """n rows of K + 3 words built with dist.pack_results and a slot column; logits and confidence hold NaNs with payloads, infinities, signed
    zeros and denormals, the exit column a negative index and the int32 extremes."""
    import torch
    rng = np.random.default_rng(seed)
    lg = rng.integers(-2 ** 31, 2 ** 31, size=(n, K), dtype=np.int64).astype(np.int32)     # arbitrary bit patterns: NaNs of every payload among them
    cf = rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x80000000, 0x00000000], dtype=np.uint32).view(np.int32)
    m = min(n, special.size)
    lg[:m, 0] = special[:m]
    cf[:m] = special[::-1][:m]
    ex = rng.integers(0, 7, n).astype(np.int32)
    ex[:3] = (-1, np.iinfo(np.int32).min, np.iinfo(np.int32).max)[:min(3, n)]
    slot = rng.permutation(4 * n)[:n].astype(np.int32)
    packed = pkg.dist.pack_results(torch.from_numpy(lg.view(np.float32)), torch.from_numpy(ex), torch.from_numpy(cf.view(np.float32)))
    assert packed.dtype == torch.int32 and tuple(packed.shape) == (n, K + 2)
    words = np.concatenate([packed.numpy(), slot[:, None]], axis=1)
    return words, lg, ex, cf, slot


@pytest.mark.parametrize("K,n", [(16, 40), (1, 1), (10, 1025), (2, 0)])
def test_unpack_stream_rows_round_trips_every_bit(pkg, K, n):
    words, lg, ex, cf, slot = _rows(pkg, K, max(n, 1), seed=K * 1000 + n)
    words, lg, ex, cf, slot = words[:n], lg[:n], ex[:n], cf[:n], slot[:n]
    before = words.copy()
    doc, logits, exit_layer, conf = pkg.unpack_stream_rows(words, K)
    assert doc.dtype == np.int32 and logits.dtype == np.float32 and exit_layer.dtype == np.int32 and conf.dtype == np.float32
    assert doc.shape == (n,) and logits.shape == (n, K) and exit_layer.shape == (n,) and conf.shape == (n,)
    assert np.array_equal(doc, slot) and np.array_equal(exit_layer, ex)
    assert np.array_equal(logits.view(np.int32), lg) and np.array_equal(conf.view(np.int32), cf)      # compared as words: NaN != NaN as floats
    assert np.array_equal(words, before)
    # copies: the caller's rows may be rewritten afterwards (they are views of a pinned buffer in the engine)
    words[:] = 0
    assert np.array_equal(doc, slot) and np.array_equal(logits.view(np.int32), lg) and np.array_equal(conf.view(np.int32), cf)
    # a strided view of a wider buffer is taken as it is
    wide = np.zeros((n, K + 5), dtype=np.int32)
    wide[:, 1:K + 4] = before
    again = pkg.unpack_stream_rows(wide[:, 1:K + 4], K)
    assert np.array_equal(again[0], slot) and np.array_equal(again[1].view(np.int32), lg)


def test_unpack_stream_rows_rejects_other_dtypes_and_widths(pkg):
    K = 4
    good = np.zeros((3, K + 3), dtype=np.int32)
    pkg.unpack_stream_rows(good, K)
    for bad in (good.astype(np.float32), good.astype(np.int64), good.view(np.uint32), good.tolist()):
        with pytest.raises(TypeError, match="int32"):
            pkg.unpack_stream_rows(bad, K)
    for bad in (np.zeros((3, K + 2), dtype=np.int32), np.zeros((3, K + 4), dtype=np.int32), np.zeros(K + 3, dtype=np.int32),
                np.zeros((1, 3, K + 3), dtype=np.int32)):
        with pytest.raises(ValueError, match=r"K \+ 3"):
            pkg.unpack_stream_rows(bad, K)
    with pytest.raises(ValueError):
        pkg.unpack_stream_rows(good, K + 1)


def test_stream_ref_chunks():
    ex = np.array([2, 0, 3, 0, 2, 3, 3], dtype=np.int32)
    got = stream_ref.chunks(ex, 5)
    assert [c.tolist() for c in got] == [[1, 3], [], [0, 4], [2, 5, 6], []] and all(c.dtype == np.int32 for c in got)
    assert stream_ref.sizes(ex, 5) == [2, 0, 2, 3, 0]
    assert sorted(np.concatenate(got).tolist()) == list(range(7))
