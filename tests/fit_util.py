"""What the tests of the device fits (head, two-layer head, distilled, weighted, gate, LTE classifier) share: device helpers of the GPU tests,
and the host tests' scaffolding -- the refusal loop, the reader of the library's symbol table, the C syntax check of the header.  A plain
module, not a conftest: nothing here is a fixture or a hook."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from .conftest import ROOT


def _torch():
    import torch
    return torch


def _dev(a, dtype=None):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def _ptr(x):
    return C.c_void_p(x.data_ptr()) if x is not None else None


def _stream():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def _gap_thresholds(conf):
    """Per exit, the middle of the widest gap between neighbouring confidences that leaves documents on both sides."""
    thr = np.empty(conf.shape[0])
    for e, row in enumerate(conf):
        s = np.sort(row)
        j = int(np.argmax(np.diff(s)))
        thr[e] = 0.5 * (s[j] + s[j + 1])
    return thr


def _refused(pkg, name, call, cases):
    """cases: {what: (keyword arguments of ``call``, needle)}.  Every call is refused before any device call, with a message that starts
    with the entry point's ``name`` and holds the needle."""
    for what, (kw, needle) in cases.items():
        assert call(**kw) != 0, (name, what)
        msg = pkg.capi.last_error()
        assert msg.startswith(name + ":") and "no HIP device" not in msg, (name, what, msg)
        assert needle in msg, (name, what, msg)


def exported_symbols(path):
    """The names in the dynamic symbol table of the built library at ``path`` (no GPU, no loading)."""
    if not os.path.exists(path):
        pytest.fail(f"{path} is missing: build() first")
    tool = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    r = subprocess.run([tool, "-D", "--defined-only", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return {ln.split()[-1] for ln in r.stdout.splitlines() if ln.strip()}


def compiles_as_c(body):
    """``body``, the statements of a main() behind include/mmee.h, passes gcc -std=c99 -Wall -Werror -fsyntax-only; skips without gcc."""
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "mmee.h"\nint main(void) {\n' + body + '}\n')
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


class _HostTensor:
    """What a fit's state_dict asks of a tensor: shape and .cpu().numpy()."""

    def __init__(self, a):
        self.a, self.shape = a, a.shape

    def cpu(self):
        return self

    def numpy(self):
        return self.a
