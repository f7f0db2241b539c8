"""What the tests of the three device fits (head, two-layer head, LTE classifier) share.  A plain module, not a conftest: nothing here is a
fixture or a hook."""
import ctypes as C

import numpy as np


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


class _HostTensor:
    """What a fit's state_dict asks of a tensor: shape and .cpu().numpy()."""

    def __init__(self, a):
        self.a, self.shape = a, a.shape

    def cpu(self):
        return self

    def numpy(self):
        return self.a
