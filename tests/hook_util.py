"""What the tests of the stand-alone kernel hooks (test_gpu_attention.py, test_gpu_rows.py, test_gpu_xprobe.py, test_gpu_exit_stage.py) share.  A plain module, not a
conftest: nothing here is a fixture or a hook of pytest."""
import ctypes as C

import numpy as np

ERR_SPLIT_OVERFLOW = 16                                 # csrc/mmee_common.h kErrSplitOverflow
SENTINEL = 0x7FA5A5A5                                   # a NaN bit pattern no kernel writes


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


def _decode_split(rows_i32, N, scale):
    """Split-f16 rows [rows, N] (int32 words, on the device) as float64, on the device."""
    torch = _torch()
    h = rows_i32.view(torch.float16).view(rows_i32.shape[0], N // 16, 2, 16)       # 64-byte groups [hi 16 | lo 16]
    return (h[:, :, 0].double() + h[:, :, 1].double()).reshape(rows_i32.shape[0], N) / scale


def _encode_split(x, scale):
    """Split-f16 rows of values the planes hold exactly, as int32 words [rows, N]."""
    xs = np.asarray(x, np.float32) * np.float32(scale)
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(np.float32)).astype(np.float16)
    assert np.array_equal((hi.astype(np.float64) + lo.astype(np.float64)) / scale, np.asarray(x, np.float64))
    rows, N = xs.shape
    planes = np.stack([hi.reshape(rows, N // 16, 16), lo.reshape(rows, N // 16, 16)], axis=2)
    return np.ascontiguousarray(planes).view(np.int32).reshape(rows, N)


def _f32(words):
    torch = _torch()
    return words.view(torch.float32).double().cpu().numpy()
