"""Numpy restatement of the result stream (include/mmee.h ee_stream_next): which documents each chunk holds, from the exit every document
left at.  Chunk e is the ascending list of the slots whose exit is e; there are E + 1 chunks, empty ones included."""
import numpy as np


def chunks(exit_layer, n_exits1):
    """(B,) exit indices -> [slots of chunk 0, ..., slots of chunk E], each an ascending int32 array."""
    ex = np.asarray(exit_layer)
    assert ex.ndim == 1 and ex.size and ex.min() >= 0 and ex.max() < n_exits1
    return [np.nonzero(ex == e)[0].astype(np.int32) for e in range(n_exits1)]


def sizes(exit_layer, n_exits1):
    return [int(c.size) for c in chunks(exit_layer, n_exits1)]
