"""numpy restatement of model cascades (include/mmee.h, behind MMEE_QUOTA_*), the oracle of tests/test_host_cascade.py and
tests/test_gpu_cascade.py: the deferral criterion (tests/csf_ref.py), the strict test, the stable selection, gather, merge, the global exit
indices and the cumulative costs.  Written from the header's text, independently of the kernels."""
import numpy as np

from . import csf_ref


def criteria(rows, criterion):
    """c of every delivered row: float64 criterion of (double) of the float32 rows (n,K)."""
    x = np.asarray(rows, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return csf_ref.csf(x, criterion)


def fires(crit, threshold, criterion):
    """The strict test in the criterion's direction; a NaN never fires."""
    with np.errstate(invalid="ignore"):
        return crit > threshold if csf_ref.SIGN[criterion] > 0 else crit < threshold


def select(crit, exit_layer, final_exit, threshold, criterion, orig=None):
    """The deferred documents of a stage: left at the final exit and the criterion does not fire.  Returns their ORIGINAL slots in the stage's
    order (int32): orig[i], or i when orig is None."""
    crit, exit_layer = np.asarray(crit, dtype=np.float64), np.asarray(exit_layer)
    defer = (exit_layer == final_exit) & ~fires(crit, threshold, criterion)
    idx = np.nonzero(defer)[0]
    return (idx if orig is None else np.asarray(orig)[idx]).astype(np.int32)


def gather(src, slots):
    """dst[j] = src[slots[j]]."""
    return np.asarray(src)[np.asarray(slots, dtype=np.int64)]


def merge(out, res, slots, exit_offset, stage):
    """A later stage's (logits, exit_layer, confidence) into the cascade's (logits, exit_layer, confidence, stage) at `slots`; returns copies."""
    lg, ex, cf, st = (np.array(a, copy=True) for a in out)
    s = np.asarray(slots, dtype=np.int64)
    lg[s], ex[s], cf[s], st[s] = res[0], np.asarray(res[1]) + exit_offset, res[2], stage
    return lg, ex, cf, st


def offsets(e1):
    """off_s of every stage from the E1_s."""
    return np.concatenate([[0], np.cumsum(e1)[:-1]]).astype(np.int64)


def global_exits(stage, local_exit, e1):
    return (offsets(e1)[np.asarray(stage)] + np.asarray(local_exit)).astype(np.int32)


def cumulative_costs(stage_costs):
    """Per-stage (E1_s, N) cost tables -> (SE1, N): row (s, e) = stage s's row e plus the final rows of all stages before it.  ValueError at 2^32."""
    rows, before = [], 0
    for c in stage_costs:
        c = np.asarray(c).astype(np.int64)
        rows.append(c + before)
        before = before + c[-1][None, :]
    out = np.concatenate(rows, axis=0)
    if out.size and out.max() >= 2 ** 32:
        raise ValueError("cumulative cost does not fit 32 bits")
    return out.astype(np.uint32)
