"""numpy restatement of the vision-first call of include/mmee.h (ee_forward_vision) over a dumped (E1, N, K) array, written from the header's
text: phase 1 decides exit 0 for every document, the survivors (ascending slots) run an ordinary thresholded scan over ALL exits -- exit 0
included, where none of them leaves -- and their results are merged into the survivors' slots with exit offset 0 and stage 1.  No GPU.

``text_calls`` records what a text source would have been asked: one entry, the survivors' slots, per call in which somebody survives."""
import numpy as np

from . import csf_ref


def exit0_leaves(crit0, thr0, sign=+1):
    """Who leaves at exit 0: the criterion strictly passes the threshold (sign +1: '>', -1: '<'; a NaN never does)."""
    c = np.asarray(crit0, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return c > thr0 if sign > 0 else c < thr0


def threshold_for(crit0, n_leave, sign=+1, min_gap=1e-9):
    """thresholds[0] that makes exactly `n_leave` of the documents leave at exit 0: the midpoint of two adjacent sorted criteria more than
    `min_gap` apart (asserted), or a value beyond every criterion for nobody / everybody."""
    c = np.sort(sign * np.asarray(crit0, dtype=np.float64))[::-1]          # surest first
    n = c.shape[0]
    assert 0 <= n_leave <= n and np.isfinite(c).all()
    if n_leave == 0:
        return float(sign * (c[0] + 1.0))
    if n_leave == n:
        return float(sign * (c[-1] - 1.0))
    assert c[n_leave - 1] - c[n_leave] > min_gap, "adjacent exit-0 criteria closer than the minimum gap"
    return float(sign * 0.5 * (c[n_leave - 1] + c[n_leave]))


def phase1(logits, table, thr0, sign=+1):
    """(leave mask (N,), survivors int32 ascending, out_logits (N,K) / out_exit (N,) / out_conf (N,) with NaN / -1 / NaN where nothing is written)."""
    logits, table = np.asarray(logits, dtype=np.float64), np.asarray(table, dtype=np.float64)
    N, K = logits.shape[1], logits.shape[2]
    leave = exit0_leaves(table[0], thr0, sign)
    out_logits, out_exit, out_conf = np.full((N, K), np.nan), np.full(N, -1, np.int32), np.full(N, np.nan)
    out_logits[leave], out_exit[leave], out_conf[leave] = logits[0, leave], 0, table[0, leave]
    return leave, np.nonzero(~leave)[0].astype(np.int32), out_logits, out_exit, out_conf


def compose(logits, thresholds, criterion, text_calls=None):
    """The two phases on a dumped (E1,N,K) array.  Returns dict(logits, exit_layer, confidence, stage, text_docs)."""
    logits = np.asarray(logits, dtype=np.float64)
    sign = csf_ref.SIGN[criterion]
    table = csf_ref.csf(logits, criterion)
    thr = np.broadcast_to(np.asarray(thresholds, dtype=np.float64).reshape(-1), (logits.shape[0],))
    leave, surv, out_logits, out_exit, out_conf = phase1(logits, table, thr[0], sign)
    stage = np.zeros(logits.shape[1], np.int32)
    if surv.size:
        if text_calls is not None:
            text_calls.append(surv.copy())
        ex, pred, conf, _ = csf_ref.scan(logits[:, surv], thr, criterion)      # phase 2: an ordinary scan of the sub-batch, exit 0 included
        out_logits[surv], out_exit[surv], out_conf[surv], stage[surv] = pred, ex, conf, 1
    return dict(logits=out_logits, exit_layer=out_exit, confidence=out_conf, stage=stage, text_docs=int(surv.size))
