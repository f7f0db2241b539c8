"""numpy restatement of the two combined exit rules of include/mmee.h (MMEE_RULE_STREAK, patient and confident; MMEE_RULE_EITHER, patience or
threshold), the oracle of tests/test_host_rule.py and tests/test_gpu_rule.py.  It builds on the agreement counter and the max-softmax of
tests/patience_ref.py.  The reference implements neither rule, so there is no reference output to pin against: these lines ARE the
specification, written from the header's text, independently of the kernels."""
import numpy as np

from .patience_ref import max_softmax, run_counters

PLAIN, STREAK, EITHER = 0, 1, 2
RULE_NAMES = {STREAK: "patient_confident", EITHER: "patience_or_threshold"}


def events(crit, thresholds, sign):
    """f (E1,N): sign > 0: crit > thr (max_confidence), sign < 0: crit < thr (entropy, LTE); strict, float64; a NaN threshold never fires."""
    crit = np.asarray(crit, dtype=np.float64)
    thr = np.broadcast_to(np.asarray(thresholds, dtype=np.float64).reshape(-1), (crit.shape[0],))[:, None]
    with np.errstate(invalid="ignore"):
        return crit > thr if sign > 0 else crit < thr


def patience_vector(t, E1):
    """A scalar is that value at every exit; a vector has one entry per exit (the final one is ignored)."""
    t = np.asarray(t, dtype=np.int64)
    if t.ndim == 0:
        return np.full(E1, int(t), dtype=np.int64)
    assert t.shape == (E1,) and np.all(t >= 1)
    return t


def streak_counters(f):
    """s_e = f_e ? s_{e-1} + 1 : 0 with s_{-1} = 0."""
    s = np.zeros(f.shape, dtype=np.int64)
    prev = np.zeros(f.shape[1], dtype=np.int64)
    for e in range(f.shape[0]):
        prev = np.where(f[e], prev + 1, 0)
        s[e] = prev
    return s


def first_or_final(hit):
    """First exit whose row is True, the final exit E when none is (the final exit's own row is never looked at)."""
    hit = hit.copy()
    hit[-1] = True
    return hit.argmax(0).astype(np.int32)


def plain_exits(crit, thresholds, sign):
    return first_or_final(events(crit, thresholds, sign))


def rule_exits(crit, store, thresholds, t, rule, sign=1):
    """crit (E1,N) criterion table or LTE scores, store (E1,N,K) the logits the agreement counter looks at (unused under STREAK)."""
    f = events(crit, thresholds, sign)
    tv = patience_vector(t, f.shape[0])[:, None]
    if rule == STREAK:
        return first_or_final(streak_counters(f) >= tv)
    if rule == EITHER:
        _, c = run_counters(store)
        return first_or_final(f | (c >= tv))
    assert rule == PLAIN
    return first_or_final(f)


def rule_policy(crit, store, thresholds, t, rule, sign=1):
    """(exits int32 (N,), predictions (N,K), confidence (N,) = the criterion entry at the chosen exit, counts (E1,))."""
    store = np.asarray(store, dtype=np.float64)
    crit = np.asarray(crit, dtype=np.float64)
    ex = rule_exits(crit, store, thresholds, t, rule, sign)
    rows = np.arange(store.shape[1])
    return ex, store[ex, rows], crit[ex, rows], np.bincount(ex, minlength=store.shape[0])


def rule_sweep(crit, store, refs, thresholds, patiences, rule, sign=1):
    """thresholds (V,E1) x patiences (P,) scalars -> integer (hits (V,P), exit sums (V,P), histogram (V,P,E1)).  The walk is done per pair:
    no sharing of work with the kernels' single walk."""
    crit = np.asarray(crit, dtype=np.float64)
    p = np.asarray(store).argmax(-1)
    _, c = run_counters(store)
    E1, N = crit.shape
    V, P = len(thresholds), len(patiences)
    hits, sums, hist = np.zeros((V, P), np.int64), np.zeros((V, P), np.int64), np.zeros((V, P, E1), np.int32)
    rows = np.arange(N)
    for v in range(V):
        f = events(crit, thresholds[v], sign)
        s = streak_counters(f)
        for j, t in enumerate(patiences):
            ex = first_or_final(s >= t) if rule == STREAK else first_or_final(f | (c >= t))
            hits[v, j] = int((p[ex, rows] == refs).sum())
            sums[v, j] = int(ex.sum())
            hist[v, j] = np.bincount(ex, minlength=E1)
    return hits, sums, hist


def msp_table(store):
    """(E1,N) float64 max-softmax of every row, summed in label order."""
    return max_softmax(np.asarray(store, dtype=np.float64))
