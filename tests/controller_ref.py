"""numpy restatement of online exit control (the definition is in include/mmee.h, behind the audit's): the thresholds of a position, the tally of
one call, the step, one log row, and the whole loop on a criterion table.  The oracle of tests/test_host_controller.py and
tests/test_gpu_controller.py, written from the header's text, not from the kernels.  Every product is a numpy operation of its own, so it is
rounded before it is added, as the definition asks."""
import numpy as np

from . import audit_ref as A


def log_words(E1):
    return 5 + 2 * (E1 - 1) + E1


def thresholds(path, p, sign):
    """(E1,) float64 of position p on path (V,E1)."""
    path = np.asarray(path, np.float64)
    V, E1 = path.shape
    assert V >= 2
    p = np.float64(p)
    if p < 0:
        return np.concatenate([np.full(E1 - 1, -np.inf if sign < 0 else np.inf), path[0, E1 - 1:]])
    q = min(p, np.float64(V - 1))
    i = min(int(np.floor(q)), V - 2)
    t = q - np.float64(i)
    a, b = path[i], path[i + 1]
    diff = b - a
    prod = diff * t
    out = a + prod
    out[E1 - 1] = a[E1 - 1]
    return out


def first_argmax(z):
    """Rows' argmax, the lowest index on ties; a row with a NaN counts as K - 1 (sweep.first_argmax)."""
    z = np.asarray(z)
    K = z.shape[-1]
    am = np.argmax(z, -1)                                                # numpy: the first maximum -- and the first NaN, replaced below
    return np.where(np.isnan(z).any(-1), K - 1, am)


def scaled32(z, temp):
    """(float)((double)z / temp): the row a decide launch writes."""
    return (np.asarray(z, np.float32).astype(np.float64) / np.float64(temp)).astype(np.float32)


def tally(doc_orig, pol, temp, delivered, out_logits, out_exit, *, cut, seed, slot_base, B, E1):
    """[sampled, disagree, delivered[E], agree[E]] int64 of one call: the final stage's documents `doc_orig` (n,) with the rows `pol` (n,K) the
    final decide launch read, the marks `delivered` [B], the results out_logits (B,K) / out_exit (B)."""
    E = E1 - 1
    o = np.asarray(doc_orig, np.int64)
    sampled = int(A.selected(cut, seed, np.arange(B) + slot_base).sum())
    shadow = np.asarray(delivered)[o] != 0
    full = first_argmax(scaled32(pol, temp)) if len(o) else np.zeros(0, np.int64)
    got = first_argmax(np.asarray(out_logits, np.float32)[o]) if len(o) else np.zeros(0, np.int64)
    differs = shadow & (full != got)
    ex = np.asarray(out_exit, np.int64)[o]
    early = shadow & (ex >= 0) & (ex < E)
    d = np.bincount(ex[early], minlength=E)[:E]
    a = np.bincount(ex[early & ~differs], minlength=E)[:E]
    return np.concatenate([[sampled, int(differs.sum())], d, a]).astype(np.int64)


def step(p, sampled, disagree, alpha, gamma, V):
    p = np.float64(p)
    if sampled == 0:
        return p
    loss = np.float64(disagree) / np.float64(sampled)
    move = np.float64(gamma) * (loss - np.float64(alpha))
    return min(np.float64(V - 1), p - move)


def advance(path, sign, alpha, gamma, state, tal, thr):
    """One call's bookkeeping: (log row as a dict, state after, thresholds of the next call).  state = (p, calls, steps, sampled_sum, disagree_sum)."""
    path = np.asarray(path, np.float64)
    V, E1 = path.shape
    E = E1 - 1
    p, calls, steps, ssum, dsum = state
    sampled, disagree = int(tal[0]), int(tal[1])
    q = step(p, sampled, disagree, alpha, gamma, V)
    row = dict(call=calls, p_before=np.float64(p), p_after=np.float64(q), sampled=sampled, disagree=disagree,
               delivered=np.asarray(tal[2:2 + E], np.int64), agree=np.asarray(tal[2 + E:2 + 2 * E], np.int64), thresholds=np.array(thr, np.float64))
    return row, (q, calls + 1, steps + (1 if sampled else 0), ssum + sampled, dsum + disagree), thresholds(path, q, sign)


def exits_of(table, thr, sign):
    """The forward's rule on a criterion table (E1,n): the first e < E1 - 1 with sign c > sign thr, strict (a NaN never fires), else E1 - 1."""
    t = np.asarray(table, np.float64)
    E1 = t.shape[0]
    with np.errstate(invalid="ignore"):
        fires = (t[:E1 - 1] < thr[:E1 - 1, None]) if sign < 0 else (t[:E1 - 1] > thr[:E1 - 1, None])
    return np.where(fires.any(0), fires.argmax(0), E1 - 1).astype(np.int32)


def rolling(table, bad, path, *, sign, cut, seed, alpha, gamma, p0, G):
    """The whole loop: groups of G consecutive documents as the calls.  Returns (exits (N,), log as a dict of stacked arrays, final p)."""
    table, bad, path = np.asarray(table, np.float64), np.asarray(bad), np.asarray(path, np.float64)
    E1, N = table.shape
    E = E1 - 1
    G = min(G, N)
    state = (np.float64(p0), 0, 0, 0, 0)
    thr = thresholds(path, p0, sign)
    exits = np.zeros(N, np.int32)
    rows = []
    for g, n0 in enumerate(range(0, N, G)):
        cnt = min(G, N - n0)
        ex = exits_of(table[:, n0:n0 + cnt], thr, sign)
        exits[n0:n0 + cnt] = ex
        sel = A.selected(cut, (seed + g) & 0xFFFFFFFF, np.arange(cnt))
        early = sel & (ex < E)
        lost = early & (bad[ex, n0 + np.arange(cnt)] != 0)
        tal = np.concatenate([[int(sel.sum()), int(lost.sum())], np.bincount(ex[early], minlength=E)[:E], np.bincount(ex[early & ~lost], minlength=E)[:E]])
        row, state, thr = advance(path, sign, alpha, gamma, state, tal, thr)
        rows.append(row)
    log = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}
    return exits, log, state[0]


def excess(log, alpha):
    """Running sum of (disagree / sampled - alpha) over the rows that sampled anybody."""
    s, d = np.asarray(log["sampled"], np.float64), np.asarray(log["disagree"], np.float64)
    return np.cumsum(np.where(s > 0, d / np.maximum(s, 1) - alpha, 0.0))


def bound(p0, gamma, alpha):
    return p0 / gamma + 1.0 - alpha
