"""numpy restatement of budgeted exits (include/mmee.h, at MMEE_QUOTA_*): the rank of a stage's documents, the two modes, one exit of one stage
on top of exit_stage_ref, and the grouped scan with its cuts.  The reference has no such feature: the header's text is the specification and
these lines restate it, written from the text and not from the kernels -- the rank here is a sort, the device's a count.  The oracle of
tests/test_quota_ref.py and tests/test_gpu_quota.py."""
import numpy as np

from . import exit_stage_ref as R

EXACT, AT_LEAST = 1, 2                                   # MMEE_QUOTA_EXACT, MMEE_QUOTA_AT_LEAST
MODE_NAME = {EXACT: "exact", AT_LEAST: "at_least"}


def precedes(c, sign, slots=None):
    """The header's relation itself, pair by pair: P[i, j] = i precedes j.  O(n^2) memory: for small n."""
    s = sign * np.asarray(c, np.float64)
    n = len(s)
    slots = np.arange(n) if slots is None else np.asarray(slots)
    nan = np.isnan(s)
    with np.errstate(invalid="ignore"):
        gt, eq = s[:, None] > s[None, :], s[:, None] == s[None, :]
    lower = slots[:, None] < slots[None, :]
    number_first = ~nan[:, None] & nan[None, :]                          # a NaN is preceded by every number ...
    both_nan = nan[:, None] & nan[None, :]                               # ... and NaNs order among themselves by slot
    return gt | (eq & lower) | number_first | (both_nan & lower)


def rank(c, sign, slots=None):
    """rank_i = the number of documents that precede i: larger sign * c first, ties by rising slot, NaN last (by slot).  A stable sort."""
    s = sign * np.asarray(c, np.float64) + 0.0                           # -0.0 == +0.0
    n = len(s)
    slots = np.arange(n) if slots is None else np.asarray(slots)
    nan = np.isnan(s)
    order = np.lexsort((slots, np.where(nan, 0.0, -s), nan))             # numbers before NaNs, falling s, rising slot
    r = np.empty(n, np.int64)
    r[order] = np.arange(n)
    return r


def fires(c, sign, thr):
    with np.errstate(invalid="ignore"):
        return sign * np.asarray(c, np.float64) > sign * thr             # strict; a NaN never fires


def leave(c, sign, q, mode, thr=None, slots=None):
    """(leave (n,) bool, rank (n,)) of one exit."""
    r = rank(c, sign, slots)
    lv = r < q
    if mode == AT_LEAST:
        lv = lv | fires(c, sign, thr)
    return lv, r


def decide(stage, crit, sign, q, mode, thr=None):
    """One exit of one stage of exit_stage_ref's form on criteria that are given: (leave, rank, the stage of the documents that stay)."""
    lv, r = leave(crit, sign, q, mode, thr, slots=stage["doc_orig"])
    return lv, r, R._next_stage(stage, ~lv, "")


def scan(table, sign, quotas, mode, thresholds=None, G=None):
    """The grouped scan: consecutive groups of G documents ranked independently, survivors of exit e ranked at e + 1, the last exit takes
    everybody.  (exits (N,) int32, cuts (groups, E1 - 1, 2): criterion of the last leaver / of the first stayer, NaN where there is none)."""
    t = np.asarray(table, np.float64)
    E1, N = t.shape
    G = N if G is None else G
    groups = (N + G - 1) // G if N else 0
    exits = np.full(N, E1 - 1, np.int32)
    cuts = np.full((groups, max(E1 - 1, 0), 2), np.nan)
    thr = None if thresholds is None else np.broadcast_to(np.asarray(thresholds, np.float64).reshape(-1), (E1,))
    for g in range(groups):
        active = np.arange(g * G, min(N, (g + 1) * G))
        for e in range(E1 - 1):
            c = t[e, active]
            lv, r = leave(c, sign, quotas[e], mode, None if thr is None else thr[e])
            m = int(lv.sum())
            assert np.array_equal(lv, r < m)                             # the leavers are the top m: the event is monotone in s
            if m > 0:
                cuts[g, e, 0] = c[r == m - 1][0]
            if m < len(active):
                cuts[g, e, 1] = c[r == m][0]
            exits[active[lv]] = e
            active = active[~lv]
    return exits, cuts


def stage_sizes(B, quotas):
    """EXACT: n_0 = B, n_{e+1} = max(0, n_e - q_e), known before the call."""
    n = [int(B)]
    for q in quotas:
        n.append(max(0, n[-1] - int(q)))
    return n


def boundary_gaps(table, sign, quotas, mode, thresholds=None):
    """The smallest distance, over the exits of a one-group scan, between the criteria on either side of the quota boundary (inf where a side
    is empty): the condition under which a device table and numpy's decide alike."""
    _, cuts = scan(table, sign, quotas, mode, thresholds)
    with np.errstate(invalid="ignore"):
        d = np.abs(cuts[0, :, 0] - cuts[0, :, 1])
    return np.where(np.isnan(d), np.inf, d)


def quotas_from_fractions(B, f):
    """q_e = R(B sum_{j <= e} f_j) - R(B sum_{j < e} f_j), R(x) = floor(x + 0.5)."""
    edges = np.floor(B * np.cumsum(np.asarray(f, np.float64)) + 0.5).astype(np.int64)
    return np.diff(np.concatenate([[0], edges])).tolist()
