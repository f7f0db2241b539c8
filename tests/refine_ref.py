"""numpy / Python-int restatement of the threshold refinement (include/mmee.h, ee_threshold_refine), written from the header's text: the
percentile table of tests/search_ref.py, the policy's exit rule, and a round that scores EVERY neighbour by a full walk of all documents --
brute force, which is the point.  ``refine(..., incremental=True)`` is a second form of the round, from the header's per-document argument
(an earlier exit takes the document for a prefix of its digits, its own exit lets it go for a suffix): the CPU tests assert the two equal, so
the argument itself is tested where no GPU is needed.  Nothing of the package is imported."""
import numpy as np

from . import search_ref as R

W_MAX = (1 << 32) - 1


def score(conf, correct, cost, table, d):
    """(hits, exit_sum, cost_sum) of digit vector d as Python ints, by a full policy walk."""
    E1, N = conf.shape
    thr = np.zeros(E1)
    thr[:E1 - 1] = table[np.arange(E1 - 1), np.asarray(d[:E1 - 1], dtype=np.int64)]
    ex = R.exits_of(conf, thr, R.POLICY)
    cols = np.arange(N)
    return int(correct[ex, cols].sum()), int(ex.sum()), int(cost[ex, cols].astype(np.int64).sum())      # < 2^56: exact in int64


def neighbours_brute(conf, correct, cost, table, d, P):
    """{(e, p): (hits, exit_sum, cost_sum)} of every vector that differs from d in digit e (p == d_e included: the vector itself)."""
    E1 = conf.shape[0]
    out = {}
    for e in range(E1 - 1):
        for p in range(P):
            dd = list(d)
            dd[e] = p
            out[(e, p)] = score(conf, correct, cost, table, dd)
    return out


def neighbours_incremental(conf, correct, cost, table, d, P):
    """The same dict from one pass over the documents: per document O(E1) pairs into difference arrays over p, then a scan."""
    E1, N = conf.shape
    base = [0, 0, 0]
    diff = [[[0, 0, 0] for _ in range(P + 1)] for _ in range(E1 - 1)]
    for n in range(N):
        k = [int((conf[e, n] > table[e]).sum()) for e in range(E1 - 1)]      # the digits whose threshold the document beats: [0, k)
        firing = [e for e in range(E1 - 1) if k[e] > d[e]]
        x0 = firing[0] if firing else E1 - 1
        x1 = firing[1] if len(firing) > 1 else E1 - 1
        val = lambda e: (int(correct[e, n]), e, int(cost[e, n]))
        v0, v1 = val(x0), val(x1)
        for j in range(3):
            base[j] += v0[j]
        for e in range(x0):
            ve = val(e)
            for j in range(3):
                diff[e][0][j] += ve[j] - v0[j]
                diff[e][k[e]][j] -= ve[j] - v0[j]
        if x0 < E1 - 1:
            for j in range(3):
                diff[x0][k[x0]][j] += v1[j] - v0[j]
    out = {}
    for e in range(E1 - 1):
        run = [0, 0, 0]
        for p in range(P):
            for j in range(3):
                run[j] += diff[e][p][j]
            out[(e, p)] = tuple(base[j] + run[j] for j in range(3))
    return out


def refine(conf, correct, cost, P, start, hit_value, budget=None, max_rounds=256, incremental=False):
    """One chain.  dict: digits (E1 ints, last 0), thresholds (E1,), hits, exit_sum, cost_sum, rounds, status, start_hits, start_cost_sum, J,
    start_J, moves = [(e, p_from, p_to)], table."""
    conf = np.asarray(conf, dtype=np.float64)
    correct = np.asarray(correct)
    E1, N = conf.shape
    cost = np.broadcast_to(np.arange(E1)[:, None], (E1, N)) if cost is None else np.asarray(cost)
    table = R.percentile_table(conf, P)
    w = min(int(hit_value), W_MAX)
    d = [min(int(x), P - 1) for x in start[:E1 - 1]] + [0]
    cur = score(conf, correct, cost, table, d)
    start_hits, start_cost = cur[0], cur[2]
    J = lambda t: w * t[0] - t[2]
    moves, status = [], 1
    if budget is not None and cur[2] > int(budget):
        status = 2
    else:
        for _ in range(max_rounds):
            nb = (neighbours_incremental if incremental else neighbours_brute)(conf, correct, cost, table, d, P)
            best = None
            for e in range(E1 - 1):
                for p in range(P):
                    if p == d[e]:
                        continue
                    t = nb[(e, p)]
                    if budget is not None and t[2] > int(budget):
                        continue
                    if best is None or J(t) > J(nb[best]):               # ties: the lowest e, then the lowest p
                        best = (e, p)
            if best is None or J(nb[best]) <= J(cur):
                status = 0
                break
            moves.append((best[0], d[best[0]], best[1]))
            d[best[0]] = best[1]
            cur = nb[best]
    thr = np.zeros(E1)
    thr[:E1 - 1] = table[np.arange(E1 - 1), np.asarray(d[:E1 - 1], dtype=np.int64)]
    return dict(digits=d, thresholds=thr, hits=cur[0], exit_sum=cur[1], cost_sum=cur[2], rounds=len(moves), status=status, start_hits=start_hits,
                start_cost_sum=start_cost, J=J(cur), start_J=w * start_hits - start_cost, moves=moves, table=table)
