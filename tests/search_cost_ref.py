"""numpy / Python-int restatement of the cost-weighted threshold search (include/mmee.h, ee_threshold_search_cost), written from the header's
text: the percentile table, the digits and the exit rules are the plain search's (tests/search_ref.py); added are cost_sum(v) as Python
integers and the front over the hits buckets with its tie rule.  Nothing of the package is imported."""
import numpy as np

from .search_ref import GRID, digits, exits_of, grid_size, percentile_table


def cost_front(hits, costs):
    """best[h] = min over {v : hits(v) = h} of (cost_sum, v), lexicographic; bucket h is kept iff its cost_sum is below that of every non-empty
    bucket with more hits.  (cost_sum, hits, vector) lists, ascending in cost_sum."""
    best = {}
    for v in range(len(hits)):
        key = (int(costs[v]), v)
        h = int(hits[v])
        if h not in best or key < best[h]:
            best[h] = key
    out = []
    lowest_above = None                                              # the lowest cost_sum among the buckets with more hits
    for h in sorted(best, reverse=True):
        c, v = best[h]
        if lowest_above is None or c < lowest_above:
            out.append((c, h, v))
            lowest_above = c
    out.reverse()
    return [c for c, _, _ in out], [h for _, h, _ in out], [v for _, _, v in out]


def search_cost(conf, correct, cost, P, source, semantics, V=None, seed=0, mixtures=None):
    """dict: table, digits, thresholds (V,E1), hits (V,), exit_sum (V,), cost_sum (V,) Python ints, and the front (cost_sum, exit_sum, hits,
    vector, thresholds), ascending in cost_sum.  ``cost`` (E1,N) non-negative integers."""
    conf = np.asarray(conf, dtype=np.float64)
    correct = np.asarray(correct)
    E1, N = conf.shape
    cost = np.asarray(cost)
    assert cost.shape == (E1, N) and int(cost.min()) >= 0 and int(cost.max()) * N < 1 << 63      # an int64 sum of N entries is then exact
    cost = cost.astype(np.int64)
    if source == GRID:
        V = grid_size(E1, P)
    table = percentile_table(conf, P)
    dg = digits(source, V, E1, P, seed, mixtures)
    thr = np.zeros((V, E1))
    thr[:, :E1 - 1] = table[np.arange(E1 - 1)[None, :], dg]
    cols = np.arange(N)
    hits, sums, costs = [], [], []
    for v in range(V):
        ex = exits_of(conf, thr[v], semantics)
        hits.append(int(correct[ex, cols].sum()))
        sums.append(int(ex.sum()))
        costs.append(int(cost[ex, cols].sum()))
    f_cost, f_hits, f_vec = cost_front(hits, costs)
    return dict(table=table, digits=dg, thresholds=thr, hits=np.array(hits, dtype=np.int64), exit_sum=np.array(sums, dtype=np.int64), cost_sum=costs,
                front_cost_sum=f_cost, front_exit_sum=[sums[v] for v in f_vec], front_hits=f_hits, front_vector=f_vec,
                front_thresholds=thr[f_vec] if f_vec else np.zeros((0, E1)))
