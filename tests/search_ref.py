"""numpy restatement of the threshold search (include/mmee.h, ee_threshold_search), written from the header's text: the percentile table in
numpy's index arithmetic and its two-branch lerp, the three digit sources, both exit rules, the exit-sum buckets with their tie rule and the
strict Pareto front.  Plain loops and Python integers; nothing of the package is imported."""
import numpy as np

GRID, SAMPLED, MIXTURES = 0, 1, 2
REFERENCE, POLICY = 0, 1
_M64 = (1 << 64) - 1


def percentile_indexes(N, P):
    """(lo, hi, t) per percentile: functions of N and P only."""
    lo, hi, t = [], [], []
    step = 100.0 / (P - 1)
    for j in range(P):
        perc = 100.0 if j == P - 1 else j * step
        x = float(N - 1) * (perc / 100.0)
        if x >= N - 1:
            lo.append(N - 1), hi.append(N - 1), t.append(x + 1.0)
        else:
            f = int(np.floor(x))
            lo.append(f), hi.append(f + 1), t.append(x - f)
    return lo, hi, t


def percentile_table(conf, P):
    """(E1, P) float64: row e < E1 - 1 the P percentiles of conf[e], row E1 - 1 zeros."""
    conf = np.asarray(conf, dtype=np.float64)
    E1, N = conf.shape
    lo, hi, t = percentile_indexes(N, P)
    table = np.zeros((E1, P))
    for e in range(E1 - 1):
        row = np.sort(conf[e])
        for j in range(P):
            a, b = np.float64(row[lo[j]]), np.float64(row[hi[j]])
            diff = b - a
            r = a + diff * np.float64(t[j])
            if t[j] >= 0.5:
                r = b - diff * (np.float64(1.0) - np.float64(t[j]))
            table[e, j] = r
    return table


def splitmix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def sampled_digit(seed, v, e, E1, P):
    z = splitmix64((seed + (v * E1 + e + 1) * 0x9E3779B97F4A7C15) & _M64)
    return ((z >> 32) * P) >> 32


def digits(source, V, E1, P, seed=0, mixtures=None):
    """(V, E1 - 1) int64: the digits of every candidate vector."""
    out = np.zeros((V, E1 - 1), dtype=np.int64)
    for v in range(V):
        for e in range(E1 - 1):
            if source == GRID:
                out[v, e] = (v // P ** e) % P
            elif source == SAMPLED:
                out[v, e] = sampled_digit(seed, v, e, E1, P)
            else:
                out[v, e] = min(int(mixtures[v, e]), P - 1)
    return out


def grid_size(E1, P):
    return P ** (E1 - 1)


def exits_of(conf, thr, semantics):
    """(N,) exits of one threshold vector (E1,)."""
    E1, N = conf.shape
    if semantics == REFERENCE:
        return (conf >= thr[:, None]).argmax(0)                     # the first that fires, 0 when none does
    fires = conf[:E1 - 1] > thr[:E1 - 1, None]
    return np.where(fires.any(0), fires.argmax(0), E1 - 1)           # strict; the final exit when nothing fires


def search(conf, correct, P, source, semantics, V=None, seed=0, mixtures=None):
    """dict: table, digits, thresholds (V,E1), hits (V,), exit_sum (V,), and the front (exit_sum, hits, vector, thresholds), ascending."""
    conf = np.asarray(conf, dtype=np.float64)
    correct = np.asarray(correct)
    E1, N = conf.shape
    if source == GRID:
        V = grid_size(E1, P)
    table = percentile_table(conf, P)
    dg = digits(source, V, E1, P, seed, mixtures)
    thr = np.zeros((V, E1))
    thr[:, :E1 - 1] = table[np.arange(E1 - 1)[None, :], dg]
    hits = np.zeros(V, dtype=np.int64)
    sums = np.zeros(V, dtype=np.int64)
    for v in range(V):
        ex = exits_of(conf, thr[v], semantics)
        hits[v] = int(correct[ex, np.arange(N)].sum())
        sums[v] = int(ex.sum())
    front = pareto_front(hits, sums, N * (E1 - 1) + 1)
    return dict(table=table, digits=dg, thresholds=thr, hits=hits, exit_sum=sums, front_exit_sum=front[0], front_hits=front[1],
                front_vector=front[2], front_thresholds=thr[front[2]] if len(front[2]) else np.zeros((0, E1)))


def pareto_front(hits, sums, n_buckets):
    """bucket[exit_sum] = max over v of hits << 32 | (0xFFFFFFFF - v); ascending scan, kept iff the hits exceed every lower bucket's."""
    bucket = {}
    for v in range(len(hits)):
        assert 0 <= sums[v] < n_buckets
        w = (int(hits[v]) << 32) | (0xFFFFFFFF - v)
        if w > bucket.get(int(sums[v]), 0):
            bucket[int(sums[v])] = w
    f_sum, f_hits, f_vec = [], [], []
    best = -1
    for s in sorted(bucket):
        h = bucket[s] >> 32
        if h > best:
            f_sum.append(s), f_hits.append(h), f_vec.append(0xFFFFFFFF - (bucket[s] & 0xFFFFFFFF))
            best = h
    return np.array(f_sum, dtype=np.int64), np.array(f_hits, dtype=np.int64), np.array(f_vec, dtype=np.int64)
