"""Risk control restated (include/mmee.h, "Risk control"): numpy and math.lgamma, the exit rule as a plain loop over documents and exits.
What ee_risk_control and ee_binomial_bounds compute, with no device and none of their code."""
import math

import numpy as np

ONE = 1 << 30
BINOMIAL, HB = 0, 1
FIXED_SEQUENCE, BONFERRONI = 0, 1


def quantise(loss):
    """float (E1,N) in [0,1] -> integer units of 2^-30, rounded up: min(2^30, ceil(l 2^30))."""
    loss = np.asarray(loss, dtype=np.float64)
    assert np.isfinite(loss).all() and loss.min() >= 0 and loss.max() <= 1
    return np.minimum(ONE, np.ceil(loss * ONE)).astype(np.int64)


def exits_of(conf, sign, thr):
    """(N,) exits of one threshold vector: the first e < E1-1 with sign conf[e,n] > sign thr[e] (strict; NaN never fires), else E1-1."""
    E1, N = conf.shape
    out = np.empty(N, dtype=np.int64)
    for n in range(N):
        ex = E1 - 1
        for e in range(E1 - 1):
            if sign * conf[e, n] > sign * thr[e]:
                ex = e
                break
        out[n] = ex
    return out


def counts(conf, sign, loss_q, cost, thr):
    """Per vector: loss_sum, exit_sum, cost_sum (Python ints) and hist (V,E1)."""
    E1, N = conf.shape
    V = len(thr)
    loss_sum, exit_sum, cost_sum, hist, exits = [], [], [], np.zeros((V, E1), dtype=np.int64), []
    cols = np.arange(N)
    for v in range(V):
        ex = exits_of(conf, sign, thr[v])
        exits.append(ex)
        loss_sum.append(int(np.asarray(loss_q, dtype=np.int64)[ex, cols].sum()))
        exit_sum.append(int(ex.sum()))
        cost_sum.append(int(ex.sum()) if cost is None else sum(int(c) for c in np.asarray(cost)[ex, cols]))
        hist[v] = np.bincount(ex, minlength=E1)
    return loss_sum, exit_sum, cost_sum, hist, exits


def xmul(c, log_value):
    return 0.0 if c == 0 else c * log_value


def binom_cdf_table(n, theta, upto=None):
    """F[k] = sum_{i <= k} exp(lgamma(n+1) - lgamma(i+1) - lgamma(n-i+1) + i log theta + (n-i) log1p(-theta)), k = 0 .. upto (default n),
    summed ascending in float64, clamped to 1."""
    upto = n if upto is None else upto
    lt = math.log(theta) if theta > 0 else -math.inf
    l1 = math.log1p(-theta) if theta < 1 else -math.inf
    lgn = math.lgamma(n + 1)
    terms = np.array([math.exp(lgn - math.lgamma(i + 1) - math.lgamma(n - i + 1) + xmul(i, lt) + xmul(n - i, l1)) for i in range(upto + 1)])
    return np.minimum(np.cumsum(terms), 1.0)


def kl(a, b):
    t1 = a * math.log(a / b) if a > 0 else 0.0
    t2 = (1 - a) * math.log((1 - a) / (1 - b)) if 1 - a > 0 else 0.0
    return t1 + t2


def pvalues(loss_sum, n, alpha, bound, F=None):
    F = binom_cdf_table(n, alpha) if F is None else F
    out = []
    for ls in loss_sum:
        if bound == BINOMIAL:
            out.append(float(F[min(ls >> 30, n)]))
        else:
            r = ls / (n * float(ONE))
            p_h = math.exp(-n * kl(r, alpha)) if r < alpha else 1.0
            p_b = min(1.0, math.e * float(F[min((ls + ONE - 1) >> 30, n)]))
            out.append(min(p_h, p_b))
    return np.array(out)


def levels(V, delta, method):
    return delta / V if method == BONFERRONI else delta


def certify(p, cost_sum, delta, method):
    """(certified (V,) bool, n_certified, selected)."""
    V = len(p)
    ok = p <= levels(V, delta, method)
    if method == FIXED_SEQUENCE:
        ok = np.cumprod(ok).astype(bool)
    best = -1
    for v in range(V):
        if ok[v] and (best < 0 or cost_sum[v] < cost_sum[best]):
            best = v
    return ok, int(ok.sum()), best


def control(conf, sign, loss_q, cost, thr, alpha, delta, bound, method):
    loss_sum, exit_sum, cost_sum, hist, exits = counts(conf, sign, loss_q, cost, thr)
    p = pvalues(loss_sum, conf.shape[1], alpha, bound)
    ok, n_ok, best = certify(p, cost_sum, delta, method)
    return dict(loss_sum=loss_sum, exit_sum=exit_sum, cost_sum=cost_sum, hist=hist, exits=exits, pvalue=p, certified=ok, n_certified=n_ok,
                selected=best)


def away_from_levels(p, V, delta, rel=1e-6):
    """The precondition of comparing certified masks exactly: no p-value within ``rel`` relative of the level either method tests it at."""
    return all(abs(x - lv) > rel * lv for x in p for lv in (delta, delta / V))


def _cdf_at(n, k, theta):
    return float(binom_cdf_table(n, theta, upto=k)[k])


def bounds(n, k, delta):
    """(upper, lower): one-sided Clopper-Pearson, 64 bisections of [0,1] each, the midpoint of the last bracket."""
    up, low = 1.0, 0.0
    if k < n:
        lo, hi = 0.0, 1.0
        for _ in range(64):
            mid = 0.5 * (lo + hi)
            if _cdf_at(n, k, mid) > delta:
                lo = mid
            else:
                hi = mid
        up = 0.5 * (lo + hi)
    if k > 0:
        lo, hi = 0.0, 1.0
        for _ in range(64):
            mid = 0.5 * (lo + hi)
            if 1.0 - _cdf_at(n, k - 1, mid) < delta:
                lo = mid
            else:
                hi = mid
        low = 0.5 * (lo + hi)
    return up, low


def synthetic_table(seed, E1, N):
    """The beta-confidence table of tests/test_gpu_search.py with agree ~ Bernoulli(clip(0.35 + 0.6 conf, 0, 1)) and the final row all 1."""
    rng = np.random.default_rng(seed)
    conf = rng.beta(2.0 + np.arange(E1)[:, None] * 1.5, 2.0, (E1, N))
    agree = (rng.random((E1, N)) < np.clip(0.35 + 0.6 * conf, 0.0, 1.0)).astype(np.uint8)
    agree[E1 - 1] = 1
    return conf, agree
