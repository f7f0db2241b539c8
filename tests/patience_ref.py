"""numpy restatement of the patience (PABEE) semantics of include/mmee.h, the oracle of tests/test_host_patience.py and
tests/test_gpu_patience.py.  The reference declares the strategy but implements none, so there is no reference output to pin against:
these lines ARE the specification, written independently of the kernels."""
import numpy as np


def run_counters(store):
    """store (E1,N,K) -> (p (E1,N) argmax with the first maximum winning, c (E1,N) run counters: c_0 = 0, c_e = c_{e-1} + 1 if p_e == p_{e-1})."""
    p = np.asarray(store).argmax(-1)
    c = np.zeros(p.shape, dtype=np.int64)
    for e in range(1, p.shape[0]):
        c[e] = np.where(p[e] == p[e - 1], c[e - 1] + 1, 0)
    return p, c


def patience_exits(store, t):
    """First exit e with c_e >= t, else the last exit E = E1 - 1."""
    _, c = run_counters(store)
    hit = c >= t
    hit[-1] = True
    return hit.argmax(0).astype(np.int32)


def max_softmax(z):
    """float64 max-softmax over the last axis, summed in label order (as the kernels sum)."""
    z = np.asarray(z, dtype=np.float64)
    m = z.max(-1, keepdims=True)
    s = np.zeros(z.shape[:-1])
    for k in range(z.shape[-1]):
        s = s + np.exp(z[..., k] - m[..., 0])
    return 1.0 / s


def patience_policy(store, t):
    """(exits int32 (N,), predictions (N,K), confidence float64 (N,), counts (E1,)) of the patience policy on a dumped array."""
    store = np.asarray(store, dtype=np.float64)
    ex = patience_exits(store, t)
    pred = store[ex, np.arange(store.shape[1])]
    return ex, pred, max_softmax(pred), np.bincount(ex, minlength=store.shape[0])


def patience_sweep(store, refs, patiences):
    """Per patience value: (hits, exit sum, histogram) as integers, and accuracy / mean exit as integer sums over N."""
    p, c = run_counters(store)
    E1, N = p.shape
    hits, sums, hist = [], [], []
    for t in patiences:
        hit = c >= t
        hit[-1] = True
        ex = hit.argmax(0)
        hits.append(int((p[ex, np.arange(N)] == refs).sum()))
        sums.append(int(ex.sum()))
        hist.append(np.bincount(ex, minlength=E1))
    hits, sums = np.array(hits), np.array(sums)
    return hits / N, sums / N, np.array(hist, dtype=np.int32), hits, sums
