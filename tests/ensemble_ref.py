"""Numpy restatement of the exit ensemble (include/mmee.h, at ee_set_ensemble) and of the objective ee_ensemble_fit minimises, with its
gradient and a reference optimum.  A plain module: nothing here touches the library or a device.

    x_e = float32(float64(z_e) / T_e)                  the scaled row as the path writes it out
    l_e = (x_e - M) - log(S)                           float64; M = max_k x_e, S = sum_k exp(x_e - M) in label order
    a_m = b[m] + sum_{j <= m} w[m][j] l_j              float64, j ascending from b[m]
    y_m = float32(a_m)

numpy has no fused multiply-add: a_m here rounds every product, the device does not.  The difference is a few float64 ulps of the largest
term, far below the float32 rounding of y_m, and can move that rounding by one place at most -- the tests compare y within one float32 ulp.
"""
import numpy as np

F64 = np.float64


def scaled(z, temperatures=None):
    """(E1,N,K) float32 logits and (E1,) temperatures -> the scaled rows x (float32), as dump-all stores them."""
    z = np.asarray(z, np.float32)
    if temperatures is None:
        return z.copy()
    t = np.asarray(temperatures, F64).reshape((-1,) + (1,) * (z.ndim - 1))
    return (z.astype(F64) / t).astype(np.float32)


def logsoftmax64(x):
    """The max-shifted float64 log-softmax over the last axis, summed in label order."""
    x = np.asarray(x, F64)
    m = x.max(-1, keepdims=True)
    s = np.zeros(x.shape[:-1] + (1,), F64)
    for k in range(x.shape[-1]):
        s[..., 0] += np.exp(x[..., k] - m[..., 0])
    return (x - m) - np.log(s)


def combine(l, w, b=None):
    """l (E1,N,K) float64, w (E1,E1), b (E1,K) or None -> a (E1,N,K) float64, accumulated j ascending from b[m]."""
    l, w = np.asarray(l, F64), np.asarray(w, F64)
    E1, N, K = l.shape
    a = np.zeros((E1, N, K), F64)
    for m in range(E1):
        acc = np.zeros((N, K), F64) if b is None else np.broadcast_to(np.asarray(b, F64)[m], (N, K)).copy()
        with np.errstate(invalid="ignore"):
            for j in range(m + 1):
                acc = acc + w[m, j] * l[j]
        a[m] = acc
    return a


def ensemble(x, w, b=None):
    """x (E1,N,K): scaled rows -> y (E1,N,K) float32.  A NaN row gives NaN from that exit on (0 * NaN is NaN)."""
    return combine(logsoftmax64(x), w, b).astype(np.float32)


def check_weights(w):
    w = np.asarray(w, F64)
    assert w.ndim == 2 and w.shape[0] == w.shape[1] and np.isfinite(w).all() and not np.triu(w, 1).any()
    return w


def random_weights(E1, K, seed=0, holes=True):
    """A non-trivial lower-triangular w with zeros below the diagonal in places, and a b."""
    rng = np.random.default_rng(seed)
    w = np.tril(rng.uniform(0.1, 0.9, (E1, E1)))
    w[np.arange(E1), np.arange(E1)] = rng.uniform(0.8, 1.5, E1)
    if holes:
        for m in range(2, E1):
            w[m, rng.integers(0, m)] = 0.0
    return w, rng.normal(0.0, 0.3, (E1, K))


def ulp_close_f32(got, want):
    """got == want or a float32 neighbour of it, NaN matching NaN; -> (ok mask, count of neighbours)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    near = (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))
    return same | near, int((~same & near).sum())


# ---- the fit's objective -------------------------------------------------------------------------------------------------------------------
def plain_nll(l, y):
    """(E1,) mean NLL of the plain exits from l = logsoftmax rows (E1,N,K)."""
    N = l.shape[1]
    return -l[:, np.arange(N), y].mean(1)


def pack(w_m, b_m):
    return np.concatenate([np.asarray(b_m, F64), np.asarray(w_m, F64)])


def objective(theta, l, y, m, l2):
    """L_m and its gradient at theta = [b_m (K), w_m[0 .. m] (m + 1)] -- the free parameters only.  l (E1,N,K) float64, y (N,)."""
    E1, N, K = l.shape
    b, w = theta[:K], theta[K:]
    assert w.shape == (m + 1,)
    a = b[None, :] + np.tensordot(w, l[:m + 1], axes=(0, 0))                   # (N,K)
    mx = a.max(1, keepdims=True)
    e = np.exp(a - mx)
    s = e.sum(1, keepdims=True)
    rows = np.arange(N)
    e_m = np.zeros(m + 1)
    e_m[m] = 1.0
    loss = ((mx[:, 0] + np.log(s[:, 0])) - a[rows, y]).mean() + 0.5 * l2 * (((w - e_m) ** 2).sum() + (b ** 2).sum())
    d = e / s
    d[rows, y] -= 1.0
    gb = d.mean(0) + l2 * b
    gw = np.einsum("nk,jnk->j", d, l[:m + 1]) / N + l2 * (w - e_m)
    return loss, np.concatenate([gb, gw])


def hessian(theta, l, y, m, l2):
    E1, N, K = l.shape
    b, w = theta[:K], theta[K:]
    a = b[None, :] + np.tensordot(w, l[:m + 1], axes=(0, 0))
    p = np.exp(a - a.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    # da/dtheta: J[n, k, :] = [e_k (K), l_j[n][k] (m + 1)]
    P = K + m + 1
    J = np.zeros((N, K, P))
    J[:, np.arange(K), np.arange(K)] = 1.0
    J[:, :, K:] = np.transpose(l[:m + 1], (1, 2, 0))
    pj = np.einsum("nk,nkp->np", p, J)
    H = np.einsum("nk,nkp,nkq->pq", p, J, J) - pj.T @ pj
    return H / N + l2 * np.eye(P)


def start(m, K):
    th = np.zeros(K + m + 1)
    th[K + m] = 1.0
    return th


def reference_optimum(l, y, m, l2, polish=8):
    """scipy L-BFGS-B from the start, then Newton steps: (theta*, loss*, |grad|)."""
    from scipy.optimize import minimize
    K = l.shape[2]
    f = lambda th: objective(th, l, y, m, l2)
    r = minimize(f, start(m, K), jac=True, method="L-BFGS-B", options=dict(maxiter=2000, ftol=1e-15, gtol=1e-10))
    th = r.x
    for _ in range(polish):
        _, g = f(th)
        if np.linalg.norm(g) <= 1e-13:
            break
        th = th - np.linalg.solve(hessian(th, l, y, m, l2), g)
    loss, g = f(th)
    return th, loss, float(np.linalg.norm(g))


def full_theta(w, b, m):
    """Row m of a fit's (w (E1,E1), b (E1,K)) as the free-parameter vector of `objective`."""
    return pack(np.asarray(w, F64)[m, :m + 1], np.asarray(b, F64)[m])
