"""Float64 numpy restatement of the weighted exit-head objective of include/mmee.h (ee_head_fit_weighted, ee_mlp_head_fit_weighted), its
gradient for both head types and both objectives, and a reference solution of the one-layer problem by scipy.

    L(theta) = (1 / W) sum_n w_n l_n(theta) + (l2 / 2) ||theta||^2,        W = sum_n w_n > 0,  w_n >= 0

l_n is the row loss of the unweighted fit: logsumexp(z_n) - z_n[y_n] when ``t`` is None (tests/headfit_ref.py, tests/mlp_headfit_ref.py), else
the mixed (1 - alpha) CE + alpha T^2 KL row loss of tests/distill_headfit_ref.py.  A row of weight zero is not looked at: its label and its
teacher row may hold anything.  ``w`` is the weight row of ONE exit, (N,)."""
import numpy as np

from . import distill_headfit_ref as DR
from . import headfit_ref as HR
from . import mlp_headfit_ref as MR


def row_terms(z, t, y, alpha, T, w):
    """The weighted rows' losses w_n l_n (N,) and w_n dl_n/dz (N,K) from the logits z (N,K); rows of weight zero are zeros and their labels
    and teacher rows are never touched."""
    z = np.asarray(z, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    keep = np.flatnonzero(w != 0.0)
    rows, D = np.zeros(z.shape[0]), np.zeros_like(z)
    zk = z[keep]
    yk = None if y is None else np.asarray(y).reshape(-1)[keep]
    if t is None:
        _, p, lse = DR._log_softmax(zk)
        r = lse - zk[np.arange(len(keep)), yk]
        d = p.copy()
        d[np.arange(len(keep)), yk] -= 1.0
    else:
        r, d = DR.row_terms(zk, np.asarray(t)[keep], yk, alpha, T)
    rows[keep] = w[keep] * r
    D[keep] = w[keep, None] * d
    return rows, D


def loss_grad(theta, X, y, K, l2, w, t=None, alpha=0.0, T=1.0):
    """(L, grad L) of the one-layer head; theta = W (K,H) row-major, then b (K,)."""
    X = np.asarray(X, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    W = float(np.asarray(w, dtype=np.float64).sum())
    rows, D = row_terms(HR.logits(theta, X, K), t, y, alpha, T, w)
    loss = float(rows.sum() / W + 0.5 * l2 * np.dot(theta, theta))
    g = np.concatenate([(D.T @ X).reshape(-1), D.sum(axis=0)]) / W + l2 * theta
    return loss, g


def mlp_loss_grad(theta, X, y, K, l2, w, t=None, alpha=0.0, T=1.0):
    """(L, grad L) of the two-layer head; theta = W1 (H,H) row-major, b1, W2 (K,H) row-major, b2."""
    X = np.asarray(X, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    H = X.shape[1]
    Wsum = float(np.asarray(w, dtype=np.float64).sum())
    W1, b1, W2, b2 = MR.split(theta, K, H)
    A = np.tanh(X @ W1.T + b1)
    rows, D = row_terms(A @ W2.T + b2, t, y, alpha, T, w)
    loss = float(rows.sum() / Wsum + 0.5 * l2 * np.dot(theta, theta))
    dA = (D @ W2) * (1.0 - A * A)
    g = MR.join(dA.T @ X, dA.sum(axis=0), D.T @ A, D.sum(axis=0)) / Wsum + l2 * theta
    return loss, g


def solve(X, y, K, l2, w, t=None, alpha=0.0, T=1.0):
    """The optimum of the weighted one-layer problem by scipy L-BFGS-B on the restatement (gtol 1e-12, ftol 1e-15, maxiter 5000), started
    again from its own result at most three times, exactly as headfit_ref.solve.  Asserts a float64 gradient norm <= 1e-8."""
    from scipy.optimize import minimize
    X = np.asarray(X, dtype=np.float64)
    x = np.zeros(K * X.shape[1] + K)
    args = (X, y, K, l2, w, t, alpha, T)
    for _ in range(4):
        r = minimize(loss_grad, x, args=args, jac=True, method="L-BFGS-B", options=dict(gtol=1e-12, ftol=1e-15, maxiter=5000))
        x = r.x
        gn = float(np.linalg.norm(loss_grad(x, *args)[1]))
        if gn <= 1e-8:
            break
    assert gn <= 1e-8, f"the scipy reference stopped at a gradient norm of {gn:.3e} > 1e-8 ({r.message})"
    return x


# ---- the weight families of the tests; S: the slab height (capi.HEAD_FIT_SLAB); each returns (E,N) float32 ------------------------------------
def family_uniform(rng, E, N):
    """(a) uniform float32 in [0.25, 4), the same row for every exit"""
    return np.tile(rng.uniform(0.25, 4.0, N).astype(np.float32), (E, 1))


def family_integers(rng, E, N, S):
    """(b) integers from {0,1,2,3} with zeros on the first row, on the last row of a slab and on row N - 1 -- where N allows them while one
    weight stays positive"""
    w = rng.integers(0, 4, N).astype(np.float32)
    w[N // 2] = 2.0
    for n in (0, S - 1, N - 1):
        if n < N and n != N // 2:
            w[n] = 0.0
    return np.tile(w, (E, 1))


def family_one_row(rng, E, N):
    """(c) all zero but one row"""
    w = np.zeros((E, N), dtype=np.float32)
    w[:, int(rng.integers(0, N))] = 1.5
    return w


def family_zero_slab(rng, E, N, S):
    """(d) one whole slab of zeros (the second), N > 2 S"""
    assert N > 2 * S
    w = rng.uniform(0.25, 4.0, N).astype(np.float32)
    w[S:2 * S] = 0.0
    return np.tile(w, (E, 1))


def family_per_exit(rng, E, N):
    """(e) a different table per exit: uniform in [0.25, 4) with a different quarter of the rows at zero"""
    w = rng.uniform(0.25, 4.0, (E, N)).astype(np.float32)
    for e in range(E):
        w[e, (np.arange(N) + e) % 4 == 0] = 0.0
    if N < 4:
        w[:, -1] = 1.0
    return w
