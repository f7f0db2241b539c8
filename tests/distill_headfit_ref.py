"""Float64 numpy restatement of the distilled exit-head objective of include/mmee.h (ee_head_fit_distill, ee_mlp_head_fit_distill), its
gradient for both head types, and a reference solution of the one-layer problem by scipy.

    z_n = head_theta(x_n)           one Linear (tests/headfit_ref.py), or dense -> tanh -> out_proj (tests/mlp_headfit_ref.py)
    q_n = softmax(t_n / T)          p_n = softmax(z_n)          pT_n = softmax(z_n / T)
    L(theta) = (1/N) sum_n [ (1 - alpha) (logsumexp(z_n) - z_n[y_n]) + alpha T^2 KL(q_n || pT_n) ] + (l2 / 2) ||theta||^2
    dL/dz_n  = (1/N) [ (1 - alpha) (p_n - onehot(y_n)) + alpha T (pT_n - q_n) ]

Every softmax is max-shifted; log q and log pT are the shifted logits minus the log of their sum of exponentials, never the log of a
probability, so a q_k that underflows to zero contributes exactly zero.  At alpha = 1 the labels are not looked at (``y`` may be None)."""
import numpy as np

from . import headfit_ref as HR
from . import mlp_headfit_ref as MR


def _log_softmax(s):
    """-> (log softmax(s), softmax(s), logsumexp(s)) along the last axis, max-shifted"""
    m = s.max(axis=1, keepdims=True)
    e = np.exp(s - m)
    tot = e.sum(axis=1, keepdims=True)
    return (s - m) - np.log(tot), e / tot, (m + np.log(tot))[:, 0]


def row_terms(z, t, y, alpha, T):
    """The data term of L without its 1/N, per row (N,), and N dL/dz (N,K), from the logits z (N,K) and the teacher's t (N,K)."""
    z = np.asarray(z, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    N = z.shape[0]
    log_q, q, _ = _log_softmax(t / T)
    log_pT, pT, _ = _log_softmax(z / T)
    kl = (q * (log_q - log_pT)).sum(axis=1)
    rows = alpha * T * T * kl
    D = alpha * T * (pT - q)
    if alpha < 1.0:
        y = np.asarray(y).reshape(-1)
        _, p, lse = _log_softmax(z)
        rows = rows + (1.0 - alpha) * (lse - z[np.arange(N), y])
        Y = np.zeros_like(p)
        Y[np.arange(N), y] = 1.0
        D = D + (1.0 - alpha) * (p - Y)
    return rows, D


def loss_grad(theta, X, t, y, K, alpha, T, l2):
    """(L, grad L) of the one-layer head; theta = W (K,H) row-major, then b (K,)."""
    X = np.asarray(X, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    N = X.shape[0]
    rows, D = row_terms(HR.logits(theta, X, K), t, y, alpha, T)
    loss = float(rows.mean() + 0.5 * l2 * np.dot(theta, theta))
    g = np.concatenate([(D.T @ X).reshape(-1), D.sum(axis=0)]) / N + l2 * theta
    return loss, g


def mlp_loss_grad(theta, X, t, y, K, alpha, T, l2):
    """(L, grad L) of the two-layer head; theta = W1 (H,H) row-major, b1, W2 (K,H) row-major, b2."""
    X = np.asarray(X, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    N, H = X.shape
    W1, b1, W2, b2 = MR.split(theta, K, H)
    A = np.tanh(X @ W1.T + b1)
    rows, D = row_terms(A @ W2.T + b2, t, y, alpha, T)
    loss = float(rows.mean() + 0.5 * l2 * np.dot(theta, theta))
    dA = (D @ W2) * (1.0 - A * A)
    g = MR.join(dA.T @ X, dA.sum(axis=0), D.T @ A, D.sum(axis=0)) / N + l2 * theta
    return loss, g


def solve(X, t, y, K, alpha, T, l2):
    """The optimum of the one-layer problem by scipy L-BFGS-B on the restatement (gtol 1e-12, ftol 1e-15, maxiter 5000), started again from
    its own result at most three times, exactly as headfit_ref.solve.  Asserts a float64 gradient norm <= 1e-8."""
    from scipy.optimize import minimize
    X = np.asarray(X, dtype=np.float64)
    x = np.zeros(K * X.shape[1] + K)
    for _ in range(4):
        r = minimize(loss_grad, x, args=(X, t, y, K, alpha, T, l2), jac=True, method="L-BFGS-B",
                     options=dict(gtol=1e-12, ftol=1e-15, maxiter=5000))
        x = r.x
        gn = float(np.linalg.norm(loss_grad(x, X, t, y, K, alpha, T, l2)[1]))
        if gn <= 1e-8:
            break
    assert gn <= 1e-8, f"the scipy reference stopped at a gradient norm of {gn:.3e} > 1e-8 ({r.message})"
    return x


def fit_problem(N, H, K, E):
    """The fit problems of the tests: features and labels of headfit_ref.teacher_problem(seed = N + H), and the teacher's logits
    t = X[-1] Wt^T with Wt = default_rng(N).standard_normal((K,H)) 2 / sqrt(H), as float32."""
    X, y = HR.teacher_problem(N, H, K, E, seed=N + H)
    Wt = np.random.default_rng(N).standard_normal((K, H)) * (2.0 / np.sqrt(H))
    t = (X[-1].astype(np.float64) @ Wt.T).astype(np.float32)
    return X, y, t
