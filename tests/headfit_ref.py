"""Float64 numpy restatement of the exit-head objective of include/mmee.h (ee_head_fit), its gradient, and a reference solution by scipy.

    L(theta) = (1/N) sum_n [logsumexp(z_n) - z_n[y_n]] + (l2 / 2)(||W||^2 + ||b||^2),      z_n = W x_n + b,  theta = (W (K,H), b (K,))

theta is one vector: W row-major, then b -- the layout of ee_debug_head_lossgrad."""
import numpy as np


def split(theta, K, H):
    theta = np.asarray(theta, dtype=np.float64)
    return theta[:K * H].reshape(K, H), theta[K * H:K * H + K]


def logits(theta, X, K):
    X = np.asarray(X, dtype=np.float64)
    W, b = split(theta, K, X.shape[1])
    return X @ W.T + b


def loss_grad(theta, X, y, K, l2):
    """(L, grad L) in float64; the logsumexp is max-shifted."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y).reshape(-1)
    N, H = X.shape
    theta = np.asarray(theta, dtype=np.float64)
    z = logits(theta, X, K)
    m = z.max(axis=1, keepdims=True)
    ez = np.exp(z - m)
    s = ez.sum(axis=1, keepdims=True)
    lse = (m + np.log(s))[:, 0]
    loss = float(np.mean(lse - z[np.arange(N), y]) + 0.5 * l2 * np.dot(theta, theta))
    D = ez / s
    D[np.arange(N), y] -= 1.0
    g = np.concatenate([(D.T @ X).reshape(-1), D.sum(axis=0)]) / N + l2 * theta
    return loss, g


def solve(X, y, K, l2):
    """The optimum by scipy L-BFGS-B on the restatement (gtol 1e-12, ftol 1e-15, maxiter 5000).  Asserts a float64 gradient norm <= 1e-8,
    so a reference that did not get there fails loudly instead of passing for the optimum.

    One run stops on ftol (a relative reduction of f below 1e-15) at a norm of 1e-8 ... 2e-8 for about a third of the test problems at
    l2 = 1e-2 (measured on the CPU: H = 64, 256, 768, three seeds each); the same solver with the same options, started again from its own
    result, reached 2e-9 ... 6e-9 in every such case.  So the run is repeated from where it stopped, at most three times, until the bar holds."""
    from scipy.optimize import minimize
    X = np.asarray(X, dtype=np.float64)
    x = np.zeros(K * X.shape[1] + K)
    for _ in range(4):
        r = minimize(loss_grad, x, args=(X, y, K, l2), jac=True, method="L-BFGS-B", options=dict(gtol=1e-12, ftol=1e-15, maxiter=5000))
        x = r.x
        gn = float(np.linalg.norm(loss_grad(x, X, y, K, l2)[1]))
        if gn <= 1e-8:
            break
    assert gn <= 1e-8, f"the scipy reference stopped at a gradient norm of {gn:.3e} > 1e-8 ({r.message})"
    return x


def teacher_problem(N, H, K, E, seed):
    """Unit-variance features (E,N,H) float32 and labels (N,) from a seeded teacher on the LAST exit's rows plus Gumbel noise."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((E, N, H)).astype(np.float32)
    T = rng.standard_normal((K, H)) * (2.0 / np.sqrt(H))
    y = (X[-1].astype(np.float64) @ T.T + rng.gumbel(size=(N, K))).argmax(axis=1).astype(np.int64)
    return X, y
