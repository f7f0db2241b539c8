"""Float64 numpy restatement of the two-layer exit-head objective of include/mmee.h (ee_mlp_head_fit), its gradient, the identity start, a
port of the L-BFGS controller as the header states it, and the seeded problems of the tests.

    a_n = tanh(W1 x_n + b1),  z_n = W2 a_n + b2
    L(theta) = (1/N) sum_n [logsumexp(z_n) - z_n[y_n]] + (l2 / 2) ||theta||^2

theta is one vector: W1 (H,H) row-major [out,in], b1 (H,), W2 (K,H) row-major, b2 (K,) -- the layout of ee_debug_mlp_head_lossgrad."""
import numpy as np

ARMIJO = 1e-4
ARMIJO_SLACK = 8.0 * np.finfo(np.float64).eps
MAX_HALVINGS = 30


def param_count(H, K):
    return H * H + H + K * H + K


def split(theta, K, H):
    theta = np.asarray(theta, dtype=np.float64)
    o1, o2, o3 = H * H, H * H + H, H * H + H + K * H
    return theta[:o1].reshape(H, H), theta[o1:o2], theta[o2:o3].reshape(K, H), theta[o3:o3 + K]


def join(W1, b1, W2, b2):
    return np.concatenate([np.asarray(W1, np.float64).reshape(-1), np.asarray(b1, np.float64).reshape(-1),
                           np.asarray(W2, np.float64).reshape(-1), np.asarray(b2, np.float64).reshape(-1)])


def init_identity(H, K):
    """W1 = I, b1 = 0, W2 = 0, b2 = 0: the one-layer head on tanh(x)."""
    return join(np.eye(H), np.zeros(H), np.zeros((K, H)), np.zeros(K))


def logits(theta, X, K):
    X = np.asarray(X, dtype=np.float64)
    W1, b1, W2, b2 = split(theta, K, X.shape[1])
    return np.tanh(X @ W1.T + b1) @ W2.T + b2


def loss_grad(theta, X, y, K, l2):
    """(L, grad L) in float64; the logsumexp is max-shifted."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y).reshape(-1)
    N, H = X.shape
    theta = np.asarray(theta, dtype=np.float64)
    W1, b1, W2, b2 = split(theta, K, H)
    A = np.tanh(X @ W1.T + b1)
    z = A @ W2.T + b2
    m = z.max(axis=1, keepdims=True)
    ez = np.exp(z - m)
    s = ez.sum(axis=1, keepdims=True)
    lse = (m + np.log(s))[:, 0]
    loss = float(np.mean(lse - z[np.arange(N), y]) + 0.5 * l2 * np.dot(theta, theta))
    D = ez / s
    D[np.arange(N), y] -= 1.0
    dA = (D @ W2) * (1.0 - A * A)
    g = join(dA.T @ X, dA.sum(axis=0), D.T @ A, D.sum(axis=0)) / N + l2 * theta
    return loss, g


def lbfgs(fun, theta0, gtol, max_evals, history=8):
    """The controller of head_fit_controller_kernel as include/mmee.h states it: Armijo test (c1 = 1e-4, the 8 eps |L| allowance), halving,
    first step 1 / ||g||, every later one from 1, a pair with s.y <= 0 skipped, two-loop recursion scaled by gamma = s.y / y.y of the last
    kept pair, restart from steepest descent when the direction is no descent, 30 halvings.  ``fun(theta) -> (L, grad L)``.
    Returns (theta, L, ||grad L||, evaluations, status, the losses of the accepted points)."""
    trial = np.array(theta0, dtype=np.float64)
    theta = g = d = None
    f = dg = gnorm = 0.0
    step, gamma, halvings, evals, stop = 1.0, 0.0, 0, 0, 0
    pairs, accepted = [], []                            # (s, y, rho), oldest first
    while not stop:
        f_trial, g_trial = fun(trial)
        evals += 1
        first = evals == 1
        if not first and not (f_trial <= f + ARMIJO * step * dg + ARMIJO_SLACK * abs(f)):       # a NaN trial loss halves too
            halvings += 1
            step *= 0.5
            stop = 3 if halvings >= MAX_HALVINGS else 2 if evals >= max_evals else 0
            if not stop:
                trial = theta + step * d
            continue
        if not first:
            s_, y_ = trial - theta, g_trial - g
            sy, yy = float(s_ @ y_), float(y_ @ y_)
            if sy > 0.0:
                if len(pairs) == history:
                    pairs.pop(0)
                pairs.append((s_, y_, 1.0 / sy))
                gamma = sy / yy
        theta, g, f = trial, np.asarray(g_trial, dtype=np.float64), float(f_trial)
        accepted.append(f)
        gg = float(g @ g)
        gnorm = np.sqrt(gg)
        halvings = 0
        stop = 1 if gnorm <= gtol else 2 if evals >= max_evals else 0
        if stop:
            break
        d = g.copy()
        alpha = []
        for s_, y_, rho in reversed(pairs):
            al = rho * float(s_ @ d)
            alpha.append(al)
            d -= al * y_
        if pairs:
            d *= gamma
        for (s_, y_, rho), al in zip(pairs, reversed(alpha)):
            beta = rho * float(y_ @ d)
            d += (al - beta) * s_
        d = -d
        dg = float(g @ d)
        if not dg < 0.0:
            d, dg, pairs = -g, -gg, []
        step = 1.0 / gnorm if first else 1.0
        trial = theta + step * d
    return theta, f, gnorm, evals, stop - 1, accepted


def problem(N, H, K, E, seed):
    """Features (E,N,H) float32 and labels (N,) of a seeded two-layer teacher on the clean rows plus Gumbel noise; exit e sees the clean rows
    plus noise that shrinks to nothing at the last exit."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((N, H))
    T1 = rng.standard_normal((H, H)) * 1.5 / np.sqrt(H)
    T2 = rng.standard_normal((K, H)) * 4 / np.sqrt(H)
    y = (np.tanh(base @ T1.T) @ T2.T + 0.5 * rng.gumbel(size=(N, K))).argmax(axis=1).astype(np.int64)
    X = np.stack([(base + 0.5 * (E - 1 - e) * rng.standard_normal((N, H))).astype(np.float32) for e in range(E)])
    return X, y
