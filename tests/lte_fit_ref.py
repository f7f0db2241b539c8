"""Float64 numpy restatement of the LTE classifier's objective of include/mmee.h (ee_lte_fit), its gradient, the targets and the scores, and a
reference solution by scipy.

    L(theta) = sum_e (1/N) sum_n l(a_{e,n}, t_{e,n}) + (l2 / 2)(||w||^2 + b^2),     a = w . x + b,  s = 1 / (1 + exp(-a)),  theta = (w (H,), b)
    "mse":  l = (s - t)^2                               dl/da = 2 (s - t) s (1 - s)
    "bce":  l = max(a, 0) + log1p(exp(-|a|)) - t a      dl/da = s - t

theta is one vector: w, then b -- the layout of ee_debug_lte_lossgrad."""
import numpy as np

LOSSES = ("mse", "bce")
# The bar of the device's loss / gradient against this restatement (tests/test_gpu_lte_fit.py): float64 sums of at most about 1e5 terms of order 1
# and exp / log1p at a few ulp sit four orders below it.  tests/test_host_lte_fit.py shows that every subtle fault moves a figure by >= 10 bars.
RTOL, ATOL = 1e-10, 1e-12


def _sigmoid(a):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-a))            # exp(-a) = inf gives exactly 0


def activations(theta, X):
    """X (E,N,H) -> a (E,N) float64."""
    X = np.asarray(X, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    return X @ theta[:-1] + theta[-1]


def loss_grad(theta, X, T, loss, l2):
    """(L, grad L) in float64.  X (E,N,H), T (E,N)."""
    assert loss in LOSSES
    X = np.asarray(X, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    E, N, H = X.shape
    a = activations(theta, X)
    s = _sigmoid(a)
    if loss == "mse":
        l = (s - T) ** 2
        d = 2.0 * (s - T) * s * (1.0 - s)
    else:
        l = np.maximum(a, 0.0) + np.log1p(np.exp(-np.abs(a))) - T * a
        d = s - T
    L = float(l.mean(axis=1).sum() + 0.5 * l2 * np.dot(theta, theta))
    g = np.concatenate([np.einsum("en,enh->h", d, X), [d.sum()]]) / N + l2 * theta
    return L, g


def targets(logits, labels):
    """1 - [argmax == y], the first maximum winning (numpy's argmax rule).  logits (E,N,K), labels (N,) -> (E,N) float64."""
    logits = np.asarray(logits)
    return (logits.argmax(-1) != np.asarray(labels).reshape(1, -1)).astype(np.float64)


def scores(X, w, b):
    """sigmoid(w . x + b) in float64 from a float32 (w, b), every operand widened first.  X (E,N,H) -> (E,N)."""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    w = np.asarray(w, dtype=np.float32).astype(np.float64).reshape(-1)
    return _sigmoid(X @ w + float(np.asarray(b, dtype=np.float32).reshape(-1)[0]))


def _solve_from(x, X, T, loss, l2):
    from scipy.optimize import minimize
    for _ in range(4):
        r = minimize(loss_grad, x, args=(X, T, loss, l2), jac=True, method="L-BFGS-B", options=dict(gtol=1e-12, ftol=1e-15, maxiter=5000))
        x = r.x
        gn = float(np.linalg.norm(loss_grad(x, X, T, loss, l2)[1]))
        if gn <= 1e-8:
            break
    assert gn <= 1e-8, f"the scipy reference stopped at a gradient norm of {gn:.3e} > 1e-8 ({r.message})"
    return x


def solve_starts(X, T, loss, l2, n_starts=2, seed=0):
    """The stationary points scipy L-BFGS-B reaches from zero and from n_starts - 1 random starts (N(0, 1/H) weights), each restarted from
    where it stopped until the float64 gradient norm is <= 1e-8 (asserted), as headfit_ref.solve does."""
    X = np.asarray(X, dtype=np.float64)
    H = X.shape[2]
    rng = np.random.default_rng(seed)
    starts = [np.zeros(H + 1)] + [rng.standard_normal(H + 1) / np.sqrt(H) for _ in range(n_starts - 1)]
    return [_solve_from(x0, X, T, loss, l2) for x0 in starts]


def solve(X, T, loss, l2):
    """The reference solution: the point reached from zero.  A second start must land within 1e-6 of it (asserted): a problem with two basins
    fails here, in the reference, not in the kernel."""
    a, b = solve_starts(X, T, loss, l2, 2)
    d = float(np.linalg.norm(a - b))
    assert d <= 1e-6, f"two starts of the scipy reference end {d:.3e} apart: the problem has more than one basin"
    return a


def problem(N, H, E, seed):
    """X ~ N(0,1) float32 (E,N,H); v ~ N(0, 4/H); t = [X.v + off_e + logistic noise < 0], off = linspace(-0.5, 1.0, E): deeper exits are
    wrong less often."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((E, N, H)).astype(np.float32)
    v = rng.standard_normal(H) * (2.0 / np.sqrt(H))
    off = np.linspace(-0.5, 1.0, E)
    T = (X.astype(np.float64) @ v + off[:, None] + rng.logistic(size=(E, N)) < 0.0).astype(np.float64)
    return X, T


def kernel_cases():
    """Named inputs (X (E,N,H) float32, T (E,N), theta (H+1,)) the host and the device tests share: binary targets, soft targets, all targets
    equal, and activations near +-770, where exp(|a|) = inf and an unshifted softplus overflows."""
    rng = np.random.default_rng(77)
    out = {}
    N, H, E = 37, 64, 3
    X = rng.standard_normal((E, N, H)).astype(np.float32)
    theta = np.concatenate([rng.standard_normal(H) * (2.0 / np.sqrt(H)), [0.3]])
    out["binary"] = (X, (rng.random((E, N)) < 0.4).astype(np.float64), theta)
    out["soft"] = (X, rng.random((E, N)), theta)
    out["all_ones"] = (X, np.ones((E, N)), theta)
    out["all_zeros"] = (X, np.zeros((E, N)), theta)
    N, H, E = 45, 256, 2
    Xl = (np.abs(rng.standard_normal((E, N, H))) + 0.5).astype(np.float32)
    Xl[:, ::2] *= -1.0
    w = np.full(H, 770.0 / (H * float(np.abs(Xl).mean())))
    out["large"] = (Xl, (rng.random((E, N)) < 0.5).astype(np.float64), np.concatenate([w, [0.25]]))
    return out
