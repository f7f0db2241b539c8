"""Float64 numpy restatement of the two-layer gate objective of include/mmee.h (ee_mlp_head_fit_gate, ee_mlp_head_fit_gate_weighted), its
gradient, and the seeded problems of the tests.  Written from the header's text, independently of the kernels; the parameter layout, the
identity start and the port of the L-BFGS controller are tests/mlp_headfit_ref.py's (split / join / init_identity / lbfgs) at K = 2.

    a_n = tanh(W1 x_n + b1),  z_n = W2 a_n + b2 in R^2                          column 1 is "correctly gated"
    L(theta) = (1 / (2 W)) sum_n w_n [bce(z_n1, c_n) + bce(z_n0, 1 - c_n)] + (l2 / 2) ||theta||^2,   W = sum_n w_n   (w = 1: W = N)
    bce(z, t) = max(z, 0) + log1p(exp(-|z|)) - t z

A row of weight zero is not looked at beyond its features: its target may be NaN."""
import numpy as np

from . import mlp_headfit_ref as MR

K = 2


def param_count(H):
    return MR.param_count(H, K)


def init_identity(H):
    return MR.init_identity(H, K)


def logits(theta, X):
    return MR.logits(theta, np.asarray(X, np.float32), K)


def loss_grad(theta, X, c, l2, w=None):
    """theta (P,), X (N,H) float32, c (N,) targets in [0,1], w (N,) weights or None -> (L, grad L (P,)) in float64."""
    X = np.asarray(X, np.float32).astype(np.float64)
    N, H = X.shape
    theta = np.asarray(theta, np.float64)
    W1, b1, W2, b2 = MR.split(theta, K, H)
    w = np.ones(N) if w is None else np.asarray(w, np.float32).astype(np.float64)
    live = w > 0.0
    c = np.where(live, np.asarray(c, np.float64), 0.0)                       # a dead row's target is not looked at
    t = np.stack([1.0 - c, c], 1)
    A = np.tanh(X @ W1.T + b1)
    z = A @ W2.T + b2
    ez = np.exp(-np.abs(z))
    bce = np.maximum(z, 0.0) + np.log1p(ez) - t * z
    sig = np.where(z >= 0.0, 1.0, ez) / (1.0 + ez)
    wn = (w / (2.0 * w.sum()))[:, None]                                      # the row's share of the data term
    loss = float((wn * bce).sum() + 0.5 * l2 * np.dot(theta, theta))
    D = wn * (sig - t)                                                       # dL/dz
    dA = (D @ W2) * (1.0 - A * A)
    g = MR.join(dA.T @ X, dA.sum(0), D.T @ A, D.sum(0)) + l2 * theta
    return loss, g


def problem(E, N, H):
    """The recipe of tests/test_gpu_gate_fit.py: unit-variance rows, targets from a planted direction; exit 0 hard (0 / 1), exit 1 soft (in
    [0,1]), exit 2 all ones; a single exit is hard at odd N and soft at even N.  -> X (E,N,H) float32, T (E,N) float64"""
    rng = np.random.default_rng(1000 * E + 10 * N + H)
    X = rng.standard_normal((E, N, H)).astype(np.float32)
    w = rng.standard_normal((E, H)) / np.sqrt(H)
    p = 1.0 / (1.0 + np.exp(-(2.0 * np.einsum("enh,eh->en", X.astype(np.float64), w) + 0.3)))
    T = np.empty((E, N))
    for e in range(E):
        kind = ("hard", "soft", "ones")[e % 3] if E > 1 else ("hard" if N % 2 else "soft")
        T[e] = (rng.random(N) < p[e]).astype(np.float64) if kind == "hard" else p[e] if kind == "soft" else 1.0
    return X, T


def kinds(E, N):
    return [("hard", "soft", "ones")[e % 3] if E > 1 else ("hard" if N % 2 else "soft") for e in range(E)]


def port(X, c, l2, gtol, max_evals, w=None, theta0=None):
    """MR.lbfgs on the restated objective from the identity start -> (theta, L, ||grad L||, evaluations, status, accepted losses)"""
    H = np.shape(X)[1]
    return MR.lbfgs(lambda th: loss_grad(th, X, c, l2, w), init_identity(H) if theta0 is None else theta0, gtol, max_evals)
