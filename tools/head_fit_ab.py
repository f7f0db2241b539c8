"""Measurement of the exit-head fit (``heads.fit_exit_heads`` / ee_head_fit) at the shape it was built for (GPU box): N = 40 000 CLS rows,
H = 768, K = 16, E = 6 exits, features resident on the device.  No pass bar; the output is what README and DESIGN quote.

Reported:
  * milliseconds per tick (loss / gradient kernel + reduce + controller) from two fits that cannot stop early (gtol = 0) with 10 and 40
    evaluations: (t40 - t10) / 30, median of five pairs -- and GB/s on the feature bytes E N H 4 a tick reads, beside the 5.4 TB/s of the
    LayerNorm row kernel (README), the project's class for row-streaming kernels;
  * milliseconds per fit at the defaults (l2 = 1e-2, gtol = 1e-9, max_evals = 2000, history = 8), the evaluations each exit used, the
    statuses and gradient norms;
  * beside it: downloading the features and running scipy L-BFGS-B (gtol 1e-9 on the projected gradient, which is a max norm: the host
    stops earlier than the device's 2-norm test, so the comparison flatters the host) on the same objective in float64 numpy with the
    BLAS threads of the environment (16 on the GPU box), per exit, and max |dlogit| between the two solutions on the fit rows.

    python tools/head_fit_ab.py [--out FILE] [--N 40000] [--no-host]
"""
import argparse
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, K, E = 768, 16, 6
L2 = 1e-2


def loss_grad(theta, X, y, l2):
    """The objective of include/mmee.h at this tool's K and H; the same expression as tests/headfit_ref.py loss_grad (keep the two in step)."""
    import numpy as np
    N = X.shape[0]
    W, b = theta[:K * H].reshape(K, H), theta[K * H:]
    z = X @ W.T + b
    m = z.max(axis=1, keepdims=True)
    ez = np.exp(z - m)
    s = ez.sum(axis=1, keepdims=True)
    loss = float(np.mean((m + np.log(s))[:, 0] - z[np.arange(N), y]) + 0.5 * l2 * np.dot(theta, theta))
    D = ez / s
    D[np.arange(N), y] -= 1.0
    return loss, np.concatenate([(D.T @ X).reshape(-1), D.sum(axis=0)]) / N + l2 * theta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "head_fit.txt"))
    ap.add_argument("--N", type=int, default=40000)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    pkg = importlib.import_module("multi-modal-early-exit_amd")
    N = a.N
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device="cuda").manual_seed(5)
    X = torch.randn((E, N, H), generator=g, device="cuda", dtype=torch.float32)
    teacher = torch.randn((K, H), generator=g, device="cuda", dtype=torch.float32) * (2.0 / H ** 0.5)
    u = torch.rand((N, K), generator=g, device="cuda", dtype=torch.float32).clamp_(1e-7, 1 - 1e-7)
    y = (X[-1] @ teacher.T - torch.log(-torch.log(u))).argmax(-1)
    # earlier exits see the last exit's rows through more noise, as earlier layers see less of the document
    for e in range(E - 1):
        mix = (e + 1) / E
        X[e] = mix * X[-1] + (1.0 - mix * mix) ** 0.5 * X[e]
    feat_bytes = E * N * H * 4
    say(f"head fit: N = {N}, H = {H}, K = {K}, E = {E}, l2 = {L2}; features {feat_bytes / 1e6:.1f} MB resident on {torch.cuda.get_device_name(0)}")

    def timed(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = pkg.fit_exit_heads(X, y, l2=L2, num_labels=K, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, fit

    timed(gtol=0.0, max_evals=3)                                        # code objects, allocator
    per = []
    for _ in range(5):
        t10, _ = timed(gtol=0.0, max_evals=10)
        t40, _ = timed(gtol=0.0, max_evals=40)
        per.append((t40 - t10) / 30.0)
    per.sort()
    ms = per[len(per) // 2]
    say(f"per tick (loss / gradient + reduce + controller, all {E} exits): {ms:.3f} ms (median of 5; min {per[0]:.3f}, max {per[-1]:.3f}) "
        f"= {feat_bytes / ms / 1e6:.1f} GB/s on the feature bytes   [LayerNorm row kernel, README: 5.4 TB/s]")
    fits = sorted((timed() for _ in range(5)), key=lambda r: r[0])
    t_fit, fit = fits[len(fits) // 2]
    say(f"per fit at the defaults (gtol 1e-9, max_evals 2000, history 8): {t_fit:.1f} ms (median of 5; min {fits[0][0]:.1f}, max {fits[-1][0]:.1f}); "
        f"evaluations {fit.evals.cpu().tolist()}, status {fit.status.cpu().tolist()}, "
        f"grad norms {['%.2e' % v for v in fit.grad_norm.cpu().tolist()]}, losses {['%.4f' % v for v in fit.loss.cpu().tolist()]}")
    if a.no_host:
        return finish(a, lines)

    from scipy.optimize import minimize
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    Xh, yh = X.cpu().numpy(), y.cpu().numpy()
    t_down = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    sols, nfev = [], []
    for e in range(E):
        X64 = Xh[e].astype(np.float64)
        r = minimize(loss_grad, np.zeros(K * H + K), args=(X64, yh, L2), jac=True, method="L-BFGS-B",
                     options=dict(gtol=1e-9, ftol=1e-15, maxiter=5000, maxcor=8))
        sols.append(r.x)
        nfev.append(int(r.nfev))
    t_host = (time.perf_counter() - t0) * 1e3
    say(f"host: download {t_down:.1f} ms + scipy L-BFGS-B float64, {os.environ.get('OMP_NUM_THREADS', '?')} threads: {t_host:.1f} ms "
        f"(evaluations {nfev}) = {t_down + t_host:.1f} ms against {t_fit:.1f} ms on the device ({(t_down + t_host) / t_fit:.1f} x)")
    w64, b64 = fit.weight64.cpu().numpy(), fit.bias64.cpu().numpy()
    dz = 0.0
    for e in range(E):
        X64 = Xh[e][:4000].astype(np.float64)
        zd = X64 @ w64[e].T + b64[e]
        zh = X64 @ sols[e][:K * H].reshape(K, H).T + sols[e][K * H:]
        dz = max(dz, float(np.abs(zd - zh).max()))
    say(f"max |dlogit| device solution against host solution, first 4000 rows of every exit: {dz:.3e}")
    finish(a, lines)


def finish(a, lines):
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
