"""Measurement of the LTE classifier fit (``heads.fit_lte_classifier`` / ee_lte_fit) at the shape it was built for (GPU box): N = 40 000 CLS
rows, H = 768, E = 6 exits, features resident on the device.  No pass bar; the output is what README and DESIGN quote.

Reported:
  * milliseconds per evaluation (loss / gradient kernel + reduce + controller: one tick) from two fits that cannot stop early (gtol = 0) with
    4 and 16 evaluations -- both well before the iteration converges: (t16 - t4) / 12, median of seven pairs, per loss -- and GB/s on the
    feature bytes E N H 4 an evaluation reads;
  * beside it, on the same box and in the same process: ``ln_rows_kernel`` through ee_debug_ln_rows over the same E N rows of H floats (it
    reads and writes a row: 2 E N H 4 bytes), host clock around calls that each end in a stream synchronise, median of seven; the hook's
    launch + synchronise is inside that time, so the kernel's own rate is a little higher than the figure;
  * milliseconds per fit at the defaults (l2 = 1e-2, gtol = 1e-9, history = 8), evaluations, status, gradient norm, per loss;
  * beside it: downloading the features and running scipy L-BFGS-B (gtol 1e-9 on the projected gradient, a max norm: the host stops earlier
    than the device's 2-norm test, so the comparison flatters the host) on the same objective in float64 numpy with the BLAS threads of the
    environment (16 on the GPU box), and the distance between the two solutions.

    python tools/lte_fit_ab.py [--out FILE] [--N 40000] [--no-host]
"""
import argparse
import ctypes as C
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, E = 768, 6
L2 = 1e-2


def loss_grad(theta, X, T, loss, l2):
    """The objective of include/mmee.h; the same expression as tests/lte_fit_ref.py loss_grad (keep the two in step).  X (E,N,H) float64."""
    import numpy as np
    En, N, Hn = X.shape
    Xf = X.reshape(En * N, Hn)                                          # matrix-vector products: the BLAS threads do the work
    T = T.reshape(-1)
    a = Xf @ theta[:-1] + theta[-1]
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-a))
    if loss == "mse":
        l, d = (s - T) ** 2, 2.0 * (s - T) * s * (1.0 - s)
    else:
        l, d = np.maximum(a, 0.0) + np.log1p(np.exp(-np.abs(a))) - T * a, s - T
    g = np.concatenate([d @ Xf, [d.sum()]]) / N + l2 * theta
    return float(l.sum() / N + 0.5 * l2 * np.dot(theta, theta)), g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lte_fit.txt"))
    ap.add_argument("--N", type=int, default=40000)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    pkg = importlib.import_module("multi-modal-early-exit_amd")
    lib = pkg.capi.load()
    N = a.N
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # the generator of tests/lte_fit_ref.problem at this shape: deeper exits are wrong less often
    g = torch.Generator(device="cuda").manual_seed(5)
    X = torch.randn((E, N, H), generator=g, device="cuda", dtype=torch.float32)
    v = torch.randn((H,), generator=g, device="cuda", dtype=torch.float32) * (2.0 / H ** 0.5)
    u = torch.rand((E, N), generator=g, device="cuda", dtype=torch.float32).clamp_(1e-7, 1 - 1e-7)
    off = torch.linspace(-0.5, 1.0, E, device="cuda").unsqueeze(1)
    T = ((X @ v + off + torch.log(u) - torch.log1p(-u)) < 0).to(torch.float64)
    feat_bytes = E * N * H * 4
    say(f"LTE fit: N = {N}, H = {H}, E = {E}, l2 = {L2}; features {feat_bytes / 1e6:.1f} MB resident on {torch.cuda.get_device_name(0)}; "
        f"share of wrong exits per exit {['%.2f' % x for x in T.mean(1).cpu().tolist()]}")

    def timed(loss, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = pkg.fit_lte_classifier(X, T, loss=loss, l2=L2, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, fit

    per_eval = {}
    for loss in ("mse", "bce"):
        timed(loss, gtol=0.0, max_evals=3)                              # code objects, allocator
        per = []
        for _ in range(7):
            t4, _ = timed(loss, gtol=0.0, max_evals=4)
            t16, _ = timed(loss, gtol=0.0, max_evals=16)
            per.append((t16 - t4) / 12.0)
        per.sort()
        ms = per_eval[loss] = per[len(per) // 2]
        say(f"{loss}: per evaluation (loss / gradient + reduce + controller, all {E} exits): {ms:.4f} ms (median of 7; min {per[0]:.4f}, "
            f"max {per[-1]:.4f}) = {feat_bytes / ms / 1e6:.1f} GB/s on the feature bytes")

    # ln_rows_kernel over the same rows, same box, same process
    rows = E * N
    src = X.view(rows, H)
    dst = torch.empty_like(src)
    n_dev = torch.tensor([rows], dtype=torch.int32, device="cuda")
    gam, bet = torch.ones(H, device="cuda"), torch.zeros(H, device="cuda")
    err = C.c_int32(-1)
    p = lambda t: C.c_void_p(t.data_ptr())

    def ln():
        pkg.capi.check(lib.ee_debug_ln_rows(p(src), p(dst), None, p(n_dev), rows, H, p(gam), p(bet), 1e-5, None, 0.0, 0, 0, None, None, None, 0.0,
                                            C.byref(err), None), None, "ee_debug_ln_rows")
    for _ in range(3):
        ln()
    t_ln = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            ln()
        t_ln.append((time.perf_counter() - t0) * 1e2)                  # ms per call
    t_ln.sort()
    ln_ms = t_ln[len(t_ln) // 2]
    ln_rate = 2 * feat_bytes / ln_ms / 1e6
    say(f"ln_rows_kernel over the same {rows} rows of {H} floats (reads and writes a row; ee_debug_ln_rows, launch + synchronise included): "
        f"{ln_ms:.4f} ms (median of 7 x 10 calls; min {t_ln[0]:.4f}, max {t_ln[-1]:.4f}) = {ln_rate:.1f} GB/s on 2 E N H 4 bytes")
    for loss, ms in per_eval.items():
        say(f"{loss}: the evaluation's rate is {feat_bytes / ms / 1e6 / ln_rate:.2f} of ln_rows_kernel's on this box")

    fits = {}
    for loss in ("mse", "bce"):
        runs = sorted((timed(loss) for _ in range(5)), key=lambda r: r[0])
        t_fit, fit = fits[loss] = runs[len(runs) // 2]
        say(f"{loss}: per fit at the defaults (gtol 1e-9, max_evals {pkg.heads.LTE_MAX_EVALS}, history 8): {t_fit:.1f} ms (median of 5; min "
            f"{runs[0][0]:.1f}, max {runs[-1][0]:.1f}); evaluations {int(fit.evals.cpu()[0])}, status {int(fit.status.cpu()[0])}, grad norm "
            f"{float(fit.grad_norm.cpu()[0]):.2e}, loss {float(fit.loss.cpu()[0]):.6f}")
    if a.no_host:
        return finish(a, lines)

    from scipy.optimize import minimize
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    Xh, Th = X.cpu().numpy(), T.cpu().numpy()
    t_down = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    X64 = Xh.astype(np.float64)
    t_widen = (time.perf_counter() - t0) * 1e3
    for loss in ("mse", "bce"):
        t0 = time.perf_counter()
        r = minimize(loss_grad, np.zeros(H + 1), args=(X64, Th, loss, L2), jac=True, method="L-BFGS-B",
                     options=dict(gtol=1e-9, ftol=1e-15, maxiter=5000, maxcor=8))
        t_host = (time.perf_counter() - t0) * 1e3
        t_fit, fit = fits[loss]
        dist = float(np.linalg.norm(fit.theta64.cpu().numpy() - r.x))
        say(f"{loss}: host: download {t_down:.1f} ms + widening {t_widen:.1f} ms + scipy L-BFGS-B float64, {os.environ.get('OMP_NUM_THREADS', '?')} "
            f"threads: {t_host:.1f} ms ({int(r.nfev)} evaluations) = {t_down + t_widen + t_host:.1f} ms against {t_fit:.1f} ms on the device "
            f"({(t_down + t_widen + t_host) / t_fit:.1f} x); ||theta_device - theta_host|| = {dist:.3e}")
    finish(a, lines)


def finish(a, lines):
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
