"""Measurement of the two-layer exit-head fit (``heads.fit_mlp_exit_heads`` / ee_mlp_head_fit) at the shape it was built for (GPU box):
N = 40 000 CLS rows, H = 768, K = 16, E = 6 exits, features resident on the device.  No pass bar; the output is what README and DESIGN quote.
The protocol is that of tools/head_fit_ab.py.

Reported:
  * milliseconds per tick (the seven launches of an evaluation + controller) from two fits that cannot stop early (gtol = 0) with 10 and 40
    evaluations: (t40 - t10) / 30, median of five pairs -- and float64 TFLOP/s on the 4 N H^2 E FLOP of the two large GEMMs
    (A = tanh(X W1^T + b1) and dW1 = dA^T X), which are all of the cost;
  * milliseconds per fit from the identity start at l2 = 1e-2, gtol = 1e-6, history = 8 and a budget of --fit-evals evaluations (one run:
    it is thousands of ticks long), the evaluations each exit used, the statuses, gradient norms and losses;
  * the route that exists without the feature: downloading the features and evaluating the same loss and gradient in float64 with torch on
    the CPU (the threads of the environment, 16 on the GPU box), median of three evaluations of all exits -- per evaluation, since a host
    L-BFGS needs about as many of them as the device's.

    python tools/mlp_head_fit_ab.py [--out FILE] [--N 40000] [--fit-evals 4000] [--no-host]
"""
import argparse
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, K, E = 768, 16, 6
L2 = 1e-2


def host_loss_grad(torch, theta, X, y, l2):
    """The objective of include/mmee.h in float64 torch on the CPU; the same expression as tests/mlp_headfit_ref.py loss_grad."""
    N = X.shape[0]
    o1, o2, o3 = H * H, H * H + H, H * H + H + K * H
    W1, b1, W2, b2 = theta[:o1].view(H, H), theta[o1:o2], theta[o2:o3].view(K, H), theta[o3:]
    A = torch.tanh(torch.addmm(b1, X, W1.t()))
    z = torch.addmm(b2, A, W2.t())
    lse = torch.logsumexp(z, dim=1)
    rows = torch.arange(N)
    loss = float((lse - z[rows, y]).mean() + 0.5 * l2 * torch.dot(theta, theta))
    D = torch.softmax(z, dim=1)
    D[rows, y] -= 1.0
    dA = (D @ W2) * (1.0 - A * A)
    g = torch.cat([(dA.t() @ X).reshape(-1), dA.sum(0), (D.t() @ A).reshape(-1), D.sum(0)]) / N + l2 * theta
    return loss, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mlp_head_fit.txt"))
    ap.add_argument("--N", type=int, default=40000)
    ap.add_argument("--fit-evals", type=int, default=4000)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("multi-modal-early-exit_amd")
    N = a.N
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device="cuda").manual_seed(5)
    X = torch.randn((E, N, H), generator=g, device="cuda", dtype=torch.float32)
    T1 = torch.randn((H, H), generator=g, device="cuda", dtype=torch.float32) * (1.5 / H ** 0.5)
    T2 = torch.randn((K, H), generator=g, device="cuda", dtype=torch.float32) * (4.0 / H ** 0.5)
    u = torch.rand((N, K), generator=g, device="cuda", dtype=torch.float32).clamp_(1e-7, 1 - 1e-7)
    y = (torch.tanh(X[-1] @ T1.T) @ T2.T - 0.5 * torch.log(-torch.log(u))).argmax(-1)
    # earlier exits see the last exit's rows through more noise, as earlier layers see less of the document
    for e in range(E - 1):
        mix = (e + 1) / E
        X[e] = mix * X[-1] + (1.0 - mix * mix) ** 0.5 * X[e]
    P = H * H + H + K * H + K
    need = pkg.capi.load().ee_mlp_head_fit_workspace_bytes(E, N, H, K, 8)
    say(f"two-layer head fit: N = {N}, H = {H}, K = {K}, E = {E}, P = {P}, l2 = {L2}; features {E * N * H * 4 / 1e6:.1f} MB resident on "
        f"{torch.cuda.get_device_name(0)}; workspace {need / 1e6:.1f} MB")

    def timed(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = pkg.fit_mlp_exit_heads(X, y, l2=L2, num_labels=K, **kw)
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
    flop = 4.0 * N * H * H * E
    say(f"per tick (seven launches of an evaluation + controller, all {E} exits): {ms:.3f} ms (median of 5; min {per[0]:.3f}, max {per[-1]:.3f}) "
        f"= {flop / ms / 1e9:.2f} float64 TFLOP/s on the {flop / 1e9:.0f} GFLOP of the two large GEMMs")
    t_fit, fit = timed(gtol=1e-6, max_evals=a.fit_evals)
    say(f"per fit from the identity start (gtol 1e-6, max_evals {a.fit_evals}, history 8): {t_fit:.1f} ms (one run); "
        f"evaluations {fit.evals.cpu().tolist()}, status {fit.status.cpu().tolist()}, "
        f"grad norms {['%.2e' % v for v in fit.grad_norm.cpu().tolist()]}, losses {['%.4f' % v for v in fit.loss.cpu().tolist()]}")
    if a.no_host:
        return finish(a, lines)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    Xh, yh = X.cpu(), y.cpu()
    t_down = (time.perf_counter() - t0) * 1e3
    theta = fit.theta64.cpu()
    host, worst = [], 0.0
    for _ in range(3):
        t0 = time.perf_counter()
        for e in range(E):
            loss, _ = host_loss_grad(torch, theta[e], Xh[e].to(torch.float64), yh, L2)
            worst = max(worst, abs(loss - float(fit.loss[e])))
        host.append((time.perf_counter() - t0) * 1e3)
    host.sort()
    say(f"host: download {t_down:.1f} ms, then float64 torch on the CPU, {torch.get_num_threads()} threads: {host[1]:.1f} ms per evaluation of all "
        f"{E} exits (median of 3) against {ms:.3f} ms per tick on the device ({host[1] / ms:.1f} x); "
        f"max |loss(host) - loss(device)| at the returned points {worst:.3e}")
    finish(a, lines)


def finish(a, lines):
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
