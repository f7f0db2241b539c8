"""Measurement of the gate-head fit (``heads.fit_gate_heads`` / ee_head_fit_gate) at the shape of BASELINE's large gate configuration (GPU box):
N = 40 000 CLS rows, H = 1024, E = 23 exits, features resident on the device.  No pass bar; the output is what README and DESIGN quote.

Reported:
  * milliseconds per evaluation (loss / gradient kernel + reduce + controller: one tick, all E exits) from two fits that cannot stop early
    (gtol = 0) with 4 and 16 evaluations: (t16 - t4) / 12, median of seven pairs, and GB/s on the feature bytes E N H 4 an evaluation reads;
  * milliseconds per fit at the defaults (l2 = 1e-2, gtol = 1e-9, max_evals = 2000, history = 8), evaluations, status, gradient norms;
  * beside it, the route that exists without it: 2 E calls of ``fit_lte_classifier(features[e:e+1], t_j, loss="bce", l2 = 2 l2)`` (column j
    of exit e is that problem), their summed time, and the largest logit difference between the two routes.

    python tools/gate_fit_ab.py [--out FILE] [--N 40000] [--E 23] [--no-lte]
"""
import argparse
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H = 1024
L2 = 1e-2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file (profiles/gate_decision.txt (b) holds one run)")
    ap.add_argument("--N", type=int, default=40000)
    ap.add_argument("--E", type=int, default=23)
    ap.add_argument("--no-lte", action="store_true")
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("multi-modal-early-exit_amd")
    pkg.capi.load()
    N, E = a.N, a.E
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # unit-variance rows; "the classifier is right here" more often at deeper exits
    g = torch.Generator(device="cuda").manual_seed(7)
    X = torch.randn((E, N, H), generator=g, device="cuda", dtype=torch.float32)
    v = torch.randn((E, H), generator=g, device="cuda", dtype=torch.float32) * (2.0 / H ** 0.5)
    u = torch.rand((E, N), generator=g, device="cuda", dtype=torch.float32).clamp_(1e-7, 1 - 1e-7)
    off = torch.linspace(-0.5, 1.5, E, device="cuda").unsqueeze(1)
    T = ((torch.einsum("enh,eh->en", X, v) + off + torch.log(u) - torch.log1p(-u)) > 0).to(torch.float64)
    feat_bytes = E * N * H * 4
    say(f"gate fit: N = {N}, H = {H}, E = {E}, l2 = {L2}; features {feat_bytes / 1e6:.1f} MB resident on {torch.cuda.get_device_name(0)}; "
        f"share of right exits, first / last exit {float(T[0].mean()):.2f} / {float(T[-1].mean()):.2f}")

    def timed(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = pkg.fit_gate_heads(X, T, l2=L2, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, fit

    timed(gtol=0.0, max_evals=3)                                        # code objects, allocator
    per = []
    for _ in range(7):
        t4, _ = timed(gtol=0.0, max_evals=4)
        t16, _ = timed(gtol=0.0, max_evals=16)
        per.append((t16 - t4) / 12.0)
    per.sort()
    ms = per[len(per) // 2]
    say(f"per evaluation (loss / gradient + reduce + controller, all {E} exits): {ms:.4f} ms (median of 7; min {per[0]:.4f}, max {per[-1]:.4f}) "
        f"= {feat_bytes / ms / 1e6:.1f} GB/s on the feature bytes")
    runs = sorted((timed() for _ in range(5)), key=lambda r: r[0])
    t_fit, fit = runs[len(runs) // 2]
    ev = fit.evals.cpu().tolist()
    say(f"per fit at the defaults (gtol 1e-9, max_evals 2000, history 8): {t_fit:.1f} ms (median of 5; min {runs[0][0]:.1f}, max {runs[-1][0]:.1f}); "
        f"evaluations {min(ev)} - {max(ev)} per exit, status {sorted(set(fit.status.cpu().tolist()))}, largest grad norm "
        f"{float(fit.grad_norm.max()):.2e}")
    if not a.no_lte:
        def lte_route():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = [[pkg.fit_lte_classifier(X[e:e + 1], t, loss="bce", l2=2.0 * L2) for t in ((1.0 - T[e:e + 1]).contiguous(), T[e:e + 1])]
                   for e in range(E)]
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out
        lte_route()
        lr = sorted((lte_route() for _ in range(3)), key=lambda r: r[0])
        t_lte, cols = lr[1]
        worst = 0.0
        z = fit.logits(X)
        for e in range(E):
            for j in (0, 1):
                th = cols[e][j].theta64
                zj = X[e].to(torch.float64) @ th[:H] + th[H]
                worst = max(worst, float((z[e, :, j] - zj).abs().max()))
        say(f"the route without it, {2 * E} calls of fit_lte_classifier(loss='bce', l2 = 2 l2) on one exit and one column each: {t_lte:.1f} ms "
            f"(median of 3; min {lr[0][0]:.1f}, max {lr[-1][0]:.1f}) against {t_fit:.1f} ms = {t_lte / t_fit:.1f} x; largest logit difference "
            f"between the routes {worst:.3e}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
