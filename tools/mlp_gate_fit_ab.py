"""Measurement of the two-layer gate-head fit (``heads.fit_mlp_gate_heads`` / ee_mlp_head_fit_gate, ee_mlp_head_fit_gate_weighted) at the shape of
BASELINE's large gate configuration (GPU box): N = 40 000 CLS rows, H = 1024, E = 23 exits, features resident on the device.  No pass bar; the
output is what README and DESIGN quote.

Reported:
  * milliseconds per evaluation (the seven launches + controller: one tick, all E exits) of the gate objective inside a fit, unweighted and
    weighted (uniform weights in [0.25, 4)), and of ``fit_mlp_exit_heads`` (ee_mlp_head_fit) at K = 2 in the same build -- the comparison
    point: one small launch of the seven differs.  Each from two fits that cannot stop early (gtol = 0) with 4 and 16 evaluations,
    (t16 - t4) / 12; the three alternate inside every round, median over the rounds, and float64 TFLOP/s on the 4 E N H^2 of the two large GEMMs;
  * one whole fit from the identity start (l2 = 1e-2, gtol = 1e-6, history 8, ``--max-evals`` ticks), evaluations and status per exit.
``--parent-ab`` measures only what the parent build has too -- the unweighted evaluations of ee_mlp_head_fit at K = 2 and of ee_head_fit_gate --
for a job that alternates processes between two builds, each running this file from a tools/ directory next to its own package and library.

``--trace ROUTE`` runs one 16-evaluation fit of one route and nothing else, for
``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/mlp_gate_fit_ab.py --trace ROUTE``: where a difference
between the routes lies, kernel by kernel.

    python tools/mlp_gate_fit_ab.py [--out FILE] [--N 40000] [--E 23] [--rounds 5] [--max-evals 400] [--parent-ab LABEL | --trace ROUTE]
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
    ap.add_argument("--out", default=None, help="also append the lines to this file (profiles/mlp_gate_fit.txt holds one run)")
    ap.add_argument("--N", type=int, default=40000)
    ap.add_argument("--E", type=int, default=23)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-evals", type=int, default=400, help="budget of the whole fit: a tick costs the same whether or not an exit still runs")
    ap.add_argument("--parent-ab", default=None, metavar="LABEL", help="only the evaluations the parent build has too; LABEL names the build")
    ap.add_argument("--trace", default=None, choices=["gate", "weighted", "ramp"],
                    help="only one 16-evaluation fit (gtol = 0) of this route: the program of a rocprofv3 --kernel-trace --stats run")
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
    y = T[-1].to(torch.int64).contiguous()                              # the ramp fit's labels (N,), K = 2
    w = (0.25 + 3.75 * torch.rand((E, N), generator=g, device="cuda", dtype=torch.float32)).contiguous()
    flop = 4.0 * E * N * H * H
    tag = f"[{a.parent_ab}] " if a.parent_ab else ""

    def timed(fn, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = fn(**kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, fit

    ramp = lambda **kw: pkg.fit_mlp_exit_heads(X, y, l2=L2, num_labels=2, **kw)
    one_layer_gate = lambda **kw: pkg.fit_gate_heads(X, T, l2=L2, **kw)
    routes = [("ee_mlp_head_fit at K = 2", ramp)]
    if a.parent_ab:
        routes.append(("ee_head_fit_gate (one layer)", one_layer_gate))
    else:
        routes = [("ee_mlp_head_fit_gate", lambda **kw: pkg.fit_mlp_gate_heads(X, T, l2=L2, **kw)),
                  ("ee_mlp_head_fit_gate_weighted", lambda **kw: pkg.fit_mlp_gate_heads(X, T, l2=L2, sample_weight=w, **kw))] + routes
    if a.trace:
        fn = dict(gate=routes[0][1], weighted=routes[1][1], ramp=routes[2][1])[a.trace]
        ms, _ = timed(fn, gtol=0.0, max_evals=16)
        print(f"{a.trace}: one fit of 16 evaluations under the profiler: {ms:.1f} ms")
        return
    say(f"{tag}two-layer gate fit: N = {N}, H = {H}, E = {E}, P = {H * H + 3 * H + 2}, l2 = {L2}; features {E * N * H * 4 / 1e6:.1f} MB resident on "
        f"{torch.cuda.get_device_name(0)}; share of right exits, first / last exit {float(T[0].mean()):.2f} / {float(T[-1].mean()):.2f}")
    for _, fn in routes:
        timed(fn, gtol=0.0, max_evals=3)                                # code objects, allocator
    per = {name: [] for name, _ in routes}
    for _ in range(a.rounds):
        for name, fn in routes:                                         # alternating inside every round
            t4, _ = timed(fn, gtol=0.0, max_evals=4)
            t16, _ = timed(fn, gtol=0.0, max_evals=16)
            per[name].append((t16 - t4) / 12.0)
    for name, _ in routes:
        p = sorted(per[name])
        ms = p[len(p) // 2]
        rate = f" = {flop / ms / 1e9:.2f} float64 TFLOP/s on the {flop / 1e9:.0f} GFLOP of the two large GEMMs" if "mlp" in name else ""
        say(f"{tag}per evaluation inside a fit, all {E} exits, {name}: {ms:.3f} ms (median of {len(p)}; min {p[0]:.3f}, max {p[-1]:.3f}){rate}")
    if not a.parent_ab:
        for name, fn in routes[:2]:
            t_fit, fit = timed(fn, gtol=1e-6, max_evals=a.max_evals)
            say(f"per fit from the identity start, {name} (gtol 1e-6, max_evals {a.max_evals}, history 8): {t_fit:.1f} ms (one run); evaluations "
                f"{fit.evals.cpu().tolist()}, status {fit.status.cpu().tolist()}, largest grad norm {float(fit.grad_norm.max()):.2e}, "
                f"losses {min(fit.loss.cpu().tolist()):.4f} - {max(fit.loss.cpu().tolist()):.4f} (start log 2 + l2 H / 2 = {0.6931 + 0.5 * L2 * H:.4f})")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
