"""Measurement of the distilled exit-head fit (``heads.fit_distilled_exit_heads`` / ee_head_fit_distill) at the shape of tools/head_fit_ab.py
(GPU box): N = 40 000 CLS rows, H = 768, K = 16, E = 6 exits, features and teacher logits resident on the device.  No pass bar and no ratio
fixed in advance; the output is what README and DESIGN quote.

Reported, all from ONE build, the labelled kernel (whose code the distilled fit leaves as it was) serving as the baseline:
  * one evaluation through the debug hooks: ee_debug_head_lossgrad against ee_debug_head_distill_lossgrad at (alpha, T) = (1, 1), (1, 2) and
    (0.5, 2), stream time between two events around the call, median of nine, alternating the four.  The hooks allocate and free their
    scratch inside the call, so this number carries that cost in all four columns alike;
  * milliseconds per tick (loss / gradient kernel + reduce + controller) from two fits that cannot stop early (gtol = 0) with 10 and 40
    evaluations, (t40 - t10) / 30, median of five pairs, for the labelled fit and the three distilled ones: the cost of an evaluation inside
    a fit, without the hooks' allocations;
  * one whole label-free fit at the defaults (alpha = 1, T = 1, l2 = 1e-2, gtol = 1e-9, max_evals = 2000, history = 8): milliseconds, the
    evaluations each exit used, statuses, gradient norms, losses, and each head's mean KL to the teacher on the fit rows.

    python tools/distill_head_fit_ab.py [--out FILE] [--N 40000]
"""
import argparse
import ctypes as C
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, K, E = 768, 16, 6
L2 = 1e-2
PAIRS = [(1.0, 1.0), (1.0, 2.0), (0.5, 2.0)]


def median(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill_head_fit.txt"))
    ap.add_argument("--N", type=int, default=40000)
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("multi-modal-early-exit_amd")
    lib = pkg.capi.load()
    N = a.N
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # the problem of tools/head_fit_ab.py, plus a teacher: the final classifier as a linear map of the last exit's rows
    g = torch.Generator(device="cuda").manual_seed(5)
    X = torch.randn((E, N, H), generator=g, device="cuda", dtype=torch.float32)
    teacher_w = torch.randn((K, H), generator=g, device="cuda", dtype=torch.float32) * (2.0 / H ** 0.5)
    u = torch.rand((N, K), generator=g, device="cuda", dtype=torch.float32).clamp_(1e-7, 1 - 1e-7)
    teacher = (X[-1] @ teacher_w.T).contiguous()
    y = (teacher - torch.log(-torch.log(u))).argmax(-1)
    for e in range(E - 1):
        mix = (e + 1) / E
        X[e] = mix * X[-1] + (1.0 - mix * mix) ** 0.5 * X[e]
    say(f"distilled head fit: N = {N}, H = {H}, K = {K}, E = {E}, l2 = {L2}; features {E * N * H * 4 / 1e6:.1f} MB and teacher logits "
        f"{N * K * 4 / 1e6:.1f} MB resident on {torch.cuda.get_device_name(0)}")

    # ---- one evaluation through the debug hooks ----
    P = K * H + K
    theta = torch.randn((E, P), generator=g, device="cuda", dtype=torch.float64) * (1.0 / H ** 0.5)
    loss = torch.zeros((E,), dtype=torch.float64, device="cuda")
    grad = torch.zeros((E, P), dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def hook(pair):
        if pair is None:
            rc = lib.ee_debug_head_lossgrad(p(X), p(y), p(theta), E, N, H, K, L2, p(loss), p(grad), stream)
        else:
            rc = lib.ee_debug_head_distill_lossgrad(p(X), p(teacher), p(y), p(theta), E, N, H, K, pair[0], pair[1], L2, p(loss), p(grad), stream)
        pkg.capi.check(rc, None, "debug hook")

    def hook_ms(pair):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        hook(pair)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    kinds = [None] + PAIRS
    for k in kinds:
        hook(k)                                                         # code objects, allocator
    samples = {k: [] for k in kinds}
    for _ in range(9):
        for k in kinds:
            samples[k].append(hook_ms(k))
    base = median(samples[None])[0]
    say("one evaluation through the debug hooks (scratch allocated and freed inside the call), median of 9 (min, max):")
    for k in kinds:
        med, lo, hi = median(samples[k])
        what = "ee_debug_head_lossgrad (labels)" if k is None else f"ee_debug_head_distill_lossgrad alpha = {k[0]}, T = {k[1]}"
        say(f"  {what:58s} {med:8.3f} ms ({lo:.3f}, {hi:.3f})   x {med / base:.3f}")

    # ---- milliseconds per tick inside a fit ----
    def timed(pair, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if pair is None:
            fit = pkg.fit_exit_heads(X, y, l2=L2, num_labels=K, **kw)
        else:
            fit = pkg.fit_distilled_exit_heads(X, teacher, None if pair[0] == 1.0 else y, alpha=pair[0], temperature=pair[1], l2=L2, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, fit

    ticks = {k: [] for k in kinds}
    for k in kinds:
        timed(k, gtol=0.0, max_evals=3)
    for _ in range(5):
        for k in kinds:
            t10, _ = timed(k, gtol=0.0, max_evals=10)
            t40, _ = timed(k, gtol=0.0, max_evals=40)
            ticks[k].append((t40 - t10) / 30.0)
    base = median(ticks[None])[0]
    say(f"per tick inside a fit (loss / gradient + reduce + controller, all {E} exits), (t40 - t10) / 30, median of 5 (min, max):")
    for k in kinds:
        med, lo, hi = median(ticks[k])
        what = "ee_head_fit (labels)" if k is None else f"ee_head_fit_distill alpha = {k[0]}, T = {k[1]}"
        say(f"  {what:58s} {med:8.3f} ms ({lo:.3f}, {hi:.3f})   x {med / base:.3f}")

    # ---- one whole label-free fit at the defaults ----
    fits = sorted((timed((1.0, 1.0)) for _ in range(5)), key=lambda r: r[0])
    t_fit, fit = fits[len(fits) // 2]
    say(f"one label-free fit at the defaults (alpha 1, T 1, gtol 1e-9, max_evals 2000, history 8): {t_fit:.1f} ms (median of 5; min "
        f"{fits[0][0]:.1f}, max {fits[-1][0]:.1f}); evaluations {fit.evals.cpu().tolist()}, status {fit.status.cpu().tolist()}, "
        f"grad norms {['%.2e' % v for v in fit.grad_norm.cpu().tolist()]}, losses {['%.4f' % v for v in fit.loss.cpu().tolist()]}")
    lq = torch.log_softmax(teacher.to(torch.float64), -1)
    lp = torch.log_softmax(fit.logits(X), -1)
    kl = (lq.exp() * (lq - lp)).sum(-1).mean(-1)
    zero = (lq.exp() * (lq + torch.log(torch.tensor(float(K), dtype=torch.float64, device="cuda")))).sum(-1).mean()
    say(f"mean KL(teacher || head) on the fit rows per exit: {['%.4f' % v for v in kl.cpu().tolist()]}; the zero head's: {float(zero):.4f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
