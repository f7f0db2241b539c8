"""Measurement of the weighted exit-head fits (``sample_weight=`` of the four fits in heads.py / ee_head_fit_weighted, ee_mlp_head_fit_weighted)
at the shape of tools/head_fit_ab.py and tools/distill_head_fit_ab.py (GPU box): N = 40 000 CLS rows, H = 768, K = 16, E = 6 exits, features,
teacher logits and the (E,N) weight table resident on the device.  No pass bar and no ratio fixed in advance; the output is what README and
DESIGN quote.

Reported:
  * from ONE build, milliseconds per tick inside a fit that cannot stop early (gtol = 0), unweighted against weighted (uniform weights in
    [0.25, 4): every row is live, the full cost of the variant), alternating the two, for the one-layer labelled fit, the one-layer distilled
    fit at (alpha, T) = (1, 1) and the two-layer labelled fit.  One-layer: (t40 - t10) / 30; two-layer (a tick is about 30 ms): (t8 - t3) / 5;
    median of five pairs (min, max).  The weighted call also makes its row scales, once: the difference of two calls does not carry that;
  * the row-scale kernel's own cost, as the difference of a weighted and an unweighted fit of ONE evaluation, median of nine;
  * with --parent-lib: the UNWEIGHTED ticks of this build against the parent build's library, each in a child process of its own (the two
    libraries export the same names), alternating parent / this, --runs runs each.  The parent's own spread is given twice -- the span of
    its run medians and the span of all its samples -- and this build's run medians are placed against both.

    python tools/weighted_head_fit_ab.py [--out FILE] [--N 40000] [--parent-lib PATH] [--runs 3]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, K, E = 768, 16, 6
L2 = 1e-2
KINDS = ("one-layer, labels", "one-layer, distilled (1, 1)", "two-layer, labels")
EVALS = {KINDS[0]: (10, 40), KINDS[1]: (10, 40), KINDS[2]: (3, 8)}


def median(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def setup(N, older_build=False):
    import torch
    pkg = importlib.import_module("multi-modal-early-exit_amd")
    if older_build:                                # a parent-commit library lacks what this commit adds: bind what it exports
        import ctypes
        lib = ctypes.CDLL(pkg.capi.lib_path())
        for name in [n for n in pkg.capi.SYMBOLS if not hasattr(lib, n)]:
            del pkg.capi.SYMBOLS[name]
    # the problem of tools/distill_head_fit_ab.py, plus a weight table
    g = torch.Generator(device="cuda").manual_seed(5)
    X = torch.randn((E, N, H), generator=g, device="cuda", dtype=torch.float32)
    teacher_w = torch.randn((K, H), generator=g, device="cuda", dtype=torch.float32) * (2.0 / H ** 0.5)
    u = torch.rand((N, K), generator=g, device="cuda", dtype=torch.float32).clamp_(1e-7, 1 - 1e-7)
    teacher = (X[-1] @ teacher_w.T).contiguous()
    y = (teacher - torch.log(-torch.log(u))).argmax(-1)
    for e in range(E - 1):
        mix = (e + 1) / E
        X[e] = mix * X[-1] + (1.0 - mix * mix) ** 0.5 * X[e]
    w = 0.25 + 3.75 * torch.rand((E, N), generator=g, device="cuda", dtype=torch.float32)
    return torch, pkg, X, y, teacher, w


def make_timed(torch, pkg, X, y, teacher):
    def timed(kind, w, max_evals):
        kw = dict(l2=L2, gtol=0.0, max_evals=max_evals)
        if w is not None:
            kw["sample_weight"] = w
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == KINDS[0]:
            pkg.fit_exit_heads(X, y, num_labels=K, **kw)
        elif kind == KINDS[1]:
            pkg.fit_distilled_exit_heads(X, teacher, **kw)
        else:
            pkg.fit_mlp_exit_heads(X, y, num_labels=K, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    return timed


def tick_ms(timed, kind, w):
    lo, hi = EVALS[kind]
    a, b = timed(kind, w, lo), timed(kind, w, hi)
    return (b - a) / (hi - lo)


def tick_child(a):
    """The unweighted ticks of whatever library MMEE_LIB names; one JSON line."""
    torch, pkg, X, y, teacher, _ = setup(a.N, older_build=True)
    timed = make_timed(torch, pkg, X, y, teacher)
    out = {}
    for kind in KINDS:
        timed(kind, None, 2)
        out[kind] = [tick_ms(timed, kind, None) for _ in range(5)]
    print("TICK_CHILD " + json.dumps({"lib": pkg.capi.lib_path(), "ticks": out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_head_fit.txt"))
    ap.add_argument("--N", type=int, default=40000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--tick-child", action="store_true")
    a = ap.parse_args()
    if a.tick_child:
        tick_child(a)
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # ---- the parent build against this one, before this process holds any device memory ----
    def child(lib):
        env = dict(os.environ)
        env.pop("MMEE_LIB", None)
        if lib:
            env["MMEE_LIB"] = os.path.abspath(lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--tick-child", "--N", str(a.N)], env=env, capture_output=True, text=True,
                           timeout=600)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("TICK_CHILD ")]
        if r.returncode != 0 or not got:
            raise SystemExit(f"the child for {lib or 'this build'} failed ({r.returncode}): {r.stderr[-800:]}")
        return json.loads(got[-1][len("TICK_CHILD "):])["ticks"]

    runs = {"parent": [], "this": []}
    if a.parent_lib:
        for _ in range(a.runs):
            runs["parent"].append(child(a.parent_lib))
            runs["this"].append(child(None))

    torch, pkg, X, y, teacher, w = setup(a.N)
    N = a.N
    say(f"weighted head fit: N = {N}, H = {H}, K = {K}, E = {E}, l2 = {L2}; features {E * N * H * 4 / 1e6:.1f} MB, weights {E * N * 4 / 1e6:.2f} MB "
        f"(float32) and their row scales {E * N * 8 / 1e6:.2f} MB (float64, in the workspace) resident on {torch.cuda.get_device_name(0)}")
    timed = make_timed(torch, pkg, X, y, teacher)

    # ---- unweighted against weighted inside a fit, one build ----
    say("per tick inside a fit (evaluation + controller, all 6 exits), unweighted | weighted (uniform weights in [0.25, 4)), alternating, "
        "median of 5 (min, max):")
    for kind in KINDS:
        for wt in (None, w):
            timed(kind, wt, 2)                                          # code objects, allocator
        ticks = {False: [], True: []}
        for _ in range(5):
            for wt in (None, w):
                ticks[wt is not None].append(tick_ms(timed, kind, wt))
        (u, ulo, uhi), (v, vlo, vhi) = median(ticks[False]), median(ticks[True])
        lo, hi = EVALS[kind]
        say(f"  {kind:30s} (t{hi} - t{lo}) / {hi - lo}: {u:8.3f} ms ({ulo:.3f}, {uhi:.3f}) | {v:8.3f} ms ({vlo:.3f}, {vhi:.3f})   x {v / u:.4f}")

    # ---- the row-scale kernel ----
    one = {False: [], True: []}
    for _ in range(9):
        for wt in (None, w):
            one[wt is not None].append(timed(KINDS[0], wt, 1))
    (u, ulo, uhi), (v, vlo, vhi) = median(one[False]), median(one[True])
    say(f"a one-layer fit of ONE evaluation, unweighted | weighted (the call that also makes the row scales: one more launch, {E * N * 12 / 1e6:.2f} MB "
        f"of traffic, and the table's conversion to float32 in Python), median of 9: {u:.3f} ms ({ulo:.3f}, {uhi:.3f}) | {v:.3f} ms "
        f"({vlo:.3f}, {vhi:.3f}): + {v - u:.3f} ms per call")

    # ---- parent against this build ----
    if a.parent_lib:
        say(f"the UNWEIGHTED tick, parent build against this build, a child process per run, alternating parent / this, {a.runs} runs each, "
            "median of 5 (min, max) per run:")
        for kind in KINDS:
            meds = {}
            for who in ("parent", "this"):
                meds[who] = []
                for i, r in enumerate(runs[who]):
                    m, lo, hi = median(r[kind])
                    meds[who].append(m)
                    say(f"  {kind:30s} {who:6s} run {i + 1}: {m:8.3f} ms ({lo:.3f}, {hi:.3f})")
            plo, phi = min(meds["parent"]), max(meds["parent"])
            slo, shi = min(min(r[kind]) for r in runs["parent"]), max(max(r[kind]) for r in runs["parent"])
            mine = median(meds["this"])[0]
            say(f"  {kind:30s} the parent's run medians span {plo:.3f} .. {phi:.3f} ms, its samples {slo:.3f} .. {shi:.3f} ms; this build's run "
                f"medians: {', '.join('%.3f' % m for m in meds['this'])} ms, their median {mine:.3f} ms: "
                f"{'inside' if plo <= mine <= phi else 'OUTSIDE'} the span of the parent's run medians; "
                f"{sum(slo <= m <= shi for m in meds['this'])} of {a.runs} run medians inside the span of the parent's samples")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
