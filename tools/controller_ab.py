"""What online exit control (include/mmee.h, behind the audit's) costs (GPU box).  No pass bar; the output is what README, DESIGN and
profiles/controller.txt quote.

  forward   LayoutLMv3-base, the default exit list, synthetic weights, split precision, audit share 0.05: a controlled forward (gamma tiny,
            so the position, and with it the work, stays put) against an audited forward given the same thresholds and, call by call, the
            same audit seed (the same documents run on to the end), alternated in one
            process: ms per forward, the launches of the "controller" role and their event time.
  replay    risk.rolling_control at E1 = 24, N = 40 000, G = 256 on a synthetic table, end to end with the log on the host, against the numpy
            restatement of tests/controller_ref.py on a downloaded table.
  bench     --bench-parent DIR: ``bench.py --gpus 1 --steps 6 --warmup 2`` of this tree and of the built parent checkout in DIR, alternating,
            three runs each, each in a process of its own.
  trace     --trace N: N controlled forwards and nothing else -- the program of
            ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/controller_ab.py --trace N``, a run of its own.
  summarise --summarise DIR: the two added kernels' rows of that run's kernel-stats CSV.

Nothing about risk on real data is measured: the weights are synthetic, no trained checkpoint exists here.

    python tools/controller_ab.py [--out FILE] [--docs 256] [--text-len 512] [--reps 10] [--bench-parent DIR [--bench-only]] [--trace N | --summarise DIR]
"""
import argparse
import csv
import glob
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FRACTION = 0.05


def summarise(directory, say):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        say(f"kernel trace: no *kernel_stats.csv under {directory}")
        return
    say(f"kernel trace (rocprofv3 --kernel-trace --stats, a run of its own; {os.path.basename(files[0])}): the two added kernels")
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            if "audit_tally" in row.get("Name", "") or "controller_step" in row.get("Name", ""):
                name = row["Name"].split("(")[0]
                say(f"  {name:<32s} calls {row.get('Calls'):>5s}  total {float(row.get('TotalDurationNs', 'nan')) / 1e3:10.1f} us  mean "
                    f"{float(row.get('AverageNs', 'nan')) / 1e3:7.2f} us  min {float(row.get('MinNs', 'nan')) / 1e3:7.2f}  max {float(row.get('MaxNs', 'nan')) / 1e3:7.2f}")


def bench_line(directory):
    out = subprocess.run([sys.executable, os.path.join(directory, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2"], cwd=directory,
                         capture_output=True, text=True, timeout=900)
    for line in reversed(out.stdout.strip().splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise RuntimeError(f"bench.py in {directory} printed no result line: {out.stderr[-400:]}")


def run_bench(a, say):
    if a.bench_parent:
        import numpy as np
        parent = os.path.abspath(a.bench_parent)
        runs = {"parent": [], "this": []}
        for _ in range(3):
            for kind, directory in (("parent", parent), ("this", ROOT)):
                runs[kind].append(bench_line(directory))
        key = next(k for k in ("docs_per_s", "docs_per_sec", "throughput", "value") if k in runs["this"][0])
        for kind, rs in runs.items():
            say(f"bench.py --gpus 1 --steps 6 --warmup 2, {kind:<6s}: {key} " + " / ".join(f"{x[key]:.1f}" for x in rs))
        par, this = [x[key] for x in runs["parent"]], [x[key] for x in runs["this"]]
        inside = min(par) <= float(np.mean(this)) <= max(par)
        say(f"  parent's own spread (max - min) {max(par) - min(par):.1f}; mean of this tree {np.mean(this):.1f}, of the parent {np.mean(par):.1f}; the mean of this "
            f"tree lies inside the parent's range: {inside}.  The bench handle sets no controller and runs none of this code.")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--docs", type=int, default=256)
    ap.add_argument("--text-len", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--bench-parent", default=None)
    ap.add_argument("--bench-only", action="store_true", help="only the bench.py alternation")
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--summarise", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")

    if a.summarise:
        summarise(a.summarise, say)
        return flush()
    if a.bench_only:
        run_bench(a, say)
        return flush()
    import numpy as np
    import torch
    pkg = importlib.import_module("multi-modal-early-exit_amd")
    from tools.audit_ab import cascade

    def timed(fn, reps):
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    # ---- forward ----
    cfg = pkg.ModelConfig.base()
    B, T = a.docs, a.text_len
    E = cfg.exit_config.num_exits
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T)
    eng.load_weights(pkg.synth.make_weights(cfg, seed=41, head_gain=4.0))
    d = pkg.synth.make_documents(cfg, B, seed=42, text_len=T, min_words=3)
    t = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}
    table = eng.forward(**t, dump_all=True, want_all=True).all_crit.cpu().numpy().astype(np.float64)
    thr, _ = cascade(np, table, 0.25)
    path = np.stack([thr + 0.05, thr, thr - 0.05])
    path[:, E] = thr[E]
    eng.set_audit(FRACTION, seed=1)

    def controlled():
        return eng.forward(**t)

    calls = [0]                            # calls since arm(): call k of either series audits under seed 1 + k, so both carry the same shadows

    def audited():
        calls[0] += 1
        return eng.forward(**t, thresholds=thr, audit_seed=calls[0])

    def arm(on):
        # position 1.0 is the vector `thr` itself; a step of 1e-9 per call moves no decision
        eng.set_controller(path if on else None, alpha=0.1, gamma=1e-9, start=1.0, seed=1, log_cap=4096)
        calls[0] = 0

    if a.trace:
        arm(True)
        for _ in range(a.trace):
            controlled()
        torch.cuda.synchronize()
        print(f"trace: {a.trace} controlled forwards done", flush=True)
        return
    say(f"online exit control in the forward: LayoutLMv3-base, exits {cfg.exit_config.exits} (E = {E}), {B} documents, T = {T}, precision {eng.precision}, "
        f"{torch.cuda.get_device_name(0)}; audit share {FRACTION}; thresholds release 0.25 of the documents that reach an exit; event-timed forwards, "
        f"{a.reps} per kind and round, 3 rounds alternated in one process")
    res, info = {"audited": [], "controlled": []}, {}
    for rnd in range(3):
        for kind, fn in (("audited", audited), ("controlled", controlled)):
            arm(kind == "controlled")
            for _ in range(2):
                out = fn()
            if rnd == 0:
                eng.profile(True)
                fn()
                prof = eng.profile_read()
                eng.profile(False)
                info[kind] = (prof.get("controller", {"launches": 0, "ms": 0.0}), sum(v["launches"] for v in prof.values()),
                              np.bincount(out.exit_layer.cpu().numpy(), minlength=E + 1).tolist())
            res[kind] += timed(fn, a.reps)
    med = {k: float(np.median(v)) for k, v in res.items()}
    for kind in res:
        ms = np.array(res[kind])
        ctl, launches, hist = info[kind]
        say(f"  {kind:<10s}: {med[kind]:8.3f} ms per forward (median of {ms.size}; min {ms.min():.3f}, max {ms.max():.3f}, std {ms.std():.3f}); profiled launches "
            f"{launches}; controller role (launches, event ms) ({ctl['launches']}, {ctl['ms']:.4f}); exit histogram {hist}")
    say(f"  controlled - audited = {med['controlled'] - med['audited']:+.3f} ms.  The audited series' own spread (max - min) is "
        f"{max(res['audited']) - min(res['audited']):.3f} ms.")
    st = eng.controller_state()
    say(f"  controller state after the run: position {st['position']:.9f}, calls {st['calls']}, sampled {st['sampled']}, disagree {st['disagree']}")
    eng.close()

    # ---- replay ----
    from tests import audit_ref as A
    from tests import controller_ref as CR
    E1, N, G = 24, 40000, 256
    rng = np.random.default_rng(5)
    tab = rng.uniform(0.0, 1.0, (E1, N))
    bad = (rng.random((E1, N)) < 0.2).astype(np.uint8)
    lam = np.linspace(0.99, 0.5, 32)
    rpath = np.repeat(lam[:, None], E1, axis=1)
    tab_dev, bad_dev = torch.from_numpy(tab).cuda(), torch.from_numpy(bad).cuda()
    kw = dict(alpha=0.1, gamma=1.0, group_size=G, fraction=FRACTION, seed=3, start=16.0, bad=bad_dev)
    r = pkg.risk.rolling_control(tab_dev, rpath, **kw)
    dev_ms = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = pkg.risk.rolling_control(tab_dev, rpath, **kw)
        dev_ms.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    ex, log, p = CR.rolling(tab_dev.cpu().numpy(), bad_dev.cpu().numpy(), rpath, sign=1.0, cut=A.cut_of(FRACTION), seed=3, alpha=0.1, gamma=1.0, p0=16.0, G=G)
    np_ms = (time.perf_counter() - t0) * 1e3
    same = np.array_equal(ex, r.exits.cpu().numpy()) and np.array_equal(log["p_after"].view(np.int64), r.log.p_after.view(np.int64))
    say(f"rolling_control: E1 = {E1}, N = {N}, G = {G} ({len(r.log.call)} groups), V = {len(lam)}, share {FRACTION}: {np.median(dev_ms):.3f} ms per call end to end "
        f"with the log on the host (median of 5; min {min(dev_ms):.3f}, max {max(dev_ms):.3f}) against {np_ms:.1f} ms for the numpy restatement on a downloaded "
        f"table (one run); exits and positions bitwise equal: {same}; excess {r.log.excess(0.1).max():.3f} <= bound {r.bound():.3f}")

    run_bench(a, say)
    say("Nothing about risk on real data is measured: synthetic weights, no trained checkpoint exists here.")
    flush()


if __name__ == "__main__":
    main()
