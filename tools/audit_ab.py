"""What audited exits (include/mmee.h, behind the cascades) cost (GPU box).  No pass bar; the output is what README, DESIGN and
profiles/audit.txt quote.

  forward   LayoutLMv3-base, the default exit list, synthetic weights, split precision: a thresholded forward that releases a quarter of the
            arriving documents at every exit, without an audit and with audited shares 0.01, 0.05, 0.25 and 1, beside the dump-all call, all
            alternated in one process: ms per forward, the documents that reached each exit, and the extra time against p x (dump-all - off)
            with p the share the hash actually selected.  The exit_decide role's launches and event time per kind (events include launch gaps).
  trace     --trace N: N audited forwards (share 0.25) and N unaudited ones and nothing else -- the program of
            ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/audit_ab.py --trace N``, a run of its own.
  summarise --summarise DIR: the decide kernels' rows of that run's kernel-stats CSV.

The agreement rates themselves are not measured: the weights are synthetic, no trained checkpoint exists here.

    python tools/audit_ab.py [--out FILE] [--docs 256] [--text-len 512] [--release 0.25] [--reps 10] [--trace N | --summarise DIR]
"""
import argparse
import csv
import glob
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHARES = (0.01, 0.05, 0.25, 1.0)


def cascade(np, table, release):
    """Per-exit thresholds on a criterion table (E+1,B) that release `release` of the documents still there, and the exits they give."""
    E1, B = table.shape
    thr, ex, here = np.full(E1, 0.5), np.full(B, E1 - 1), np.ones(B, bool)
    for e in range(E1 - 1):
        s = np.sort(table[e, here])
        k = max(1, int(round(release * s.size)))
        if s.size < 2 or k >= s.size:
            thr[e] = 2.0
            continue
        thr[e] = 0.5 * (s[-k - 1] + s[-k])
        leave = here & (table[e] > thr[e])
        ex[leave], here = e, here & ~leave
    return thr, ex


def summarise(directory, say):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        say(f"kernel trace: no *kernel_stats.csv under {directory}")
        return
    say(f"kernel trace (rocprofv3 --kernel-trace --stats, a run of its own; {os.path.basename(files[0])}): the decide kernels")
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            if "exit_decide" in row.get("Name", ""):
                name = row["Name"].split("(")[0]
                say(f"  {name:<48s} calls {row.get('Calls'):>5s}  total {float(row.get('TotalDurationNs', 'nan')) / 1e3:10.1f} us  mean "
                    f"{float(row.get('AverageNs', 'nan')) / 1e3:7.2f} us  min {float(row.get('MinNs', 'nan')) / 1e3:7.2f}  max {float(row.get('MaxNs', 'nan')) / 1e3:7.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--docs", type=int, default=256)
    ap.add_argument("--text-len", type=int, default=512)
    ap.add_argument("--release", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
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
    import numpy as np
    import torch
    pkg = importlib.import_module("multi-modal-early-exit_amd")

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

    cfg = pkg.ModelConfig.base()
    B, T = a.docs, a.text_len
    E = cfg.exit_config.num_exits
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T)
    eng.load_weights(pkg.synth.make_weights(cfg, seed=41, head_gain=4.0))
    d = pkg.synth.make_documents(cfg, B, seed=42, text_len=T, min_words=3)
    t = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}
    table = eng.forward(**t, dump_all=True, want_all=True).all_crit.cpu().numpy().astype(np.float64)
    thr, want = cascade(np, table, a.release)
    kinds = [("off", 0.0)] + [(f"p={p:g}", p) for p in SHARES] + [("dump-all", None)]

    def call(share):
        if share is None:
            return eng.forward(**t, dump_all=True, want_all=True)
        eng.set_audit(share or None, seed=a.seed)
        return eng.forward(**t, thresholds=thr, want_all=True)

    if a.trace:
        for share in (0.25, 0.0):
            for _ in range(a.trace):
                call(share)
        torch.cuda.synchronize()
        print(f"trace: {a.trace} audited (share 0.25) and {a.trace} unaudited forwards done", flush=True)
        return
    say(f"audited exits in the forward: LayoutLMv3-base, exits {cfg.exit_config.exits} (E = {E}), {B} documents, T = {T}, precision {eng.precision}, "
        f"{torch.cuda.get_device_name(0)}; thresholds release {a.release:.2f} of the documents that reach an exit; audit seed {a.seed}; every call with "
        f"want_all=True; event-timed forwards, {a.reps} per kind and round, 3 rounds alternated in one process")
    res, info = {k: [] for k, _ in kinds}, {}
    base = None
    for rnd in range(3):
        for kind, share in kinds:
            for _ in range(2):
                out = call(share)
            if rnd == 0:
                eng.profile(True)
                call(share)
                prof = eng.profile_read()
                eng.profile(False)
                ex = out.exit_layer.cpu().numpy()
                if base is None:
                    base = {f: getattr(out, f).cpu().numpy().view(np.int32) for f in ("logits", "exit_layer", "confidence")}
                same = share is None or all(np.array_equal(getattr(out, f).cpu().numpy().view(np.int32), base[f]) for f in base)
                info[kind] = (eng.stage_counts()["docs"], eng.stage_counts()["rows"], int(out.audit_mask.sum()) if out.audit_mask is not None else 0,
                              (prof["exit_decide"]["launches"], round(prof["exit_decide"]["ms"], 4)), sum(v["launches"] for v in prof.values()), same,
                              np.bincount(ex, minlength=E + 1).tolist())
            res[kind] += timed(lambda: call(share), a.reps)
    med = {k: float(np.median(v)) for k, v in res.items()}
    gap = med["dump-all"] - med["off"]
    for kind, share in kinds:
        ms = np.array(res[kind])
        docs, rows, nsel, decide, launches, same, hist = info[kind]
        line = (f"  {kind:<8s}: {med[kind]:8.3f} ms per forward (median of {ms.size}; min {ms.min():.3f}, max {ms.max():.3f}, std {ms.std():.3f}); documents "
                f"reaching each exit {docs}; rows {rows}; profiled launches {launches}; exit_decide (launches, event ms) {decide}")
        if share:
            p = nsel / B
            line += (f"; selected {nsel} of {B} (p = {p:.4f}); extra over off {med[kind] - med['off']:+.3f} ms against p x (dump-all - off) = {p * gap:.3f} ms; "
                     f"results bitwise those of off: {same}")
        elif share == 0.0:
            line += f"; exit histogram {hist}"
        say(line)
    say(f"  dump-all - off = {gap:.3f} ms.  The off series' own spread (max - min) is {max(res['off']) - min(res['off']):.3f} ms.")
    say("  The agreement rates are not measured: synthetic weights, no trained checkpoint exists here.")
    eng.close()
    flush()


if __name__ == "__main__":
    main()
