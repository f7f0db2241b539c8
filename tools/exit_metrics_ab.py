"""A/B of the device-side evaluation report (ee_exit_metrics / metrics.exit_report) against the route that exists without it (GPU box).

The reference's shape: E1 = 7 exits, N = 40 000 documents, K = 16 labels; synthetic logits from the generator of tests/conftest.py
(``sweep_ref_inputs``), one operating point (``criterion_scan_device`` at every exit's median confidence).  Logits, labels and exits are on the
device before either clock starts.  One process, alternating blocks:

  (a) ``metrics.exit_report(logits, refs, exits=)``: one device call, the (8, 8) result downloaded
  (b) the host route: download the (E1, N, K) float64 array, then numpy per exit and for the operating point in the style of
      tests/metrics_ref.py -- softmax, argmax, Brier, NLL, confusion counts and macro F1, the risk-coverage loop (a Python loop over the sorted
      documents, as the reference's ``rc_curve_stats`` is) -- with ``calibration.expected_calibration_error`` for the ECE

Every block ends in a device synchronise and is timed with the host clock; reported: each block, the median, the spread (max - min), the
largest relative difference between the two routes' numbers, and route (a) alone at other N (the counting sort is O(N^2) per row).

    python tools/exit_metrics_ab.py [--out FILE] [--rounds R]      the table (also printed)
    python tools/exit_metrics_ab.py --trace R                      R calls of (a) on device-resident inputs and nothing else: the program of
                                                                   ``rocprofv3 --kernel-trace --output-format csv`` (no counters in that run)
    python tools/exit_metrics_ab.py --summarise CSV R [--out FILE] per kernel of the last R calls of that trace: calls, median, min, max
                                                                   microseconds (appended to FILE)
"""
import argparse
import collections
import csv
import importlib
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

E1, N, K = 7, 40000, 16
SCALING = (10000, 20000, 40000, 80000, 160000)


def summarise(path, rounds, out):
    import numpy as np
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    idx = [i for i, r in enumerate(rows) if "metrics_rows_kernel" in r["Kernel_Name"]]        # one per call
    sel = rows[idx[-rounds]:]
    acc = collections.defaultdict(list)
    for r in sel:
        name = re.sub(r"^(void )?(mmee::)?", "", r["Kernel_Name"]).split("(")[0]
        if name.startswith("metrics_"):
            acc[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    lines = [f"kernel trace, last {rounds} ee_exit_metrics calls, E1 = {E1} (+ the operating point), N = {N}, K = {K}, microseconds per launch",
             f"{'kernel':<28} {'calls':>5} {'median':>10} {'min':>10} {'max':>10}"]
    for name, ts in sorted(acc.items(), key=lambda kv: -float(np.median(kv[1]))):
        lines.append(f"{name:<28} {len(ts):>5} {float(np.median(ts)):>10.1f} {min(ts):>10.1f} {max(ts):>10.1f}")
    total = sum(float(np.median(ts)) for ts in acc.values())
    if "metrics_sort_kernel" in acc and total > 0:
        lines.append(f"metrics_sort_kernel is {100.0 * float(np.median(acc['metrics_sort_kernel'])) / total:.0f} % of the three kernels' {total:.0f} us")
    print("\n".join(lines))
    if out:
        with open(out, "a") as f:
            f.write("\n" + "\n".join(lines) + "\n")


def host_route(pkg, MR, logits_dev, refs_dev, exits_dev):
    import numpy as np
    L, refs, ex = logits_dev.cpu().numpy(), refs_dev.cpu().numpy(), exits_dev.cpu().numpy()
    n = L.shape[1]
    rows = []
    for z in list(L) + [L[ex, np.arange(n)]]:
        q = MR.row_quantities(z, refs)
        cm = MR.confusion_matrix(refs, q["pred"], z.shape[-1])
        hits = int(np.count_nonzero(q["correct"]))
        rows.append([hits / n, float(q["brier"].sum() / n), float(q["nll"].sum() / n), hits / n, MR.f1_macro(cm),
                     pkg.calibration.expected_calibration_error(refs, z), MR.aurc(q["conf"], q["correct"]), float(q["conf"].sum() / n)])
    return np.array(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--summarise", nargs=2, default=None)
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise[0], int(a.summarise[1]), a.out)
        return
    import numpy as np
    import torch
    from tests import metrics_ref as MR
    from tests.conftest import sweep_ref_inputs
    pkg = importlib.import_module("multi-modal-early-exit_amd")
    sync = torch.cuda.synchronize

    def inputs(n):
        logits, refs = sweep_ref_inputs(seed=2024, E1=E1, N=n, K=K)
        L, y = torch.from_numpy(logits).cuda(), torch.from_numpy(refs).cuda()
        conf, _ = pkg.sweep.msp_table(L, y)
        thr = conf.median(dim=1).values.cpu().numpy()
        ex = pkg.criterion_scan_device(L, thr, "max_confidence")[0]
        sync()
        return L, y, ex

    L, y, ex = inputs(N)

    def route_a():
        r = pkg.exit_report(L, y, exits=ex)
        sync()
        return r

    if a.trace:
        for _ in range(a.trace + 2):
            route_a()
        return

    def route_b():
        r = host_route(pkg, MR, L, y, ex)
        sync()
        return r

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(f):
        sync()
        t0 = time.perf_counter()
        out = f()
        return 1e3 * (time.perf_counter() - t0), out

    say(f"evaluation report A/B: E1 = {E1} exits and one operating point, N = {N}, K = {K}, inputs resident on the device; "
        f"{torch.cuda.get_device_name(0)}")
    ra, rb = route_a(), route_b()                                  # warm-up of both routes, and what they compute
    got = np.stack([getattr(ra, name) for name in pkg.metrics.FIELDS], axis=1)
    rel = np.abs(got - rb) / np.maximum(np.abs(rb), 1e-300)
    say(f"largest relative difference between the routes over the {got.size} numbers: {rel.max():.2e}; exit histogram {ra.exit_hist.tolist()}")
    ta, tb = [], []
    for _ in range(a.rounds):
        ta.append(timed(route_a)[0])
        tb.append(timed(route_b)[0])
    fmt = lambda xs: " ".join(f"{x:.2f}" for x in xs)
    say(f"(a) exit_report on the device     ms per block: {fmt(ta)}   median {np.median(ta):.2f}  spread {max(ta) - min(ta):.2f}")
    say(f"(b) download + numpy on the host  ms per block: {fmt(tb)}   median {np.median(tb):.2f}  spread {max(tb) - min(tb):.2f}")
    say(f"(b) / (a) = {np.median(tb) / np.median(ta):.1f}; the download of (b) alone is {L.numel() * 8 / 1e6:.1f} MB")
    say("route (a) alone at other N (ms per call, median of the rounds; x4 per doubling = the O(N^2) counting sort dominates):")
    for n in SCALING:
        Ln, yn, exn = (L, y, ex) if n == N else inputs(n)
        pkg.exit_report(Ln, yn, exits=exn)
        ts = [timed(lambda: (pkg.exit_report(Ln, yn, exits=exn), sync()))[0] for _ in range(a.rounds)]
        say(f"  N = {n:>7}: {np.median(ts):8.2f}  spread {max(ts) - min(ts):.2f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
