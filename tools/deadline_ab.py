"""What deadline exits (include/mmee.h, behind the controller's) cost and what they buy (GPU box).  No pass bar; the output is what README,
DESIGN and profiles/deadline.txt quote.

  clock     two ``clock_stamp()`` 2 ms apart: the spread of s_memrealtime over the CUs inside one stamp (the design's precondition).
  overhead  LayoutLMv3-base, the default exit list, synthetic weights, split precision, thresholds releasing a quarter per exit: a deadline
            call that never cuts (budget 10 s) against the plain call, alternated in one process, 30 each; the "deadline" role's launches.
  tail      a cut forced at every exit: elapsed[E1 - 1] - elapsed[cut_exit] from the log (the empty launches behind the cut), and the whole
            call against the plain call whose thresholds release everybody at that exit -- the same launches.
  claim     the quota paragraph's 20 resident batches (tools/quota_exit_ab.py, same seeds): per-forward time under fixed thresholds without a
            deadline; with a deadline at that series' median and eta = eta_from_logs of a stamps-only pass over OTHER batches (seeds 200 + i);
            the worst overshoot over the budget; the documents cut per batch.  The same with eta = the stretch to the NEXT check plus the tail
            (--tail-ms), and with zero eta.
  bench     --bench-parent DIR: ``bench.py --gpus 1 --steps 6 --warmup 2`` of this tree and of the built parent checkout in DIR, alternating,
            three runs each, each in a process of its own.
  trace     --trace N: N deadline forwards and nothing else -- the program of
            ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/deadline_ab.py --trace N``, a run of its own.
  summarise --summarise DIR: the two added kernels' rows of that run's kernel-stats CSV.

ACCURACY IS NOT MEASURED: the weights are synthetic, no trained checkpoint exists here.

    python tools/deadline_ab.py [--out FILE] [--only clock,overhead,tail,claim] [--docs 256] [--text-len 512] [--reps 30] [--batches 20] [--tail-ms 0.8]
                                [--bench-parent DIR [--bench-only]] [--trace N | --summarise DIR]
"""
import argparse
import csv
import glob
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summarise(directory, say):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        say(f"kernel trace: no *kernel_stats.csv under {directory}")
        return
    say(f"kernel trace (rocprofv3 --kernel-trace --stats, a run of its own; {os.path.basename(files[0])}): the two added kernels")
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            if "deadline_begin" in row.get("Name", "") or "deadline_check" in row.get("Name", ""):
                name = row["Name"].split("(")[0]
                say(f"  {name:<32s} calls {row.get('Calls'):>5s}  total {float(row.get('TotalDurationNs', 'nan')) / 1e3:10.1f} us  mean "
                    f"{float(row.get('AverageNs', 'nan')) / 1e3:7.2f} us  min {float(row.get('MinNs', 'nan')) / 1e3:7.2f}  max {float(row.get('MaxNs', 'nan')) / 1e3:7.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--only", default="clock,overhead,tail,claim")
    ap.add_argument("--docs", type=int, default=256)
    ap.add_argument("--text-len", type=int, default=512)
    ap.add_argument("--release", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--tail-ms", type=float, default=0.8, help="claim: the tail behind a cut (the `tail` series measures it)")
    ap.add_argument("--bench-parent", default=None)
    ap.add_argument("--bench-only", action="store_true", help="only the bench.py alternation")
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--summarise", default=None)
    a = ap.parse_args()
    only = set(a.only.split(","))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")

    from tools.controller_ab import run_bench
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

    def batch(cfg, B, T, seed, min_words=3):
        d = pkg.synth.make_documents(cfg, B, seed=seed, text_len=T, min_words=min_words)
        return {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}

    def stats(ms):
        ms = np.asarray(ms)
        return f"mean {ms.mean():.3f}, median {np.median(ms):.3f}, min {ms.min():.3f}, max {ms.max():.3f}, std {ms.std():.3f}"

    cfg = pkg.ModelConfig.base()
    B, T = a.docs, a.text_len
    E = cfg.exit_config.num_exits
    name = torch.cuda.get_device_name(0)
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T)
    eng.load_weights(pkg.synth.make_weights(cfg, seed=41, head_gain=4.0))
    t = batch(cfg, B, T, 42)
    table = eng.forward(**t, dump_all=True, want_all=True).all_crit.cpu().numpy().astype(np.float64)
    thr, want = cascade(np, table, a.release)
    sign = -1.0 if cfg.exit_config.inference_strategy.value == "entropy" else 1.0
    fires = np.inf if sign < 0 else -np.inf
    head = (f"LayoutLMv3-base, exits {cfg.exit_config.exits} (E = {E}), {B} documents, T = {T}, precision {eng.precision}, {name}; thresholds release "
            f"{a.release:.2f} of the documents that reach an exit (exit histogram {np.bincount(want, minlength=E + 1).tolist()})")

    if a.trace:
        eng.set_deadline(10e3)
        for _ in range(a.trace):
            eng.forward(**t, thresholds=thr)
        torch.cuda.synchronize()
        print(f"trace: {a.trace} deadline forwards done", flush=True)
        return

    if "clock" in only:
        sa = eng.clock_stamp()
        torch.cuda.synchronize()
        time.sleep(0.002)
        sb = eng.clock_stamp()
        torch.cuda.synchronize()
        ra, rb = sa.cpu().numpy()[1::2], sb.cpu().numpy()[1::2]
        m = (ra != 0) & (rb != 0)
        say(f"s_memrealtime, two stamps 2 ms apart, {int(m.sum())} CU slots filled in both ({name}): spread inside stamp A {int(ra[m].max() - ra[m].min())} ticks of 10 ns, "
            f"inside stamp B {int(rb[m].max() - rb[m].min())}; min(B) - max(A) = {int(rb[m].min() - ra[m].max())} ticks.  (2048 one-wave workgroups per stamp: the "
            "spread includes the time the stamp's own dispatch takes.)")

    if "overhead" in only:
        say("deadline exits in the forward: " + head)
        say(f"  a deadline call that never cuts (budget 10 s, zero eta) against the plain call, event-timed, {a.reps // 3} per kind and round, 3 rounds alternated in one process")
        res, info = {"plain": [], "deadline": []}, {}
        for rnd in range(3):
            for kind in ("plain", "deadline"):
                eng.set_deadline(10e3 if kind == "deadline" else None)
                fn = lambda: eng.forward(**t, thresholds=thr)
                for _ in range(2):
                    out = fn()
                if rnd == 0:
                    eng.profile(True)
                    fn()
                    prof = eng.profile_read()
                    eng.profile(False)
                    info[kind] = (prof.get("deadline", {"launches": 0, "ms": 0.0}), sum(v["launches"] for v in prof.values()),
                                  np.bincount(out.exit_layer.cpu().numpy(), minlength=E + 1).tolist())
                res[kind] += timed(fn, a.reps // 3)
        for kind in res:
            dl, launches, hist = info[kind]
            say(f"  {kind:<8s}: ms per forward {stats(res[kind])} ({len(res[kind])} calls); profiled launches {launches}; deadline role (launches, event ms) "
                f"({dl['launches']}, {dl['ms']:.4f}); exit histogram {hist}")
        say(f"  deadline - plain = {np.mean(res['deadline']) - np.mean(res['plain']):+.4f} ms (means), {np.median(res['deadline']) - np.median(res['plain']):+.4f} ms "
            f"(medians).  The plain series' own spread (max - min) is {max(res['plain']) - min(res['plain']):.3f} ms.")
        log = eng.deadline_log()
        say(f"  the log's timeline of the last deadline call, ms from the begin launch to the check in front of each exit: "
            f"{np.round(log.elapsed_ns[-1].astype(np.float64) / 1e6, 3).tolist()}")

    if "tail" in only:
        say(f"the tail behind a cut: a cut forced at every exit (budget 2^62 ns, eta 2^63 ns at that exit), {a.reps // 3} event-timed calls each, alternated with the "
            "plain call whose thresholds release everybody at that exit (the same launches, plus the deadline's E1 + 1)")
        for e_star in range(E):
            eta = np.zeros(E + 1)
            eta[e_star] = 2.0 ** 63 / 1e6
            thr_p = thr.copy()
            thr_p[e_star:E] = fires
            ms = {"cut": [], "plain": []}
            for rnd in range(3):
                eng.set_deadline(2.0 ** 62 / 1e6, eta_ms=eta, log_cap=64)
                eng.forward(**t, thresholds=thr)
                ms["cut"] += timed(lambda: eng.forward(**t, thresholds=thr), a.reps // 9 + 1)
                log = eng.deadline_log()
                eng.set_deadline(None)
                eng.forward(**t, thresholds=thr_p)
                ms["plain"] += timed(lambda: eng.forward(**t, thresholds=thr_p), a.reps // 9 + 1)
            el = log.elapsed_ns.astype(np.float64) / 1e6
            assert (log.cut_exit == e_star).all()
            tail = el[:, E] - el[:, e_star]
            say(f"  cut at exit {e_star}: to the cut {np.median(el[:, e_star]):7.3f} ms, tail of empty launches {np.median(tail):6.3f} ms (max {tail.max():.3f}); whole call "
                f"{np.median(ms['cut']):7.3f} ms cut, {np.median(ms['plain']):7.3f} ms plain under thr', difference {np.median(ms['cut']) - np.median(ms['plain']):+.3f} ms")

    if "claim" in only:
        say(f"the claim: per-forward time over {a.batches} different resident batches (seed 100 + i, at least 3 + 24 i words per document, as in "
            f"tools/quota_exit_ab.py), fixed thresholds, 3 event-timed forwards each after a warm-up (median): " + head)
        mw = lambda bi: 3 + (24 * bi) % (T - 32)
        # eta from a stamps-only pass over OTHER batches
        eng.set_deadline(None, stamps_only=True, log_cap=4 * a.batches)
        for bi in range(a.batches):
            tb = batch(cfg, B, T, 200 + bi, min_words=mw(bi))
            for _ in range(2):
                eng.forward(**tb, thresholds=thr)
            del tb
        stamps = eng.deadline_log()
        eta = pkg.eta_from_logs(stamps)
        say(f"  eta_from_logs (maximum) of a stamps-only pass over {a.batches} other batches (seeds 200 + i), ms: {np.round(eta, 3).tolist()}")
        # a second table a caller may pass: not "the time to the end if nobody is cut here" but "the time to the end if everybody is cut at
        # the NEXT exit" = the stretch to the next check plus the tail of empty launches behind a cut; the last exit below the final one has
        # no next cut, its entry is eta_from_logs' own
        eta_next = pkg.eta_to_next_exit(stamps, a.tail_ms)
        say(f"  eta_to_next_exit (maximum stretch between two checks over the same logs + {a.tail_ms} ms tail), ms: {np.round(eta_next, 3).tolist()}")
        eng.set_deadline(None)
        per, batches = [], []
        for bi in range(a.batches):
            tb = batch(cfg, B, T, 100 + bi, min_words=mw(bi))
            batches.append(tb)
            eng.forward(**tb, thresholds=thr)
            per.append(float(np.median(timed(lambda: eng.forward(**tb, thresholds=thr), 3))))
        per = np.array(per)
        budget = float(np.median(per))
        say(f"  no deadline   : per-batch ms min {per.min():.3f}, median {budget:.3f}, max {per.max():.3f}, max - min {per.max() - per.min():.3f} "
            f"({100 * (per.max() - per.min()) / budget:.1f} % of the median)")
        for tag, eta_ms in (("eta from logs", eta), ("eta to next", eta_next), ("zero eta", None)):
            eng.set_deadline(budget, eta_ms=eta_ms, log_cap=8 * a.batches)
            got, dev_ms, cut_docs, cut_at = [], [], [], []
            for tb in batches:
                eng.forward(**tb, thresholds=thr)
                got.append(float(np.median(timed(lambda: eng.forward(**tb, thresholds=thr), 3))))
                log = eng.deadline_log()
                dev_ms.append(float(log.elapsed_ns[-1, E]) / 1e6)
                ce = int(log.cut_exit[-1])
                cut_at.append(ce)
                if ce >= 0:
                    out = eng.forward(**tb, thresholds=thr)
                    eng.set_deadline(None)
                    plain_exit = eng.forward(**tb, thresholds=thr).exit_layer.cpu().numpy()
                    eng.set_deadline(budget, eta_ms=eta_ms, log_cap=8 * a.batches)
                    cut_docs.append(int((plain_exit > out.exit_layer.cpu().numpy()).sum()))
                else:
                    cut_docs.append(0)
            got = np.array(got)
            say(f"  deadline at the median, {tag:<13s}: per-batch ms min {got.min():.3f}, median {np.median(got):.3f}, max {got.max():.3f}, max - min "
                f"{got.max() - got.min():.3f} ({100 * (got.max() - got.min()) / budget:.1f} % of the budget); worst overshoot over the budget "
                f"{got.max() - budget:+.3f} ms event-timed, {max(dev_ms) - budget:+.3f} ms on the device clock up to the last check; batches cut "
                f"{int((np.array(cut_at) >= 0).sum())} of {a.batches}, cut_exit per batch {cut_at}; documents that left earlier than under the plain thresholds, per batch {cut_docs}")
        say("  ACCURACY IS NOT MEASURED: synthetic weights, no trained checkpoint exists here.  What a cut costs in accuracy is the accuracy of the exit it releases at.")
    eng.close()
    run_bench(a, say)
    flush()


if __name__ == "__main__":
    main()
