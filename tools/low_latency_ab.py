"""A/B of the low-latency mode (MMEE_FLAG_LOW_LATENCY, ``forward(low_latency=True)``) against the flag-off path of the same build (GPU box).

One process; LayoutLMv3-base with exits 2 / 4 / 6 / 8 / 10, T = 512, 200 different synthetic documents.  For B in {1, 2, 4, 8}, with
``whole_layers=True`` and with the default schedule: every forward is followed by a synchronise, a block is one pass over the 200 documents in
batches of B; after a warm-up of the shape, flag off and flag on alternate in blocks, three blocks each.  Reported per (B, schedule): the S the
rule gave, median and mean milliseconds per forward of every block, the flag-off spread (max - min of its three block medians) and the
verdict: "faster" when the flag-on median is below the flag-off median by more than that spread, "slower" when above by more than it.
Then max |dlogit| between flag on and flag off over the 200 documents (dump-all, every exit, B = 1) and the exit indices that differ.

    python tools/low_latency_ab.py [--out FILE]            the table (also printed)
    python tools/low_latency_ab.py --trace N               N synchronised flagged B = 1 whole-layers forwards, nothing else: the program of
                                                           ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python ...``
    python tools/low_latency_ab.py --summarise CSV N       per-kernel calls / mean / share of the last N forwards of that run's kernel trace
"""
import argparse
import collections
import csv
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EXITS = dict(exits=[2, 4, 6, 8, 10], encoder_layer_strategy="ramp")
THR = [0.524, 0.542, 0.507, 0.431, 0.884, 2.0]           # the thresholds of tools/small_batch_probe.py: documents leave at every exit
KEYS = ("input_ids", "attention_mask", "bbox", "pixel_values")
N_DOCS, T = 200, 512


def summarise(path, n_fwd):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    idx = [i for i, r in enumerate(rows) if "doc_prep" in r["Kernel_Name"]]       # one per forward
    sel = rows[idx[-n_fwd]:]
    acc = collections.defaultdict(lambda: [0, 0.0])
    for r in sel:
        n = r["Kernel_Name"].replace("void mmee::", "")[:90]
        acc[n][0] += 1
        acc[n][1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    tot = sum(v[1] for v in acc.values())
    span = (int(sel[-1]["End_Timestamp"]) - int(sel[0]["Start_Timestamp"])) / 1e3
    print(f"last {n_fwd} forwards (B = 1, whole layers, low_latency, synchronised): {len(sel)} kernels, {len(sel) / n_fwd:.1f} per forward; summed kernel time "
          f"{tot / n_fwd:.1f} us per forward; span {span / n_fwd:.1f} us per forward (incl. host gaps between forwards)")
    for n, (c, t) in sorted(acc.items(), key=lambda kv: -kv[1][1])[:28]:
        print(f"{c / n_fwd:6.1f} x {t / c:7.1f} us = {t / n_fwd:7.1f} us/fwd ({100 * t / tot:4.1f} %)  {n}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--summarise", nargs=2, default=None)
    ap.add_argument("--batches", default="1,2,4,8")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise[0], int(a.summarise[1]))
        return
    import numpy as np
    import torch
    pkg = importlib.import_module("multi-modal-early-exit_amd")
    cfg = pkg.ModelConfig.base(EE_config=EXITS)
    eng = pkg.EarlyExitEngine(cfg, max_docs=8, max_text_len=T)
    eng.load_weights(pkg.synth.make_weights(cfg, seed=1234, head_gain=6.0))
    d = pkg.synth.make_documents(cfg, N_DOCS, seed=900, text_len=T)
    t = {k: torch.from_numpy(d[k]).cuda() for k in KEYS}
    sync = torch.cuda.synchronize
    batch = lambda B, j: {k: v[j * B:(j + 1) * B] for k, v in t.items()}

    if a.trace:
        for j in range(a.trace + 10):
            eng.forward(**batch(1, j % N_DOCS), thresholds=THR, whole_layers=True, low_latency=True)
            sync()
        print("S =", eng.last_k_splits())
        return

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rule = pkg.capi.load().ee_low_latency_k_splits
    H, I, Pv = cfg.hidden_size, cfg.intermediate_size, (cfg.input_size // cfg.patch_size) ** 2 + 1
    say(f"low-latency A/B: LayoutLMv3-base, exits 2/4/6/8/10, T = {T}, {N_DOCS} documents, {cus} CUs, thresholds {THR}")
    say("rule  B: S(attention output) / S(FFN down)   " + "  ".join(f"{B}: {rule(B * (T + Pv), H, H, cus)} / {rule(B * (T + Pv), H, I, cus)}" for B in range(1, 9)))

    def block(B, kw):
        ms = []
        for j in range(N_DOCS // B):
            b = batch(B, j)
            t0 = time.perf_counter()
            eng.forward(**b, thresholds=THR, **kw)
            sync()
            ms.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ms)), float(np.mean(ms))

    say(f"{'B':>2} {'schedule':<13} {'S':<7} {'flag off: median (mean) ms of 3 blocks':<46} {'flag on':<46} {'off':>7} {'spread':>7} {'on':>7} {'on/off':>7}  verdict")
    for B in [int(x) for x in a.batches.split(",")]:
        for name, sched in (("whole_layers", dict(whole_layers=True)), ("default", dict())):
            for low in (False, True):                   # warm-up of the shape, both forms
                for j in range(6):
                    eng.forward(**batch(B, j), thresholds=THR, low_latency=low, **sched)
                sync()
            S = eng.last_k_splits()
            off, on = [], []
            for _ in range(3):
                off.append(block(B, dict(sched)))
                on.append(block(B, dict(sched, low_latency=True)))
            m_off, m_on = float(np.median([x[0] for x in off])), float(np.median([x[0] for x in on]))
            spread = max(x[0] for x in off) - min(x[0] for x in off)
            verdict = "faster" if m_on < m_off - spread else ("slower" if m_on > m_off + spread else "within the spread")
            if S == (1, 1):
                verdict += " (rule declined: the same launches)"
            fmt = lambda xs: " ".join(f"{m:.3f} ({mean:.3f})" for m, mean in xs)
            say(f"{B:>2} {name:<13} {f'{S[0]} / {S[1]}':<7} {fmt(off):<46} {fmt(on):<46} {m_off:7.3f} {spread:7.3f} {m_on:7.3f} {m_on / m_off:7.3f}  {verdict}")

    # flag on against flag off on every document: every exit's logits (dump-all), and the exits of the thresholded forward
    worst, flips = 0.0, 0
    for j in range(N_DOCS):
        b = batch(1, j)
        x = eng.forward(**b, dump_all=True, want_all=True).all_logits
        y = eng.forward(**b, dump_all=True, want_all=True, low_latency=True).all_logits
        worst = max(worst, float((x - y).abs().max()))
        ex = eng.forward(**b, thresholds=THR, whole_layers=True).exit_layer
        ey = eng.forward(**b, thresholds=THR, whole_layers=True, low_latency=True).exit_layer
        flips += int((ex != ey).sum())
    eng.check()
    say(f"max |dlogit| flag on vs flag off over {N_DOCS} documents x {eng.E + 1} exits (B = 1, S = {eng.last_k_splits()}): {worst:.3e}; "
        f"exit indices that differ at these thresholds: {flips}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
