"""Measurement of the encoder-free feature pass (``heads.collect_embedding_features`` / ee_embedding_inputs) against the dump-all collection
(``heads.collect_exit_features(..., embedding_exits=True)``) on the same build (GPU box).  No pass bar; the output is what README quotes.

LayoutLMv3-base with the reference's default exit list ["text_avg", "vision_avg", 1, 4, 8], T = 512, split precision, ``--docs`` synthetic
documents resident on the device in batches of ``--batch``.  Reported:
  * microseconds per document of ``collect_embedding_features`` and of ``collect_exit_features(..., embedding_exits=True)`` over the same
    batches: the two alternate inside every round, each pass ends in a synchronise, median over the rounds (min, max), and their ratio;
  * from a kernel trace of this program's own ``--trace`` run (a child process under ``rocprofv3 --kernel-trace``): calls and mean duration
    per ee_embedding_inputs call of every kernel of the pass -- embed_text, patch split + patch GEMM, embed_visual, pool_finish, prep.

    python tools/embedding_features_ab.py [--out FILE] [--docs 256] [--batch 64] [--rounds 5] [--no-trace]
    python tools/embedding_features_ab.py --trace N            N synchronised embedding passes of one batch, nothing else
    python tools/embedding_features_ab.py --summarise CSV N    the per-kernel table of the last N passes of that run's kernel trace
"""
import argparse
import collections
import csv
import glob
import importlib
import os
import shutil
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EXITS = dict(exits=["text_avg", "vision_avg", 1, 4, 8], encoder_layer_strategy="ramp")       # EE/models/EE_modules.py:186-188
KEYS = ("input_ids", "attention_mask", "bbox", "pixel_values")
T = 512


def summarise(path, n_calls, say=print):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    idx = [i for i, r in enumerate(rows) if "doc_prep" in r["Kernel_Name"]]       # one per call
    sel = rows[idx[-n_calls]:]
    acc = collections.defaultdict(lambda: [0, 0.0])
    for r in sel:
        n = r["Kernel_Name"].replace("void mmee::", "")[:90]
        acc[n][0] += 1
        acc[n][1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    tot = sum(v[1] for v in acc.values())
    span = (int(sel[-1]["End_Timestamp"]) - int(sel[0]["Start_Timestamp"])) / 1e3
    say(f"kernel trace, last {n_calls} ee_embedding_inputs calls (synchronised): {len(sel) / n_calls:.1f} kernels per call; summed kernel time "
        f"{tot / n_calls:.1f} us per call; span {span / n_calls:.1f} us per call (incl. host gaps between calls)")
    for n, (c, t) in sorted(acc.items(), key=lambda kv: -kv[1][1]):
        say(f"{c / n_calls:6.1f} x {t / c:8.1f} us = {t / n_calls:8.1f} us/call ({100 * t / tot:4.1f} %)  {n}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the lines to this file (profiles/embedding_features.txt holds one run)")
    ap.add_argument("--docs", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--summarise", nargs=2, default=None)
    ap.add_argument("--no-trace", action="store_true", help="skip the child process under rocprofv3")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise[0], int(a.summarise[1]))
        return
    import torch
    pkg = importlib.import_module("multi-modal-early-exit_amd")
    cfg = pkg.ModelConfig.base(EE_config=EXITS)
    B = a.batch
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision="split")
    eng.load_weights(pkg.synth.make_weights(cfg, seed=1234))
    n_docs = B if a.trace else a.docs
    d = pkg.synth.make_documents(cfg, n_docs, seed=900, text_len=T)
    t = {k: torch.from_numpy(d[k]).cuda() for k in KEYS}
    batches = [{k: v[i:i + B] for k, v in t.items()} for i in range(0, n_docs, B)]
    sync = torch.cuda.synchronize

    if a.trace:
        for _ in range(a.trace + 5):
            eng.embedding_inputs(**batches[0])
            sync()
        return

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return (time.perf_counter() - t0) * 1e6 / n_docs, out

    layers = cfg.exit_config.exit_head_num_layers
    routes = [("collect_embedding_features (stage 0 alone)", lambda: pkg.collect_embedding_features(eng, batches)),
              ("collect_exit_features(embedding_exits=True) (dump-all forward + stage 0)",
               lambda: pkg.collect_exit_features(eng, batches, head_layers=layers, embedding_exits=True))]
    say(f"embedding features: LayoutLMv3-base, exits {EXITS['exits']}, T = {T}, split precision, {n_docs} documents in batches of {B}, resident on "
        f"{torch.cuda.get_device_name(0)}")
    shapes = [tuple(timed(fn)[1].shape) for _, fn in routes]           # warm-up: code objects, allocator
    per = {name: [] for name, _ in routes}
    for _ in range(a.rounds):
        for name, fn in routes:                                         # alternating inside every round
            per[name].append(timed(fn)[0])
    med = {}
    for (name, _), shape in zip(routes, shapes):
        p = sorted(per[name])
        med[name] = p[len(p) // 2]
        say(f"{name}: {med[name]:.2f} us per document (median of {len(p)} passes; min {p[0]:.2f}, max {p[-1]:.2f}); features {shape}")
    say(f"ratio of the medians: {med[routes[1][0]] / med[routes[0][0]]:.1f}")
    eng.close()

    if not a.no_trace:
        tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        n = 20
        with tempfile.TemporaryDirectory() as tmp:
            r = subprocess.run([tool, "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
                                "--trace", str(n), "--batch", str(B)], capture_output=True, text=True)
            found = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
            if r.returncode or not found:
                say(f"kernel trace: rocprofv3 returned {r.returncode}, {len(found)} trace file(s): {r.stderr[-400:]}")
            else:
                say(f"batch of {B} documents per call:")
                summarise(found[0], n, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
