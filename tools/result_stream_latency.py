"""What the result stream (MMEE_FLAG_STREAM_RESULTS, ``EarlyExitEngine.forward_stream``) buys and costs (GPU box; same box, one process
for everything that is compared with itself).

LayoutLMv3-base with exits 2 / 4 / 6 / 8 / 10, T = 512, B = 1024 synthetic documents on ONE handle, thresholds calibrated on the batch's own
dump so that every exit releases a fifth of the documents that reach it (the mix of ``bench.py --release 0.2``: mean exit layer ~7.4 of 12).

(a) Arrival.  Per exit, the host time from the call of ``forward_stream`` to the moment its chunk is in the caller's hands, as a fraction of
    the time the same forward WITHOUT the flag takes from its call to the end of a synchronise, with the cumulative share of the documents
    delivered by then.  Medians over ``--repeats`` forwards.  The claim is the ordering: the first non-empty chunk arrives before the flag-off
    forward completes.
(b) Cost.  Documents per second over blocks of ``--block`` forwards, the forms alternating block by block:
      off        flag off, forwards enqueued back to back, one synchronise per block (pipelined);
      off_sync   flag off, a synchronise behind every forward (what a caller who consumes every result pays without the flag);
      on         flag on, every stream drained before the next forward (a flagged forward waits on the host for the one before, by contract);
    and, with ``--parent-lib PATH`` (a libmmee_hip.so built from the parent commit), `off` on that build in child processes before and after.
    The flag-on loss is compared with (E + 1) x the per-launch time ``ee_profile_read`` reports for the emit_leavers role in this very run.

    python tools/result_stream_latency.py [--out FILE] [--parent-lib PATH]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EXITS = dict(exits=[2, 4, 6, 8, 10], encoder_layer_strategy="ramp")
LAYER_OF_EXIT = [2, 4, 6, 8, 10, 12]
KEYS = ("input_ids", "attention_mask", "bbox", "pixel_values")
B, T, RELEASE = 1024, 512, 0.2


def calibrate(conf, release):
    """Per-exit thresholds in the widest gap near the quantile at which an exit releases `release` of the documents that reach it."""
    import numpy as np
    E1, n = conf.shape
    active = np.ones(n, dtype=bool)
    thr = np.full(E1, 2.0)
    for e in range(E1 - 1):
        c = np.sort(conf[e, active])
        k = min(max(int(round((1.0 - release) * len(c))), 1), len(c) - 1)
        lo, hi = max(1, k - 3), min(len(c) - 1, k + 3)
        j = lo + int(np.argmax(c[lo:hi + 1] - c[lo - 1:hi]))
        thr[e] = 0.5 * (c[j - 1] + c[j])
        active &= ~(conf[e] > thr[e])
    return thr


def setup(batch, older_build=False):
    import torch
    pkg = importlib.import_module("multi-modal-early-exit_amd")
    if older_build:                                # a parent-commit library lacks what this commit adds: bind what it exports
        import ctypes
        lib = ctypes.CDLL(pkg.capi.lib_path())
        for name in [n for n in pkg.capi.SYMBOLS if not hasattr(lib, n)]:
            del pkg.capi.SYMBOLS[name]
    cfg = pkg.ModelConfig.base(EE_config=EXITS)
    eng = pkg.EarlyExitEngine(cfg, max_docs=batch, max_text_len=T)
    eng.load_weights(pkg.synth.make_weights(cfg, seed=1234, head_gain=6.0))
    d = pkg.synth.make_documents(cfg, batch, seed=900, text_len=T)
    return pkg, eng, {k: torch.from_numpy(d[k]).cuda() for k in KEYS}


def block_rate(eng, t, thr, form, n_fwd):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n_fwd):
        if form == "on":
            for _chunk in eng.forward_stream(**t, thresholds=thr):
                pass
        else:
            eng.forward(**t, thresholds=thr)
            if form == "off_sync":
                torch.cuda.synchronize()
    torch.cuda.synchronize()
    return n_fwd * int(t["pixel_values"].shape[0]) / (time.perf_counter() - t0)


def cost_child(a):
    """`off` blocks on whatever library MMEE_LIB names; one JSON line."""
    pkg, eng, t = setup(a.batch, older_build=True)
    thr = [float(x) for x in a.thresholds.split(",")]
    for _ in range(3):
        eng.forward(**t, thresholds=thr)
    rates = [block_rate(eng, t, thr, "off", a.block) for _ in range(a.blocks)]
    eng.check()
    print("COST_CHILD " + json.dumps({"lib": pkg.capi.lib_path(), "rates": rates}), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--batch", type=int, default=B)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--block", type=int, default=6)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--thresholds", default="")
    ap.add_argument("--cost-child", action="store_true")
    a = ap.parse_args()
    if a.cost_child:
        cost_child(a)
        return
    import numpy as np
    import torch
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    pkg, eng, t = setup(a.batch)
    sync = torch.cuda.synchronize
    E1 = eng.E + 1
    dump = eng.forward(**t, dump_all=True, want_all=True)
    thr = calibrate(dump.all_crit.cpu().numpy().astype(np.float64), RELEASE)
    eng.check()
    say(f"result stream: LayoutLMv3-base, exits 2/4/6/8/10, T = {T}, B = {a.batch} on one handle, default schedule, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs")
    say("thresholds (every exit releases a fifth of the documents that reach it): " + ", ".join(f"{x:.6f}" for x in thr))

    def parent_blocks(tag):
        if not a.parent_lib:
            return None
        cmd = [sys.executable, os.path.abspath(__file__), "--cost-child", "--batch", str(a.batch), "--block", str(a.block), "--blocks", str(a.blocks),
               "--thresholds", ",".join(repr(float(x)) for x in thr)]
        r = subprocess.run(cmd, env=dict(os.environ, MMEE_LIB=os.path.abspath(a.parent_lib)), capture_output=True, text=True, timeout=600)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("COST_CHILD ")]
        if r.returncode != 0 or not got:
            say(f"parent build ({tag}): the child failed ({r.returncode}): {r.stderr[-400:]}")
            return None
        return json.loads(got[-1][len("COST_CHILD "):])["rates"]

    parent_before = parent_blocks("before")

    for form in ("off", "on"):                     # warm-up of both forms
        for _ in range(3):
            block_rate(eng, t, thr, form, 1)

    # ---- (a) arrival ----------------------------------------------------------------------------------------------------------------------
    off_ms, arrive, total_on = [], [], []
    for _ in range(a.repeats):
        sync()
        t0 = time.perf_counter()
        eng.forward(**t, thresholds=thr)
        sync()
        off_ms.append(1e3 * (time.perf_counter() - t0))
        sync()
        t0 = time.perf_counter()
        st = eng.forward_stream(**t, thresholds=thr)
        enq = 1e3 * (time.perf_counter() - t0)
        row = [(1e3 * (time.perf_counter() - t0), ch.doc_index.size) for ch in st]
        sync()
        total_on.append(1e3 * (time.perf_counter() - t0))
        arrive.append((enq, row))
    eng.check()
    ex = st.output.exit_layer.cpu().numpy()
    sizes = [n for _, n in arrive[-1][1]]
    assert sizes == np.bincount(ex, minlength=E1).tolist() and sum(sizes) == a.batch
    t_off = float(np.median(off_ms))
    say()
    say(f"(a) arrival, medians of {a.repeats} forwards.  Flag off, call to the end of a synchronise: {t_off:.2f} ms "
        f"(min {min(off_ms):.2f}, max {max(off_ms):.2f}); flag on, call to the end of a synchronise: {float(np.median(total_on)):.2f} ms; "
        f"the flagged call itself returns after {float(np.median([e for e, _ in arrive])):.2f} ms")
    say(f"mean exit layer {float(np.array(LAYER_OF_EXIT)[ex].mean()):.2f} of 12")
    say(f"{'exit':>4} {'layer':>5} {'documents':>9} {'cumulative share':>16} {'arrival ms':>10} {'/ flag-off forward':>18}")
    cum, first = 0, None
    for e in range(E1):
        ms = float(np.median([r[e][0] for _, r in arrive]))
        cum += sizes[e]
        if first is None and sizes[e]:
            first = (e, ms)
        say(f"{e:>4} {LAYER_OF_EXIT[e]:>5} {sizes[e]:>9} {cum / a.batch:>16.3f} {ms:>10.2f} {ms / t_off:>18.3f}")
    ok = first is not None and first[1] < t_off
    say(f"first non-empty chunk: exit {first[0]} after {first[1]:.2f} ms = {first[1] / t_off:.3f} of the flag-off forward: "
        + ("BEFORE it completes" if ok else "NOT before it completes: the events are not where they should be"))

    # ---- (b) cost ---------------------------------------------------------------------------------------------------------------------------
    forms = ("off", "off_sync", "on")
    rates = {f: [] for f in forms}
    for _ in range(a.blocks):
        for f in forms:
            rates[f].append(block_rate(eng, t, thr, f, a.block))
    eng.profile(True)
    for _chunk in eng.forward_stream(**t, thresholds=thr):
        pass
    prof = eng.profile_read()
    eng.profile(False)
    eng.check()
    emit = prof["emit_leavers"]
    emit_us = 1e3 * emit["ms"] / max(emit["launches"], 1)
    parent_after = parent_blocks("after")

    def line(name, xs):
        xs = [float(x) for x in xs]
        say(f"{name:<34} median {np.median(xs):9.1f} docs/s   spread (max - min) {max(xs) - min(xs):7.1f}   blocks " + " ".join(f"{x:.1f}" for x in xs))
        return float(np.median(xs))

    say()
    say(f"(b) cost: {a.blocks} blocks of {a.block} forwards per form, forms alternating")
    m = {f: line({"off": "this build, flag off, pipelined", "off_sync": "this build, flag off, synchronised", "on": "this build, flag on, drained"}[f],
                 rates[f]) for f in forms}
    if parent_before and parent_after:
        p = line("parent build, flag off, pipelined", parent_before + parent_after)
        sp = max(parent_before + parent_after) - min(parent_before + parent_after)
        say(f"flag off against the parent: {100 * (m['off'] / p - 1):+.2f} % (the parent's own spread: {100 * sp / p:.2f} %): "
            + ("within it" if abs(m["off"] - p) <= sp else "OUTSIDE it"))
    else:
        say("parent build: not measured (no --parent-lib)")
    fwd_off, fwd_sync, fwd_on = (1e3 * a.batch / m[f] for f in forms)
    say(f"per forward: {fwd_off:.3f} ms pipelined, {fwd_sync:.3f} ms synchronised, {fwd_on:.3f} ms flag on")
    say(f"emit_leavers: {emit['launches']} launches, {emit_us:.1f} us each between its events -> (E + 1) x = {1e-3 * emit_us * E1:.3f} ms per forward")
    say(f"flag on costs {fwd_on - fwd_sync:+.3f} ms per forward against the synchronised flag-off forward (the like-for-like form: a drained stream "
        f"ends where a synchronise does) and {fwd_on - fwd_off:+.3f} ms against the pipelined one, whose next forward is enqueued while this one runs; "
        f"a flagged forward waits on the host for the one before, so {fwd_sync - fwd_off:+.3f} ms of that is the exposed enqueue, flag or no flag")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
