"""What the vision-first call (include/mmee.h at ee_forward_vision; EarlyExitEngine.forward_vision / forward_vision_first) costs (GPU box).  No
pass bar; the output is what README, DESIGN and profiles/vision_first.txt quote.  TIME ONLY: no trained checkpoint and no OCR engine exist here,
so neither the accuracy of a vision-only exit nor real OCR time saved is measured.

  kernels   (a) the program of a kernel trace of its own: vision_pool_kernel (ee_debug_vision_pool), embed_visual_kernel with vis_part set
            (ee_debug_embed, T = 1) and ln_rows_kernel (ee_debug_ln_rows, the same B Pv rows) on the same vis_raw, LayoutLMv3-base shape.
                rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/vision_first_ab.py --only kernels
                python tools/vision_first_ab.py --summarise DIR --out profiles/vision_first.txt
  phase1    (b) forward_vision at LayoutLMv3-base, B = 256 and B = 1024: docs/s over device events.  ``--only phase1_trace`` is the program of the
            kernel trace that gives the time per kernel (ee_profile times nothing inside ee_forward_vision); ``--summarise DIR --all``.
  seam      (c) forward_vision_first (dict route: no OCR is involved) against the one-call forward on the same 256 documents at T = 512, with
            thresholds[0] from the device's own dump so that 0 / 25 / 50 / 90 % leave at exit 0; the two alternate in one process, 30 calls
            each; phase 1 alone and the gather alone beside them.

    python tools/vision_first_ab.py [--out FILE] [--only phase1,seam] [--docs 256] [--text-len 512] [--release 0.2]
"""
import argparse
import csv
import ctypes as C
import glob
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VISION_EE = dict(exits=["vision_avg", "text_visual_concat", 2, 4, 6, 8, 10], encoder_layer_strategy="ramp", inference_strategy="max_confidence")
H, PV, KB = 768, 197, 1024          # the kernel A/B: LayoutLMv3-base rows, 1024 documents


def summarise(directory, say, every):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        say(f"kernel trace: no *kernel_stats.csv under {directory}")
        return
    say(f"kernel trace (rocprofv3 --kernel-trace --stats, a run of its own; {os.path.basename(files[0])})" +
        ("" if every else f": H = {H}, Pv = {PV}, B = {KB}; bytes = reads + writes of the launch's arguments"))
    rows_b = KB * PV * H * 4
    part_b = KB * ((PV + 31) // 32) * H * 4
    moved = {"vision_pool_kernel": KB * (PV - 1) * H * 4 + part_b,                      # vis_raw in, vis_part out
             "embed_visual_kernel": KB * (PV - 1) * H * 4 + rows_b + 2 * part_b,       # vis_raw in; X rows, vis_part and cat_part out
             "ln_rows_kernel": 2 * rows_b}                                              # rows in, rows out
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            name = name.rsplit("(", 1)[0] if name.endswith(")") else name      # without the argument list; "(anonymous namespace)::" stays
            key = next((k for k in moved if k in name), None)
            if not every and key is None and "pool_finish" not in name:
                continue
            mean = float(row.get("AverageNs", "nan"))
            line = (f"  {name[:72]:<72s} calls {row.get('Calls'):>5s}  mean {mean / 1e3:9.2f} us  min {float(row.get('MinNs', 'nan')) / 1e3:9.2f}  max "
                    f"{float(row.get('MaxNs', 'nan')) / 1e3:9.2f}")
            if key and not every:
                line += f"  {moved[key] / 1e6:7.1f} MB  {moved[key] / mean / 1e3:5.2f} TB/s"
            say(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--only", default="phase1,seam")
    ap.add_argument("--docs", type=int, default=256)
    ap.add_argument("--text-len", type=int, default=512)
    ap.add_argument("--release", type=float, default=0.2)
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--all", action="store_true", help="--summarise: every kernel of the trace")
    a = ap.parse_args()
    only = set(a.only.split(","))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def finish():
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")

    if a.summarise:
        summarise(a.summarise, say, a.all)
        return finish()
    import numpy as np
    import torch
    pkg = importlib.import_module("multi-modal-early-exit_amd")
    lib = pkg.capi.load()
    name = torch.cuda.get_device_name(0)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def events(fn, reps, warm=3):
        """ms per call over device events."""
        for _ in range(warm):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def stats(ms):
        ms = np.asarray(ms)
        return f"{ms.mean():.3f} ms (mean of {ms.size}; std {ms.std():.3f}, min {ms.min():.3f}, max {ms.max():.3f})"

    if "kernels" in only:
        g = torch.Generator(device="cuda").manual_seed(1)
        r = lambda *s: torch.randn(s, device="cuda", generator=g) * 0.05
        vis_raw, cls, pos = r(KB, PV - 1, H), r(H), r(PV, H)
        gam, bet = 1 + r(H), r(H)
        nch = (PV + 31) // 32
        part, pooled = torch.empty((KB * nch, H), device="cuda"), torch.empty((KB, H), device="cuda")
        ea = pkg.capi.DebugEmbedArgs()
        T, cs, ss = 1, 128, 128
        hold = dict(input_ids=torch.full((KB, T), 5, dtype=torch.int64, device="cuda"), bbox=torch.zeros((KB, T, 4), dtype=torch.int64, device="cuda"),
                    word=r(16, H), type=r(1, H), pos=r(8, H), xtab=r(8, cs), ytab=r(8, cs), htab=r(8, ss), wtab=r(8, ss), text_ln_g=gam, text_ln_b=bet,
                    vis_ln_g=gam, vis_ln_b=bet, ln2_g=gam, ln2_b=bet, cls_token=cls, pos_embed=pos, vis_raw=vis_raw,
                    X=torch.empty((KB * (T + PV), H), device="cuda"), vis_part=torch.empty((KB * nch, H), device="cuda"),
                    cat_part=torch.empty((KB * (nch + 1), H), device="cuda"), pooled_vis=torch.empty((KB, H), device="cuda"),
                    pooled_cat=torch.empty((KB, H), device="cuda"))
        for k, v in dict(B=KB, T=T, G=14, pad_id=1, vocab=16, max_2d=8, max_pos=8, type_vocab=1, dense_rows=0, H=H, cs=cs, ss=ss, text_eps=1e-5,
                         vis_eps=1e-6, eps2=1e-5, split_scale=0.0).items():
            setattr(ea, k, v)
        for k, v in hold.items():
            setattr(ea, k, v.data_ptr())
        err = C.c_int32(0)
        rows = KB * PV
        src, dst = torch.randn((rows, H), device="cuda"), torch.empty((rows, H), device="cuda")
        n_rows = torch.tensor([rows], dtype=torch.int32, device="cuda")
        for _ in range(10):
            pkg.capi.check(lib.ee_debug_vision_pool(ptr(vis_raw), ptr(cls), ptr(pos), ptr(gam), ptr(bet), 1e-6, KB, PV, H, ptr(part), ptr(pooled), stream()),
                           None, "ee_debug_vision_pool")
            pkg.capi.check(lib.ee_debug_embed(C.byref(ea), C.byref(err), stream()), None, "ee_debug_embed")
            pkg.capi.check(lib.ee_debug_ln_rows(ptr(src), ptr(dst), None, ptr(n_rows), rows, H, ptr(gam), ptr(bet), 1e-5, None, 0.0, 0, 0, None, None, None,
                                                0.0, C.byref(err), stream()), None, "ee_debug_ln_rows")
        torch.cuda.synchronize()
        same = bool(torch.equal(pooled, hold["pooled_vis"]))
        print(f"kernels: 10 rounds done; pooled rows of vision_pool_kernel bit-equal to embed_visual_kernel's: {same}", flush=True)
        return

    cfg = pkg.ModelConfig.base(EE_config=dict(VISION_EE))
    W = pkg.synth.make_weights(cfg, seed=41, head_gain=4.0)
    B, T = a.docs, a.text_len
    d = pkg.synth.make_documents(cfg, B, seed=42, text_len=T, min_words=3)
    t = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}

    if only & {"phase1", "phase1_trace"}:
        for nb in (256, 1024):
            eng = pkg.EarlyExitEngine(cfg, max_docs=nb, max_text_len=16, precision="split")
            eng.load_weights(W)
            px = t["pixel_values"].repeat((nb + B - 1) // B, 1, 1, 1)[:nb].contiguous()
            thr = np.full(eng.E + 1, 0.5)
            if "phase1_trace" in only:
                for _ in range(5):
                    eng.forward_vision(px, thresholds=thr)
                torch.cuda.synchronize()
                print(f"phase1_trace: 5 forward_vision calls of {nb} documents done", flush=True)
            else:
                ms = [events(lambda: eng.forward_vision(px, thresholds=thr), 20) for _ in range(3)]
                say(f"phase 1 throughput: forward_vision, LayoutLMv3-base, split precision, B = {nb}, {name}: " +
                    ", ".join(f"{m:.3f} ms = {nb / m * 1e3:.0f} docs/s" for m in ms) + " (three blocks of 20 calls, device events)")
            eng.close()

    if "seam" in only:
        eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision="split")
        eng.load_weights(W)
        crit = eng.forward(**t, dump_all=True, want_all=True).all_crit.cpu().numpy().astype(np.float64)
        text = {k: t[k] for k in ("input_ids", "attention_mask", "bbox")}
        px = t["pixel_values"]
        say(f"cost of the seam: LayoutLMv3-base exits {VISION_EE['exits']}, synthetic weights, {B} documents, T = {T}, split precision, {name}; every later "
            f"exit releases {a.release:.2f} of the documents that reach it; forward_vision_first (dict route) and forward alternate in one process, 6 rounds "
            f"of 5 calls each, host clock around a device synchronise")
        for share in (0.0, 0.25, 0.5, 0.9):
            thr, here = np.full(eng.E + 1, 0.5), np.ones(B, bool)
            for e in range(eng.E):
                s = np.sort(crit[e, here])
                k = int(round((share if e == 0 else a.release) * s.size))
                thr[e] = 2.0 if k <= 0 or s.size < 2 else (-1.0 if k >= s.size else 0.5 * (s[-k - 1] + s[-k]))
                here = here & ~(crit[e] > thr[e])
            one = eng.forward(**t, thresholds=thr)
            two = eng.forward_vision_first(px, text, thresholds=thr)
            same = all(bool(torch.equal(getattr(one, f), getattr(two, f))) for f in ("logits", "exit_layer", "confidence"))
            res = {"vf": [], "one": []}
            for _ in range(6):
                res["vf"] += [wall(lambda: eng.forward_vision_first(px, text, thresholds=thr)) for _ in range(5)]
                res["one"] += [wall(lambda: eng.forward(**t, thresholds=thr)) for _ in range(5)]
            p1 = [wall(lambda: eng.forward_vision(px, thresholds=thr)) for _ in range(10)]
            m = two.text_docs
            say(f"  {100 * share:3.0f} % leave at exit 0 ({B - m} documents; {m} run with text; bits equal to forward: {same})")
            say(f"      forward_vision_first: {stats(res['vf'])}")
            say(f"      forward             : {stats(res['one'])}")
            say(f"      difference of the means {np.mean(res['vf']) - np.mean(res['one']):+.3f} ms; phase 1 alone {stats(p1)}")
        # the gather alone: all B rows of the four arrays, as the 0 % row gathers them
        slots, count = torch.arange(B, dtype=torch.int32, device="cuda"), torch.tensor([B], dtype=torch.int32, device="cuda")
        src = dict(text, pixel_values=px)
        dst = {k: torch.empty_like(v) for k, v in src.items()}
        descs = (pkg.capi.CascadeDesc * pkg.capi.CASCADE_MAX_ARRAYS)()
        for i, (k, v) in enumerate(src.items()):
            descs[i].src, descs[i].dst, descs[i].row_bytes = v.data_ptr(), dst[k].data_ptr(), (v.numel() // B) * v.element_size()
        ms = events(lambda: pkg.capi.check(lib.ee_cascade_gather(descs, len(src), ptr(slots), ptr(count), B, stream()), None, "ee_cascade_gather"), 20)
        say(f"  the gather alone, all {B} rows of input_ids / attention_mask / bbox / pixel_values: {ms:.3f} ms (device events, 20 calls)")
        eng.close()
    finish()


if __name__ == "__main__":
    main()
