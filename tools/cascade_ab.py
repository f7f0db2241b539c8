"""What a model cascade (include/mmee.h, behind MMEE_QUOTA_*; CascadeEngine) costs and buys (GPU box).  No pass bar; the output is what README,
DESIGN and profiles/cascade.txt quote.  TIME ONLY: no trained checkpoint exists here, and on synthetic weights a large model is not more
accurate than a small one, so accuracy is not measured.

  seam      LayoutLMv3-base (default exits) -> LayoutLMv3-large (default exits), synthetic weights, split precision: one CascadeEngine.forward
            against the composition by hand (forward, download of confidence and exit_layer, host decision, torch.index_select per input,
            second forward, index scatter), alternated in one process.  Inside each model every exit releases --release of the documents
            that reach it; the deferral threshold sits where --defer of the call's documents are deferred.
  trace     the same cascade forward a few times and nothing else, for a kernel trace collected in a run of its own.
  gather    ee_cascade_gather alone on base-model pixel rows (602 112 bytes each), 64 and 256 deferred rows out of 512, against
            torch.index_select on the same tensors in the same process: achieved bytes per second, read plus write.
  buys      ms per call of the base model alone, the large model alone, and the cascade at 10 / 25 / 50 % deferred.

    python tools/cascade_ab.py [--out FILE] [--only seam,gather,buys] [--docs 256] [--text-len 512] [--release 0.1] [--defer 0.25] [--reps 5]
"""
import argparse
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def release_thresholds(np, table, release):
    """Per-exit thresholds on a max-softmax table (E+1,B) that release `release` of the documents still there; the documents at the final exit."""
    E1, B = table.shape
    thr, here = np.full(E1, 0.5), np.ones(B, bool)
    for e in range(E1 - 1):
        s = np.sort(table[e, here])
        k = max(1, int(round(release * s.size)))
        if s.size < 2 or k >= s.size:
            thr[e] = 2.0
            continue
        thr[e] = 0.5 * (s[-k - 1] + s[-k])
        here = here & ~(table[e] > thr[e])
    return thr, here


def defer_threshold(np, final_crit, at_final, share, B):
    """The final threshold under which `share` of the call's B documents are deferred: the midpoint below the k-th lowest criterion at the final exit."""
    s = np.sort(final_crit[at_final])
    k = min(int(round(share * B)), s.size)
    if k <= 0:
        return -1.0, 0
    return (2.0 if k == s.size else 0.5 * (s[k - 1] + s[k])), k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--only", default="seam,gather,buys")
    ap.add_argument("--docs", type=int, default=256)
    ap.add_argument("--text-len", type=int, default=512)
    ap.add_argument("--release", type=float, default=0.1)
    ap.add_argument("--defer", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    only = set(a.only.split(","))
    import numpy as np
    import torch
    pkg = importlib.import_module("multi-modal-early-exit_amd")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def wall(fn, reps):
        """Host clock around work that ends in a device synchronise (the cascade synchronises inside: events alone would not see the host part)."""
        ms = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        return ms

    def stats(ms):
        ms = np.asarray(ms)
        return f"{np.median(ms):.3f} ms (median of {ms.size}; min {ms.min():.3f}, max {ms.max():.3f}, std {ms.std():.3f})"

    name = torch.cuda.get_device_name(0)
    B, T = a.docs, a.text_len

    if only & {"seam", "trace", "buys"}:
        cb, cl = pkg.ModelConfig.base(), pkg.ModelConfig.large()
        base = pkg.EarlyExitEngine(cb, max_docs=B, max_text_len=T, precision="split")
        base.load_weights(pkg.synth.make_weights(cb, seed=41, head_gain=4.0))
        large = pkg.EarlyExitEngine(cl, max_docs=B, max_text_len=T, precision="split")
        large.load_weights(pkg.synth.make_weights(cl, seed=43, head_gain=4.0))
        d = pkg.synth.make_documents(cb, B, seed=42, text_len=T, min_words=3)
        t = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}
        casc = pkg.CascadeEngine([base, large])
        Eb, El = base.E, large.E
        tb = base.forward(**t, dump_all=True, want_all=True).all_crit.cpu().numpy().astype(np.float64)
        tl = large.forward(**t, dump_all=True, want_all=True).all_crit.cpu().numpy().astype(np.float64)
        thr_b, at_final = release_thresholds(np, tb, a.release)
        thr_l, _ = release_thresholds(np, tl, a.release)
        head = (f"LayoutLMv3-base exits {cb.exit_config.exits} (E = {Eb}) -> LayoutLMv3-large (E = {El}), synthetic weights, {B} documents, T = {T}, precision "
                f"split, {name}; inside each model every exit releases {a.release:.2f} of the documents that reach it ({int(at_final.sum())} of {B} reach the "
                f"base model's final exit)")

        def with_share(share):
            thr = thr_b.copy()
            thr[-1], k = defer_threshold(np, tb[-1], at_final, share, B)
            return thr, k

        def hand(thr):
            o = base.forward(**t, thresholds=thr)
            conf, ex = o.confidence.cpu().numpy(), o.exit_layer.cpu().numpy()                 # the download
            sel = np.nonzero((ex == Eb) & ~(conf > np.float32(thr[-1])))[0]                   # the host decision, on the float32 the forward reports
            if sel.size == 0:
                return o, 0
            idx = torch.from_numpy(sel).cuda()
            o2 = large.forward(**{k: torch.index_select(v, 0, idx) for k, v in t.items()}, thresholds=thr_l)
            o.logits.index_copy_(0, idx, o2.logits)
            o.exit_layer.index_copy_(0, idx, o2.exit_layer + (Eb + 1))
            o.confidence.index_copy_(0, idx, o2.confidence)
            return o, int(sel.size)

        if "trace" in only:
            thr, k = with_share(a.defer)
            for _ in range(3):
                casc.forward(t, thresholds=[thr, thr_l])
            torch.cuda.synchronize()
            print(f"trace: 3 cascade forwards done, {k} documents deferred", flush=True)
        if "seam" in only:
            thr, k = with_share(a.defer)
            say("cost of the seam: " + head + f"; deferral threshold at {a.defer:.2f} of the call ({k} documents)")
            res = {"cascade": [], "hand": []}
            got = casc.forward(t, thresholds=[thr, thr_l])
            oh, nh = hand(thr)
            same = bool(torch.equal(got.exit_layer, oh.exit_layer))
            for rnd in range(5):                                                               # alternated in one process
                res["cascade"] += wall(lambda: casc.forward(t, thresholds=[thr, thr_l]), a.reps)
                res["hand"] += wall(lambda: hand(thr), a.reps)
            say(f"  CascadeEngine.forward: {stats(res['cascade'])}; stage_docs {got.stage_docs}")
            say(f"  by hand              : {stats(res['hand'])}; {nh} documents to the second model; exit indices equal to the cascade's: {same}")
            dlt = np.median(res["cascade"]) - np.median(res["hand"])
            say(f"  cascade - by hand: {dlt:+.3f} ms per call ({100 * dlt / np.median(res['hand']):+.2f} %); the hand composition's own spread (max - min over "
                f"its {len(res['hand'])} calls in 5 alternated rounds): {max(res['hand']) - min(res['hand']):.3f} ms")
        if "buys" in only:
            say("what the cascade buys, TIME ONLY (accuracy is not measured: no trained checkpoint exists here, and on synthetic weights a large model "
                "is not more accurate than a small one): " + head)
            for _ in range(2):
                base.forward(**t, thresholds=thr_b)
                large.forward(**t, thresholds=thr_l)
            say(f"  base alone : {stats(wall(lambda: base.forward(**t, thresholds=thr_b), 3 * a.reps))}")
            say(f"  large alone: {stats(wall(lambda: large.forward(**t, thresholds=thr_l), 3 * a.reps))}")
            for share in (0.10, 0.25, 0.50):
                thr, k = with_share(share)
                out = casc.forward(t, thresholds=[thr, thr_l])
                say(f"  cascade, {100 * share:.0f} % deferred ({k} documents; stage_docs {out.stage_docs}): "
                    f"{stats(wall(lambda: casc.forward(t, thresholds=[thr, thr_l]), 3 * a.reps))}")
        base.close()
        large.close()
        del t

    if "gather" in only:
        import ctypes as C
        lib = pkg.capi.load()
        R, rows = 512, 3 * 224 * 224
        px = torch.randn((R, rows), dtype=torch.float32, device="cuda")
        rb = rows * 4
        say(f"the gather alone: pixel rows of a base model ({rb} bytes), {R} source rows ({R * rb / 1e6:.0f} MB), deferred rows ascending random slots, "
            f"device events around 20 calls after 3 warm-up calls, {name}; bytes = 2 x rows x row bytes (read plus write); for scale, not as a bar: README "
            f"reports 5.4-5.7 TB/s for ln_rows_kernel")
        rng = np.random.default_rng(3)
        for m in (64, 256):
            idx = torch.from_numpy(np.sort(rng.choice(R, m, replace=False))).cuda()
            slots, count = idx.to(torch.int32), torch.tensor([m], dtype=torch.int32, device="cuda")
            dst, dst_t = torch.empty((m, rows), dtype=torch.float32, device="cuda"), torch.empty((m, rows), dtype=torch.float32, device="cuda")
            desc = (pkg.capi.CascadeDesc * 8)()
            desc[0].src, desc[0].dst, desc[0].row_bytes = px.data_ptr(), dst.data_ptr(), rb
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

            def ours():
                pkg.capi.check(lib.ee_cascade_gather(desc, 1, C.c_void_p(slots.data_ptr()), C.c_void_p(count.data_ptr()), m, stream), None, "ee_cascade_gather")

            def theirs():
                torch.index_select(px, 0, idx, out=dst_t)

            res = {}
            for label, fn in (("ee_cascade_gather", ours), ("torch.index_select(out=)", theirs), ("ee_cascade_gather again", ours)):
                for _ in range(3):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                res[label] = e0.elapsed_time(e1) / 20
            assert torch.equal(dst, dst_t)
            say(f"  {m:>3d} rows ({2 * m * rb / 1e6:.0f} MB moved): " + "; ".join(f"{k} {1e3 * v:.1f} us = {2 * m * rb / (v * 1e-3) / 1e12:.2f} TB/s" for k, v in res.items()))

    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
