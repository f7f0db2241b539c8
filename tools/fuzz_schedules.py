"""Randomised cross-check of the exit-layer schedules (GPU box only): for random shapes / exit sets / strategies / thresholds the
probe-first, whole-layer, default, pinned and cost-model-suggested schedules and the dump-all rows must agree bit for bit, and the X-space probe within tolerance.  Not a test (minutes); run after touching
the layer loop of csrc/capi_forward.hip:  python tools/fuzz_schedules.py [n_cases [seed [large|big]]].  Each case draws its label count from
{2, 10, 16, 64}."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("multi-modal-early-exit_amd")
_np = lambda t: t.detach().cpu().numpy()


def softmax64(x):
    x = x.astype(np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


BIG = False                # fourth argument "big": bench-sized cases (L = 12, H = 768, hundreds of ragged documents of up to 512 tokens)


def one(case, rng):
    L = 12 if BIG else int(rng.integers(2, 6))
    exits = sorted(rng.choice(np.arange(1, L + 1), size=int(rng.integers(1, L + 1)), replace=False).tolist())
    strat = ["ramp", "gate"][int(rng.integers(0, 2))]
    emb = [[], ["vision_avg"], ["text_avg", "text_visual_concat"]][int(rng.integers(0, 3))]
    ee = dict(exits=emb + exits, encoder_layer_strategy=strat)
    H = 768 if BIG else HS[int(rng.integers(0, len(HS)))]
    K = int(rng.choice([2, 10, 16, 64]))                                 # label count: the exit kernels index by K (ee_create takes 1..64)
    cs = {256: (40, 48), 768: (128, 128), 1024: (171, 170)}[H]           # 6 spatial slices: 4 coordinate + 2 shape sizes sum to H
    cfg = pkg.ModelConfig.base(EE_config=ee, num_hidden_layers=L, hidden_size=H, intermediate_size=4 * H if H >= 768 else 512,
                               num_attention_heads=H // 64, coordinate_size=cs[0], shape_size=cs[1], num_labels=K)
    B = int(rng.choice([100, 300, 512] if BIG else [1, 5, 33, 96]))
    T = 512 if BIG else int(rng.choice([16, 130, 512]))
    W = pkg.synth.make_weights(cfg, seed=int(rng.integers(1, 1 << 30)), head_gain=6.0)
    docs = pkg.synth.make_documents(cfg, B, seed=int(rng.integers(1, 1 << 30)), text_len=T, min_words=1)
    args = (docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"])
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision="split", xprobe=False)      # bit-identity between schedules is asserted; the X-space probe is asked for explicitly
    eng.load_weights(W)
    E1 = len(ee["exits"]) + 1
    temps = rng.uniform(0.5, 3.0, size=E1) if rng.integers(0, 2) else None
    dense = bool(rng.integers(0, 2))
    full = eng.forward(*args, dump_all=True, want_all=True, temperatures=temps, dense_rows=dense)
    store = _np(full.all_logits).astype(np.float64)
    conf = softmax64(store / (temps[:, None, None] if temps is not None else 1.0)).max(-1)
    thr = np.full(E1, 2.0)
    active = np.ones(B, dtype=bool)
    for e in range(E1 - 1):
        c = np.sort(conf[e, active])
        if len(c) < 2:
            continue
        j = int(rng.integers(1, len(c)))
        thr[e] = 0.5 * (c[j - 1] + c[j])
        if c[j] - c[j - 1] < 1e-6:
            thr[e] = 2.0
        active &= ~(conf[e] > thr[e])
    outs = []
    # round 5: the default schedule probes every decision layer and never changes by itself; mixed schedules exist as PINNED masks -- here a
    # random subset of the layers (outs[3]), then whatever the cost model suggests for the forward before it (outs[4]), then the default again
    pins = [None, None, None, sorted(rng.choice(np.arange(L), size=int(rng.integers(0, L + 1)), replace=False).tolist()), "suggest", False]
    for kw, pin in zip((dict(probe_always=True), dict(whole_layers=True), dict(), dict(), dict(), dict()), pins):
        if pin == "suggest":
            eng.pin_schedule(None)
        elif pin is not None:
            eng.pin_schedule(pin)
        o = eng.forward(*args, thresholds=thr, temperatures=temps, dense_rows=dense, **kw)
        eng.check()
        outs.append((_np(o.exit_layer), _np(o.logits), _np(o.confidence), eng.layer_plan()["docs_probe"]))
    ex = outs[0][0]
    want = _np(full.all_logits)[ex, np.arange(B)]
    ok = all(np.array_equal(o[0], ex) and np.array_equal(o[1], outs[0][1]) and np.array_equal(o[2], outs[0][2]) for o in outs)
    ok = ok and np.array_equal(outs[0][1], want)
    # the X-space probe (MMEE_FLAG_XPROBE; 12 heads x 768 only, other shapes ignore the flag): a re-association, so a tolerance -- same exits
    # unless a confidence sits within 1e-5 of its threshold, logits within 1e-4
    ox = eng.forward(*args, thresholds=thr, temperatures=temps, dense_rows=dense, probe_always=True, xprobe=True)
    eng.check()
    exx, lgx = _np(ox.exit_layer), _np(ox.logits)
    diff = exx != ex
    near = np.zeros(B, dtype=bool)
    for e in range(E1 - 1):
        near |= np.abs(conf[e] - thr[e]) < 1e-5
    xok = bool((~diff | near).all()) and float(np.abs(lgx[~diff] - outs[0][1][~diff]).max(initial=0.0)) <= 1e-4
    xrows = eng.layer_plan()["rows_qkv"]
    ok = ok and xok
    print(f"case {case}: L={L} H={H} K={K} exits={ee['exits']} {strat} B={B} T={T} dense={dense} temps={temps is not None} "
          f"left at {np.bincount(ex, minlength=E1).tolist()} probes {outs[0][3]} pinned {outs[3][3]} suggested {outs[4][3]} xprobe dlogit "
          f"{float(np.abs(lgx[~diff] - outs[0][1][~diff]).max(initial=0.0)):.1e} flips {int(diff.sum())} rows_qkv {xrows}: {'ok' if ok else 'MISMATCH'}", flush=True)
    eng.close()
    return ok


HS = [256, 768]            # third argument "large": also LayoutLMv3-large rows (H = 1024, 16 heads: the X-space probe falls back to K | V)

if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[3] == "large":
        HS = [256, 768, 1024]
    if len(sys.argv) > 3 and sys.argv[3] == "big":
        BIG = True
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 2026)
    bad = sum(not one(i, rng) for i in range(n))
    print("mismatches:", bad)
    sys.exit(1 if bad else 0)
