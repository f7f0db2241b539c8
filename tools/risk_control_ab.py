"""Measurements of risk control (ee_risk_control / ee_binomial_bounds, risk.py) at the large model's shape (GPU box).

E1 = 24 exits, N = 40 000 documents, the synthetic confidence table of tests/test_gpu_risk.py at that size (agreement by confidence, the
final row all 1); V = 101 shared thresholds and V = 4096 random threshold vectors sorted by their mean; the unit cost (the exit index) and a
per-document cost table.  The tables are on the device before any clock starts.  One process:

  (a) time: ``risk_control`` end to end (results on the host), every block ending in a device synchronise, host clock; alternating with the
      same computation on the host -- the table downloaded, exits by numpy, p-values by scipy.stats.binom.cdf -- whose download is timed apart.
  (b) one ``binomial_bounds`` call at Q = 24, n = 40 000, against scipy.stats.beta.ppf on the host.
  (c) accuracy: the restatement (tests/risk_ref.py) and the device against scipy over the cases of tests/test_host_risk.py /
      tests/test_gpu_risk.py: the two measured deviations the tests' bar is made of.

    python tools/risk_control_ab.py [--out FILE] [--rounds R]          the table (also printed)
    python tools/risk_control_ab.py --trace R                          R calls at V = 4096 and R at V = 101, unit cost, and R binomial_bounds
                                                                       calls, device-resident inputs and nothing else: the program of
                                                                       ``rocprofv3 --kernel-trace --output-format csv`` (no counters in that run)
    python tools/risk_control_ab.py --summarise CSV [--out FILE]       per kernel of that trace: calls, median, min, max microseconds
                                                                       (appended to FILE)
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

E1, N = 24, 40000
ALPHA, DELTA = 0.1, 0.05


def table(seed=5):
    import numpy as np
    rng = np.random.default_rng(seed)
    conf = rng.beta(2.0 + np.arange(E1)[:, None] * 1.5, 2.0, (E1, N))
    agree = (rng.random((E1, N)) < np.clip(0.35 + 0.6 * conf, 0.0, 1.0)).astype(np.uint8)
    agree[E1 - 1] = 1
    return conf, agree


def candidates(V, seed=9):
    import numpy as np
    if V == 101:
        return np.ascontiguousarray(np.broadcast_to(np.linspace(1.0, 0.0, V)[:, None], (V, E1)))
    thr = np.random.default_rng(seed).random((V, E1))
    return np.ascontiguousarray(thr[np.argsort(-thr.mean(1), kind="stable")])      # most conservative first, roughly


def host_route(conf, agree, cost, thr):
    """The same integers, p-values and selection with numpy and scipy (fixed sequence, binomial bound)."""
    import numpy as np
    from scipy import stats
    cols = np.arange(conf.shape[1])
    wrong = 1 - agree.astype(np.int64)
    loss_sum, cost_sum = np.empty(len(thr), dtype=np.int64), np.empty(len(thr), dtype=np.int64)
    for v, th in enumerate(thr):
        fired = conf[:-1] > th[:-1, None]
        ex = np.where(fired.any(0), fired.argmax(0), conf.shape[0] - 1)
        loss_sum[v] = wrong[ex, cols].sum()
        cost_sum[v] = ex.sum() if cost is None else cost[ex, cols].sum()
    p = stats.binom.cdf(loss_sum, conf.shape[1], ALPHA)
    ok = np.cumprod(p <= DELTA).astype(bool)
    sel = int(np.flatnonzero(ok)[np.argmin(cost_sum[ok], axis=0)]) if ok.any() else -1
    return loss_sum, cost_sum, p, sel


def summarise(path, out):
    import numpy as np
    rows = [r for r in csv.DictReader(open(path)) if re.search(r"risk_|binomial_bounds", r["Kernel_Name"])]
    acc = collections.defaultdict(list)
    for r in rows:
        name = re.sub(r"^(void )?(\(anonymous namespace\)::)?", "", r["Kernel_Name"]).split("(")[0]
        acc[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    lines = ["kernel trace of risk_control calls (V = 4096 and V = 101, unit cost) and binomial_bounds calls (Q = 24, n = 40 000), microseconds "
             "per launch; risk_count_kernel's two populations are the two V",
             f"{'kernel':<34} {'calls':>6} {'median':>10} {'min':>10} {'max':>10}"]
    for name, ts in sorted(acc.items(), key=lambda kv: -float(np.sum(kv[1]))):
        lines.append(f"{name:<34} {len(ts):>6} {float(np.median(ts)):>10.1f} {min(ts):>10.1f} {max(ts):>10.1f}")
    print("\n".join(lines))
    if out:
        with open(out, "a") as f:
            f.write("\n" + "\n".join(lines) + "\n")


def accuracy(pkg, say):
    """(c): both deviations from scipy over the tests' cases."""
    import numpy as np
    from scipy import stats
    from tests import risk_ref as R
    from tests.test_host_risk import BOUND_CASES, CDF_ALPHA, CDF_N
    worst_ref = worst_dev = 0.0
    for n in CDF_N:
        conf = np.linspace(0.0, 1.0, n + 2)[1:-1][None, :].repeat(2, 0)            # under threshold t exactly #{conf > t} documents leave at exit 0
        correct = np.stack([np.zeros(n, dtype=np.uint8), np.ones(n, dtype=np.uint8)])       # ... each with loss 1: every k = 0 .. n is some vector's count
        lam = np.concatenate([[1.0], (conf[0, ::-1] + np.concatenate([conf[0, ::-1][1:], [0.0]])) / 2])
        for alpha in CDF_ALPHA:
            S = stats.binom.cdf(np.arange(n + 1), n, alpha)
            F = R.binom_cdf_table(n, alpha)
            big = S >= 1e-280
            worst_ref = max(worst_ref, float((np.abs(F[big] - S[big]) / S[big]).max()))
            res = pkg.risk.risk_control((conf, correct), alpha=alpha, delta=DELTA, lambdas=lam)
            k = (res.loss_sum >> 30).astype(np.int64)
            assert sorted(k.tolist()) == list(range(n + 1))
            want = S[k]
            big = want >= 1e-280
            worst_dev = max(worst_dev, float((np.abs(res.pvalue[big] - want[big]) / want[big]).max()))
    say(f"binomial p-values against scipy.stats.binom.cdf where it is >= 1e-280, every k = 0 .. n, n in {CDF_N}, alpha in {CDF_ALPHA}:")
    say(f"  restatement (math.lgamma, numpy cumsum)  max relative deviation {worst_ref:.3e}")
    say(f"  device (risk_cdf_kernel)                 max relative deviation {worst_dev:.3e}")
    n, k = np.array([c[0] for c in BOUND_CASES]), np.array([c[1] for c in BOUND_CASES])
    up, low = pkg.risk.binomial_bounds(n, k, DELTA)
    ref_abs = dev_abs = 0.0
    for i, (ni, ki) in enumerate(BOUND_CASES):
        su = 1.0 if ki == ni else float(stats.beta.ppf(1 - DELTA, ki + 1, ni - ki))
        sl = 0.0 if ki == 0 else float(stats.beta.ppf(DELTA, ki, ni - ki + 1))
        ru, rl = R.bounds(ni, ki, DELTA)
        ref_abs = max(ref_abs, abs(ru - su), abs(rl - sl))
        dev_abs = max(dev_abs, abs(up[i] - su), abs(low[i] - sl))
    say(f"Clopper-Pearson bounds at delta = {DELTA} against scipy.stats.beta.ppf, (n, k) in {BOUND_CASES}:")
    say(f"  restatement  max absolute deviation {ref_abs:.3e}")
    say(f"  device       max absolute deviation {dev_abs:.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--summarise", default=None)
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.out)
        return
    import numpy as np
    import torch
    from scipy import stats
    pkg = importlib.import_module("multi-modal-early-exit_amd")
    risk = pkg.risk
    conf_h, agree_h = table()
    conf, agree = torch.from_numpy(conf_h).cuda(), torch.from_numpy(agree_h).cuda()
    doc_cost_h = (np.arange(1, E1 + 1)[:, None] * np.random.default_rng(2024).integers(18, 513, N)[None, :]).astype(np.int64)
    doc_cost = torch.from_numpy(doc_cost_h).cuda()
    sync = torch.cuda.synchronize
    sync()
    qn, qk = np.full(24, N), np.linspace(0, N // 10, 24).astype(np.int64)

    if a.trace:
        for V in (4096, 101):
            thr = candidates(V)
            for _ in range(a.trace):
                risk.risk_control((conf, agree), alpha=ALPHA, delta=DELTA, thresholds=thr)
                sync()
        for _ in range(a.trace):
            risk.binomial_bounds(qn, qk, DELTA)
            sync()
        return

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(f):
        sync()
        t0 = time.perf_counter()
        out = f()
        sync()
        return 1e3 * (time.perf_counter() - t0), out

    fmt = lambda xs: " ".join(f"{x:.2f}" for x in xs)
    say(f"risk control: E1 = {E1}, N = {N}, alpha = {ALPHA}, delta = {DELTA}, fixed sequence, binomial bound; {torch.cuda.get_device_name(0)}")
    say()
    say("(a) ms per call.  device: risk_control end to end, results on the host.  host: the table already downloaded, exits by numpy, p-values by "
        "scipy; its download apart")
    t_dl = [timed(lambda: (conf.cpu().numpy(), agree.cpu().numpy(), doc_cost.cpu().numpy()))[0] for _ in range(a.rounds)]
    say(f"download of conf, agree and the cost table ({(conf_h.nbytes + agree_h.nbytes + doc_cost_h.nbytes) / 1e6:.1f} MB): {fmt(t_dl)}   median {np.median(t_dl):.2f}")
    for V in (101, 4096):
        thr = candidates(V)
        for cname, c_dev, c_host in (("unit", None, None), ("per-document", doc_cost, doc_cost_h)):
            f_dev = lambda: risk.risk_control((conf, agree), alpha=ALPHA, delta=DELTA, thresholds=thr, cost=c_dev)
            res = f_dev()                                            # warm-up
            host_rounds = a.rounds if V == 101 else 1
            td, th = [], []
            for i in range(a.rounds):
                td.append(timed(f_dev)[0])
                if i < host_rounds:
                    t0 = time.perf_counter()
                    ref = host_route(conf_h, agree_h, c_host, thr)
                    th.append(1e3 * (time.perf_counter() - t0))
            same = bool(np.array_equal(res.loss_sum >> 30, ref[0]) and np.array_equal(res.cost_sum.astype(np.int64), ref[1]) and res.selected == ref[3])
            say(f"V = {V:<4} cost = {cname:<12}: device {fmt(td)}   median {np.median(td):.2f}  spread {max(td) - min(td):.2f};  host {fmt(th)}   median "
                f"{np.median(th):.1f};  host / device = {np.median(th) / np.median(td):.0f};  certified {res.n_certified}, selected {res.selected}, "
                f"same integers and selection: {same}")
    say()
    say("(b) binomial_bounds, Q = 24 queries at n = 40 000 (k = 0 .. 4000), both bounds, ms per call")
    risk.binomial_bounds(qn, qk, DELTA)
    tb = [timed(lambda: risk.binomial_bounds(qn, qk, DELTA))[0] for _ in range(a.rounds)]
    t0 = time.perf_counter()
    stats.beta.ppf(1 - DELTA, qk + 1, qn - qk), stats.beta.ppf(DELTA, np.maximum(qk, 1), qn - qk + 1)
    say(f"device {fmt(tb)}   median {np.median(tb):.2f};  scipy.stats.beta.ppf on the host {1e3 * (time.perf_counter() - t0):.2f}")
    say()
    say("(c) accuracy")
    accuracy(pkg, say)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
