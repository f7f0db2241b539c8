"""numpy float64 restatement of the exit stage (csrc/exit_stage.hip): the exit heads' output projection with the LTE score, ONE exit decision of
ONE stage with its stream compaction, the row-map expansion and the CLS / padded hidden-state outputs.  The oracle of
tests/test_host_exit_stage_ref.py and tests/test_gpu_exit_stage.py, written from the semantics include/mmee.h and the comments of exit_stage.hip
state (and, for the policies, from the whole-store restatements csf_ref / patience_ref / rule_ref / lte_ref it must chain up to), not from the
kernels' loops: nothing here walks documents in waves or chunks -- the next stage is "the survivors in their order, their lengths scanned".

``mut`` names ONE deliberate fault of a subtly wrong kernel; tests/test_host_exit_stage_ref.py shows that the inputs built below, which are the
GPU test's own, see each of them: an integer output differs, or a float output moves by at least ten times its tolerance.

Also here, so that both tests build the same inputs: the stages, the logits that force a leave pattern, the decision edges and the chained
store."""
import math

import numpy as np

from . import csf_ref
from .hook_util import SENTINEL
from .rule_ref import EITHER, PLAIN, STREAK

F32, F64 = np.float32, np.float64
THRESHOLD, PATIENCE, LTE = 0, 1, 2                                       # ee_debug_exit_decide's mode
KERNELS = [(THRESHOLD, PLAIN), (THRESHOLD, STREAK), (THRESHOLD, EITHER), (PATIENCE, PLAIN), (LTE, PLAIN), (LTE, STREAK), (LTE, EITHER)]
KERNEL_IDS = ["threshold", "threshold_streak", "threshold_either", "patience", "lte", "lte_streak", "lte_either"]
CRIT_CODE = {"max_confidence": 0, "entropy": 1, "margin": 3}             # MMEE_CRIT_*
DIRTY = np.int32(np.uint32(0xA5A5A5A5).astype(np.int64) - (1 << 32))     # what a state array holds before exit 0 writes it
MIN_GAP = 1e-5                                                           # as tests/test_gpu_margin.py: >> 2^-23, the rounding of a stored criterion <= 1
MUTATIONS = ("ge", "carry_dropped", "wave_inclusive", "off_all_lengths", "sumsq_32", "margin_skip_all_max", "argmax_last", "argmax_unscaled",
             "streak_no_reset", "state_dense", "state_read_exit0", "meta_from_xphys", "lte_le", "head_tail_dropped", "gather_ignored",
             "text_dst_copied")


def tolerance(err32):
    """The project's rule for a float32 path: 2 x the error of the same operation in float32, floored at 1e-6."""
    return np.maximum(2.0 * np.asarray(err32, F64), 1e-6)


# ---------------------------------------------------------------------------------------------------------------------------------------
# head_out
# ---------------------------------------------------------------------------------------------------------------------------------------
def _head_rows(x, H, gather, mut):
    rows = np.asarray(x)[:, :H]
    if gather is not None and mut != "gather_ignored":
        rows = rows[np.asarray(gather)]
    elif gather is not None:
        rows = rows[:len(gather)]
    if mut == "head_tail_dropped":                                       # the columns of the last group of 256 are never added
        rows = rows.copy()
        rows[:, 256 * ((H - 1) // 256):] = 0
    return rows


def head_out_ref(x, W, b, gather=None, n=None, mut=""):
    """x (rows, ld >= H) f32, W (Ko, H), b (Ko,): float64 x[gather[i]] . W[o] + b[o] for the first n documents."""
    H = W.shape[1]
    rows = _head_rows(x, H, gather, mut).astype(F64)
    n = len(rows) if n is None else n
    return rows[:n] @ W.astype(F64).T + b.astype(F64)


def head_out_f32(x, W, b, gather=None, n=None):
    """The same in torch float32 on the CPU: the yardstick."""
    import torch
    H = W.shape[1]
    rows = np.ascontiguousarray(_head_rows(x, H, gather, ""), dtype=F32)
    n = len(rows) if n is None else n
    y = torch.from_numpy(rows[:n]) @ torch.from_numpy(np.ascontiguousarray(W)).T + torch.from_numpy(np.ascontiguousarray(b))
    assert y.dtype == torch.float32
    return y.numpy()


HEAD_H = (128, 256, 384, 512, 640, 768, 896, 1024)
HEAD_KO = (1, 2, 16, 17)
HEAD_N = (1, 4, 5, 257)                                                  # one wave, a full block, a block plus one, many blocks
LTE_SPLIT_SCALE = 16.0


def grid_rows(rows, cols, seed=0, lim=3.9):
    """f32 values k 2^-14 with 0 < |x| < lim: split planes of scale 16 hold them exactly (11 bits in the hi plane, the rest in the lo plane)."""
    rng = np.random.default_rng(300 + seed)
    k = rng.integers(1, int(lim * 2 ** 14), (rows, cols)) * rng.choice([-1, 1], (rows, cols))
    return (k * 2.0 ** -14).astype(F32)


def head_cases(H, lte):
    """The head_out cases of one hidden size: every document count, with Ko, the gather and the row stride cycled against them.  lte: 0 no
    score, 1 f32 rows, 2 rows that split planes hold exactly; the score's row map differs from the projection's."""
    hi = HEAD_H.index(H)
    out = []
    for j, n in enumerate(HEAD_N):
        rng = np.random.default_rng(H * 10 + n + lte)
        Ko, ld, in_rows = HEAD_KO[(j + hi) % 4], H + 8 * ((j + hi // 2) % 2), n + 3
        c = dict(H=H, n=n, Ko=Ko, ld=ld, in_rows=in_rows, max_docs=300 if n == 257 else n, gather=None, lte_gather=None,
                 x=rng.standard_normal((in_rows, ld)).astype(F32), W=(rng.standard_normal((Ko, H)) / np.sqrt(H)).astype(F32),
                 b=rng.standard_normal(Ko).astype(F32))
        if (j + hi + lte) % 2 == 0:                                      # a map with repeats that never names the document's own row
            c["gather"] = (np.arange(n) + 1 + rng.integers(0, in_rows - 1, n)) % in_rows
        if lte:
            c.update(lte_rows=n + 2, lte_ld=H + 8 * ((j + hi // 2 + 1) % 2), lte_w=(rng.standard_normal(H) / np.sqrt(H)).astype(F32),
                     lte_b=np.array([0.125], F32))
            c["lte_x"] = rng.standard_normal((n + 2, c["lte_ld"])).astype(F32) if lte == 1 else grid_rows(n + 2, c["lte_ld"], seed=H + n)
            if c["gather"] is not None or j % 2:
                g = (np.arange(n) + 1 + rng.integers(0, n + 1, n)) % (n + 2)
                c["lte_gather"] = np.where(c["gather"] == g, (g + 1) % (n + 2), g) if c["gather"] is not None else g
        out.append(c)
    return out


def lte_score_ref(x, w, b, gather=None, n=None, mut=""):
    """sigmoid(w . x[gather[i]] + b) with the dot exact (a product of two float32 is exact in float64; math.fsum adds them exactly), and the
    distance dt of the plain float64 np.dot from the exact dot, per row: (scores (n,), dt (n,))."""
    H = len(w)
    rows = _head_rows(x, H, gather, mut).astype(F64)
    n = len(rows) if n is None else n
    w64, b64 = np.asarray(w, F32).astype(F64), float(np.asarray(b, F32).reshape(-1)[0])
    exact = np.array([math.fsum(rows[i] * w64) for i in range(n)], F64).reshape(n)
    plain = np.array([np.dot(rows[i], w64) for i in range(n)], F64).reshape(n)
    return 1.0 / (1.0 + np.exp(-(exact + b64))), np.abs(plain - exact)


# ---------------------------------------------------------------------------------------------------------------------------------------
# criteria
# ---------------------------------------------------------------------------------------------------------------------------------------
def criterion64(x, criterion, mut=""):
    """csf_ref's criterion of float64 rows x (n, K)."""
    with np.errstate(invalid="ignore", over="ignore"):
        if criterion == "margin" and mut == "margin_skip_all_max":       # the second value skips EVERY label that holds the maximum
            m1 = x.max(-1, keepdims=True)
            rest = np.where(x == m1, -np.inf, x).max(-1)
            S = csf_ref._sum_in_label_order(np.exp(x - m1))
            return (1.0 - np.exp(rest - m1[..., 0])) / S
        return csf_ref.csf(x, criterion)


def crit_f32(z, criterion):
    """The criterion as the model computes it on an exit head's raw logits, every operation in float32: the yardstick of out_head_crit."""
    z = np.asarray(z, F32)

    def total(terms):
        s = np.zeros(terms.shape[:-1], F32)
        for k in range(terms.shape[-1]):
            s = (s + terms[..., k]).astype(F32)
        return s

    with np.errstate(invalid="ignore", over="ignore"):
        if criterion == "entropy":
            e = np.exp(z)
            A, B = total(e), total(z * e)
            return (np.log(A) - B / A).astype(F32)
        m = z.max(-1)
        s = total(np.exp(z - m[..., None]))
        if criterion == "max_confidence":
            return (F32(1) / s).astype(F32)
        srt = np.sort(z, -1)
        second = np.exp(srt[..., -2] - m) if z.shape[-1] > 1 else np.zeros_like(m)
        return ((F32(1) - second) / s).astype(F32)


def argmax_first(v, mut=""):
    if mut == "argmax_last":
        return v.shape[-1] - 1 - np.argmax(v[..., ::-1], -1)
    return np.argmax(v, -1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# one exit of one stage
# ---------------------------------------------------------------------------------------------------------------------------------------
def make_stage(n, B, seed=0, lens=None):
    """n documents in B > n original slots: doc_orig a random injection, ragged lengths 1..40 (or `lens`), the rows of X in another order than
    the dense one and with holes, so that x_phys differs from doc_off everywhere but by chance."""
    rng = np.random.default_rng(1000 + seed)
    assert B > n
    lens = rng.integers(1, 41, n) if lens is None else np.asarray(lens)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    order = rng.permutation(n)
    phys = np.zeros(n, np.int64)
    phys[order] = np.concatenate([[0], np.cumsum(lens[order] + 3)])[:n] + 5
    return dict(n=n, doc_orig=rng.permutation(B)[:n].astype(np.int64), doc_off=off, x_phys=phys, n_rows=int(off[-1]),
                sum_len_sq=int((lens.astype(object) ** 2).sum()) if n else 0)


def _next_stage(stage, keep, mut):
    """The stage of the documents that stay: in their order, new dense offsets = the exclusive scan of THEIR lengths and the total behind it,
    n_x_src = x_phys, n_meta_src = the old dense offset.  Arrays of n + 72 entries, SENTINEL where nothing is written."""
    n = stage["n"]
    lens = np.diff(stage["doc_off"])
    keep = keep.astype(np.int64)
    klen = keep * lens
    k, off = np.cumsum(keep) - keep, np.cumsum(klen) - klen
    docs, rows = int(keep.sum()), int(klen.sum())
    idx = np.arange(n)
    if mut == "off_all_lengths":
        off, rows = stage["doc_off"][:-1].copy(), int(lens.sum())
    if mut == "carry_dropped" and n:                                     # every 1024 documents the count starts again
        start = (idx // 1024) * 1024
        docs, rows = docs - int(k[start[-1]]), rows - int(off[start[-1]])
        k, off = k - k[start], off - off[start]
    if mut == "wave_inclusive" and n:                                    # a document also counts the survivors of its own group of 64
        w = idx // 64
        k = k + np.bincount(w, keep)[w].astype(np.int64)
        off = off + np.bincount(w, klen)[w].astype(np.int64)
    out = {name: np.full(n + 72, SENTINEL, np.int64) for name in ("n_doc_orig", "n_doc_off", "n_x_src", "n_meta_src")}
    s = np.nonzero(keep)[0]
    out["n_doc_orig"][k[s]] = stage["doc_orig"][s]
    out["n_doc_off"][k[s]] = off[s]
    out["n_x_src"][k[s]] = stage["x_phys"][s]
    out["n_meta_src"][k[s]] = stage["x_phys"][s] if mut == "meta_from_xphys" else stage["doc_off"][s]
    out["n_doc_off"][docs] = rows
    sq = sum(int(l) ** 2 for l in lens[s])
    out.update(n=docs, n_rows=rows, sum_len_sq=sq & 0xFFFFFFFF if mut == "sumsq_32" else sq)
    return out


def as_stage(nxt):
    """The next stage of decide_ref as the stage of the following exit."""
    n = nxt["n"]
    return dict(n=n, doc_orig=nxt["n_doc_orig"][:n], doc_off=nxt["n_doc_off"][:n + 1], x_phys=nxt["n_x_src"][:n], n_rows=nxt["n_rows"],
                sum_len_sq=nxt["sum_len_sq"])


def decide_ref(stage, logits, *, mode, rule, criterion, thr, temp, patience, exit_index, B, state=None, head_logits=None, lte_score=None,
               is_final=False, no_exit=False, mut=""):
    """One exit of one stage.  logits (n, K) f32 by dense index; state (prev, run) int arrays [B] by ORIGINAL slot (None: dirty).
    Returns leave (n,), scaled32 (n, K) f32 = (float)((double)z / temp), crit (n,) float64 (what out_all_crit / out_conf carry), head_crit (n,)
    float64 or None, state (prev, run) after the exit, next = the stage of the stayers (_next_stage)."""
    n = stage["n"]
    orig = stage["doc_orig"]
    z = np.asarray(logits, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        x = csf_ref.scaled(z[None], [temp])[0]
        s32 = x.astype(F32)
        if mode == THRESHOLD:
            crit = criterion64(x, criterion, mut)
            if criterion == "entropy":
                event = crit <= thr if mut == "ge" else crit < thr
            else:
                event = crit >= thr if mut == "ge" else crit > thr
        elif mode == PATIENCE:
            crit, event = criterion64(x, "max_confidence"), None
        else:                                                            # an exit without a score: 1.0, nobody leaves
            crit = np.ones(n) if lte_score is None else np.asarray(lte_score, F64)
            event = np.zeros(n, bool) if lte_score is None else (crit <= thr if mut == "lte_le" else crit < thr)
    prev, run = (np.full(B, DIRTY, np.int64), np.full(B, DIRTY, np.int64)) if state is None else (state[0].astype(np.int64), state[1].astype(np.int64))
    slot = np.arange(n) if mut == "state_dense" else orig
    later = exit_index > 0 or mut == "state_read_exit0"
    if mode == PATIENCE or rule == EITHER:                               # PABEE's counter on the argmax of the scaled logits as written out
        am = argmax_first(z if mut == "argmax_unscaled" else s32, mut)
        c = np.where(prev[slot] == am, run[slot] + 1, 0) if later else np.zeros(n, np.int64)
        prev[slot], run[slot] = am, c
        agreed = c >= patience
        leave = agreed if mode == PATIENCE else event | agreed
    elif rule == STREAK:
        before = run[slot] if later else np.zeros(n, np.int64)
        s = np.where(event, before + 1, before if mut == "streak_no_reset" else 0)
        run[slot] = s
        leave = s >= patience
    else:
        leave = event
    if no_exit:
        leave = np.zeros(n, bool)
    if is_final:
        leave = np.ones(n, bool)
    head_crit = None
    if head_logits is not None:
        head_crit = criterion64(np.asarray(head_logits, F32).astype(F64), "max_confidence" if mode == PATIENCE else criterion)
    return dict(leave=leave, scaled32=s32, crit=crit, head_crit=head_crit, state=(prev, run), next=_next_stage(stage, ~leave, mut))


def compact_ref(nxt, meta_old, cap):
    """Row map and metadata of the next stage: new dense row off[k] + t <- physical row n_x_src[k] + t, metadata row n_meta_src[k] + t.
    (row_src (cap,), meta_new (cap, 4)), SENTINEL where nothing is written."""
    row_src, meta_new = np.full(cap, SENTINEL, np.int64), np.full((cap, 4), SENTINEL, np.int64)
    for k in range(nxt["n"]):
        o, ln = nxt["n_doc_off"][k], nxt["n_doc_off"][k + 1] - nxt["n_doc_off"][k]
        row_src[o:o + ln] = nxt["n_x_src"][k] + np.arange(ln)
        meta_new[o:o + ln] = meta_old[nxt["n_meta_src"][k]:nxt["n_meta_src"][k] + ln]
    return row_src, meta_new


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs that force a leave pattern through the logits (single-exit cases)
# ---------------------------------------------------------------------------------------------------------------------------------------
PATTERNS = ("nobody", "everybody", "lane63", "lane0", "alternating", "random", "waves_3_15", "first_chunk")
SINGLE_N = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)
SINGLE_EXIT = 2                                                          # the exit index of the single-exit cases: state is read
SINGLE_T = 2


def pattern_mask(pattern, n, seed=0):
    i = np.arange(n)
    rnd = np.random.default_rng(77 + seed).random(n) < 0.4
    return {"nobody": np.zeros(n, bool), "everybody": np.ones(n, bool), "lane63": i % 64 == 63, "lane0": i % 64 == 0, "alternating": i % 2 == 0,
            "random": rnd, "waves_3_15": np.isin((i % 1024) // 64, (3, 15)) | rnd, "first_chunk": (i < 1024) | rnd}[pattern]


def _peaked(rng, n, K, sharp):
    """(n, K) f32 logits: `sharp` rows hold one label 9 above the rest, the others are nearly flat."""
    z = rng.standard_normal((n, K)) * 0.2
    top = rng.integers(0, K, n)
    z[np.arange(n), top] += np.where(sharp, 9.0, 0.0) + rng.random(n) * 0.5
    return z.astype(F32)


def single_case(kernel, criterion, n, pattern, K, seed=0, head=False, lens=None, B=None):
    """Everything one ee_debug_exit_decide call takes, such that exactly the documents of `pattern` leave: sharp rows against flat ones with the
    threshold in the gap between the two groups' reference criteria (event), and state that agrees / has a streak for the leavers only.
    K = 1 cannot tell documents apart: the criterion is a constant, the event is all-or-nothing (the pattern's majority)."""
    mode, rule = kernel
    rng = np.random.default_rng(seed * 7919 + n * 31 + K)
    B = B or n + 37
    stage = make_stage(n, B, seed, lens)
    want = pattern_mask(pattern, n, seed)
    temp = (1.0, 3.0, 0.5)[seed % 3]
    if K == 1:
        want = np.full(n, bool(want.mean() > 0.5) if n else False)
    # under EITHER the event releases the even leavers and the agreement counter the odd ones
    by_event = want & (np.arange(n) % 2 == 0) if rule == EITHER and K > 1 else want
    by_agree = want & ~by_event if rule == EITHER and K > 1 else want
    z = _peaked(rng, n, K, by_event if mode == THRESHOLD else rng.random(n) < 0.5) * F32(temp)
    if K == 1 and criterion == "entropy" and mode == THRESHOLD:
        z[:] = 0                                                         # log(e^x) - x is 0 in exact arithmetic only: rounding noise of either side at x != 0
    x = csf_ref.scaled(z[None], [temp])[0]
    lte_score = None
    if mode == THRESHOLD:
        crit, sign = criterion64(x, criterion), csf_ref.SIGN[criterion]
    elif mode == LTE:
        lte_score = np.where(by_event, 0.05 + 0.3 * rng.random(n), 0.6 + 0.35 * rng.random(n))
        crit, sign = lte_score, -1
    thr, gap = 0.5, np.inf
    if mode != PATIENCE:
        v = sign * crit                                                  # fires on v > sign * thr
        lo = v[~by_event].max() if (~by_event).any() else (v.min() - 2e-3 if n else 0.0)
        hi = v[by_event].min() if by_event.any() else lo + 2e-3
        assert hi > lo, (kernel, criterion, pattern, n, K)
        thr, gap = sign * 0.5 * (lo + hi), (hi - lo) if n else np.inf
    # state by original slot: leavers agree with their previous argmax at run t - 1 (a streak of t - 1), the others do not; untouched slots dirty
    prev, run = np.full(B, DIRTY, np.int64), np.full(B, DIRTY, np.int64)
    am = argmax_first(x.astype(F32))
    o = stage["doc_orig"]
    if mode == PATIENCE or rule == EITHER:
        prev[o] = np.where(by_agree, am, (am + 1) % max(K, 2))
        run[o] = np.where(by_agree, SINGLE_T - 1, 5)
        if K == 1:
            prev[o], run[o] = (0, SINGLE_T - 1) if want.all() and n else (1, 5)
    elif rule == STREAK:
        run[o] = SINGLE_T - 1
    # gate-style head logits in [-1, 1]: the float32 entropy rounds log A and B / A at THEIR magnitude, whatever the entropy's; below 2 the
    # rule's floor of 1e-6 is eight float32 steps (at |z| ~ 6 it would be two, fewer than any float32 evaluation of the expression needs)
    head_logits = rng.uniform(-1.0, 1.0, (n, 2)).astype(F32) if head else None
    return dict(kernel=kernel, mode=mode, rule=rule, criterion=criterion, n=n, B=B, K=K, stage=stage, logits=z, head_logits=head_logits, lte_score=lte_score,
                thr=float(thr), temp=temp, patience=SINGLE_T, exit_index=SINGLE_EXIT, state=(prev, run), want=want, gap=float(gap))


def run_case(c, mut="", **over):
    kw = dict(mode=c["mode"], rule=c["rule"], criterion=c["criterion"], thr=c["thr"], temp=c["temp"], patience=c["patience"],
              exit_index=c["exit_index"], B=c["B"], state=c["state"], head_logits=c["head_logits"], lte_score=c["lte_score"], mut=mut)
    kw.update(over)
    return decide_ref(c["stage"], c["logits"], **kw)


def single_plan(n, kernel_index):
    """The (pattern, criterion, K, head) combinations the GPU test runs at stage size n for one kernel: every pattern, the criteria, K and the
    gate-style head cycled against them so that the whole matrix meets every value of each."""
    crits, Ks = list(csf_ref.CRITERIA), (2, 10, 17, 1)
    shift = SINGLE_N.index(n) + kernel_index
    return [(p, crits[(j + shift) % 3], Ks[(j + shift // 3) % 4], (j + shift) % 2 == 0) for j, p in enumerate(PATTERNS)]


def exit0_case(kernel):
    """Exit 0 on state that would release everybody if it were read: every document's previous argmax is its argmax, every run is 7."""
    c = single_case(kernel, "max_confidence", 65, "random", 10, seed=2)
    prev, run = c["state"]
    o = c["stage"]["doc_orig"]
    prev[o], run[o] = argmax_first(csf_ref.scaled(c["logits"][None], [c["temp"]])[0].astype(F32)), 7
    return dict(c, exit_index=0, want=None)


def big_case():
    """n = 2049, every document 1500 rows: sum_len_sq above 2^32 and 3.07 M rows; only lane 63 of every group of 64 leaves."""
    return single_case((THRESHOLD, PLAIN), "max_confidence", 2049, "lane63", 10, seed=5, lens=np.full(2049, 1500))


# ---------------------------------------------------------------------------------------------------------------------------------------
# decision edges: criteria that are exact in float64, thresholds equal to them and one step to either side
# ---------------------------------------------------------------------------------------------------------------------------------------
def collision_pair(temp=3.0):
    """Two float32 logits z0 < z1 with (float)(z0 / temp) == (float)(z1 / temp)."""
    for base in np.arange(1.0, 2.0, 1.0 / 64).astype(F32):
        z0 = F32(base)
        z1 = np.nextafter(z0, F32(np.inf))
        if F32(F64(z0) / temp) == F32(F64(z1) / temp):
            return z0, z1
    raise AssertionError("no colliding pair")


def edge_cases():
    """(name, mode, criterion, logits (1, K), lte_score or None, exact criterion, [(thr, fires)]) with the threshold AT the value and one float64
    step to either side."""
    inf = np.inf
    step = lambda v, fire_dir: [(v, False), (np.nextafter(v, fire_dir), True), (np.nextafter(v, -fire_dir), False)]
    out = []
    for crit, z, val in (("max_confidence", [0.7], 1.0), ("margin", [0.7], 1.0), ("entropy", [0.0], 0.0), ("max_confidence", [1.25, 1.25], 0.5),
                         ("margin", [1.25, 1.25], 0.0), ("margin", [-2.0, 0.5, 0.5], 0.0)):
        out.append((f"{crit}_K{len(z)}", THRESHOLD, crit, np.array([z], F32), None, val, step(val, inf if crit == "entropy" else -inf)))
    for score in (0.3, 0.7310585786300049, 1.0 / 3.0):
        out.append((f"lte_{score:.3f}", LTE, "max_confidence", np.array([[0.1, 0.2]], F32), np.array([score]), score, step(score, inf)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the chained store: E1 exits, the whole-store restatements' inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
CHAIN_N, CHAIN_B, CHAIN_E1, CHAIN_K, CHAIN_T = 1025, 1100, 5, 10, 2
CHAIN_TEMPS = np.array([1.0, 3.0, 0.5, 1.7, 1.0])
CHAIN_POSITION = {+1: 0.75, -1: 0.25}                                    # an exit's event releases about a quarter of all documents


def chain_inputs(seed=3):
    """store (E1, B, K) f32 logits by original slot whose argmax often stays from exit to exit (and, under temperature 3, some top pairs that
    round to one scaled value), LTE scores (E1, B), the stage-0 batch (1025 documents, two of them 257 and 600 rows long) and its metadata."""
    rng = np.random.default_rng(seed)
    E1, B, K = CHAIN_E1, CHAIN_B, CHAIN_K
    base = rng.standard_normal((B, K))
    store = (base[None] * np.linspace(0.6, 2.0, E1)[:, None, None] + rng.standard_normal((E1, B, K)) * 0.7) * CHAIN_TEMPS[:, None, None]
    store = store.astype(F32)
    z0, z1 = collision_pair(3.0)
    for b in range(0, B, 9):                                             # exit 1 (temperature 3): labels 2 < 5 collide as the two largest
        store[1, b] = np.minimum(store[1, b], F32(0.5))
        store[1, b, 2], store[1, b, 5] = z0, z1
    scores = rng.random((E1, B))
    lens = rng.integers(1, 41, CHAIN_N)
    lens[[7, 1000]] = (257, 600)
    stage = make_stage(CHAIN_N, B, seed, lens)
    meta = rng.integers(0, 1 << 20, (stage["n_rows"], 4)).astype(np.int64)
    return dict(store=store, scores=scores, stage=stage, meta=meta, x_rows=int((stage["x_phys"] + lens).max()))


def chain_tables(ci, kernel, criterion):
    """(scaled float64 store, criterion table (E1, B) the event reads, its sign, thresholds in gaps of the table, gap widths)."""
    from . import lte_ref
    mode, _ = kernel
    x = csf_ref.scaled(ci["store"], CHAIN_TEMPS)
    if mode == LTE:
        table, sign = ci["scores"], -1
        thr, width = lte_ref.gap_thresholds(table, CHAIN_POSITION[-1], MIN_GAP)
    else:
        crit = "max_confidence" if mode == PATIENCE else criterion
        table, sign = csf_ref.csf(x, crit), csf_ref.SIGN[crit]
        thr, width = csf_ref.gap_thresholds(table, CHAIN_POSITION[sign], MIN_GAP)
    return x, table, sign, thr, width


def chain_ref(ci, kernel, criterion, mut=""):
    """The E1 exits one after the other, the n_* outputs of one the stage of the next.  Returns per-exit results and, by original slot, the exit,
    the scaled logits and the criterion every document left with."""
    mode, rule = kernel
    _, _, _, thr, _ = chain_tables(ci, kernel, criterion)
    B, E1 = CHAIN_B, CHAIN_E1
    stage, state, steps = ci["stage"], None, []
    ex, logit, conf = np.full(B, -1, np.int64), np.full((B, CHAIN_K), np.nan, F32), np.full(B, np.nan)
    for e in range(E1):
        o = stage["doc_orig"]
        r = decide_ref(stage, ci["store"][e][o], mode=mode, rule=rule, criterion=criterion, thr=float(thr[e]), temp=float(CHAIN_TEMPS[e]),
                       patience=CHAIN_T, exit_index=e, B=B, state=state, lte_score=ci["scores"][e][o] if mode == LTE else None,
                       is_final=e == E1 - 1, mut=mut)
        lv = r["leave"]
        ex[o[lv]], logit[o[lv]], conf[o[lv]] = e, r["scaled32"][lv], r["crit"][lv]
        steps.append(dict(r, stage=stage))
        stage, state = as_stage(r["next"]), r["state"]
    return dict(steps=steps, exit=ex, logits=logit, conf=conf)


def chain_whole_store(ci, kernel, criterion):
    """The exits of every original slot by the restatements the project already trusts, on the whole store."""
    from . import lte_ref, patience_ref, rule_ref
    mode, rule = kernel
    x, table, sign, thr, _ = chain_tables(ci, kernel, criterion)
    s32 = x.astype(F32).astype(F64)                                      # the agreement counter looks at the scaled logits as written out
    if mode == PATIENCE:
        return patience_ref.patience_exits(s32, CHAIN_T)
    if rule != PLAIN:
        return rule_ref.rule_exits(table, s32, thr, CHAIN_T, rule, sign)
    if mode == LTE:
        return lte_ref.lte_exits(table, thr)
    return csf_ref.scan(x, thr, criterion)[0]


# ---------------------------------------------------------------------------------------------------------------------------------------
# CLS rows and padded hidden states
# ---------------------------------------------------------------------------------------------------------------------------------------
def gather_cls_ref(X, x_phys, doc_orig, out_rows):
    """out[doc_orig ? doc_orig[i] : i] = X[x_phys[i]]; (values (out_rows, H) float64, written (out_rows,))."""
    out, written = np.zeros((out_rows, X.shape[1]), F64), np.zeros(out_rows, bool)
    dst = np.arange(len(x_phys)) if doc_orig is None else np.asarray(doc_orig)
    out[dst], written[dst] = X[np.asarray(x_phys, np.int64)], True
    return out, written


def rows_to_padded_ref(X, B, T, Pv, text_dst, ntext, doc_off, mut=""):
    """(B, T + Pv, H): position p < T = row doc_off[d] + text_dst[d][p] of X, zeros where text_dst < 0; position T + v = the v-th visual row,
    behind the document's ntext[d] text rows (image-only, text_dst None: behind nothing)."""
    out = np.zeros((B, T + Pv, X.shape[1]), F64)
    for d in range(B):
        for p in range(T):
            t = text_dst[d][p]
            if t >= 0:
                out[d, p] = X[doc_off[d] + t]
            elif mut == "text_dst_copied":
                out[d, p] = X[(doc_off[d] + t) % len(X)]
        first = doc_off[d] + (ntext[d] if text_dst is not None else 0)
        out[d, T:] = X[first:first + Pv]
    return out


def padded_case(T, Pv, B=3, seed=0):
    """A ragged layout of B documents: text_dst (B, T) with some dropped positions, ntext, doc_off and the row count."""
    rng = np.random.default_rng(50 + seed + 10 * T + Pv)
    text_dst = np.full((B, T), -1, np.int64)
    ntext = np.zeros(B, np.int64)
    for d in range(B):
        kept = np.ones(T, bool) if T == 1 and d == 0 else rng.random(T) < 0.7
        if d == 1 or T == 1 and d == 2:
            kept[-1] = False                                             # at least one dropped position
        text_dst[d, kept] = np.arange(kept.sum())
        ntext[d] = kept.sum()
    doc_off = np.concatenate([[0], np.cumsum(ntext + Pv)]).astype(np.int64)
    return text_dst, ntext, doc_off[:B], int(doc_off[B])
