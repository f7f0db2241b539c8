"""numpy float64 restatement of the three confidence scoring functions of include/mmee.h (max-softmax, entropy, and the margin of
MMEE_CRIT_MARGIN) and of the thresholding policy on them, the oracle of tests/test_host_margin.py and tests/test_gpu_margin.py.  The
reference names a margin (CSF_dict, EE/thresh.py:55-61) but its top12_margin_np subtracts the two smallest raw logits and is never called, so
there is no reference output to pin against: these lines ARE the specification, written from the header's text, independently of the
kernels."""
import numpy as np

CRITERIA = ("max_confidence", "entropy", "margin")
SIGN = {"max_confidence": +1, "entropy": -1, "margin": +1}      # +1: leave on crit > thr, -1: on crit < thr


def _sum_in_label_order(terms):
    """sum over the last axis, k = 0 .. K-1 one after the other (np.sum adds pairwise)."""
    s = np.zeros(terms.shape[:-1])
    for k in range(terms.shape[-1]):
        s = s + terms[..., k]
    return s


def max_softmax(x):
    """1 / sum_k exp(x_k - max x)."""
    x = np.asarray(x, dtype=np.float64)
    return 1.0 / _sum_in_label_order(np.exp(x - x.max(-1, keepdims=True)))


def entropy(x):
    """The reference's expression (EE/thresh.py:41-45): log A - B / A with A = sum e^x, B = sum x e^x, no max shift."""
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(x)
    A, B = _sum_in_label_order(e), _sum_in_label_order(x * e)
    return np.log(A) - B / A


def margin(x):
    """x (..., K) float64, already divided by the temperature.  m1 the maximum, m2 the second largest value counting multiplicity,
    S = sum_k exp(x_k - m1) in label order: (1 - exp(m2 - m1)) / S.  K = 1: the second probability is 0."""
    x = np.asarray(x, dtype=np.float64)
    srt = np.sort(x, axis=-1)
    m1 = srt[..., -1]
    S = _sum_in_label_order(np.exp(x - m1[..., None]))
    second = np.exp(srt[..., -2] - m1) if x.shape[-1] > 1 else np.zeros(m1.shape)
    return (1.0 - second) / S


def csf(x, criterion):
    return {"max_confidence": max_softmax, "entropy": entropy, "margin": margin}[criterion](x)


def scaled(z, temperatures=None):
    """(double)z / T: z (E1,N,K) float32 policy logits, temperatures (E1,) or None."""
    x = np.asarray(z).astype(np.float64)
    return x if temperatures is None else x / np.asarray(temperatures, dtype=np.float64)[:, None, None]


def exits(table, thresholds, sign=+1):
    """First exit e < E1 - 1 whose criterion strictly passes its threshold (sign +1: '>', -1: '<'; a NaN never does), else the last exit."""
    t = np.asarray(table, dtype=np.float64)
    thr = np.broadcast_to(np.asarray(thresholds, dtype=np.float64).reshape(-1), (t.shape[0],))[:, None]
    with np.errstate(invalid="ignore"):
        hit = t > thr if sign > 0 else t < thr
    hit[-1] = True
    return hit.argmax(0).astype(np.int32)


def scan(logits, thresholds, criterion):
    """(exits int32 (N,), predictions (N,K), confidence (N,) = the criterion at the chosen exit, counts (E1,)) on a dumped (E1,N,K) array."""
    logits = np.asarray(logits, dtype=np.float64)
    table = csf(logits, criterion)
    ex = exits(table, thresholds, SIGN[criterion])
    rows = np.arange(logits.shape[1])
    return ex, logits[ex, rows], table[ex, rows], np.bincount(ex, minlength=logits.shape[0])


def gap_thresholds(table, position, min_gap):
    """Per-exit thresholds at the midpoint of a gap between two neighbours of that exit's sorted criteria: the gap of width >= min_gap nearest
    to the position `position` x N.  Returns (thresholds (E1,), widths (E1,)); the final exit, which has no test, gets 0.5 and inf.  Raises when
    an exit has no gap that wide."""
    t = np.asarray(table, dtype=np.float64)
    E1, N = t.shape
    thr, width = np.full(E1, 0.5), np.full(E1, np.inf)
    for e in range(E1 - 1):
        srt = np.sort(t[e])
        gaps = np.diff(srt)
        ok = np.nonzero(gaps >= min_gap)[0]
        if ok.size == 0:
            raise ValueError(f"exit {e}: no gap of width >= {min_gap}")
        i = ok[np.abs(ok + 1 - position * N).argmin()]
        thr[e], width[e] = 0.5 * (srt[i] + srt[i + 1]), gaps[i]
    return thr, width


def threshold_sweep(table, correct, thresholds):
    """The reference's sweep (EE/thresh.py:184-215) on a CSF table: exits = (table >= thr[:, None]).argmax(0) -- the first exit whose value
    reaches its threshold, exit 0 when none does.  Integer (hits (V,), exit sums (V,), histogram (V,E1))."""
    table = np.asarray(table, dtype=np.float64)
    E1, N = table.shape
    hits, sums, hist = [], [], []
    for thr in np.asarray(thresholds, dtype=np.float64):
        ex = (table >= thr[:, None]).argmax(0)
        hits.append(int(np.asarray(correct)[ex, np.arange(N)].sum()))
        sums.append(int(ex.sum()))
        hist.append(np.bincount(ex, minlength=E1))
    return np.array(hits), np.array(sums), np.array(hist)
