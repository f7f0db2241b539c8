"""numpy restatement of the evaluation report (include/mmee.h, ee_exit_metrics), written from the header's text: the row quantities, the seven
metrics and the average confidence, per exit and for one operating point.  float64 throughout; the stable sort is ``np.argsort(kind="stable")``.
Nothing of the package is imported."""
import numpy as np

NAMES = ("accuracy", "brier_loss", "nll", "f1_micro", "f1_macro", "ece", "aurc", "average_confidence")


def row_quantities(logits, references, temperature=None):
    """One row of logits (N,K): dict of pred int64 (N,), conf, brier, nll float64 (N,), correct bool (N,).  ``temperature``: a scalar or (N,)."""
    z = np.asarray(logits, dtype=np.float64)
    y = np.asarray(references).reshape(-1)
    if temperature is not None:
        z = z / (np.asarray(temperature, dtype=np.float64).reshape(-1, 1) if np.ndim(temperature) else np.float64(temperature))
    m = z.max(-1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(-1, keepdims=True)
    p = e / s
    pred = z.argmax(-1)                                               # the first maximum
    onehot = np.zeros_like(p)
    onehot[np.arange(len(y)), y] = 1.0
    return dict(pred=pred, conf=p.max(-1), correct=pred == y, brier=((p - onehot) ** 2).sum(-1),
                nll=np.log(s[:, 0]) - (z[np.arange(len(y)), y] - m[:, 0]))


def confusion_matrix(references, pred, K):
    cm = np.zeros((K, K), dtype=np.int64)
    np.add.at(cm, (np.asarray(references).reshape(-1), np.asarray(pred).reshape(-1)), 1)
    return cm


def f1_macro(cm):
    """Per class 2TP / (2TP + FP + FN) from integer counts, 0 where the denominator is 0, averaged over the classes that occur in the
    references or the predictions."""
    total, n = 0.0, 0
    for c in range(cm.shape[0]):
        truth, preds = int(cm[c, :].sum()), int(cm[:, c].sum())
        if truth + preds == 0:
            continue
        total += (2 * int(cm[c, c])) / float(truth + preds)
        n += 1
    return total / n if n else 0.0


def default_bins(N):
    return max(1, min(N - 1, 100))


def ece(conf, correct, n_bins=None):
    """Equal-mass bins, upper-edge proxy, p = 1, on the top-label confidences: the expressions of calibration.expected_calibration_error."""
    conf = np.asarray(conf, dtype=np.float64)
    correct = np.asarray(correct).astype(np.float64)
    N = conf.shape[0]
    n_bins = default_bins(N) if n_bins is None or n_bins <= 0 else int(n_bins)
    srt = np.sort(conf)
    edges = np.concatenate([srt[(np.arange(n_bins) * N) // n_bins], [1.0]])
    idx = np.clip(np.searchsorted(edges, conf, side="right") - 1, 0, n_bins - 1)
    cnt = np.bincount(idx, minlength=n_bins).astype(np.float64)
    acc = np.divide(np.bincount(idx, weights=correct, minlength=n_bins), cnt, out=np.zeros(n_bins), where=cnt > 0)
    w = cnt / N
    return float(np.sum(w * np.abs(acc - edges[1:]) ** 1) ** (1.0 / 1))


def aurc(conf, correct):
    """The risk-coverage curve of the header: ascending confidence, ties in document order."""
    conf = np.asarray(conf, dtype=np.float64)
    N = conf.shape[0]
    order = np.argsort(conf, kind="stable")
    c = conf[order]
    r = [0 if ok else 1 for ok in np.asarray(correct)[order]]
    err = sum(r)                                                      # S_0, a Python integer
    risks, weights = [err / N], []
    t = 0
    for i in range(N - 1):
        err -= r[i]                                                   # S_{i+1}
        t += 1
        if i == 0 or c[i] != c[i - 1]:
            risks.append(err / (N - 1 - i))
            weights.append(t / N)
            t = 0
    if t > 0:
        risks.append(risks[-1])
        weights.append(t / N)
    return float(sum((risks[j] + risks[j + 1]) * 0.5 * weights[j] for j in range(len(weights))))


def table_row(conf, correct, n_bins=None):
    """The metrics a (conf, correct) row defines; the others are NaN."""
    conf = np.asarray(conf, dtype=np.float64)
    hits = int(np.count_nonzero(correct))
    N = conf.shape[0]
    return dict(accuracy=hits / N, brier_loss=float("nan"), nll=float("nan"), f1_micro=hits / N, f1_macro=float("nan"),
                ece=ece(conf, correct, n_bins), aurc=aurc(conf, correct), average_confidence=float(conf.sum() / N))


def logits_row(logits, references, temperature=None, n_bins=None, K=None):
    """(metrics dict, confusion (K,K)) of one row of logits (N,K)."""
    q = row_quantities(logits, references, temperature)
    N = len(q["conf"])
    out = table_row(q["conf"], q["correct"], n_bins)
    cm = confusion_matrix(references, q["pred"], K or np.shape(logits)[-1])
    out.update(brier_loss=float(q["brier"].sum() / N), nll=float(q["nll"].sum() / N), f1_macro=f1_macro(cm))
    return out, cm


def report(logits, references=None, temperatures=None, exits=None, n_bins=None):
    """dict: every name of NAMES as (R,) float64, ``confusion`` (R,K,K) int64 or None, ``exit_hist`` (E1,) int64 or None.  ``logits`` (E1,N,K)
    with ``references``, or the pair (conf (E1,N), correct (E1,N))."""
    rows, cms = [], []
    if isinstance(logits, tuple):
        conf, correct = np.asarray(logits[0], dtype=np.float64), np.asarray(logits[1])
        E1, N = conf.shape
        for e in range(E1):
            rows.append(table_row(conf[e], correct[e], n_bins))
        if exits is not None:
            ex = np.asarray(exits).reshape(-1)
            rows.append(table_row(conf[ex, np.arange(N)], correct[ex, np.arange(N)], n_bins))
    else:
        L = np.asarray(logits, dtype=np.float64)
        E1, N, K = L.shape
        T = None if temperatures is None else np.asarray(temperatures, dtype=np.float64)
        for e in range(E1):
            m, cm = logits_row(L[e], references, None if T is None else T[e], n_bins)
            rows.append(m), cms.append(cm)
        if exits is not None:
            ex = np.asarray(exits).reshape(-1)
            m, cm = logits_row(L[ex, np.arange(N)], references, None if T is None else T[ex], n_bins)
            rows.append(m), cms.append(cm)
    out = {k: np.array([r[k] for r in rows], dtype=np.float64) for k in NAMES}
    out["confusion"] = np.stack(cms) if cms else None
    out["exit_hist"] = None if exits is None else np.bincount(np.asarray(exits).reshape(-1), minlength=E1).astype(np.int64)
    return out
