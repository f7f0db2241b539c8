"""numpy float64 restatement of the learning-to-exit (LTE) semantics of include/mmee.h (``ee_config.use_lte``), the oracle of
tests/test_host_lte.py and tests/test_gpu_lte.py.  The reference's own wiring of LTE cannot run (batch size 1, a layer index compared with an
exit count), so there is no reference output to pin against: these lines ARE the specification, written independently of the kernels."""
import numpy as np


def lte_score(x, w, b):
    """x (..., H) float32 CLS rows, w (1, H) or (H,), b (1,) -> float64 sigmoid(w . x + b), every operand widened to float64 first."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    w = np.asarray(w, dtype=np.float32).astype(np.float64).reshape(-1)
    t = x @ w + float(np.asarray(b, dtype=np.float32).reshape(-1)[0])
    return 1.0 / (1.0 + np.exp(-t))


def lte_scores(hidden_cls, w, b, encoder_exit_layers, n_embedding_exits=0):
    """hidden_cls (L+1, B, H): the CLS row entering layer 0 and leaving every layer.  -> (E1, B) float64: 1.0 in the rows of the embedding-level
    exits (they have no CLS row), the score of the row leaving layer l for an encoder exit at the 1-based layer l, and of the last row for the
    final classifier."""
    hidden_cls = np.asarray(hidden_cls)
    rows = [np.ones(hidden_cls.shape[1]) for _ in range(n_embedding_exits)]
    rows += [lte_score(hidden_cls[int(l)], w, b) for l in encoder_exit_layers]
    rows.append(lte_score(hidden_cls[-1], w, b))
    return np.stack(rows)


def lte_exits(scores, thresholds, n_embedding_exits=0):
    """First encoder exit e (n_embedding_exits <= e < E1 - 1) with scores[e, n] < thresholds[e] (strict, float64), else the last exit.
    Embedding-level exits never release anybody, whatever their rows and thresholds hold."""
    s = np.asarray(scores, dtype=np.float64)
    E1 = s.shape[0]
    thr = np.broadcast_to(np.asarray(thresholds, dtype=np.float64).reshape(-1), (E1,))
    hit = s < thr[:, None]
    hit[:n_embedding_exits] = False
    hit[-1] = True
    return hit.argmax(0).astype(np.int32)


def lte_policy(scores, logits, thresholds, n_embedding_exits=0):
    """(exits int32 (N,), predictions (N,K) = the logits row of the chosen exit, counts (E1,)) on dumped arrays."""
    logits = np.asarray(logits, dtype=np.float64)
    ex = lte_exits(scores, thresholds, n_embedding_exits)
    return ex, logits[ex, np.arange(logits.shape[1])], np.bincount(ex, minlength=logits.shape[0])


def gap_thresholds(scores, quantile, min_gap, n_embedding_exits=0):
    """Per-exit thresholds at the midpoint of a gap between two neighbours of the sorted scores of that exit: the gap of width >= min_gap
    whose position is nearest to `quantile` of the documents.  Returns (thresholds (E1,), the chosen gaps' widths (E1,)); rows without a CLS
    score (embedding exits) and the final exit get threshold 0.5 and width inf.  Raises when an exit has no gap that wide."""
    s = np.asarray(scores, dtype=np.float64)
    E1, N = s.shape
    thr, width = np.full(E1, 0.5), np.full(E1, np.inf)
    for e in range(n_embedding_exits, E1 - 1):
        srt = np.sort(s[e])
        gaps = np.diff(srt)
        ok = np.nonzero(gaps >= min_gap)[0]
        if ok.size == 0:
            raise ValueError(f"exit {e}: no gap of width >= {min_gap}")
        i = ok[np.abs(ok + 1 - quantile * N).argmin()]
        thr[e], width[e] = 0.5 * (srt[i] + srt[i + 1]), gaps[i]
    return thr, width
