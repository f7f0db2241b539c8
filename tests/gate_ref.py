"""numpy float64 restatement of the gate decision (include/mmee.h MMEE_CRIT_GATE) and of the gate objective (ee_head_fit_gate), the oracle
of tests/test_host_gate.py, tests/test_gpu_gate.py and tests/test_gpu_gate_fit.py.  The reference's evaluation never lets a gate decide and
has no fit of gate heads on a frozen backbone, so there is no reference output to pin against: these lines ARE the specification, written from
the header's text, independently of the kernels.

    gate score     g = 1 / (1 + exp((double)h0 - (double)h1))      h = the gate head's two raw float32 logits; column 1 is "correctly gated"
    event          g > thr   (strict; a NaN never fires)           no temperature enters g
    what leaves    the scaled policy row (float)((double)z / T)    z = classifier(gate input)
    final exit     no gate: the criterion written out is the max-softmax of the scaled final logits, everybody leaves
    objective      L(W, b) = 1/(2N) sum_n [bce(z_1, c) + bce(z_0, 1 - c)] + l2/2 (|W|^2 + |b|^2),   z = W x + b,   bce(z, t) = softplus(z) - t z
"""
import numpy as np

F32, F64 = np.float32, np.float64
CRIT_GATE = 4                                                            # MMEE_CRIT_GATE
MIN_GAP = 1e-9                                                           # thresholds sit in gaps of the sorted reference scores wider than this
MIN_DIST = 1e-12                                                         # and no document's score may be closer than this to its threshold
PLAIN, STREAK, EITHER = 0, 1, 2                                          # MMEE_RULE_*


# ---------------------------------------------------------------------------------------------------------------------------------------
# the score, the table, the policy on dumped arrays
# ---------------------------------------------------------------------------------------------------------------------------------------
def gate_score(head_logits):
    """head_logits (..., 2) float32 -> g (...,) float64."""
    h = np.asarray(head_logits, F32).astype(F64)
    with np.errstate(over="ignore", invalid="ignore"):
        return 1.0 / (1.0 + np.exp(h[..., 0] - h[..., 1]))


def max_softmax(x):
    """1 / sum_k exp(x_k - max x), the sum in label order."""
    x = np.asarray(x, F64)
    t = np.exp(x - x.max(-1, keepdims=True))
    s = np.zeros(t.shape[:-1])
    for k in range(t.shape[-1]):
        s = s + t[..., k]
    return 1.0 / s


def gate_table(head_logits, final_logits):
    """head_logits (E,N,2) f32, final_logits (N,K) float64 -> (E+1,N): the gate scores, then the max-softmax of the final row."""
    head_logits = np.asarray(head_logits, F32).reshape(-1, np.shape(final_logits)[0], 2)
    return np.concatenate([gate_score(head_logits), max_softmax(final_logits)[None]], 0)


def fires(score, thr):
    with np.errstate(invalid="ignore"):
        return np.asarray(score, F64) > thr


def gate_exits(table, thresholds):
    """First e < E1 - 1 with table[e, n] > thresholds[e], else E1 - 1."""
    t = np.asarray(table, F64)
    thr = np.broadcast_to(np.asarray(thresholds, F64).reshape(-1), (t.shape[0],))[:, None]
    hit = fires(t, thr)
    hit[-1] = True
    return hit.argmax(0).astype(np.int32)


def gate_scan(table, logits, thresholds):
    """(exits (N,), predictions (N,K) = the policy row of the chosen exit, confidence (N,) = its table entry, counts (E1,))."""
    logits = np.asarray(logits, F64)
    ex = gate_exits(table, thresholds)
    rows = np.arange(logits.shape[1])
    return ex, logits[ex, rows], np.asarray(table, F64)[ex, rows], np.bincount(ex, minlength=logits.shape[0])


def midpoint_threshold(scores, position=0.5, min_gap=MIN_GAP):
    """A threshold at the midpoint of two adjacent sorted scores whose gap exceeds min_gap, the gap nearest to `position` x n.  Returns
    (threshold, distance of the nearest score).  Fewer than two distinct scores: a threshold off to one side."""
    s = np.sort(np.asarray(scores, F64).reshape(-1))
    s = s[np.isfinite(s)]
    gaps = np.diff(s)
    ok = np.nonzero(gaps > min_gap)[0]
    if ok.size == 0:
        thr = (s[-1] + 1.0) if s.size else 0.5
        return float(thr), float(np.abs(s - thr).min()) if s.size else np.inf
    i = ok[np.abs(ok + 1 - position * s.size).argmin()]
    thr = 0.5 * (s[i] + s[i + 1])
    return float(thr), float(np.abs(s - thr).min())


def assert_clear(scores, thr, what=""):
    """The condition of the decision tests: no document's reference score within MIN_DIST of its threshold."""
    s = np.asarray(scores, F64).reshape(-1)
    s = s[np.isfinite(s)]
    d = np.abs(s - thr).min() if s.size else np.inf
    assert d > MIN_DIST, (what, "a reference score within 1e-12 of its threshold", float(d))


def cascade_thresholds(scores, min_gap=MIN_GAP):
    """Per-exit thresholds for a forward: scores (E,N) float64 reference gate scores.  Exit e's threshold sits at a gap midpoint of the scores
    of the documents that are STILL THERE at e (by this very restatement), placed so that about 1 / (E + 1 - e) of them leave: every exit
    releases somebody and somebody reaches the end.  Every score of a document still there keeps MIN_DIST from its threshold (asserted).
    Returns (thresholds (E+1,), exits (N,)); the final entry, which no test reads, is 0.5."""
    scores = np.asarray(scores, F64)
    E, N = scores.shape
    thr, ex, here = np.full(E + 1, 0.5), np.full(N, E, np.int32), np.ones(N, bool)
    for e in range(E):
        s = scores[e, here]
        thr[e], _ = midpoint_threshold(s, 1.0 - 1.0 / (E + 1 - e), min_gap)
        assert_clear(s, thr[e], f"exit {e}")
        leave = here & fires(scores[e], thr[e])
        assert leave.any() and (here & ~leave).any(), (e, int(leave.sum()), int(here.sum()))
        ex[leave], here = e, here & ~leave
    return thr, ex


# ---------------------------------------------------------------------------------------------------------------------------------------
# one exit of one stage (ee_debug_exit_decide under MMEE_CRIT_GATE): the event from the gate logits, the rule, the scaled rows
# ---------------------------------------------------------------------------------------------------------------------------------------
def decide(stage, logits, head_logits, *, thr, temp, rule=PLAIN, patience=1, exit_index=0, B=None, state=None, is_final=False, no_exit=False,
           dirty=0):
    """stage: dict(n, doc_orig (n,)).  logits (n,K) f32 policy logits, head_logits (n,2) f32.  state (prev, run) int arrays [B] by original slot.
    Returns leave (n,), scaled32 (n,K) f32, crit (n,) float64 (out_all_crit / out_conf), head_crit (n,) float64 (out_head_crit), state."""
    n, orig = stage["n"], np.asarray(stage["doc_orig"], np.int64)
    z = np.asarray(logits, F32).reshape(n, -1)
    x = z.astype(F64) / F64(temp)
    s32 = x.astype(F32)
    g = gate_score(np.asarray(head_logits, F32).reshape(n, 2))
    crit = max_softmax(x) if is_final else g
    with np.errstate(invalid="ignore"):
        event = crit > thr
    prev, run = (np.full(B, dirty, np.int64), np.full(B, dirty, np.int64)) if state is None else (state[0].astype(np.int64), state[1].astype(np.int64))
    later = exit_index > 0
    if rule == EITHER:
        am = np.argmax(s32, -1) if n else np.zeros(0, np.int64)
        c = np.where(prev[orig] == am, run[orig] + 1, 0) if later else np.zeros(n, np.int64)
        prev[orig], run[orig] = am, c
        leave = event | (c >= patience)
    elif rule == STREAK:
        before = run[orig] if later else np.zeros(n, np.int64)
        s = np.where(event, before + 1, 0)
        run[orig] = s
        leave = s >= patience
    else:
        leave = event
    if no_exit:
        leave = np.zeros(n, bool)
    if is_final:
        leave = np.ones(n, bool)
    return dict(leave=leave, scaled32=s32, crit=crit, head_crit=g, state=(prev, run))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the gate objective
# ---------------------------------------------------------------------------------------------------------------------------------------
def softplus(z):
    z = np.asarray(z, F64)
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def gate_lossgrad(theta, X, c, l2):
    """theta (2H + 2,) = W (2,H) row-major then b (2,); X (N,H) f32, c (N,) targets in [0,1].  (loss, grad (2H + 2,)) in float64."""
    X = np.asarray(X, F32).astype(F64)
    N, H = X.shape
    theta = np.asarray(theta, F64)
    W, b = theta[:2 * H].reshape(2, H), theta[2 * H:]
    z = X @ W.T + b                                                      # (N,2)
    t = np.stack([1.0 - np.asarray(c, F64), np.asarray(c, F64)], 1)      # column 1 is "correctly gated"
    loss = (softplus(z) - t * z).sum() / (2.0 * N) + 0.5 * l2 * (theta ** 2).sum()
    ez = np.exp(-np.abs(z))
    r = (np.where(z >= 0, 1.0, ez) / (1.0 + ez) - t) / (2.0 * N)         # dL/dz = (sigmoid(z) - t) / 2N, without overflow
    g = np.concatenate([(r.T @ X).reshape(-1), r.sum(0)]) + l2 * theta
    return float(loss), g


def gate_fit(X, c, l2, theta0=None, rounds=4, want=1e-10):
    """The unique optimum (l2 > 0) by scipy's L-BFGS-B in float64, restarted from its own result (a restart drops the stale curvature pairs)
    until the gradient's largest entry is below `want` or `rounds` runs are spent.  Returns (theta (2H + 2,), max |grad|)."""
    from scipy.optimize import minimize
    H = np.shape(X)[1]
    x = np.zeros(2 * H + 2) if theta0 is None else np.asarray(theta0, F64)
    gmax = np.inf
    for _ in range(rounds):
        res = minimize(gate_lossgrad, x, args=(X, c, l2), jac=True, method="L-BFGS-B",
                       options=dict(maxiter=20000, maxfun=40000, ftol=1e-17, gtol=1e-12, maxcor=30))
        x = res.x
        gmax = float(np.abs(gate_lossgrad(x, X, c, l2)[1]).max())
        if gmax <= want:
            break
    return x, gmax


def gate_logits(theta, X):
    X = np.asarray(X, F32).astype(F64)
    H = X.shape[1]
    return X @ np.asarray(theta, F64)[:2 * H].reshape(2, H).T + np.asarray(theta, F64)[2 * H:]
