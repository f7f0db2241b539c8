"""Deadline exits restated in numpy and Python integers, written from the definition in include/mmee.h (behind the controller's): the
conversion of clock ticks to ns, the saturating add, the cut rule, what one check launch writes, and the thresholds a cut call is equal to.
Python integers do not wrap, so every modulo and every saturation of the 64-bit arithmetic is written out."""
import numpy as np

M64 = 2 ** 64
NONE = M64 - 1                  # MMEE_DEADLINE_NONE
OFF = M64 - 2                   # MMEE_DEADLINE_OFF
STATE_WORDS = 3                 # t0 (ticks), cut_exit, cut_by
MAX_E1 = 64


def log_words(E1):
    return 4 + E1               # call, budget_ns, cut_exit, cut_by, elapsed_ns[E1]


def sat_add(a, b):
    return min(int(a) + int(b), NONE)


def ticks_to_ns(d, khz):
    """(d / khz) 10^6 + (d % khz) 10^6 / khz in integers, 2^64 - 1 where that would not fit."""
    q, r = divmod(int(d), int(khz))
    if q > (NONE - 999999) // 10 ** 6:
        return NONE
    return q * 10 ** 6 + r * 10 ** 6 // int(khz)


def always_fires(sign):
    """The threshold every criterion that is not a NaN passes: -inf under the `>` criteria, +inf under entropy."""
    return np.inf if sign < 0 else -np.inf


def rule(t0, now, khz, budget, eta, host_word, call, exit_index, E1, prev_cut_exit, prev_cut_by):
    """(elapsed_ns, cut_exit, cut_by) after the check in front of exit `exit_index` of deadline call number `call`."""
    elapsed = ticks_to_ns((int(now) - int(t0)) % M64, khz)
    if prev_cut_exit >= 0 or exit_index >= E1 - 1:
        return elapsed, prev_cut_exit, prev_cut_by
    if budget != NONE and sat_add(elapsed, eta) >= budget:
        return elapsed, exit_index, 1
    if host_word >= call:
        return elapsed, exit_index, 2
    return elapsed, -1, 0


def check(state, thr, row, *, t0, now, khz, budget, eta, host_word, call, exit_index, sign):
    """One check launch on copies: state (3,) int64, thr (E1,) float64, row (4 + E1,) int64 (uint64 words kept as their int64 bit patterns)
    or None.  Returns the three as the launch leaves them."""
    state, thr = np.array(state, np.int64), np.array(thr, np.float64)
    row = None if row is None else np.array(row, np.int64)
    E1 = len(thr)
    elapsed, cut_exit, cut_by = rule(t0, now, khz, budget, eta, host_word, call, exit_index, E1, int(state[1]), int(state[2]))
    cut_now = state[1] < 0 and cut_exit >= 0
    if cut_now:
        thr[exit_index:E1 - 1] = always_fires(sign)
        state[1], state[2] = cut_exit, cut_by
    if row is not None:
        row[4 + exit_index] = np.array([elapsed], np.uint64).view(np.int64)[0]
        if cut_now:
            row[2], row[3] = cut_exit, cut_by
    return state, thr, row


def call_log(thr, sign, *, khz, budget, eta, t0, nows, host_words, call):
    """A whole deadline call: the begin launch, then one check per exit at clock nows[e] with the host word host_words[e].
    Returns (thr as the last decide launch reads it, log row)."""
    E1 = len(thr)
    state = np.array([t0, -1, 0], np.int64)
    row = np.zeros(log_words(E1), np.int64)
    row[0], row[1], row[2] = call, np.array([budget], np.uint64).view(np.int64)[0], -1
    cur = np.array(thr, np.float64)
    for e in range(E1):
        state, cur, row = check(state, cur, row, t0=t0, now=nows[e], khz=khz, budget=budget, eta=eta[e], host_word=host_words[e], call=call,
                                exit_index=e, sign=sign)
    return cur, row


def cut_thresholds(thr, cut_exit, sign):
    """thr' of the definition: thr below cut_exit, the always-fires value from cut_exit to the last exit below the final one.  The final
    exit's entry is kept (no forward reads it)."""
    out = np.array(thr, np.float64)
    if cut_exit >= 0:
        out[cut_exit:len(out) - 1] = always_fires(sign)
    return out
