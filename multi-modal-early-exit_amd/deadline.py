"""Deadline exits on the host side: the lookahead table ``EarlyExitEngine.set_deadline(eta_ms=)`` takes, measured from deadline logs.

The definition of a deadline call is in include/mmee.h.  Its log holds, per call, the device time from the begin launch to the check in front
of every exit's decision.  Over calls nobody cut, ``elapsed[E1 - 1] - elapsed[e]`` is what the definition calls eta: the time from the decision
at exit ``e`` to (the last check of) the call if nobody is cut there.  No device code lives here."""
from __future__ import annotations

import math
from typing import Iterable, Union

import numpy as np


def _rows(logs):
    """(T,) cut_exit and (T,E1) elapsed_ns of one log or of several with the same number of exits."""
    if hasattr(logs, "elapsed_ns"):
        logs = [logs]
    logs = list(logs)
    if not logs:
        raise ValueError("eta_from_logs: no log given")
    E1 = {int(np.asarray(lg.elapsed_ns).reshape(len(np.asarray(lg.cut_exit)), -1).shape[1]) for lg in logs if len(np.asarray(lg.cut_exit))}
    if len(E1) > 1:
        raise ValueError(f"eta_from_logs: the logs disagree on the number of exits: {sorted(E1)}")
    if not E1:
        raise ValueError("eta_from_logs: the logs hold no call")
    e1 = E1.pop()
    cut = np.concatenate([np.asarray(lg.cut_exit, dtype=np.int64).reshape(-1) for lg in logs])
    el = np.concatenate([np.asarray(lg.elapsed_ns).astype(np.uint64).reshape(-1, e1) for lg in logs if len(np.asarray(lg.cut_exit))])
    return cut, el


def eta_from_logs(logs: Union[object, Iterable[object]], quantile: float = 1.0) -> np.ndarray:
    """``(E1,)`` float64 milliseconds: per exit ``e``, ``elapsed[E1 - 1] - elapsed[e]`` over the UNCUT calls of ``logs`` (a ``DeadlineLog`` or
    several; a stamps-only pass gives them) -- the maximum, or with ``quantile`` q in (0, 1] the smallest observed value that at least a share q
    of the calls stay at or below (an observation, never an interpolation).  The last entry is 0.  Pass it to ``set_deadline(eta_ms=)``: the
    cut then falls at the last exit the budget still allows.  The estimate is as good as the logged calls resemble the served ones: measure on
    the shapes and thresholds that are served."""
    if not 0.0 < float(quantile) <= 1.0:
        raise ValueError(f"eta_from_logs: quantile {quantile} outside (0, 1]")
    cut, el = _rows(logs)
    el = el[cut < 0]
    if el.shape[0] == 0:
        raise ValueError("eta_from_logs: every logged call was cut: eta is the time to the end if nobody is cut (log a stamps-only pass)")
    if np.any(el[:, 1:] < el[:, :-1]):
        raise ValueError("eta_from_logs: a logged call's stamps decrease: the rows are not elapsed times of one clock")
    rest = np.sort(el[:, -1:] - el, axis=0)                         # uint64, no wrap: the stamps do not decrease
    k = min(rest.shape[0] - 1, max(0, math.ceil(float(quantile) * rest.shape[0]) - 1))
    return rest[k].astype(np.float64) / 1e6


def eta_to_next_exit(logs: Union[object, Iterable[object]], tail_ms: float, quantile: float = 1.0) -> np.ndarray:
    """``(E1,)`` float64 milliseconds, the less conservative table: per exit ``e`` below the last one that can cut, the stretch
    ``elapsed[e + 1] - elapsed[e]`` to the NEXT check over the uncut calls of ``logs`` (maximum, or ``quantile`` as in ``eta_from_logs``) plus
    ``tail_ms``, the tail of empty launches behind a cut (``elapsed[E1 - 1] - elapsed[cut_exit]`` of cut calls' rows) -- the time to the end
    of the call if everybody is cut at the next exit instead of this one.  The last exit below the final one has no later cut: its entry, and
    the final 0, are ``eta_from_logs``' own.  ``eta_from_logs`` asks "would the uncut call still finish?" and so, at its maximum, cuts at exit
    0 whenever the budget lies below the slowest logged call; this table asks "can the cut wait one more exit?"."""
    if not float(tail_ms) >= 0.0:
        raise ValueError(f"eta_to_next_exit: tail_ms {tail_ms} is not a time >= 0")
    eta = eta_from_logs(logs, quantile)
    cut, el = _rows(logs)
    el = el[cut < 0]
    step = np.sort(el[:, 1:] - el[:, :-1], axis=0)
    k = min(step.shape[0] - 1, max(0, math.ceil(float(quantile) * step.shape[0]) - 1))
    E = eta.shape[0] - 1
    if E >= 2:
        eta[:E - 1] = step[k, :E - 1].astype(np.float64) / 1e6 + float(tail_ms)
    return eta
