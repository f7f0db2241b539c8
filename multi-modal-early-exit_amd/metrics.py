"""The evaluation report on the device: counterpart of ``evaluate_checkpoint`` (EE/eval.py:175-181), which scores every exit with
``METRICS = [accuracy, brier_loss, nll, f1_micro, f1_macro, ece_logits, aurc_logits]``, and of ``eval_model`` (EE/eval.py:87-112), which scores
the predictions of the chosen exit policy with the same list through ``calc_metrics`` (EE/utils.py:226-237).

``exit_report`` takes the dumped logits (or a criterion table) where they are -- on the device -- and returns the seven metrics and the average
confidence per exit and, with ``exits``, for that operating point (ee_exit_metrics; the semantics are written out in include/mmee.h).  ECE: only
the scheme ``ece_logits`` asks for (equal-mass bins, upper-edge proxy, p = 1), i.e. ``calibration.expected_calibration_error`` with its
defaults; AURC: ties between confidences are taken in document order.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

from . import capi
from .engine import _require_torch_cuda, torch
from .policy import _f64_on, _on, _ptr

# the columns of ee_exit_metrics' output (capi.METRIC_*) under the names of the reference's functions
FIELDS = ("accuracy", "brier_loss", "nll", "f1_micro", "f1_macro", "ece", "aurc", "average_confidence")
# METRICS of EE/eval.py:175-181 with "_logits" stripped
REFERENCE_NAMES = ("accuracy", "brier_loss", "nll", "f1_micro", "f1_macro", "ece", "aurc")


@dataclass
class ExitReport:
    """``R = E1 + 1`` rows with an operating point (``policy = E1``, the last row), else ``R = E1`` (``policy = None``).  numpy arrays on the host."""
    accuracy: np.ndarray                    # (R,) hits / N
    brier_loss: np.ndarray                  # (R,) NaN from a (conf, correct) table
    nll: np.ndarray                         # (R,) NaN from a table
    f1_micro: np.ndarray                    # (R,) = accuracy (single-label multiclass)
    f1_macro: np.ndarray                    # (R,) NaN from a table
    ece: np.ndarray                         # (R,)
    aurc: np.ndarray                        # (R,)
    average_confidence: np.ndarray          # (R,)
    num_samples: int
    exit_hist: Optional[np.ndarray] = None  # (E1,) int64: documents per exit of the operating point
    confusion: Optional[np.ndarray] = None  # (R,K,K) int64: [row][reference][prediction] (``want_confusion=True``)
    policy: Optional[int] = None            # the index of the operating-point row

    @property
    def num_exits(self) -> int:
        return len(self.accuracy) - (0 if self.policy is None else 1)

    def as_reference_dict(self) -> Dict[str, float]:
        """The reference's keys: ``f"exit_{e} _{name}"`` (with that space, EE/eval.py:179-181) for every exit, and the operating point under the
        plain names, as ``calc_metrics`` returns them."""
        out = {}
        for e in range(self.num_exits):
            for name in REFERENCE_NAMES:
                out[f"exit_{e} _{name}"] = float(getattr(self, name)[e])
        if self.policy is not None:
            for name in REFERENCE_NAMES:
                out[name] = float(getattr(self, name)[self.policy])
        return out

    def efficiency(self, cost=None) -> dict:
        """What EE/large_scale.py:100-103 reports next to the accuracy: ``exit_distribution`` = {exit: fraction of the documents that leave there}
        and, with a per-exit ``cost`` (E1,) -- the reference's FLOPs per exit, or ``sweep.exit_costs`` of one document --,
        ``"GFLOPs reduction" = 1 - sum_e frac_e cost_e / cost_last``.  On the host, from ``exit_hist``."""
        if self.exit_hist is None:
            raise ValueError("efficiency needs an operating point: exit_report(..., exits=...)")
        frac = self.exit_hist.astype(np.float64) / float(self.num_samples)
        out = {"exit_distribution": {e: float(f) for e, f in enumerate(frac)}}
        if cost is not None:
            c = np.asarray(cost, dtype=np.float64)
            if c.ndim == 2:
                raise NotImplementedError("a per-document cost (E1,N) needs the exits, which the report does not keep: pass a per-exit cost (E1,)")
            if c.shape != frac.shape:
                raise ValueError(f"cost: shape ({len(frac)},), not {c.shape}")
            if not c[-1] > 0:
                raise ValueError("cost: the final exit's cost must be positive")
            out["GFLOPs reduction"] = float(1.0 - np.sum(frac * c) / c[-1])
        return out


def _is_tensor(x):
    return torch is not None and isinstance(x, torch.Tensor)


def _shape(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.shape(x)


def _range(x):
    """(min, max) of an integer array, numpy or torch, as Python integers."""
    if _is_tensor(x):
        return int(x.min()), int(x.max())
    a = np.asarray(x)
    return int(a.min()), int(a.max())


def exit_report(logits, references=None, temperatures=None, exits=None, n_bins: Optional[int] = None, want_confusion: bool = False,
                device=None) -> ExitReport:
    """How does every exit, and one operating point, score?  ``logits`` (E1,N,K) or (N,K) (numpy / torch, evaluated as float64) with
    ``references`` (N,), or the pair ``(conf (E1,N), correct (E1,N))`` that ``threshold_search`` accepts (``csf_table`` / ``msp_table``): then
    Brier, NLL and macro F1 are NaN and there is no confusion matrix.  ``temperatures`` (E1,): the logits are divided by their exit's temperature
    first (``calibration.fit_temperatures``).  ``exits`` (N,) integers in [0, E1) -- from ``early_exit``, ``criterion_scan_device`` or a
    ``Policy`` --: one more row, the operating point, in which document n is scored at exit ``exits[n]``, and ``exit_hist``.  ``n_bins``: the
    ECE bins, default ``max(1, min(N - 1, 100))``, at most 1024; only the equal-mass / upper-edge / p = 1 scheme is built.

    Everything is validated on the host before anything is enqueued: shapes, labels in [0, K), exits in [0, E1), temperatures finite and
    positive (``ValueError``).  One device call; the only download is the (R, 8) result (and the optional counts)."""
    pair = isinstance(logits, tuple)
    if pair:
        if len(logits) != 2:
            raise ValueError("a precomputed table is the pair (conf (E1,N), correct (E1,N))")
        if temperatures is not None:
            raise ValueError("temperatures scale logits: a (conf, correct) table has none")
        if want_confusion:
            raise ValueError("a (conf, correct) table has no predictions: no confusion matrix")
        shp = _shape(logits[0])
        if len(shp) != 2 or _shape(logits[1]) != shp:
            raise ValueError("table: conf (E1,N) and correct (E1,N)")
        (E1, N), K = shp, 0
    else:
        shp = _shape(logits)
        if len(shp) == 2:
            shp = (1,) + shp
        if len(shp) != 3:
            raise ValueError("logits must have shape (num_exits + 1, num_samples, num_labels) or (num_samples, num_labels)")
        E1, N, K = shp
        if references is None:
            raise ValueError("logits need the references")
        if _shape(references) != (N,):
            raise ValueError(f"references: shape ({N},), not {_shape(references)}")
    if E1 < 1 or N < 1 or (not pair and K < 1):
        raise ValueError("the report needs at least one exit, one document and one label")
    if N > 1 << 20:
        raise ValueError(f"N = {N}: more than 2^20 documents (the device sorts every row by counting, O(N^2))")
    if not pair:
        lo, hi = _range(references)
        if lo < 0 or hi >= K:
            raise ValueError(f"references: every label must be in [0, {K}) (found {lo} .. {hi})")
    if exits is not None:
        if _shape(exits) != (N,):
            raise ValueError(f"exits: shape ({N},), not {_shape(exits)}")
        lo, hi = _range(exits)
        if lo < 0 or hi >= E1:
            raise ValueError(f"exits: every exit must be in [0, {E1}) (found {lo} .. {hi})")
    T_host = None
    if temperatures is not None:
        T_host = (temperatures.detach().cpu().numpy() if _is_tensor(temperatures) else np.asarray(temperatures)).astype(np.float64).reshape(-1)
        if T_host.shape != (E1,):
            raise ValueError(f"temperatures: shape ({E1},), not {T_host.shape}")
        if not (np.isfinite(T_host).all() and (T_host > 0).all()):
            raise ValueError("temperatures must be finite and positive")
    bins = 0 if n_bins is None else int(n_bins)
    if n_bins is not None and not 1 <= bins <= 1024:
        raise ValueError(f"n_bins = {n_bins}: 1 .. 1024 (default: max(1, min(N - 1, 100)))")

    lib = capi.load()
    dev = _require_torch_cuda(device)
    L = refs = cf = cr = None
    if pair:
        cf, cr = _f64_on(dev, logits[0]).reshape(E1, N), _on(dev, logits[1], torch.uint8).reshape(E1, N)
    else:
        L, refs = _f64_on(dev, logits).reshape(E1, N, K), _on(dev, references, torch.int64)
    T = torch.from_numpy(T_host).to(dev) if T_host is not None else None
    ex = _on(dev, exits, torch.int32) if exits is not None else None
    R = E1 + (1 if ex is not None else 0)
    out = torch.empty((R, capi.METRIC_COUNT), dtype=torch.float64, device=dev)
    cm = torch.empty((R, K, K), dtype=torch.int64, device=dev) if want_confusion else None
    hist = torch.empty((E1,), dtype=torch.int64, device=dev) if ex is not None else None
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        capi.check(lib.ee_exit_metrics(_ptr(L), _ptr(refs), _ptr(cf), _ptr(cr), _ptr(T), _ptr(ex), E1, N, K, bins, _ptr(out), _ptr(cm), _ptr(hist),
                                       stream), None, "ee_exit_metrics")
    o = out.cpu().numpy()
    cols = {name: np.ascontiguousarray(o[:, getattr(capi, code)]) for name, code in zip(FIELDS, _CODES)}
    return ExitReport(num_samples=int(N), exit_hist=hist.cpu().numpy() if hist is not None else None,
                      confusion=cm.cpu().numpy() if cm is not None else None, policy=E1 if ex is not None else None, **cols)


_CODES = ("METRIC_ACCURACY", "METRIC_BRIER", "METRIC_NLL", "METRIC_F1_MICRO", "METRIC_F1_MACRO", "METRIC_ECE", "METRIC_AURC", "METRIC_AVG_CONF")
