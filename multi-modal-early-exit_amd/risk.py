"""Risk-controlled exit thresholds (the definition is in include/mmee.h, "Risk control"; the kernels in csrc/risk_control.hip).

``threshold_sweep``, ``threshold_search`` (also with ``cost=``), ``threshold_refine`` and ``QuotaScan.thresholds()`` return the point that
looks best on the table they were given.  ``risk_control`` says what a point promises on the next batch: the user states a risk level
``alpha`` and a failure probability ``delta``, hands over a list of candidate threshold vectors ordered from the most conservative to the
most aggressive, and gets the cheapest one whose risk is at most ``alpha`` with probability at least ``1 - delta`` over the draw of the
calibration table -- Learn-then-Test (Angelopoulos et al. 2021) with fixed-sequence testing, as CATs (Schuster et al., EMNLP 2021) and
"Fast yet Safe" (Jazbec et al., NeurIPS 2024) use it; along a front found on other data (``path_from_front``) it is Pareto testing
(Laufer-Goldshtein et al. 2023).

The promise holds if the calibration documents are exchangeable with the documents served and the candidate list was fixed without looking at
the calibration table.  A front searched on the same table does not qualify: split the table, search on one part, certify on the other.  The
risk is marginal over all documents; a document that runs to the final exit contributes its final-exit loss.

``rolling_control`` replays the online controller (``EarlyExitEngine.set_controller``; include/mmee.h, "Online exit control") on a dumped
table before deployment: the same kernels' arithmetic, group by group, in one launch.  Its promise needs no exchangeability -- it is an
inequality on the observed sequence -- and is about the audited estimate only.

Not built: the WSR betting bound, conditional (per-exit) risk control, several risks at once, a ranked scorer for millions of vectors, and
patience / rule / learning-to-exit / gate decisions (a gate or LTE table can be passed as a precomputed table, with plain-threshold semantics).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import capi
from .engine import ControllerLog, _require_torch_cuda, torch
from .policy import _f64_on, _on, _ptr, threshold_criterion
from .sweep import RefineResult, SearchResult, _stream, csf_table, final_predictions

LOSS_ONE = 1 << 30                              # a loss of 1 in the units of the integer table
_BOUNDS = {"binomial": capi.RISK_BINOMIAL, "hb": capi.RISK_HB}
_METHODS = {"fixed_sequence": capi.RISK_FIXED_SEQUENCE, "bonferroni": capi.RISK_BONFERRONI}
_RISKS = ("error", "consistency", "gap")


def binomial_bounds(n, k, delta: float, device=None):
    """One-sided Clopper-Pearson bounds, each at ``delta``, of ``k`` events in ``n`` trials (ee_binomial_bounds): ``(upper, lower)``, floats for
    scalar counts and float64 arrays (Q,) for arrays.  ``P(theta <= upper) >= 1 - delta`` and ``P(theta >= lower) >= 1 - delta``, each on its
    own.  64 bisections on the device; the same counts give the same bits."""
    scalar = np.ndim(n) == 0 and np.ndim(k) == 0
    na, ka = np.broadcast_arrays(np.atleast_1d(np.asarray(n)), np.atleast_1d(np.asarray(k)))
    if na.ndim != 1 or na.dtype.kind not in "iu" or ka.dtype.kind not in "iu":
        raise ValueError("binomial_bounds: n and k are integers or integer arrays (Q,)")
    if na.size and (int(na.min()) < 1 or int(na.max()) >= 1 << 24 or int(ka.min()) < 0 or bool((ka > na).any())):
        raise ValueError("binomial_bounds: need 1 <= n < 2^24 and 0 <= k <= n in every query")
    Q = int(na.size)
    lib = capi.load()
    dev = _require_torch_cuda(device)
    nc, kc = (C.c_int32 * Q)(*[int(x) for x in na]), (C.c_int32 * Q)(*[int(x) for x in ka])
    up = torch.empty((Q,), dtype=torch.float64, device=dev)
    lo = torch.empty((Q,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        capi.check(lib.ee_binomial_bounds(nc, kc, Q, float(delta), _ptr(up), _ptr(lo), _stream()), None, "ee_binomial_bounds")
    both = torch.stack([up, lo]).cpu().numpy()
    return (float(both[0, 0]), float(both[1, 0])) if scalar else (both[0], both[1])


@dataclass
class RiskResult:
    """What ``risk_control`` found: one row per candidate vector, numpy on the host.  ``thresholds`` are REAL thresholds of the criterion, so
    that a row goes to ``forward(thresholds=)`` unchanged."""
    thresholds: np.ndarray                  # (V, E1), in the caller's order
    loss_sum: np.ndarray                    # (V,) uint64, units of 2^-30
    exit_sum: np.ndarray                    # (V,) int64
    cost_sum: np.ndarray                    # (V,) uint64; = exit_sum without a cost
    risk: np.ndarray                        # (V,) loss_sum / (N 2^30): the empirical risk on the calibration table
    pvalue: np.ndarray                      # (V,) of H0: risk(v) > alpha
    certified: np.ndarray                   # (V,) bool
    n_certified: int
    selected: int                           # the certified vector of least cost_sum, ties to the lowest index; -1 when none is certified
    num_samples: int
    alpha: float
    delta: float
    bound: str                              # "binomial" / "hb"
    method: str                             # "fixed_sequence" / "bonferroni"
    binary: bool                            # the loss table holds only 0 and 1
    hist: Optional[np.ndarray] = None       # (V, E1) int32 exit histograms (``want_hist=True``)

    def select(self):
        """The selected vector as a plain list of E1 floats (what ``EarlyExitEngine.forward(thresholds=)`` takes).  ``ValueError`` when nothing is
        certified."""
        if self.selected < 0:
            V = len(self.pvalue)
            level = self.delta / V if self.method == "bonferroni" else self.delta
            need = int(math.ceil(math.log(level) / math.log1p(-self.alpha)))
            raise ValueError(f"no candidate is certified at alpha = {self.alpha}, delta = {self.delta} ({self.method}, {V} candidates, "
                             f"N = {self.num_samples}; first p-value {self.pvalue[0]:.3g}): even a vector without a single loss needs "
                             f"N >= ceil(log({level:.3g}) / log(1 - alpha)) = {need} calibration documents to pass")
        return self.thresholds[self.selected].tolist()

    def upper_bound(self, v: Optional[int] = None, delta: Optional[float] = None) -> float:
        """The one-sided Clopper-Pearson upper bound (``binomial_bounds``) on the risk of vector ``v`` (default: the selected one) at ``delta``
        (default: the call's), for a binary loss.  It is a statement about that one vector taken alone, not about the selection."""
        if not self.binary:
            raise ValueError("upper_bound is the binomial bound: the loss table is not binary")
        v = self.selected if v is None else int(v)
        if not 0 <= v < len(self.loss_sum):
            raise IndexError(f"vector {v} of {len(self.loss_sum)}" if v >= 0 else "nothing is selected")
        return binomial_bounds(self.num_samples, int(self.loss_sum[v]) >> 30, self.delta if delta is None else delta)[0]


def path_from_front(result):
    """The front of a ``SearchResult`` (``threshold_search``, also with ``cost=``) or of a ``RefineResult`` as candidates (F,E1) for
    ``risk_control(thresholds=)``, deepest first: from the entry of highest cost and accuracy to the cheapest.  Certifying along it is Pareto
    testing -- valid only when the front was searched on OTHER documents than the ones ``risk_control`` sees."""
    if isinstance(result, SearchResult):
        return np.ascontiguousarray(result.front_thresholds[::-1], dtype=np.float64)
    if isinstance(result, RefineResult):
        return np.ascontiguousarray(result.thresholds[result.front()[::-1]], dtype=np.float64)
    raise ValueError("path_from_front takes a SearchResult or a RefineResult")


def _candidates(lambdas, thresholds, E1, sign, criterion):
    if lambdas is not None and thresholds is not None:
        raise ValueError("give the candidates as lambdas (G,) or as thresholds (V,E1), not both")
    if thresholds is not None:
        th = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64))
        if th.ndim != 2 or th.shape[1] != E1 or th.shape[0] < 1:
            raise ValueError(f"thresholds: an array (V,{E1}), V >= 1, most conservative first")
        return th
    if lambdas is None:
        if sign < 0:
            raise ValueError(f'criterion "{criterion}" has no default candidates (its range depends on the number of labels): pass lambdas, '
                             "rising from the most conservative threshold")
        lambdas = np.linspace(1.0, 0.0, 101)
    lam = np.asarray(lambdas, dtype=np.float64).reshape(-1)
    if lam.size < 1 or not np.all(np.isfinite(lam)) or (lam.size > 1 and not np.all(sign * np.diff(lam) < 0)):
        raise ValueError("lambdas must move strictly towards the aggressive side: falling for max_confidence / margin, rising for entropy")
    return np.array(np.broadcast_to(lam[:, None], (lam.size, E1)))       # a copy: contiguous and writable


def risk_control(logits, references=None, *, criterion="max_confidence", risk: str = "consistency", loss=None, alpha: float, delta: float,
                 lambdas=None, thresholds=None, method: str = "fixed_sequence", bound: Optional[str] = None, cost=None, want_hist: bool = False,
                 device=None) -> RiskResult:
    """Certify candidate thresholds on a calibration table (ee_risk_control; include/mmee.h): every candidate is scored under the forward's own
    rule (strict test, the final exit as fall-back), gets the p-value of "its risk exceeds ``alpha``", and the cheapest certified one is selected.

    ``logits`` (E1,N,K) -- a dumped array, or ``AuditSample.logits`` --, or a precomputed pair ``(table, correct)`` as
    ``csf_table(..., as_csf=True)`` returns it and ``threshold_search`` accepts it (``references`` is then not read; ``correct`` may be None
    with ``loss=``).  ``risk`` chooses the loss of leaving at exit e, built on the device from ``csf_table``'s ``correct``:
    ``"error"`` -- ``1 - correct``, needs labels as ``references``; ``"consistency"`` -- the same against the full model's own answers,
    ``references`` default to ``final_predictions(logits)``: label-free; ``"gap"`` -- 1 where exit e is wrong and the final exit is right,
    needs labels.  These are binary and use the exact binomial p-value by default.  ``loss``: any float table (E1,N) with values in [0,1]
    instead (then ``risk`` is not read); it defaults to ``bound="hb"``, the Hoeffding-Bentkus p-value.

    Candidates: ``lambdas`` (G,) -- one threshold shared by every exit, strictly monotone towards the aggressive side; the default
    ``np.linspace(1, 0, 101)`` serves max-confidence and margin, entropy must pass its own -- or ``thresholds`` (V,E1), an explicit path, most
    conservative first (``path_from_front``).  ``method``: ``"fixed_sequence"`` -- certified while every earlier candidate passed at
    ``delta`` -- or ``"bonferroni"`` -- every candidate on its own at ``delta / V``.  ``cost``: as in ``threshold_search`` ((E1,) or (E1,N)
    integers below 2^32); without it the cost is the exit index.  ``want_hist`` also returns every candidate's exit histogram."""
    st = threshold_criterion(criterion)
    if method not in _METHODS:
        raise ValueError(f'method "{method}": choose "fixed_sequence" or "bonferroni"')
    if bound is not None and bound not in _BOUNDS:
        raise ValueError(f'bound "{bound}": choose "binomial" or "hb"')
    if loss is None and risk not in _RISKS:
        raise ValueError(f'risk "{risk}": choose "error", "consistency" or "gap", or pass a loss table')
    if not (0.0 < float(alpha) < 1.0 and 0.0 < float(delta) < 1.0):
        raise ValueError("alpha and delta must lie in (0, 1)")
    pair = isinstance(logits, tuple)
    if pair and len(logits) != 2:
        raise ValueError("a precomputed table is the pair (table (E1,N), correct (E1,N))")
    sign = -1.0 if st.value == "entropy" else 1.0
    lib = capi.load()
    dev = _require_torch_cuda(device)
    if pair:
        table = _f64_on(dev, logits[0])
        if sign < 0:
            table = -table                                              # as_csf hands the entropy over negated: the real table back (exact)
        corr = None if logits[1] is None else _on(dev, logits[1], torch.uint8)
    else:
        L = _f64_on(dev, logits)
        if L.dim() != 3:
            raise ValueError("logits must have shape (num_exits + 1, num_samples, num_labels)")
        refs = references
        if loss is None:
            if refs is None and risk != "consistency":
                raise ValueError(f'risk "{risk}" needs labels as references')
            if refs is None:
                refs = final_predictions(L, device=dev)
        table, corr = csf_table(L, refs, criterion=st, device=dev)
    if table.dim() != 2:
        raise ValueError("table (E1,N)")
    E1, N = (int(x) for x in table.shape)
    loss_f = loss_q = None
    if loss is not None:
        loss_f = _f64_on(dev, loss)
        if tuple(loss_f.shape) != (E1, N):
            raise ValueError(f"loss: a float table ({E1},{N})")
        bound = bound or "hb"
    else:
        if corr is None or tuple(corr.shape) != (E1, N):
            raise ValueError("table (E1,N), correct (E1,N)")
        wrong = (corr == 0).to(torch.int32)
        if risk == "gap":
            wrong = wrong * (corr[E1 - 1:E1] != 0).to(torch.int32)
        loss_q = (wrong * LOSS_ONE).contiguous()                        # uint32 words, 0 or 2^30
        bound = bound or "binomial"
    th_host = _candidates(lambdas, thresholds, E1, sign, st.value)
    V = int(th_host.shape[0])
    if V > 65536:
        raise ValueError(f"{V} candidates: one call takes at most 65536")
    cs = None
    if cost is not None:
        cost_host = cost.cpu().numpy() if torch is not None and isinstance(cost, torch.Tensor) else np.asarray(cost)
        if cost_host.dtype.kind not in "iu":
            raise ValueError(f"cost: an integer array, not {cost_host.dtype} (round it in the unit you choose)")
        if cost_host.shape not in ((E1,), (E1, N)):
            raise ValueError(f"cost: shape ({E1},) or ({E1},{N}), not {cost_host.shape}")
        if cost_host.size and (int(cost_host.min()) < 0 or int(cost_host.max()) >= 1 << 32):
            raise ValueError("cost: every value must be in [0, 2^32)")
        c2 = cost_host if cost_host.ndim == 2 else np.broadcast_to(cost_host[:, None], (E1, N))
        cs = torch.from_numpy(np.ascontiguousarray(c2.astype(np.uint32)).view(np.int32)).to(dev)      # uint32 words
    th = torch.from_numpy(th_host).to(dev)
    sums = torch.empty((3, V), dtype=torch.int64, device=dev)           # loss_sum (uint64 words), exit_sum, cost_sum (uint64 words)
    hist = torch.empty((V, E1), dtype=torch.int32, device=dev) if want_hist else None
    pval = torch.empty((V,), dtype=torch.float64, device=dev)
    cert = torch.empty((V,), dtype=torch.uint8, device=dev)
    picked = torch.empty((2,), dtype=torch.int32, device=dev)           # n_certified, selected
    with torch.cuda.device(dev):
        capi.check(lib.ee_risk_control(_ptr(table), sign, _ptr(loss_f), _ptr(loss_q), _ptr(cs), E1, N, _ptr(th), V, float(alpha), float(delta),
                                       _BOUNDS[bound], _METHODS[method], _ptr(sums[0]), _ptr(sums[1]), _ptr(sums[2]), _ptr(hist), _ptr(pval),
                                       _ptr(cert), _ptr(picked[0:1]), _ptr(picked[1:2]), _stream()), None, "ee_risk_control")
    sums_h, picked_h = sums.cpu().numpy(), picked.cpu().numpy()
    loss_sum = sums_h[0].view(np.uint64)
    binary = loss is None or bound == "binomial"                         # the binomial bound refuses a table that is not 0 / 1
    return RiskResult(thresholds=th_host, loss_sum=loss_sum, exit_sum=sums_h[1], cost_sum=sums_h[2].view(np.uint64),
                      risk=loss_sum / (float(N) * LOSS_ONE), pvalue=pval.cpu().numpy(), certified=cert.cpu().numpy().astype(bool),
                      n_certified=int(picked_h[0]), selected=int(picked_h[1]), num_samples=N, alpha=float(alpha), delta=float(delta), bound=bound,
                      method=method, binary=binary, hist=None if hist is None else hist.cpu().numpy())


@dataclass
class RollingResult:
    """What ``rolling_control`` replayed: ``exits`` goes unchanged into ``metrics.exit_report(exits=)``; ``log`` has one row per group."""
    exits: "torch.Tensor"                   # (N,) int32 on the device: where every document left under its group's thresholds
    log: ControllerLog                      # numpy on the host
    position: float                         # the position after the last group
    alpha: float
    gamma: float
    start: float
    group_size: int

    def bound(self) -> float:
        """``start / gamma + 1 - alpha``: what ``log.excess(alpha)`` stays at or below at every prefix."""
        return self.start / self.gamma + 1.0 - self.alpha


def rolling_control(logits, path, *, criterion="max_confidence", alpha: float, gamma: float, group_size: int, fraction: float, seed: int = 0,
                    start: float = 0.0, bad=None, device=None) -> RollingResult:
    """Replay online exit control on a dumped table (ee_rolling_control; the definition is in include/mmee.h): consecutive groups of
    ``group_size`` documents play the forwards of an engine under ``set_audit(fraction)`` and ``set_controller(path, alpha=, gamma=, start=,
    seed=)``; group t audits its slots under ``seed + t``.  One launch, with the functions the forward's own launches call, so a forward's
    ``controller_log()`` and this replay of its concatenated dump-all table agree bit for bit.

    ``logits`` (E1,N,K), or a precomputed criterion table (E1,N) -- real thresholds' scale, e.g. ``sweep.gate_table`` -- with ``bad=``.
    ``path``: (V,E1), a ``RiskResult`` (its candidates; pass ``start=result.selected`` to begin where it certified) or a
    ``SearchResult`` / ``RefineResult`` through ``path_from_front``.  ``bad`` (E1,N) 0 / 1: delivering document n at exit e is a loss; ``None`` builds the
    consistency table on the device -- ``csf_table``'s ``correct`` against ``final_predictions``, as ``risk_control(risk="consistency")`` --
    and any other table is an offline what-if."""
    st = threshold_criterion(criterion)
    sign = -1.0 if st.value == "entropy" else 1.0
    if isinstance(path, RiskResult):
        path = path.thresholds
    elif isinstance(path, (SearchResult, RefineResult)):
        path = path_from_front(path)
    if not (0.0 < float(alpha) < 1.0):
        raise ValueError("alpha must lie in (0, 1)")
    if not (float(gamma) > 0.0 and math.isfinite(float(gamma))):
        raise ValueError("gamma must be positive and finite")
    if int(group_size) < 1:
        raise ValueError("group_size: a group holds at least one document")
    cut = capi.audit_cut(fraction)
    if cut < 1:
        raise ValueError("fraction 0 audits nobody: the controller would never step")
    lib = capi.load()
    dev = _require_torch_cuda(device)
    L = _f64_on(dev, logits)
    if L.dim() == 3:
        table, corr = csf_table(L, final_predictions(L, device=dev) if bad is None else None, criterion=st, device=dev)
        if bad is None:
            bad = corr == 0
    elif L.dim() == 2:
        table = L.contiguous()
        if bad is None:
            raise ValueError("a precomputed criterion table (E1,N) needs bad= (E1,N): there are no logits to build the consistency table from")
    else:
        raise ValueError("logits (E1,N,K), or a criterion table (E1,N) with bad=")
    E1, N = (int(x) for x in table.shape)
    bad_t = (_on(dev, bad, torch.uint8) != 0).to(torch.uint8).contiguous()
    if tuple(bad_t.shape) != (E1, N):
        raise ValueError(f"bad: a 0 / 1 table ({E1},{N})")
    th = np.ascontiguousarray(np.asarray(path, dtype=np.float64))
    if th.ndim != 2 or th.shape[1] != E1 or th.shape[0] < 2:
        raise ValueError(f"path: an array (V,{E1}), V >= 2, most conservative first")
    if not np.all(np.isfinite(th)):
        raise ValueError("path: every entry must be finite")
    V, G = int(th.shape[0]), min(int(group_size), N)
    if not 0.0 <= float(start) <= V - 1:
        raise ValueError(f"start {start} outside [0, V - 1 = {V - 1}]")
    T = (N + G - 1) // G
    W = capi.controller_log_words(E1)
    th_dev = torch.from_numpy(th).to(dev)
    exits = torch.empty((N,), dtype=torch.int32, device=dev)
    log = torch.empty((T, W), dtype=torch.int64, device=dev)
    pos = torch.empty((1,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        capi.check(lib.ee_rolling_control(_ptr(table), sign, _ptr(bad_t), E1, N, _ptr(th_dev), V, cut, int(seed) & 0xFFFFFFFF, float(alpha),
                                          float(gamma), float(start), G, _ptr(exits), _ptr(log), _ptr(pos), _stream()), None, "ee_rolling_control")
    return RollingResult(exits=exits, log=ControllerLog.from_rows(log.cpu().numpy(), E1), position=float(pos.cpu().numpy()[0]), alpha=float(alpha),
                         gamma=float(gamma), start=float(start), group_size=G)
