"""Audited exits, the reading side (the definition is in include/mmee.h; the forward's side is ``EarlyExitEngine.set_audit``).

An audited call with ``want_all=True`` returns, for the hashed sample ``output.audit_mask`` of its documents, every exit's row: a sampled
dump-all table of the traffic that was served.  ``sample`` gathers those columns, ``AuditSample.concat`` accumulates them over calls, and
``consistency`` counts what the early-exit literature controls and a thresholded forward throws away: how often the answer a document was
delivered with is the answer the full model gives it (the consistency of CATs, Schuster et al., EMNLP 2021; the risk of "Fast yet Safe",
Jazbec et al., NeurIPS 2024).

``AuditSample.logits`` is an ordinary (E1,n,K) dumped array: ``sweep.csf_table``, ``sweep.threshold_search``, ``sweep.threshold_refine``,
``metrics.exit_report``, ``calibration.fit_temperatures`` and ``heads.fit_exit_ensemble`` take it unchanged.  Those tools score against
references; live traffic has none, and ``AuditSample.references()`` -- the final exit's own predictions, ``sweep.final_predictions`` -- makes
"correct" read "agrees with the full model".

Plain torch ops on the device and one small download per report.  ``consistency(x, delta=)`` adds a one-sided Clopper-Pearson lower bound on
every agreement rate (``risk.binomial_bounds``, one launch), and ``certify`` hands the sample to ``risk.risk_control``: thresholds whose
disagreement with the full model is at most ``alpha`` with probability ``1 - delta``.  Not built: a selection that depends on content, a
per-exit share, audits under quotas, result streams, captured graphs or cascade stages, and bounds that hold for all exits at once.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from .engine import EngineOutput, torch


@dataclass
class AuditSample:
    """The audited documents of one or more calls: device tensors, n documents."""
    index: "torch.Tensor"                   # (n,)  int64   -- the documents' slots in their call (``concat``: each call's own numbering)
    logits: "torch.Tensor"                  # (E1,n,K) float32 -- the selected columns of ``all_logits``, complete
    crit: "torch.Tensor"                    # (E1,n) float32 -- the selected columns of ``all_crit``
    exit_layer: "torch.Tensor"              # (n,)  int32   -- where each document was delivered

    @property
    def num_samples(self) -> int:
        return int(self.index.shape[0])

    def references(self) -> "torch.Tensor":
        """(n,) int64: the final exit's predictions, lowest index on ties -- the references of a label-free table."""
        from .sweep import first_argmax
        return first_argmax(self.logits[-1])

    @staticmethod
    def concat(samples: Sequence["AuditSample"]) -> "AuditSample":
        samples = list(samples)
        if not samples:
            raise ValueError("AuditSample.concat: no samples")
        if any(s.logits.shape[0] != samples[0].logits.shape[0] or s.logits.shape[2] != samples[0].logits.shape[2] for s in samples):
            raise ValueError("AuditSample.concat: the samples come from models with different exits or labels")
        return AuditSample(torch.cat([s.index for s in samples], 0), torch.cat([s.logits for s in samples], 1),
                           torch.cat([s.crit for s in samples], 1), torch.cat([s.exit_layer for s in samples], 0))


def sample(out: EngineOutput) -> AuditSample:
    """The audited columns of an audited ``forward(..., want_all=True)``: an index gather on the device, in ascending slot order."""
    if out.audit_mask is None:
        raise ValueError("audit.sample: the call was not audited (set_audit / audit_fraction=; a dump-all call ignores the audit)")
    if out.all_logits is None or out.all_crit is None:
        raise ValueError("audit.sample: the audited columns live in all_logits / all_crit: run the forward with want_all=True")
    idx = torch.nonzero(out.audit_mask, as_tuple=False).reshape(-1)
    return AuditSample(idx, out.all_logits.index_select(1, idx), out.all_crit.index_select(1, idx), out.exit_layer.index_select(0, idx))


@dataclass
class ConsistencyReport:
    """Agreement of the delivered answer with the full model's, per exit below the final one and pooled.  numpy on the host."""
    delivered: np.ndarray                   # (E,) int64: audited documents delivered at exit e
    agree: np.ndarray                       # (E,) int64: of those, argmax(delivered row) == argmax(final row), lowest index on ties
    rate: np.ndarray                        # (E,) agree / delivered, NaN where nobody was delivered
    num_samples: int                        # audited documents, those that reached the final exit by themselves included
    pooled_delivered: int = 0
    pooled_agree: int = 0
    pooled_rate: float = float("nan")
    # ``consistency(x, delta=)`` only: 1 - the one-sided Clopper-Pearson upper bound, at delta, of the disagreements among the delivered.  Each
    # entry holds with probability 1 - delta ON ITS OWN: there is no correction across the exits, nor between them and the pooled figure
    rate_lower: Optional[np.ndarray] = None     # (E,), NaN where nobody was delivered
    pooled_rate_lower: Optional[float] = None


def _with_bounds(rep: ConsistencyReport, delta) -> ConsistencyReport:
    """``rep`` with ``rate_lower`` / ``pooled_rate_lower`` at ``delta``: one ``binomial_bounds`` call over the exits that delivered anybody and
    the pooled counts."""
    if delta is None:
        return rep
    from .risk import binomial_bounds
    rep.rate_lower, rep.pooled_rate_lower = np.full(rep.delivered.shape, np.nan), float("nan")
    n = np.append(rep.delivered, rep.pooled_delivered).astype(np.int64)
    k = n - np.append(rep.agree, rep.pooled_agree).astype(np.int64)
    at = np.nonzero(n > 0)[0]
    if len(at):
        lower = 1.0 - binomial_bounds(n[at], k[at], delta)[0]
        E = len(rep.delivered)
        rep.rate_lower[at[at < E]] = lower[at < E]
        if n[E] > 0:
            rep.pooled_rate_lower = float(lower[-1])
    return rep


def certify(sample: AuditSample, alpha: float, delta: float, **kw):
    """``risk.risk_control`` on the audited table with the label-free risk: the cheapest of the candidate thresholds (``lambdas=`` /
    ``thresholds=``; every other keyword of ``risk_control`` passes through) whose answers disagree with the full model's on at most ``alpha``
    of the documents, with probability at least ``1 - delta`` over the audited sample.  The sample must be exchangeable with the traffic to be
    served, and the candidates fixed without looking at it."""
    from .risk import risk_control
    return risk_control(sample.logits, risk="consistency", alpha=alpha, delta=delta, **kw)


def consistency(out_or_sample, delta: Optional[float] = None) -> ConsistencyReport:
    """``ConsistencyReport`` of an audited output (``want_all=True``) or of an ``AuditSample``.  A document delivered at the final exit is the
    full model's answer by construction and is counted in ``num_samples`` only.  Counts and rates; with ``delta`` also ``rate_lower`` (E,) and
    ``pooled_rate_lower``: 1 - the one-sided Clopper-Pearson upper bound of the disagreements at ``delta`` each, with no correction across
    the exits.  Without ``delta`` the report and its single download are what they were before the bounds existed."""
    from .sweep import first_argmax
    s = out_or_sample if isinstance(out_or_sample, AuditSample) else sample(out_or_sample)
    E1, n, _ = s.logits.shape
    E = E1 - 1
    if n == 0 or E == 0:
        z = np.zeros((E,), dtype=np.int64)
        return _with_bounds(ConsistencyReport(z, z.copy(), np.full((E,), np.nan), int(n)), delta)
    ex = s.exit_layer.to(torch.int64)
    early = ex < E
    row = s.logits[ex.clamp(max=E), torch.arange(n, device=ex.device)]                     # (n,K): the row each document was delivered with
    same = (first_argmax(row) == first_argmax(s.logits[E])) & early
    count = lambda m: torch.bincount(ex, weights=m.to(torch.float64), minlength=E1)[:E]     # exact: whole numbers far below 2^53
    counts = torch.stack([count(early), count(same)]).cpu().numpy().astype(np.int64)         # the one download
    d, a = counts[0], counts[1]
    with np.errstate(invalid="ignore", divide="ignore"):
        rate = np.where(d > 0, a / np.maximum(d, 1), np.nan)
    pd, pa = int(d.sum()), int(a.sum())
    return _with_bounds(ConsistencyReport(d, a, rate, int(n), pd, pa, pa / pd if pd else float("nan")), delta)
