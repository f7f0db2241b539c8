"""Device-side multi-threshold search: the counterpart of EE/thresh.py:184-215 / EE/large_scale.py:42-128.

The reference builds a CSF table ``msp = max softmax`` of the dumped logits once, derives candidate threshold vectors
from its percentiles, and then, for every threshold vector, computes ``(CSF >= thr[:, None]).argmax(0)`` and the
accuracy / mean exit of the induced exits in an 8-process CPU pool.  Here the table stays in HBM and one workgroup
handles one threshold vector.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .engine import _require_torch_cuda, torch
from .policy import _f64_on, _on, _ptr


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def msp_table(logits, references=None, device=None):
    """(conf float64 (E1,N), correct uint8 (E1,N) | None) on the device from logits (E1,N,K)."""
    lib = capi.load()
    dev = _require_torch_cuda(device)
    L = _f64_on(dev, logits)
    E1, N, K = L.shape
    conf = torch.empty((E1, N), dtype=torch.float64, device=dev)
    refs = corr = None
    if references is not None:
        refs = _on(dev, references, torch.int64)
        corr = torch.empty((E1, N), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        capi.check(lib.ee_msp_table(_ptr(L), _ptr(refs), E1, N, K, _ptr(conf), _ptr(corr), _stream()), None, "ee_msp_table")
    return conf, corr


def csf_table(logits, references=None, criterion="max_confidence", as_csf: bool = False, device=None):
    """The table of one of the three confidence scoring functions (CSF_dict, EE/thresh.py:55-61) on the device (ee_csf_table):
    ``(table float64 (E1,N), correct uint8 (E1,N) | None)`` from logits (E1,N,K).  ``criterion``: "max_confidence" (``msp_table`` bit for bit),
    "entropy" (the reference's ``log A - B / A``, lower is surer) or "margin" (include/mmee.h MMEE_CRIT_MARGIN).  ``as_csf=True`` returns the
    value the reference thresholds with ``>=`` -- the entropy negated (exact), the other two unchanged -- so that ``threshold_sweep`` and
    ``rule_sweep`` (sign +1) take the table directly."""
    from .policy import threshold_criterion
    st = threshold_criterion(criterion)
    lib = capi.load()
    dev = _require_torch_cuda(device)
    L = _f64_on(dev, logits)
    if L.dim() != 3:
        raise ValueError("logits must have shape (num_exits + 1, num_samples, num_labels)")
    E1, N, K = L.shape
    table = torch.empty((E1, N), dtype=torch.float64, device=dev)
    refs = corr = None
    if references is not None:
        refs = _on(dev, references, torch.int64)
        if tuple(refs.shape) != (N,):
            raise ValueError("references (N,)")
        corr = torch.empty((E1, N), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        capi.check(lib.ee_csf_table(_ptr(L), _ptr(refs), E1, N, K, st.code, _ptr(table), _ptr(corr), _stream()), None, "ee_csf_table")
    if as_csf and st.value == "entropy":
        table = -table
    return table, corr


def patience_sweep(logits, references, patiences, want_hist: bool = False, device=None):
    """Every patience value of ``patiences`` (V,) over one dumped array ``logits`` (E1,N,K) with labels ``references`` (N,): for each t the
    exits of the patience policy (include/mmee.h), the accuracy of the predictions at those exits and the mean exit (ee_patience_sweep: the
    run sequence of a document is computed once for all t; integer sums, deterministic).  Returns device tensors
    ``(accuracy (V,), mean_exit (V,), hist (V,E1) | None)``."""
    from .config import check_patience
    lib = capi.load()
    dev = _require_torch_cuda(device)
    pats = [check_patience(t) for t in np.asarray(patiences).reshape(-1).tolist()]
    L, refs = _f64_on(dev, logits), _on(dev, references, torch.int64)
    if L.dim() != 3 or tuple(refs.shape) != (L.shape[1],):
        raise ValueError("logits (E1,N,K), references (N,)")
    E1, N, K = L.shape
    V = len(pats)
    pt = torch.tensor(pats, dtype=torch.int32, device=dev)
    acc = torch.empty((V,), dtype=torch.float64, device=dev)
    mex = torch.empty((V,), dtype=torch.float64, device=dev)
    hist = torch.empty((V, E1), dtype=torch.int32, device=dev) if want_hist else None
    with torch.cuda.device(dev):
        capi.check(lib.ee_patience_sweep(_ptr(L), _ptr(refs), E1, N, K, _ptr(pt), V, _ptr(acc), _ptr(mex), _ptr(hist), _stream()), None,
                   "ee_patience_sweep")
    return acc, mex, hist


def rule_sweep(criterion, logits, references, thresholds, patiences, rule, sign: float = 1.0, want_hist: bool = False, device=None):
    """V threshold vectors x P patience values of a combined exit rule ("patient_confident" / "patience_or_threshold", include/mmee.h
    MMEE_RULE_*) in one call (ee_rule_sweep), with the POLICY's semantics -- strict compares, the final exit when nothing qualifies -- as
    ``patience_sweep`` follows its policy's, not ``threshold_sweep``'s ``>=`` / exit 0.  ``criterion`` (E1,N): ``msp_table(logits)[0]`` or any
    other criterion table; ``sign`` +1: the test is ``criterion > threshold``, -1: ``criterion < threshold`` (table and thresholds are
    negated, which is exact); ``logits`` (E1,N,K), ``references`` (N,), ``thresholds`` (V,E1), ``patiences`` (P,) integers >= 1, each used at
    every exit.  A document's streak is walked once per threshold vector; every patience value is a lookup.  Returns device tensors
    ``(accuracy (V,P), mean_exit (V,P), hist (V,P,E1) | None)``, all from integer sums."""
    from .config import ExitRule, check_patience
    r = rule if isinstance(rule, ExitRule) else ExitRule(str(rule))
    if r == ExitRule.PLAIN:
        raise ValueError('rule_sweep evaluates "patient_confident" and "patience_or_threshold"')
    if float(sign) not in (1.0, -1.0):
        raise ValueError("sign must be +1 or -1")
    lib = capi.load()
    dev = _require_torch_cuda(device)
    pats = [check_patience(t) for t in np.asarray(patiences).reshape(-1).tolist()]
    cf, L, refs, th = _f64_on(dev, criterion), _f64_on(dev, logits), _on(dev, references, torch.int64), _f64_on(dev, thresholds)
    if L.dim() != 3 or tuple(cf.shape) != tuple(L.shape[:2]) or tuple(refs.shape) != (L.shape[1],) or th.dim() != 2 or th.shape[1] != L.shape[0]:
        raise ValueError("criterion (E1,N), logits (E1,N,K), references (N,), thresholds (V,E1)")
    if float(sign) < 0:
        cf, th = -cf, -th
    E1, N, K = L.shape
    V, P = th.shape[0], len(pats)
    pt = (C.c_int32 * P)(*pats)
    acc = torch.empty((V, P), dtype=torch.float64, device=dev)
    mex = torch.empty((V, P), dtype=torch.float64, device=dev)
    hist = torch.empty((V, P, E1), dtype=torch.int32, device=dev) if want_hist else None
    with torch.cuda.device(dev):
        capi.check(lib.ee_rule_sweep(_ptr(cf), _ptr(L), _ptr(refs), E1, N, K, _ptr(th), V, pt, P, r.code, _ptr(acc), _ptr(mex), _ptr(hist),
                                     _stream()), None, "ee_rule_sweep")
    return acc, mex, hist


def lte_sweep(scores, correct, thresholds, want_hist: bool = False, device=None):
    """Many LTE threshold vectors over one table of scores: ``threshold_sweep`` on ``-scores`` / ``-thresholds`` (negation is exact), so
    exits = (scores <= thr[v][:, None]).argmax(0) -- the first exit whose score is AT OR BELOW its threshold, exit 0 when none is.  The
    policy (``Policy.lte_policy``, the forward pass) is strict (``<``) and falls back to the LAST exit: the same strict / non-strict,
    first / last difference the reference's sweep (EE/thresh.py:184-215) has against its policy (EE/policy.py:33).  No kernel of its own.
    ``scores`` (E1,N), ``correct`` (E1,N), ``thresholds`` (V,E1); returns ``(accuracy (V,), mean_exit (V,), hist (V,E1) | None)``."""
    dev = _require_torch_cuda(device)
    return threshold_sweep(-_f64_on(dev, scores), correct, -_f64_on(dev, thresholds), want_hist=want_hist, device=dev)


def threshold_sweep(conf, correct, thresholds, want_hist: bool = False, device=None):
    """For each threshold vector v: exits = (conf >= thr[v][:, None]).argmax(0); returns device tensors
    ``(accuracy (V,), mean_exit (V,), hist (V,E1) | None)``."""
    lib = capi.load()
    dev = _require_torch_cuda(device)
    cf, cr, th = _f64_on(dev, conf), _on(dev, correct, torch.uint8), _f64_on(dev, thresholds)
    E1, N = cf.shape
    if th.dim() != 2 or th.shape[1] != E1 or tuple(cr.shape) != (E1, N):
        raise ValueError("conf (E1,N), correct (E1,N), thresholds (V,E1)")
    V = th.shape[0]
    acc = torch.empty((V,), dtype=torch.float64, device=dev)
    mex = torch.empty((V,), dtype=torch.float64, device=dev)
    hist = torch.empty((V, E1), dtype=torch.int32, device=dev) if want_hist else None
    with torch.cuda.device(dev):
        capi.check(lib.ee_threshold_sweep(_ptr(cf), _ptr(cr), E1, N, _ptr(th), V, _ptr(acc), _ptr(mex), _ptr(hist), _stream()), None,
                   "ee_threshold_sweep")
    return acc, mex, hist
