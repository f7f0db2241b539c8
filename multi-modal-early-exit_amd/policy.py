"""``Policy`` — same constructor, method names, config keys and return contract as EE/policy.py:7-111, evaluated on
the MI355X (ee_policy_scan) instead of a nested Python loop over N x (E+1) scipy softmaxes.

    policy = Policy(logits=logits, config=config)           # logits: np.ndarray (E+1, N, K)
    exits_store, predictions, exit_distribution = getattr(policy, config["exit_policy"])()     # EE/eval.py:91-98

Returns ``(np.int32 (N,), torch.float64 (N,K) on config["device"], {exit_id: fraction})`` exactly as the reference.
There is no CPU fallback: without the HIP library / a GPU the call raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import capi
from .engine import _require_torch_cuda, torch


def _on(dev, x, dtype):
    """``x`` (numpy array, tensor or sequence) as a contiguous tensor of ``dtype`` on ``dev``."""
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else torch.as_tensor(x)
    return t.to(dev, dtype=dtype).contiguous()


def _f64_on(dev, x):
    return _on(dev, x, torch.float64)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _threshold_vector(thresholds, E1):
    """A scalar or (E1,) thresholds as the ``double[E1]`` the C ABI reads."""
    thr = np.broadcast_to(np.asarray(thresholds, dtype=np.float64).reshape(-1), (E1,)) if np.ndim(thresholds) \
        else np.full((E1,), float(thresholds))
    return (C.c_double * E1)(*[float(t) for t in thr])


def _run_scan(name, dev, shape, want_conf, call):
    """Allocates the outputs of a scan over logits of ``shape`` (E1,N,K) and runs ``call(exits, pred, conf, counts, stream)`` -- the ctypes
    call of entry point ``name`` -- on the current stream of ``dev``.  Returns (exits, pred, conf | None, counts)."""
    E1, N, K = shape
    exits = torch.empty((N,), dtype=torch.int32, device=dev)
    pred = torch.empty((N, K), dtype=torch.float64, device=dev)
    conf = torch.empty((N,), dtype=torch.float64, device=dev) if want_conf else None
    counts = torch.zeros((E1,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = call(_ptr(exits), _ptr(pred), _ptr(conf), _ptr(counts), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    capi.check(rc, None, name)
    return exits, pred, conf, counts


def policy_scan_device(logits, thresholds, device=None, want_conf: bool = False):
    """First exit whose float64 max-softmax is strictly above its threshold, else the last exit.

    ``logits`` (E1,N,K) numpy / torch (any float dtype; evaluated as float64 like the harness' store,
    EE/utils.py:160-164); ``thresholds`` scalar or (E1,).  Returns device tensors (exits int32, predictions float64,
    confidence float64 | None, counts int32)."""
    lib = capi.load()
    dev = _require_torch_cuda(device)
    L = _f64_on(dev, logits)
    if L.dim() != 3:
        raise ValueError("logits must have shape (num_exits + 1, num_samples, num_labels)")
    E1, N, K = L.shape
    thr_c = _threshold_vector(thresholds, E1)
    return _run_scan("ee_policy_scan", dev, L.shape, want_conf,
                     lambda exits, pred, conf, counts, stream: lib.ee_policy_scan(_ptr(L), E1, N, K, thr_c, exits, pred, conf, counts, stream))


def threshold_criterion(criterion):
    """``criterion`` ("max_confidence" / "entropy" / "margin", or the enum) as an ``EarlyExitInference`` that has a threshold test on one
    logits row; patience, lte and unknown names are a ``ValueError``."""
    from .config import EarlyExitInference
    st = criterion if isinstance(criterion, EarlyExitInference) else EarlyExitInference(str(criterion))
    if st not in (EarlyExitInference.MAX_CONFIDENCE, EarlyExitInference.ENTROPY, EarlyExitInference.MARGIN):
        raise ValueError(f'criterion "{st}" is not a threshold criterion on a logits row: choose "max_confidence", "entropy" or "margin"')
    return st


def criterion_scan_device(logits, thresholds, criterion, device=None, want_conf: bool = False):
    """``policy_scan_device`` under any threshold criterion (ee_criterion_scan): the first exit whose float64 ``criterion`` ("max_confidence",
    "entropy", "margin"; include/mmee.h) strictly passes its threshold in the criterion's direction (``>``; entropy ``<``), else the last exit.
    Same inputs and returns; the confidence is the criterion at the chosen exit.  "max_confidence" is ``policy_scan_device`` bit for bit."""
    st = threshold_criterion(criterion)
    lib = capi.load()
    dev = _require_torch_cuda(device)
    L = _f64_on(dev, logits)
    if L.dim() != 3:
        raise ValueError("logits must have shape (num_exits + 1, num_samples, num_labels)")
    E1, N, K = L.shape
    thr_c = _threshold_vector(thresholds, E1)
    return _run_scan("ee_criterion_scan", dev, L.shape, want_conf,
                     lambda exits, pred, conf, counts, stream: lib.ee_criterion_scan(_ptr(L), E1, N, K, st.code, thr_c, exits, pred, conf, counts,
                                                                                     stream))


def patience_scan_device(logits, patience: int, device=None, want_conf: bool = False):
    """Patience (include/mmee.h MMEE_CRIT_PATIENCE) on a dumped array: the first exit where the argmax has stayed the same for ``patience``
    exits in a row, else the last exit.  Same inputs and returns as ``policy_scan_device`` (ee_patience_scan)."""
    from .config import check_patience
    t = check_patience(patience)
    lib = capi.load()
    dev = _require_torch_cuda(device)
    L = _f64_on(dev, logits)
    if L.dim() != 3:
        raise ValueError("logits must have shape (num_exits + 1, num_samples, num_labels)")
    E1, N, K = L.shape
    return _run_scan("ee_patience_scan", dev, L.shape, want_conf,
                     lambda exits, pred, conf, counts, stream: lib.ee_patience_scan(_ptr(L), E1, N, K, t, exits, pred, conf, counts, stream))


def lte_scan_device(scores, logits, thresholds, device=None):
    """Learning-to-exit (include/mmee.h ``use_lte``) on dumped arrays: the first exit e < E1 - 1 whose score is strictly below its threshold,
    else the last exit.  ``scores`` (E1,N) (rows of embedding-level exits hold 1.0), ``logits`` (E1,N,K), ``thresholds`` scalar or (E1,).
    Returns device tensors (exits int32, predictions float64, counts int32) (ee_lte_scan)."""
    lib = capi.load()
    dev = _require_torch_cuda(device)
    S, L = _f64_on(dev, scores), _f64_on(dev, logits)
    if L.dim() != 3 or tuple(S.shape) != tuple(L.shape[:2]):
        raise ValueError("scores must have shape (num_exits + 1, num_samples) and logits (num_exits + 1, num_samples, num_labels)")
    E1, N, K = L.shape
    thr_c = _threshold_vector(thresholds, E1)
    exits, pred, _, counts = _run_scan(
        "ee_lte_scan", dev, L.shape, False,
        lambda exits, pred, conf, counts, stream: lib.ee_lte_scan(_ptr(S), _ptr(L), E1, N, K, thr_c, exits, pred, counts, stream))
    return exits, pred, counts


def gate_scan_device(scores, logits, thresholds, device=None, want_conf: bool = False):
    """The gate decision (include/mmee.h MMEE_CRIT_GATE) on dumped arrays (ee_gate_scan): the first exit e < E1 - 1 whose gate score is strictly
    above its threshold, else the last exit.  ``scores`` (E1,N) (``sweep.gate_table``), ``logits`` (E1,N,K) (the policy logits,
    ``classifier(gate input)``), ``thresholds`` scalar or (E1,).  Returns device tensors (exits int32, predictions float64, confidence
    float64 | None = the table entry of the chosen exit, counts int32)."""
    lib = capi.load()
    dev = _require_torch_cuda(device)
    S, L = _f64_on(dev, scores), _f64_on(dev, logits)
    if L.dim() != 3 or tuple(S.shape) != tuple(L.shape[:2]):
        raise ValueError("scores must have shape (num_exits + 1, num_samples) and logits (num_exits + 1, num_samples, num_labels)")
    E1, N, K = L.shape
    thr_c = _threshold_vector(thresholds, E1)
    return _run_scan("ee_gate_scan", dev, L.shape, want_conf,
                     lambda exits, pred, conf, counts, stream: lib.ee_gate_scan(_ptr(S), _ptr(L), E1, N, K, thr_c, exits, pred, conf, counts, stream))


def rule_scan_device(criterion, logits, thresholds, patience, rule, sign: float = 1.0, device=None, want_conf: bool = False):
    """The combined exit rules (include/mmee.h MMEE_RULE_*) on dumped arrays (ee_rule_scan).  ``criterion`` (E1,N): the criterion table
    (``sweep.msp_table`` for max-softmax) or the LTE scores; ``sign`` +1: the test is ``criterion > threshold``, -1: ``criterion <
    threshold`` (entropy, LTE).  ``logits`` (E1,N,K); ``thresholds`` scalar or (E1,); ``patience`` an int or one entry per exit; ``rule``
    "patient_confident" (the test has held at ``patience`` exits in a row) or "patience_or_threshold" (the test fires, or the argmax has been
    the same for ``patience`` exits).  Returns device tensors (exits int32, predictions float64, confidence float64 | None = the criterion
    entry of the chosen exit, counts int32)."""
    from .config import ExitRule, check_patience_spec
    r = rule if isinstance(rule, ExitRule) else ExitRule(str(rule))
    if r == ExitRule.PLAIN:
        raise ValueError('rule_scan_device evaluates "patient_confident" and "patience_or_threshold"; "plain" is policy_scan_device')
    if float(sign) not in (1.0, -1.0):
        raise ValueError("sign must be +1 (criterion > threshold) or -1 (criterion < threshold)")
    lib = capi.load()
    dev = _require_torch_cuda(device)
    Cr, L = _f64_on(dev, criterion), _f64_on(dev, logits)
    if L.dim() != 3 or tuple(Cr.shape) != tuple(L.shape[:2]):
        raise ValueError("criterion must have shape (num_exits + 1, num_samples) and logits (num_exits + 1, num_samples, num_labels)")
    E1, N, K = L.shape
    t = check_patience_spec(patience, E1)
    pat_c = (C.c_int32 * E1)(*(t if isinstance(t, list) else [t] * E1))
    thr_c = _threshold_vector(thresholds, E1)
    return _run_scan("ee_rule_scan", dev, L.shape, want_conf,
                     lambda exits, pred, conf, counts, stream: lib.ee_rule_scan(_ptr(Cr), float(sign), _ptr(L), E1, N, K, thr_c, pat_c, r.code,
                                                                                exits, pred, conf, counts, stream))


class QuotaScan:
    """What ``quota_scan_device`` returns: ``exits`` (N,) int32 on the device -- it goes unchanged into ``metrics.exit_report(exits=)``,
    ``reach_weights`` and ``ExitReport.efficiency`` -- and ``cuts`` (groups, E1 - 1, 2) float64 on the device or ``None``: the criterion of the
    last leaver and of the first stayer of every group at every exit, NaN where there is none."""

    def __init__(self, exits, cuts, sign: float, group: int, quotas, mode: str):
        self.exits, self.cuts, self.sign, self.group, self.quotas, self.mode = exits, cuts, float(sign), int(group), list(quotas), mode

    def counts(self) -> np.ndarray:
        """The exit histogram (E1,) of ``exits``, on the host."""
        return np.bincount(self.exits.cpu().numpy(), minlength=len(self.quotas) + 1)

    def thresholds(self, group: int = 0) -> np.ndarray:
        """MSDNet's thresholds from the cuts of one group (scan a validation table with ``group_size = N``): per exit the midpoint between the
        criterion of the last leaver and of the first stayer, (E1,) float64 with the final exit's entry 0 (never read: the final exit takes
        everybody).  A plain thresholded forward with these releases, on the scanned table, exactly the scan's leavers (when no cut
        straddles a tie), and about that share of a like batch.  Where nobody left the threshold is the unreachable side of the
        criterion's direction (``sign * inf``), where nobody stayed the other one."""
        if self.cuts is None:
            raise ValueError("QuotaScan.thresholds: the scan ran with want_cuts=False")
        c = self.cuts[group].cpu().numpy()
        last, first = c[:, 0], c[:, 1]
        thr = 0.5 * (last + first)
        thr = np.where(np.isnan(last), self.sign * np.inf, np.where(np.isnan(first), -self.sign * np.inf, thr))
        return np.concatenate([thr, [0.0]])


def quota_scan_device(table, quotas, mode: str = "exact", thresholds=None, group_size: Optional[int] = None, sign: float = 1.0,
                      want_cuts: bool = True, device=None) -> QuotaScan:
    """Budgeted exits (include/mmee.h MMEE_QUOTA_*) on a criterion table (ee_quota_scan).  ``table`` (E1,N): the criterion of every document
    at every exit (``sweep.csf_table`` / ``sweep.gate_table`` / the table of an ensembled array); ``sign`` -1 for entropy, else +1;
    ``quotas``: one integer per exit below the last; ``mode`` "exact" or "at_least" (which needs ``thresholds``, scalar or (E1,));
    ``group_size`` G (default N): consecutive groups of G documents are ranked independently, as N / G forwards of G documents would be."""
    if str(mode) not in capi.QUOTA_MODES:
        raise ValueError(f'quota_scan_device: mode "{mode}" is neither "exact" nor "at_least"')
    if float(sign) not in (1.0, -1.0):
        raise ValueError("sign must be +1 (larger is more confident) or -1 (entropy)")
    lib = capi.load()
    dev = _require_torch_cuda(device)
    T = _f64_on(dev, table)
    if T.dim() != 2:
        raise ValueError("table must have shape (num_exits + 1, num_samples)")
    E1, N = T.shape
    q = [int(v) for v in np.asarray(quotas).reshape(-1)]
    if len(q) != E1 - 1:
        raise ValueError(f"quota_scan_device: {len(q)} quotas, the table has {E1 - 1} exits below the last one")
    if mode == "at_least" and thresholds is None:
        raise ValueError('quota_scan_device: mode "at_least" needs thresholds')
    G = N if group_size is None else int(group_size)
    if G < 1 and N > 0:
        raise ValueError("group_size must be >= 1")
    G = max(G, 1)
    groups = (N + G - 1) // G if N else 0
    exits = torch.empty((N,), dtype=torch.int32, device=dev)
    work = torch.empty((max(N, 1),), dtype=torch.int32, device=dev)
    cuts = torch.empty((groups, E1 - 1, 2), dtype=torch.float64, device=dev) if want_cuts else None
    q_c = (C.c_int32 * max(E1 - 1, 1))(*q)
    thr_c = None if thresholds is None else _threshold_vector(thresholds, E1)
    with torch.cuda.device(dev):
        rc = lib.ee_quota_scan(_ptr(T), float(sign), E1, N, q_c, capi.QUOTA_MODES[str(mode)], thr_c, G, _ptr(exits), _ptr(cuts), _ptr(work),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    capi.check(rc, None, "ee_quota_scan")
    return QuotaScan(exits, cuts, sign, G, q, str(mode))


class Policy:
    def __init__(self, logits, config) -> None:
        self.logits = logits
        self.config = config

    def _finish(self, thresholds=None, patience=None, lte_scores=None, rule=None, criterion=None, gate_scores=None):
        num_exits, num_samples = self.logits.shape[0], self.logits.shape[1]
        if gate_scores is not None:
            exits, pred, _, counts = gate_scan_device(gate_scores, self.logits, thresholds)
        elif rule is not None:
            if lte_scores is not None:
                crit, sign = lte_scores, -1.0
            else:
                from .sweep import csf_table
                st = threshold_criterion(criterion or "max_confidence")
                crit, sign = csf_table(self.logits, criterion=st)[0], (-1.0 if st.value == "entropy" else 1.0)
            exits, pred, _, counts = rule_scan_device(crit, self.logits, thresholds, patience, rule, sign=sign)
        elif criterion is not None:
            exits, pred, _, counts = criterion_scan_device(self.logits, thresholds, criterion)
        elif lte_scores is not None:
            exits, pred, counts = lte_scan_device(lte_scores, self.logits, thresholds)
        elif patience is not None:
            exits, pred, _, counts = patience_scan_device(self.logits, patience)
        else:
            exits, pred, _, counts = policy_scan_device(self.logits, thresholds)
        exits_store = exits.cpu().numpy().astype(np.int32)
        tgt = self.config.get("device", "cpu")
        predictions = pred.to(tgt) if str(tgt) != str(pred.device) else pred
        c = counts.cpu().numpy()
        exit_distribution = {exit_id: int(c[exit_id]) / num_samples for exit_id in range(0, num_exits)}
        return exits_store, predictions, exit_distribution

    def max_confidence_global_thresholding_policy(self):
        """EE/policy.py:12-53: one global threshold ``config["exit_threshold"]``."""
        return self._finish(float(self.config["exit_threshold"]))

    def _exit_thresholds(self, who):
        """``config["exit_thresholds"]`` (per exit) or the global ``config["exit_threshold"]``."""
        thr = self.config.get("exit_thresholds")
        if thr is None:
            if self.config.get("exit_threshold") is None:
                raise ValueError(f'{who} needs config["exit_thresholds"] (per exit) or config["exit_threshold"]')
            thr = float(self.config["exit_threshold"])
        return thr

    def entropy_global_thresholding_policy(self):
        """The thresholding policy under the entropy criterion (CSF "entropy", EE/thresh.py:41-45, 55-61): the first exit whose float64
        entropy ``log A - B / A`` is strictly BELOW its threshold, else the last.  Thresholds: ``config["exit_thresholds"]`` (per exit) or the
        global ``config["exit_threshold"]``.  ``config["exit_policy"] = "entropy_global_thresholding_policy"`` selects it through
        EE/eval.py:91-98's ``getattr`` dispatch."""
        return self._finish(self._exit_thresholds("entropy_global_thresholding_policy"), criterion="entropy")

    def margin_global_thresholding_policy(self):
        """The thresholding policy under the margin criterion (include/mmee.h MMEE_CRIT_MARGIN: top-1 minus top-2 softmax probability): the
        first exit whose float64 margin is strictly above its threshold, else the last.  Same configuration keys as
        ``entropy_global_thresholding_policy``."""
        return self._finish(self._exit_thresholds("margin_global_thresholding_policy"), criterion="margin")

    def patience_policy(self):
        """Patience-based early exit (PABEE; the reference declares it, EE/models/EE_modules.py:123-124, and implements no policy for it):
        ``config["patience"]`` = t >= 1, exit at the first e where the argmax has been the same for t exits in a row, else the last.
        ``config["exit_policy"] = "patience_policy"`` selects it through EE/eval.py:91-98's ``getattr`` dispatch."""
        if self.config.get("patience") is None:
            raise ValueError('patience_policy needs config["patience"] (an integer >= 1)')
        return self._finish(patience=self.config["patience"])

    def lte_policy(self):
        """Learning-to-exit (EE/models/LayoutLMv3.py:229-268 on dumped arrays): ``config["lte_scores"]`` (E1,N), the ``all_crit`` rows of a
        ``use_lte`` dump; exit at the first e before the last whose score is strictly below ``config["lte_thresholds"][e]`` (per exit) or,
        without that key, the global ``config["exit_threshold"]``.  ``config["exit_policy"] = "lte_policy"`` selects it through
        EE/eval.py:91-98's ``getattr`` dispatch."""
        if self.config.get("lte_scores") is None:
            raise ValueError('lte_policy needs config["lte_scores"] (the (num_exits + 1, num_samples) LTE scores of the dump)')
        thr = self.config.get("lte_thresholds")
        if thr is None:
            if self.config.get("exit_threshold") is None:
                raise ValueError('lte_policy needs config["lte_thresholds"] (per exit) or config["exit_threshold"]')
            thr = float(self.config["exit_threshold"])
        return self._finish(thr, lte_scores=self.config["lte_scores"])

    def gate_policy(self):
        """The gate decision (include/mmee.h MMEE_CRIT_GATE; the reference's design note EE/models/EE_modules.py:21-31, which its evaluation never
        runs) on dumped arrays: ``config["gate_scores"]`` (E1,N), ``sweep.gate_table`` of a gate handle's dump; exit at the first e before the
        last whose gate score is strictly above ``config["exit_thresholds"][e]`` (per exit) or the global ``config["exit_threshold"]``, else
        the last.  ``self.logits`` are the policy logits (``classifier(gate input)``), whose rows are the predictions.
        ``config["exit_policy"] = "gate_policy"`` selects it through EE/eval.py:91-98's ``getattr`` dispatch."""
        scores = self.config.get("gate_scores")
        if scores is None:
            raise ValueError('gate_policy needs config["gate_scores"] (the (num_exits + 1, num_samples) table of sweep.gate_table)')
        if tuple(np.shape(scores)) != tuple(self.logits.shape[:2]):
            raise ValueError(f'gate_policy: config["gate_scores"] has shape {tuple(np.shape(scores))}, the logits say '
                             f'{tuple(self.logits.shape[:2])} (num_exits + 1, num_samples)')
        return self._finish(self._exit_thresholds("gate_policy"), gate_scores=scores)

    def _rule_policy(self, rule):
        if self.config.get("patience") is None:
            raise ValueError(f'{rule}_policy needs config["patience"] (an integer >= 1, or one per exit)')
        lte = self.config.get("lte_scores")
        thr = self.config.get("lte_thresholds" if lte is not None else "exit_thresholds")
        if thr is None:
            if self.config.get("exit_threshold") is None:
                raise ValueError(f'{rule}_policy needs config["exit_thresholds"] (per exit) or config["exit_threshold"]')
            thr = float(self.config["exit_threshold"])
        return self._finish(thr, patience=self.config["patience"], lte_scores=lte, rule=rule, criterion=self.config.get("criterion", "max_confidence"))

    def patient_confident_policy(self):
        """Patient and confident (PCEE-BERT, Zhang et al. 2022; include/mmee.h MMEE_RULE_STREAK; the reference has no counterpart): exit at the
        first e where the confidence test ``max-softmax > threshold`` has held at ``config["patience"]`` exits in a row (an int, or one
        entry per exit), else the last.  Thresholds: ``config["exit_thresholds"]`` (per exit) or the global ``config["exit_threshold"]``.
        With ``config["lte_scores"]`` the test is the LTE one (``score < config["lte_thresholds"][e]`` or the global threshold).
        ``config["criterion"]`` ("max_confidence", the default; "entropy"; "margin") picks the table and the direction of the test
        (``sweep.csf_table``).
        ``config["exit_policy"] = "patient_confident_policy"`` selects it through EE/eval.py:91-98's ``getattr`` dispatch."""
        return self._rule_policy("patient_confident")

    def patience_or_threshold_policy(self):
        """Patience or threshold (PABEE's hybrid; include/mmee.h MMEE_RULE_EITHER): exit at the first e where the confidence test fires or
        the argmax has stayed the same for ``config["patience"]`` exits in a row: the earlier of the threshold policy's and
        ``patience_policy``'s exits.  Same configuration keys as ``patient_confident_policy``."""
        return self._rule_policy("patience_or_threshold")

    def quota_policy(self):
        """Budgeted exits (include/mmee.h MMEE_QUOTA_*; MSDNet's budgeted batch classification) on dumped arrays: ``config["quotas"]``, one
        integer per exit below the last, is how many documents of every group of ``config["quota_group"]`` consecutive documents (default:
        all of them, one group) leave at that exit, the most confident by ``config["criterion"]`` ("max_confidence", the default; "entropy";
        "margin") first.  ``config["quota_mode"]`` "exact" (default) or "at_least", which also releases whoever passes
        ``config["exit_thresholds"]`` / ``config["exit_threshold"]``.  Unlike every other policy here, a document's exit depends on the
        other documents of its group.  ``config["exit_policy"] = "quota_policy"`` selects it through EE/eval.py:91-98's ``getattr`` dispatch."""
        from .sweep import csf_table
        if self.config.get("quotas") is None:
            raise ValueError('quota_policy needs config["quotas"] (one integer per exit below the last)')
        st = threshold_criterion(self.config.get("criterion", "max_confidence"))
        mode = str(self.config.get("quota_mode", "exact"))
        thr = self._exit_thresholds("quota_policy (quota_mode at_least)") if mode == "at_least" else None
        table = csf_table(self.logits, criterion=st)[0]
        scan = quota_scan_device(table, self.config["quotas"], mode=mode, thresholds=thr, group_size=self.config.get("quota_group"),
                                 sign=-1.0 if st.value == "entropy" else 1.0, want_cuts=False)
        num_exits, num_samples = self.logits.shape[0], self.logits.shape[1]
        L = _f64_on(scan.exits.device, self.logits)
        pred = L[scan.exits.long(), torch.arange(num_samples, device=L.device)]
        exits_store = scan.exits.cpu().numpy().astype(np.int32)
        tgt = self.config.get("device", "cpu")
        predictions = pred.to(tgt) if str(tgt) != str(pred.device) else pred
        c = np.bincount(exits_store, minlength=num_exits)
        return exits_store, predictions, {exit_id: int(c[exit_id]) / num_samples for exit_id in range(0, num_exits)}

    def accuracy_calibration_heuristic(self):
        """EE/policy.py:55-111: per-exit thresholds minmax_eps(1 - accuracy/ece)."""
        if "calibration_metrics" not in self.config:
            raise Exception("calibration_metrics not in config -> Set calibrate flag to True")
        num_exits = self.logits.shape[0]
        accuracies = self.config["calibration_metrics"]["accuracy"]
        ece = self.config["calibration_metrics"]["ece"]
        metrics = [1 - (accuracies[i] / ece[i]) for i in range(0, num_exits)]
        epsilon = self.config["epsilon"]
        thresholds = (np.array(metrics) - (np.min(metrics) - epsilon)) / (
            (np.max(metrics) + epsilon) - (np.min(metrics) - epsilon))
        return self._finish(thresholds)
