"""Device-side multi-threshold search: the counterpart of EE/thresh.py:184-215 / EE/large_scale.py:42-128.

The reference builds a CSF table ``msp = max softmax`` of the dumped logits once, derives candidate threshold vectors
from its percentiles, and then, for every threshold vector, computes ``(CSF >= thr[:, None]).argmax(0)`` and the
accuracy / mean exit of the induced exits in an 8-process CPU pool.  Here the table stays in HBM and one workgroup
handles one threshold vector.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

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


def first_argmax(z):
    """argmax over the last axis of a device tensor, the lowest index on ties (torch.argmax promises no order among ties); a row without a
    maximum (NaN) counts as label K - 1."""
    K = z.shape[-1]
    idx = torch.arange(K, device=z.device, dtype=torch.int64).expand_as(z)
    return torch.where(z == z.max(dim=-1, keepdim=True).values, idx, torch.full_like(idx, K)).min(dim=-1).values.clamp_(max=K - 1)


def final_predictions(logits, device=None):
    """(N,) int64 on the device: the argmax of the final exit's row of logits (E1,N,K), the lowest index on ties (as ``exit_report`` counts a
    prediction).  Handed to ``threshold_search``, ``threshold_refine``, ``exit_report`` or the fits as ``references``, "correct" reads "agrees
    with the full model": the label-free table of live traffic (``audit.sample``) has nothing else."""
    dev = _require_torch_cuda(device)
    L = _f64_on(dev, logits)
    if L.dim() != 3:
        raise ValueError("logits must have shape (num_exits + 1, num_samples, num_labels)")
    return first_argmax(L[-1])


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


def gate_table(head_logits, final_logits, device=None):
    """The criterion table of the gate decision (include/mmee.h MMEE_CRIT_GATE; ee_gate_table): float64 (E+1,N) on the device from a gate
    handle's dump, ``head_logits`` (E,N,2) float32 (``EngineOutput.head_logits``) and ``final_logits`` (N,K) (the last row of ``all_logits``).
    Rows 0 .. E-1 are the gate scores with the bits the forward decides on, row E the max-softmax of the final logits (``msp_table``'s).
    With ``msp_table(all_logits, references)[1]`` as ``correct`` it goes unchanged into ``threshold_sweep``, ``rule_sweep`` (sign +1),
    ``threshold_search`` and ``metrics.exit_report(conf=, correct=)``; ``policy.gate_scan_device`` runs the policy on it."""
    lib = capi.load()
    dev = _require_torch_cuda(device)
    Hl, F = _on(dev, head_logits, torch.float32), _f64_on(dev, final_logits)
    if Hl.dim() != 3 or Hl.shape[2] != 2 or F.dim() != 2 or F.shape[0] != Hl.shape[1] or F.shape[0] < 1:
        raise ValueError("head_logits must have shape (num_exits, num_samples, 2) and final_logits (num_samples, num_labels)")
    E, N, K = Hl.shape[0], F.shape[0], F.shape[1]
    table = torch.empty((E + 1, N), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        capi.check(lib.ee_gate_table(_ptr(Hl), _ptr(F), E, N, K, _ptr(table), _stream()), None, "ee_gate_table")
    return table


def ensemble_logits(logits, weights, bias=None, device=None):
    """The exit ensemble (include/mmee.h, at ee_set_ensemble) on a dumped array (ee_ensemble_logits): ``logits`` (E1,N,K), the UN-ensembled
    scaled rows a dump-all forward returns in ``all_logits``; ``weights`` (E1,E1) lower triangular, ``bias`` (E1,K) or None (numpy or device
    tensors, taken as float64; an ``EnsembleFit`` holds both).  Returns float64 (E1,N,K) on the device: row m of document n is the ensemble
    row y_m by the device functions of the forward's own launch -- every value exactly a float32, with the bits ``engine.forward`` returns
    after ``engine.set_ensemble``.  A NaN row (an exit the document never reached) gives NaN from that exit on.  The result is a logits array
    like any other: it goes unchanged into ``csf_table``, ``criterion_scan_device`` / ``patience_scan_device`` / ``rule_scan_device``,
    ``threshold_sweep``, ``threshold_search`` (also with ``cost=``), ``threshold_refine``, ``metrics.exit_report`` and ``Policy``."""
    lib = capi.load()
    dev = _require_torch_cuda(device)
    L = _f64_on(dev, logits)
    if L.dim() != 3:
        raise ValueError("logits must have shape (num_exits + 1, num_samples, num_labels)")
    E1, N, K = L.shape
    W = _f64_on(dev, weights)
    Bs = None if bias is None else _f64_on(dev, bias)
    if tuple(W.shape) != (E1, E1) or (Bs is not None and tuple(Bs.shape) != (E1, K)):
        raise ValueError(f"weights must be (E1,E1) = {(E1, E1)} and bias (E1,K) = {(E1, K)} or None")
    out = torch.empty((E1, N, K), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        capi.check(lib.ee_ensemble_logits(_ptr(L), E1, N, K, _ptr(W), _ptr(Bs), _ptr(out), _stream()), None, "ee_ensemble_logits")
    return out


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


_MASK64 = (1 << 64) - 1


def search_digits(source, v, E1: int, P: int, seed: int = 0, mixtures=None):
    """The E1 - 1 digits of candidate vector ``v`` of a threshold search, by the rules of include/mmee.h (MMEE_SEARCH_GRID / _SAMPLED /
    _MIXTURES): plain Python integers, no device."""
    v = int(v)
    if source == capi.SEARCH_GRID:
        return [(v // P ** e) % P for e in range(E1 - 1)]
    if source == capi.SEARCH_SAMPLED:
        out = []
        for e in range(E1 - 1):
            z = (seed + (v * E1 + e + 1) * 0x9E3779B97F4A7C15) & _MASK64
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
            z ^= z >> 31
            out.append(((z >> 32) * P) >> 32)
        return out
    return [min(int(d), P - 1) for d in np.asarray(mixtures)[v, :E1 - 1]]


@dataclass
class SearchResult:
    """What ``threshold_search`` found.  The front is on the host (numpy), ascending by mean exit and, strictly, by accuracy; ``accuracy`` /
    ``mean_exit`` of all V vectors (``want_all=True``) stay device tensors.  Thresholds are REAL thresholds of the criterion (for entropy: the
    negated table negated back), so that a row goes to ``forward(thresholds=)`` unchanged."""
    table: np.ndarray                       # (E1, P) candidate thresholds per exit; row E1 - 1 is 0
    front_thresholds: np.ndarray            # (F, E1)
    front_accuracy: np.ndarray              # (F,) hits / N
    front_mean_exit: np.ndarray             # (F,) exit_sum / N
    front_vector: np.ndarray                # (F,) uint32 indices of the front's vectors
    front_hits: np.ndarray                  # (F,) int32
    front_exit_sum: np.ndarray              # (F,) int32
    num_vectors: int
    num_samples: int
    source: int
    seed: int = 0
    mixtures: Optional[np.ndarray] = None
    accuracy: Optional["torch.Tensor"] = None
    mean_exit: Optional["torch.Tensor"] = None
    # a cost-weighted search (``threshold_search(cost=)``): the front is the one of (cost_sum down, hits up), ascending by cost and, strictly,
    # by accuracy; ``front_exit_sum`` / ``front_mean_exit`` stay filled but are NOT monotone along it
    front_cost_sum: Optional[np.ndarray] = None      # (F,) uint64
    front_mean_cost: Optional[np.ndarray] = None     # (F,) cost_sum / N
    cost_sum: Optional["torch.Tensor"] = None        # (V,) int64 device tensor (``want_all=True``)
    semantics: Optional[str] = None                  # "policy" / "reference", as ``threshold_search`` ran; ``threshold_refine(start=)`` asks for it

    def digits(self, v):
        """The percentile index per exit (E1 - 1 of them) of candidate vector ``v``: ``table[e, digits(v)[e]]`` are its thresholds."""
        if not 0 <= int(v) < self.num_vectors:
            raise IndexError(f"vector {v} of {self.num_vectors}")
        return search_digits(self.source, v, self.table.shape[0], self.table.shape[1], self.seed, self.mixtures)

    def select(self, min_accuracy=None, max_mean_exit=None, max_mean_cost=None):
        """One operating point of the front as a plain list of E1 floats (what ``EarlyExitEngine.forward(thresholds=)`` and
        ``model.early_exit(thresholds=)`` take): with ``min_accuracy`` the CHEAPEST entry whose accuracy reaches it (lowest mean exit; on a
        cost result lowest mean cost), with ``max_mean_exit`` / ``max_mean_cost`` the entry of HIGHEST accuracy within the budget.  Exactly one
        of the three; ``max_mean_exit`` belongs to a result without costs and ``max_mean_cost`` to one with them.  ``ValueError`` when no
        entry qualifies."""
        return self.front_thresholds[self.select_index(min_accuracy, max_mean_exit, max_mean_cost)].tolist()

    def select_index(self, min_accuracy=None, max_mean_exit=None, max_mean_cost=None) -> int:
        if sum(x is not None for x in (min_accuracy, max_mean_exit, max_mean_cost)) != 1:
            raise ValueError("select takes exactly one of min_accuracy, max_mean_exit and max_mean_cost")
        with_cost = self.front_cost_sum is not None
        if max_mean_exit is not None and with_cost:
            raise ValueError("this front is ordered by cost, the mean exit is not monotone along it: give the budget as max_mean_cost")
        if max_mean_cost is not None and not with_cost:
            raise ValueError("max_mean_cost needs a cost-weighted result: threshold_search(cost=...)")
        if min_accuracy is not None:
            ok = np.nonzero(self.front_accuracy >= float(min_accuracy))[0]
            if not len(ok):
                raise ValueError(f"no front entry reaches accuracy {min_accuracy} (best: {self.front_accuracy.max() if len(self.front_accuracy) else None})")
            return int(ok[0])                   # accuracy rises along the front: the first is the cheapest
        if max_mean_cost is not None:
            ok = np.nonzero(self.front_mean_cost <= float(max_mean_cost))[0]
            if not len(ok):
                raise ValueError(f"no front entry has a mean cost <= {max_mean_cost} (lowest: {self.front_mean_cost.min() if len(self.front_mean_cost) else None})")
            return int(ok[-1])
        ok = np.nonzero(self.front_mean_exit <= float(max_mean_exit))[0]
        if not len(ok):
            raise ValueError(f"no front entry has a mean exit <= {max_mean_exit} (lowest: {self.front_mean_exit.min() if len(self.front_mean_exit) else None})")
        return int(ok[-1])


_SEARCH_SEMANTICS = {"reference": capi.SEARCH_REFERENCE, "policy": capi.SEARCH_POLICY}


def threshold_search(logits, references=None, criterion="max_confidence", num_per_exit: int = 10, mixtures="grid", seed: int = 42,
                     semantics: str = "policy", want_all: bool = False, device=None, cost=None) -> SearchResult:
    """Which thresholds should a deployment run?  Candidate thresholds = ``num_per_exit`` percentiles of every exit's criterion table
    (``np.percentile(table[e], linspace(0, 100, num_per_exit))`` bit for bit), candidate vectors = ``mixtures`` of them, each scored on the
    dumped array, and the accuracy / mean-exit Pareto front of the scores, all on the device (ee_threshold_search; include/mmee.h).

    ``logits`` (E1,N,K) with ``references`` (N,), or a precomputed pair ``(table, correct)`` as ``csf_table(..., as_csf=True)`` returns it
    (``references`` is then not read).  ``mixtures``: ``"grid"`` -- all ``num_per_exit ** (E1 - 1)`` vectors --, an int V -- V vectors drawn by the
    counter-based hash of ``seed`` --, or an integer array (V,E1) of percentile indices (the reference's own ``np.random.randint`` draw, for
    one).  ``semantics``: ``"policy"`` -- what a forward does: strict compare, the final exit when nothing fires -- or ``"reference"`` --
    ``threshold_sweep``'s ``>=`` / exit 0.  ``want_all`` also returns the accuracy and mean exit of every vector (device tensors).

    ``cost``: an integer array (E1,) -- a per-exit cost, the same for every document: the reference's per-exit FLOPs, or its latency
    ``(e + 1) / (E + 1)`` in integer units -- or (E1,N) -- what document n costs when it leaves at exit e (``exit_costs``), values in
    [0, 2^32).  The front is then the accuracy / cost front (ee_threshold_search_cost): ``front_cost_sum`` / ``front_mean_cost`` are filled,
    the entries ascend by cost, and ``want_all`` also returns every vector's ``cost_sum``.  Without it the call is the exit-index search."""
    from .policy import threshold_criterion
    st = threshold_criterion(criterion)
    if semantics not in _SEARCH_SEMANTICS:
        raise ValueError(f'semantics "{semantics}": choose "policy" or "reference"')
    P = int(num_per_exit)
    if not 2 <= P <= 64:
        raise ValueError(f"num_per_exit = {num_per_exit}: 2 .. 64 thresholds per exit")
    pair = isinstance(logits, tuple)
    if pair:
        if len(logits) != 2:
            raise ValueError("a precomputed table is the pair (table (E1,N), correct (E1,N))")
        E1 = int(logits[0].shape[0])
    else:
        if references is None:
            raise ValueError("logits need the references")
        E1 = int(np.shape(logits)[0])
    mix_host = None
    if isinstance(mixtures, str):
        if mixtures != "grid":
            raise ValueError('mixtures: "grid", a number of sampled vectors, or an array (V,E1) of percentile indices')
        source, V = capi.SEARCH_GRID, P ** (E1 - 1)
        if V >= 1 << 32:
            raise ValueError(f"the grid of {P} thresholds at {E1 - 1} exits has {P}^{E1 - 1} >= 2^32 vectors: sample it (mixtures=V)")
    elif np.ndim(mixtures) == 0:
        source, V = capi.SEARCH_SAMPLED, int(mixtures)
        if not 1 <= V < 1 << 32:
            raise ValueError("mixtures = V: 1 <= V < 2^32 sampled vectors")
    else:
        mix_host = mixtures.cpu().numpy() if torch is not None and isinstance(mixtures, torch.Tensor) else np.asarray(mixtures)
        if mix_host.ndim != 2 or mix_host.shape[1] != E1 or mix_host.shape[0] < 1 or mix_host.dtype.kind not in "iu":
            raise ValueError(f"mixtures: an integer array (V,{E1}) of percentile indices, V >= 1")
        if mix_host[:, :E1 - 1].min() < 0 or mix_host[:, :E1 - 1].max() >= P:
            raise ValueError(f"mixtures: every percentile index must be in [0, {P})")
        mix_host = np.clip(mix_host, 0, P - 1).astype(np.uint8)        # the final exit's digit is unused
        source, V = capi.SEARCH_MIXTURES, int(mix_host.shape[0])
    cost_host = None
    if cost is not None:
        cost_host = cost.cpu().numpy() if torch is not None and isinstance(cost, torch.Tensor) else np.asarray(cost)
        if cost_host.dtype.kind not in "iu":
            raise ValueError(f"cost: an integer array, not {cost_host.dtype} (round it in the unit you choose)")
        n_docs = int(logits[0].shape[1]) if pair else int(np.shape(logits)[1])
        if cost_host.shape not in ((E1,), (E1, n_docs)):
            raise ValueError(f"cost: shape ({E1},) or ({E1},{n_docs}), not {cost_host.shape}")
        if cost_host.size and (int(cost_host.min()) < 0 or int(cost_host.max()) >= 1 << 32):
            raise ValueError("cost: every value must be in [0, 2^32)")
    lib = capi.load()
    dev = _require_torch_cuda(device)
    if pair:
        cf, cr = _f64_on(dev, logits[0]), _on(dev, logits[1], torch.uint8)
    else:
        cf, cr = csf_table(logits, references, criterion=st, as_csf=True, device=dev)
    if cf.dim() != 2 or tuple(cr.shape) != tuple(cf.shape):
        raise ValueError("table (E1,N), correct (E1,N)")
    E1, N = cf.shape
    mix = torch.from_numpy(mix_host).to(dev) if mix_host is not None else None
    table = torch.empty((E1, P), dtype=torch.float64, device=dev)
    acc = torch.empty((V,), dtype=torch.float64, device=dev) if want_all else None
    mex = torch.empty((V,), dtype=torch.float64, device=dev) if want_all else None
    f_count = torch.zeros((1,), dtype=torch.int32, device=dev)
    f_sum = torch.empty((N + 1,), dtype=torch.int32, device=dev)
    f_hits = torch.empty((N + 1,), dtype=torch.int32, device=dev)
    f_vec = torch.empty((N + 1,), dtype=torch.int32, device=dev)        # uint32 words
    f_thr = torch.empty((N + 1, E1), dtype=torch.float64, device=dev)
    sign = -1.0 if st.value == "entropy" else 1.0                       # the search ran on the negated entropy: real thresholds back (exact)
    extra = {}
    if cost_host is None:
        with torch.cuda.device(dev):
            capi.check(lib.ee_threshold_search(_ptr(cf), _ptr(cr), E1, N, P, source, V, int(seed) & _MASK64, _ptr(mix), _SEARCH_SEMANTICS[semantics],
                                               _ptr(table), _ptr(acc), _ptr(mex), _ptr(f_count), _ptr(f_sum), _ptr(f_hits), _ptr(f_vec), _ptr(f_thr),
                                               _stream()), None, "ee_threshold_search")
        F = int(f_count.item())
    else:
        c2 = cost_host if cost_host.ndim == 2 else np.broadcast_to(cost_host[:, None], (E1, N))
        cs = torch.from_numpy(np.ascontiguousarray(c2.astype(np.uint32)).view(np.int32)).to(dev)      # uint32 words
        csum = torch.empty((V,), dtype=torch.int64, device=dev) if want_all else None                  # uint64 words below 2^56
        f_cost = torch.empty((N + 1,), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            capi.check(lib.ee_threshold_search_cost(_ptr(cf), _ptr(cr), _ptr(cs), E1, N, P, source, V, int(seed) & _MASK64, _ptr(mix),
                                                    _SEARCH_SEMANTICS[semantics], _ptr(table), _ptr(acc), _ptr(mex), _ptr(csum), _ptr(f_count),
                                                    _ptr(f_cost), _ptr(f_sum), _ptr(f_hits), _ptr(f_vec), _ptr(f_thr), _stream()), None,
                       "ee_threshold_search_cost")
        F = int(f_count.item())
        costs = f_cost[:F].cpu().numpy().view(np.uint64)
        extra = dict(front_cost_sum=costs, front_mean_cost=costs / float(N), cost_sum=csum)
    hits, sums = f_hits[:F].cpu().numpy(), f_sum[:F].cpu().numpy()
    return SearchResult(table=sign * table.cpu().numpy(), front_thresholds=sign * f_thr[:F].cpu().numpy(), front_accuracy=hits / float(N),
                        front_mean_exit=sums / float(N), front_vector=f_vec[:F].cpu().numpy().view(np.uint32), front_hits=hits, front_exit_sum=sums,
                        num_vectors=V, num_samples=int(N), source=source, seed=int(seed) & _MASK64, mixtures=mix_host, accuracy=acc, mean_exit=mex,
                        semantics=semantics, **extra)


def exit_costs(cfg, attention_mask=None, text_rows=None, unit: float = 1e6, ocr_cost=None) -> np.ndarray:
    """The path's own cost model, for ``threshold_search(cost=)``: ``(E1, N) uint32``, entry (e, n) = the work of document n when it leaves at
    exit e, in units of ``unit`` FLOPs (``np.rint(F / unit)``).  No device is needed.

    ``F(e, n) = 2 num_patches (C p^2) H  +  l_e (2 S_n (4 H^2 + 2 H I) + 4 S_n^2 H)  +  (e + 1) (2 H^2 + 2 H K)``: the patch projection, ``l_e``
    encoder layers -- the layer exit e sits behind: 0 for the embedding-level exits, ``num_hidden_layers`` for the final one -- of four H x H
    and two H x I GEMMs and the two attention products over the document's ``S_n`` rows, and the e + 1 exit heads evaluated on the way.
    ``S_n`` = the text rows the packed layout keeps (the index of the last kept position of ``attention_mask`` (N,T) + 1; or ``text_rows`` (N,)
    directly) + ``cfg.visual_len``; for ``arch="beit"`` ``S_n = visual_len`` (N from ``text_rows``' or the mask's length).

    This is ALGORITHMIC work, the figure ``roofline.achieved`` divides by: not measured time, and neither the probes nor the exit tail are in
    it.  ``ValueError`` when an entry would reach 2^32: choose a larger ``unit``.

    ``ocr_cost``: what reading a document's text costs, a scalar or ``(N,)`` in the same ``unit`` (already divided by it), finite and >= 0.
    A vision-first call (``EarlyExitEngine.forward_vision_first``) pays it only for the documents that stay behind ``vision_avg``, so it is
    added to every exit behind ``vision_avg`` and -- every exit needs the text then -- to none when the exit list has no ``vision_avg``
    (an image-only model included).  ``None`` (default): the table without it, bit for bit.  ``threshold_search(cost=)``,
    ``threshold_refine``, ``risk_control(cost=)`` and ``ExitReport.efficiency`` take the table unchanged: which ``thresholds[0]`` is worth
    how much OCR is then a search that already exists."""
    if (attention_mask is None) == (text_rows is None):
        raise ValueError("exit_costs takes exactly one of attention_mask (N,T) and text_rows (N,)")
    if attention_mask is not None:
        am = attention_mask.cpu().numpy() if torch is not None and isinstance(attention_mask, torch.Tensor) else np.asarray(attention_mask)
        if am.ndim != 2:
            raise ValueError("attention_mask (N,T)")
        kept = am != 0
        rows = np.where(kept.any(1), am.shape[1] - np.argmax(kept[:, ::-1], axis=1), 0).astype(np.int64)
    else:
        rows = np.asarray(text_rows).astype(np.int64).reshape(-1)
        if rows.size and rows.min() < 0:
            raise ValueError("text_rows must be >= 0")
    ee = cfg.exit_config
    layers = [0] * len(ee.embedding_exits) + list(ee.encoder_exit_layers) + [cfg.num_hidden_layers]
    H, I, K = cfg.hidden_size, cfg.intermediate_size, cfg.num_labels
    S = (np.zeros_like(rows) if cfg.arch == "beit" else rows) + cfg.visual_len
    per_layer = 2 * S * (4 * H * H + 2 * H * I) + 4 * S * S * H                                 # (N,) int64: exact
    patch = 2 * cfg.num_patches * (cfg.num_channels * cfg.patch_size ** 2) * H
    F = patch + np.asarray(layers, dtype=np.int64)[:, None] * per_layer[None, :] + (np.arange(len(layers), dtype=np.int64)[:, None] + 1) * (2 * H * H + 2 * H * K)
    out = np.rint(F / float(unit))
    if ocr_cost is not None:
        oc = np.asarray(ocr_cost, dtype=np.float64)
        if oc.ndim > 1 or (oc.ndim == 1 and oc.shape[0] != rows.shape[0]):
            raise ValueError(f"exit_costs: ocr_cost is a scalar or ({rows.shape[0]},), one entry per document; got {oc.shape}")
        if oc.size and (not np.isfinite(oc).all() or oc.min() < 0):
            raise ValueError("exit_costs: ocr_cost must be finite and >= 0")
        if len(ee.embedding_exits) and str(ee.embedding_exits[0]) == "vision_avg":
            out = np.rint(F / float(unit) + np.concatenate([np.zeros((1, rows.shape[0])), np.broadcast_to(oc, (len(layers) - 1, rows.shape[0]))]))
    if out.size and out.max() >= float(1 << 32):
        raise ValueError(f"exit_costs: {out.max():.0f} units of {unit:g} FLOPs do not fit 32 bits: choose a larger unit")
    return out.astype(np.uint32)


# ---- budgeted exits: quotas from shares and from a compute budget (host code; include/mmee.h MMEE_QUOTA_*) ---------------------------------------
def quotas_from_fractions(B: int, fractions, num_exits: Optional[int] = None) -> list:
    """Integer quotas of a call of ``B`` documents from per-exit shares: ``q_e = R(B * sum_{j <= e} f_j) - R(B * sum_{j < e} f_j)`` with
    ``R(x) = floor(x + 0.5)`` and the running sums ``np.cumsum`` of the float64 shares.  The rounding never drifts: the quotas through exit e sum to
    ``R(B * sum_{j <= e} f_j)``, so shares summing to 1 release everybody before the final exit only when they say so.  ``fractions``: one
    share per exit below the final one (``num_exits`` of them when given; one more entry, the final exit's own share, is accepted and not
    used: the final exit takes whoever is left).  Shares are >= 0 and sum to at most 1 (+ 1e-9)."""
    f = np.asarray(fractions, dtype=np.float64).reshape(-1)
    B = int(B)
    if B < 0:
        raise ValueError("quotas_from_fractions: B must be >= 0")
    if num_exits is not None:
        if f.shape[0] == num_exits + 1:
            f = f[:num_exits]
        elif f.shape[0] != num_exits:
            raise ValueError(f"quota_fractions: {f.shape[0]} shares, the model has {num_exits} exits below the final one")
    if f.size and (not np.isfinite(f).all() or f.min() < 0 or f.sum() > 1.0 + 1e-9):
        raise ValueError("quota_fractions: shares are finite, >= 0 and sum to at most 1")
    edges = np.floor(B * np.cumsum(f) + 0.5).astype(np.int64)
    return [int(v) for v in np.diff(np.concatenate([[0], edges]))]


def budget_quotas(cost, budget: float, B: int, q: Optional[float] = None):
    """MSDNet's budgeted batch classification (Huang et al., ICLR 2018, section 4 and appendix): the share of a batch that leaves at exit e is
    geometric, ``p_e = q^e / sum_j q^j`` over the ``E1`` exits, and the batch then costs ``sum_e p_e cost_e`` per document.  ``cost`` (E1,): the
    cost of a document that leaves at exit e, rising with e -- e.g. ``exit_costs(...).mean(1)``.  Without ``q`` it is found by bisection (on
    log q) so that the expected cost equals ``budget``; ``ValueError`` when the budget is outside ``[cost[0], cost[E1 - 1]]``, the cost of
    releasing everybody at the first / the final exit.  With ``q`` given the budget is not read.  Returns ``(quotas, p, q)``: the integer
    quotas of a call of ``B`` documents for the E1 - 1 exits below the final one (``quotas_from_fractions``), the shares ``p`` (E1,) and q.
    Host code; no device."""
    c = np.asarray(cost, dtype=np.float64).reshape(-1)
    E1 = c.shape[0]
    if E1 < 1 or not np.isfinite(c).all() or (np.diff(c) < 0).any():
        raise ValueError("budget_quotas: cost is (E1,), finite and non-decreasing in the exit")
    e = np.arange(E1, dtype=np.float64)

    def shares(logq):
        w = e * logq
        w = np.exp(w - w.max())
        return w / w.sum()

    if q is None:
        budget = float(budget)
        if not (c[0] <= budget <= c[-1]):
            raise ValueError(f"budget_quotas: budget {budget:g} outside [cost_0, cost_E] = [{c[0]:g}, {c[-1]:g}]")
        if c[-1] == c[0]:
            logq = 0.0
        else:
            lo, hi = -745.0 / max(E1 - 1, 1) - 1.0, 745.0 / max(E1 - 1, 1) + 1.0      # p = (1, 0, ..) and (.., 0, 1) to the last bit of float64
            for _ in range(200):                                                       # the expected cost rises with q
                mid = 0.5 * (lo + hi)
                if float(shares(mid) @ c) < budget:
                    lo = mid
                else:
                    hi = mid
            logq = 0.5 * (lo + hi)
        p = shares(logq)
        qv = float(np.exp(logq))
    else:
        qv = float(q)
        if not (qv > 0 and np.isfinite(qv)):
            raise ValueError("budget_quotas: q must be positive and finite")
        p = shares(np.log(qv))
    return quotas_from_fractions(B, p[:-1]), p, qv


# ---- the threshold refinement (ee_threshold_refine) -------------------------------------------------------------------------------------------
_REFINE_STATUS = {0: "no admissible single-exit change improves J", 1: "max_rounds reached", 2: "the start is over its budget"}


def _pareto_min_cost_max_hits(cost_sum, hits):
    """Indices of the strict Pareto front of (cost down, hits up), ascending in cost (and, strictly, in hits); among equal (cost, hits) the
    lowest index."""
    order = sorted(range(len(hits)), key=lambda i: (int(cost_sum[i]), -int(hits[i]), i))
    keep, best = [], -1
    for i in order:
        if int(hits[i]) > best:
            keep.append(i)
            best = int(hits[i])
    return keep


@dataclass
class RefineResult:
    """What ``threshold_refine`` found: one row per chain, numpy on the host.  ``thresholds`` are REAL thresholds of the criterion (for entropy
    the negated table negated back), so that a row goes to ``forward(thresholds=)`` unchanged.  ``status``: 0 -- no admissible single-exit change
    improves J --, 1 -- ``max_rounds`` moves made --, 2 -- the start was already over its budget (the row describes the start)."""
    table: np.ndarray                       # (E1, P)
    digits: np.ndarray                      # (S, E1) uint8, last column 0
    thresholds: np.ndarray                  # (S, E1)
    hits: np.ndarray                        # (S,) int32
    exit_sum: np.ndarray                    # (S,) int32
    cost_sum: np.ndarray                    # (S,) uint64
    rounds: np.ndarray                      # (S,) int32: moves made
    status: np.ndarray                      # (S,) int32
    start_hits: np.ndarray                  # (S,) int32
    start_cost_sum: np.ndarray              # (S,) uint64
    hit_value: np.ndarray                   # (S,) uint64, as the chains took it (min(w, 2^32 - 1))
    num_samples: int

    @property
    def accuracy(self):
        return self.hits / float(self.num_samples)

    @property
    def mean_cost(self):
        return self.cost_sum / float(self.num_samples)

    @property
    def mean_exit(self):
        return self.exit_sum / float(self.num_samples)

    @property
    def J(self):
        """w hits - cost_sum of every chain's final vector: Python ints."""
        return [int(w) * int(h) - int(c) for w, h, c in zip(self.hit_value, self.hits, self.cost_sum)]

    @property
    def start_J(self):
        return [int(w) * int(h) - int(c) for w, h, c in zip(self.hit_value, self.start_hits, self.start_cost_sum)]

    def front(self):
        """The chains on the strict Pareto front of (cost_sum down, hits up), as indices ascending in cost; ties go to the lowest chain."""
        return _pareto_min_cost_max_hits(self.cost_sum, self.hits)

    def select_index(self, min_accuracy=None, max_mean_cost=None, max_mean_exit=None) -> int:
        if sum(x is not None for x in (min_accuracy, max_mean_cost, max_mean_exit)) != 1:
            raise ValueError("select takes exactly one of min_accuracy, max_mean_cost and max_mean_exit")
        acc, mc, me = self.accuracy, self.mean_cost, self.mean_exit
        if min_accuracy is not None:
            ok = [i for i in self.front() if acc[i] >= float(min_accuracy)]
            if not ok:
                raise ValueError(f"no chain reaches accuracy {min_accuracy} (best: {acc.max() if len(acc) else None})")
            return ok[0]                         # accuracy rises along the front: the first is the cheapest
        if max_mean_cost is not None:
            ok = [i for i in self.front() if mc[i] <= float(max_mean_cost)]
            if not ok:
                raise ValueError(f"no chain has a mean cost <= {max_mean_cost} (lowest: {mc.min() if len(mc) else None})")
            return ok[-1]
        ok = [i for i in range(len(me)) if me[i] <= float(max_mean_exit)]
        if not ok:
            raise ValueError(f"no chain has a mean exit <= {max_mean_exit} (lowest: {me.min() if len(me) else None})")
        return max(ok, key=lambda i: (int(self.hits[i]), -int(self.exit_sum[i]), -i))

    def select(self, min_accuracy=None, max_mean_cost=None, max_mean_exit=None):
        """One chain's thresholds as a plain list of E1 floats (what ``forward(thresholds=)`` takes), with ``SearchResult.select``'s meaning:
        ``min_accuracy`` -- the CHEAPEST chain whose accuracy reaches it --, ``max_mean_cost`` / ``max_mean_exit`` -- the chain of HIGHEST accuracy
        within the budget (the mean exit is not monotone along a cost front, so that one looks at every chain; at equal hits the lower mean exit,
        then the lower chain).  Exactly one of the three; ``ValueError`` when no chain qualifies."""
        return self.thresholds[self.select_index(min_accuracy, max_mean_cost, max_mean_exit)].tolist()


def front_hit_values(result: SearchResult) -> np.ndarray:
    """The natural trade-offs along a cost front, for ``threshold_refine(hit_value=)``: the ceilings of ``d cost_sum / d hits`` between
    neighbouring front entries (F - 1 of them, uint64, clipped to 2^32 - 1): what the front itself pays for one more correct document there.
    A front without costs (``threshold_search`` without ``cost=``) is read with its exit sums, the cost ``cost[e][n] = e``."""
    cost = result.front_cost_sum if result.front_cost_sum is not None else result.front_exit_sum
    out = []
    for i in range(len(result.front_hits) - 1):
        dc, dh = int(cost[i + 1]) - int(cost[i]), int(result.front_hits[i + 1]) - int(result.front_hits[i])
        if dh <= 0 or dc < 0:
            raise ValueError("not a front: hits and cost must rise along it")
        out.append(min(-(-dc // dh), (1 << 32) - 1))
    return np.array(out, dtype=np.uint64)


def _host_ints(x, what):
    a = x.cpu().numpy() if torch is not None and isinstance(x, torch.Tensor) else np.asarray(x)
    if a.dtype.kind not in "iu":
        raise ValueError(f"{what}: integers, not {a.dtype}")
    return a


def threshold_refine(logits, references=None, criterion="max_confidence", num_per_exit: int = 10, start=None, hit_value=None, budget=None,
                     cost=None, max_rounds: int = 256, device=None, budget_mean=None) -> RefineResult:
    """Improve candidate threshold vectors by coordinate search on the device (ee_threshold_refine; include/mmee.h): every chain repeatedly takes
    the single-exit change of largest ``J = hit_value * hits - cost_sum`` among those within its budget, until none improves J or ``max_rounds``
    moves are made.  For the models whose grid ``threshold_search`` cannot enumerate (any E1 <= 64); the exit rule is the policy's.

    ``logits`` / ``references`` / ``criterion`` / ``num_per_exit`` / ``cost``: as in ``threshold_search`` (an array with references, or a pair
    ``(table, correct)``; ``cost`` (E1,) or (E1,N) integers, ``None``: the exit index).  ``start``: ``None`` -- one start with every digit
    ``P - 1``: each exit's threshold is its maximum, nobody leaves early --, an integer array (S0,E1) of digits, or a ``SearchResult`` of the SAME
    table with ``semantics="policy"``: its front entries are the starts.  ``hit_value``: an int or an integer array (W,) in [0, 2^32): what one
    more correct document is worth in cost units (``front_hit_values``); with W > 1 the chains are the cross product, S = S0 W, chain s = (start
    s // W, value s % W).  ``budget``: ``None``, an int or (S,) ints on ``cost_sum``; ``budget_mean`` the same divided by N."""
    from .policy import threshold_criterion
    st = threshold_criterion(criterion)
    P = int(num_per_exit)
    if not 2 <= P <= 64:
        raise ValueError(f"num_per_exit = {num_per_exit}: 2 .. 64 thresholds per exit")
    if not 1 <= int(max_rounds) <= 4096:
        raise ValueError(f"max_rounds = {max_rounds}: 1 .. 4096")
    pair = isinstance(logits, tuple)
    if pair:
        if len(logits) != 2:
            raise ValueError("a precomputed table is the pair (table (E1,N), correct (E1,N))")
        E1, n_docs = int(logits[0].shape[0]), int(logits[0].shape[1])
    else:
        if references is None:
            raise ValueError("logits need the references")
        E1, n_docs = int(np.shape(logits)[0]), int(np.shape(logits)[1])
    if not 2 <= E1 <= 64:
        raise ValueError(f"E1 = {E1}: 2 .. 64 exits")
    if hit_value is None:
        raise ValueError("hit_value: what one more correct document is worth in cost units (an int, or an integer array; front_hit_values)")
    w = np.atleast_1d(_host_ints(hit_value, "hit_value"))
    if w.ndim != 1 or w.size < 1 or int(w.min()) < 0 or int(w.max()) >= 1 << 32:
        raise ValueError("hit_value: an int or an integer array (W,) with W >= 1 and values in [0, 2^32)")
    start_result = start if isinstance(start, SearchResult) else None
    if start is None:
        dg = np.full((1, E1), P - 1, dtype=np.int64)
    elif start_result is not None:
        if start_result.table.shape != (E1, P):
            raise ValueError(f"start: a SearchResult with a table {start_result.table.shape}, this call's is ({E1}, {P})")
        if start_result.semantics != "policy":
            raise ValueError('start: a SearchResult of semantics="policy" (the refinement walks as a forward does)')
        if len(start_result.front_vector) < 1:
            raise ValueError("start: an empty front")
        dg = np.zeros((len(start_result.front_vector), E1), dtype=np.int64)
        for i, v in enumerate(start_result.front_vector):
            dg[i, :E1 - 1] = start_result.digits(v)
    else:
        dg = _host_ints(start, "start")
        if dg.ndim != 2 or dg.shape[1] != E1 or dg.shape[0] < 1:
            raise ValueError(f"start: an integer array (S0,{E1}) of percentile indices, S0 >= 1")
        if dg[:, :E1 - 1].min() < 0 or dg[:, :E1 - 1].max() >= P:
            raise ValueError(f"start: every percentile index must be in [0, {P})")
    S0, W = int(dg.shape[0]), int(w.size)
    S = S0 * W
    if S > 4096:
        raise ValueError(f"{S0} starts x {W} hit values = {S} chains, more than 4096")
    dg = np.repeat(np.clip(dg, 0, P - 1).astype(np.uint8), W, axis=0)                    # chain s = (start s // W, value s % W)
    dg[:, E1 - 1] = 0
    w_s = np.tile(w.astype(np.uint64), S0)
    if budget is not None and budget_mean is not None:
        raise ValueError("budget and budget_mean are one argument in two units: give one")
    if budget_mean is not None:
        bm = np.atleast_1d(np.asarray(budget_mean, dtype=np.float64))
        if (bm < 0).any():
            raise ValueError("budget_mean must be >= 0")
        budget = np.floor(bm * n_docs).astype(np.uint64)
    b_s = None
    if budget is not None:
        b = np.atleast_1d(_host_ints(budget, "budget"))
        if b.shape not in ((1,), (S,)) or (b.dtype.kind == "i" and int(b.min()) < 0):
            raise ValueError(f"budget: an int or ({S},) ints >= 0 (one per chain), not {b.shape}")
        b_s = np.broadcast_to(b.astype(np.uint64), (S,)).copy()
    cost_host = None
    if cost is not None:
        cost_host = _host_ints(cost, "cost")
        if cost_host.shape not in ((E1,), (E1, n_docs)):
            raise ValueError(f"cost: shape ({E1},) or ({E1},{n_docs}), not {cost_host.shape}")
        if cost_host.size and (int(cost_host.min()) < 0 or int(cost_host.max()) >= 1 << 32):
            raise ValueError("cost: every value must be in [0, 2^32)")
    lib = capi.load()
    dev = _require_torch_cuda(device)
    if pair:
        cf, cr = _f64_on(dev, logits[0]), _on(dev, logits[1], torch.uint8)
    else:
        cf, cr = csf_table(logits, references, criterion=st, as_csf=True, device=dev)
    if cf.dim() != 2 or tuple(cr.shape) != tuple(cf.shape):
        raise ValueError("table (E1,N), correct (E1,N)")
    E1, N = cf.shape
    cs = None
    if cost_host is not None:
        c2 = cost_host if cost_host.ndim == 2 else np.broadcast_to(cost_host[:, None], (E1, N))
        cs = torch.from_numpy(np.ascontiguousarray(c2.astype(np.uint32)).view(np.int32)).to(dev)      # uint32 words
    u64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)                   # uint64 words
    st_dev, w_dev, b_dev = torch.from_numpy(dg).to(dev), u64(w_s), (u64(b_s) if b_s is not None else None)
    i32 = lambda: torch.empty((S,), dtype=torch.int32, device=dev)
    i64 = lambda: torch.empty((S,), dtype=torch.int64, device=dev)
    digits = torch.empty((S, E1), dtype=torch.uint8, device=dev)
    thr = torch.empty((S, E1), dtype=torch.float64, device=dev)
    table = torch.empty((E1, P), dtype=torch.float64, device=dev)
    hits, xsum, rounds, status, s_hits, csum, s_csum = i32(), i32(), i32(), i32(), i32(), i64(), i64()
    with torch.cuda.device(dev):
        capi.check(lib.ee_threshold_refine(_ptr(cf), _ptr(cr), _ptr(cs), E1, N, P, S, _ptr(st_dev), _ptr(w_dev), _ptr(b_dev), int(max_rounds),
                                           _ptr(digits), _ptr(thr), _ptr(hits), _ptr(xsum), _ptr(csum), _ptr(rounds), _ptr(status), _ptr(s_hits),
                                           _ptr(s_csum), _ptr(table), _stream()), None, "ee_threshold_refine")
    sign = -1.0 if st.value == "entropy" else 1.0                       # the chains ran on the negated entropy: real thresholds back (exact)
    table_host = sign * table.cpu().numpy()
    if start_result is not None and not np.array_equal(np.ascontiguousarray(start_result.table).view(np.int64), np.ascontiguousarray(table_host).view(np.int64)):
        raise ValueError("start: the SearchResult's percentile table is not this call's, bit for bit: another table, criterion or num_per_exit")
    host = lambda t: t.cpu().numpy()
    return RefineResult(table=table_host, digits=host(digits), thresholds=sign * host(thr), hits=host(hits), exit_sum=host(xsum),
                        cost_sum=host(csum).view(np.uint64), rounds=host(rounds), status=host(status), start_hits=host(s_hits),
                        start_cost_sum=host(s_csum).view(np.uint64), hit_value=w_s, num_samples=int(N))
