"""Model cascades: the cheap model runs on every document and passes on only the ones it is unsure about (CascadeBERT, Li et al., Findings of
EMNLP 2021) -- the complement, one level up, of the exits inside one encoder.  include/mmee.h has THE definition (behind MMEE_QUOTA_*): a
cascade is one early-exit model whose exit list is the concatenation of its stages' exit lists, so every dumped-array tool (``csf_table``,
the scans, ``threshold_sweep``, ``threshold_search`` also with ``cost=``, ``threshold_refine``, ``exit_report``, ``Policy``,
``quota_scan_device``) takes ``CascadeEngine.dump`` unchanged, and choosing the deferral threshold is the search that already exists.

A stage is an ``EarlyExitEngine`` and runs its ordinary forward; between two stages three launches of csrc/cascade.hip select the deferred
documents, gather their inputs from the caller's arrays and merge the next stage's answers into the caller's slots.  ONE 4-byte read per stage
boundary crosses to the host -- the number of deferred documents, which the next ``ee_forward`` takes by value -- and nothing else.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import capi
from .engine import EarlyExitEngine, torch
from .microbatch import MicroBatchedEngine
from .policy import _ptr, threshold_criterion

_LAYOUT_KEYS = ("input_ids", "attention_mask", "bbox", "pixel_values", "token_type_ids", "position_ids")
_IMAGE_KEYS = ("pixel_values",)
# per-call flags of EarlyExitEngine.forward a cascade hands to every stage; everything else belongs to one handle
_FORWARD_FLAGS = ("dense_rows", "validate", "whole_layers", "probe_always", "xprobe", "one_term", "low_latency")
_DUMP_FLAGS = ("dump_all", "want_all", "want_head", "want_hidden_cls", "want_hidden_states", "want_attentions")


@dataclass
class CascadeOutput:
    logits: "torch.Tensor"                  # (B,K) float32 -- of the last stage the document ran in
    exit_layer: "torch.Tensor"              # (B,)  int32   -- GLOBAL exit index: off_s + the stage's local exit
    confidence: "torch.Tensor"              # (B,)  float32 -- that stage's criterion at that exit
    stage: "torch.Tensor"                   # (B,)  int32   -- the last stage the document ran in
    stage_docs: List[int]                   # host: the documents each stage ran (0 for a stage nobody reached)


def exit_counts(stages) -> List[int]:
    """E1_s of every stage: engines, or model configurations."""
    return [int(s.E if hasattr(s, "E") else s.exit_config.num_exits) + 1 for s in stages]


def flat_thresholds(per_stage) -> np.ndarray:
    """One (E1_s,) vector per stage -> the flat (SE1,) float64 vector, the thresholds of the concatenated exit list."""
    parts = [np.asarray(t, dtype=np.float64).reshape(-1) for t in per_stage]
    if not parts:
        raise ValueError("flat_thresholds: no stage")
    return np.concatenate(parts)


def split_thresholds(flat, stages) -> List[np.ndarray]:
    """The flat (SE1,) vector (what ``threshold_search(...).select()`` returns on the concatenated table) -> one (E1_s,) vector per stage.
    ``stages``: the engines, their configurations, or the E1_s themselves."""
    e1 = [int(s) for s in stages] if all(isinstance(s, (int, np.integer)) for s in stages) else exit_counts(stages)
    v = np.asarray(flat, dtype=np.float64).reshape(-1)
    if v.shape[0] != sum(e1):
        raise ValueError(f"split_thresholds: {v.shape[0]} thresholds for {sum(e1)} exits ({' + '.join(map(str, e1))})")
    cuts = np.cumsum([0] + e1)
    return [v[cuts[s]:cuts[s + 1]].copy() for s in range(len(e1))]


def exit_costs(cfgs, attention_mask=None, text_rows=None, unit: float = 1e6) -> np.ndarray:
    """``sweep.exit_costs`` of a cascade, for ``threshold_search(cost=)`` on the concatenated table: ``(SE1, N) uint32``.  The row of global
    exit (s, e) is stage s's ``sweep.exit_costs`` row e plus the final-exit rows of all stages before it -- a document that leaves in stage s
    ran every earlier stage to its end.  ``cfgs``: the stages' model configurations (image-only stages ignore the text rows).  Algorithmic
    work, as there; ``ValueError`` when an entry would reach 2^32: choose a larger ``unit``."""
    from .sweep import exit_costs as stage_costs
    cfgs = list(cfgs)
    if not cfgs:
        raise ValueError("exit_costs: no stage")
    rows, before = [], None
    for cfg in cfgs:
        c = stage_costs(cfg, attention_mask=attention_mask, text_rows=text_rows, unit=unit).astype(np.int64)
        before = np.zeros(c.shape[1], dtype=np.int64) if before is None else before
        rows.append(c + before[None, :])
        before = before + c[-1]
    out = np.concatenate(rows, axis=0)
    if out.size and out.max() >= (1 << 32):
        raise ValueError(f"exit_costs: {out.max():.0f} units of {unit:g} FLOPs do not fit 32 bits: choose a larger unit")
    return out.astype(np.uint32)


class CascadeEngine:
    """``stages``: two or more finalised ``EarlyExitEngine`` on one device with one ``num_labels``.  ``defer_criterion``: None (every stage
    defers on its own threshold criterion; gate, patience and LTE handles on "max_confidence"), one name for every stage, or one entry
    (a name or None) per stage that can defer."""

    def __init__(self, stages: Sequence[EarlyExitEngine], defer_criterion=None):
        stages = list(stages)
        if len(stages) < 2:
            raise ValueError("a cascade has at least two stages (one stage is an EarlyExitEngine)")
        for s, eng in enumerate(stages):
            if isinstance(eng, MicroBatchedEngine):
                raise TypeError(f"stage {s}: a MicroBatchedEngine cannot be a stage (its slices own their streams and handles; a later stage's "
                                "batch is small by design: use an EarlyExitEngine)")
            if not isinstance(eng, EarlyExitEngine):
                raise TypeError(f"stage {s}: expected an EarlyExitEngine, got {type(eng).__name__}")
            if not eng._finalized:
                raise capi.MMEEError(f"stage {s}: load_weights() has not been called")
        if any(eng.device != stages[0].device for eng in stages):
            raise ValueError(f"the stages of a cascade live on one device, got {[str(e.device) for e in stages]} (stages on different GPUs are not built)")
        if any(eng.K != stages[0].K for eng in stages):
            raise ValueError(f"the stages of a cascade share num_labels, got {[e.K for e in stages]}")
        self.stages = stages
        self.S, self.K, self.device = len(stages), stages[0].K, stages[0].device
        self.E1 = exit_counts(stages)
        self.offsets = [int(o) for o in np.cumsum([0] + self.E1[:-1])]
        self.num_exits = sum(self.E1)
        if defer_criterion is None or isinstance(defer_criterion, str) or not isinstance(defer_criterion, (list, tuple)):
            defer_criterion = [defer_criterion] * (self.S - 1)
        defer_criterion = list(defer_criterion)
        if len(defer_criterion) not in (self.S - 1, self.S):
            raise ValueError(f"defer_criterion: one entry per stage that can defer ({self.S - 1}), got {len(defer_criterion)}")
        self.defer_criterion = [self._stage_criterion(eng) if c is None else threshold_criterion(c)
                                for eng, c in zip(stages[:-1], defer_criterion)]
        self.lib = stages[0].lib
        self._count_host = None

    @staticmethod
    def _stage_criterion(eng):
        from .config import EarlyExitInference
        st = eng.exit_config.inference_strategy
        st = st if isinstance(st, EarlyExitInference) else EarlyExitInference(str(st))
        if eng.use_lte or st not in (EarlyExitInference.MAX_CONFIDENCE, EarlyExitInference.ENTROPY, EarlyExitInference.MARGIN):
            return EarlyExitInference.MAX_CONFIDENCE     # what gate, patience and LTE handles report at the final exit anyway
        return st

    def close(self):
        for eng in self.stages:
            eng.close()

    # ---- refused -------------------------------------------------------------------------------------------------------------------------
    def forward_stream(self, *args, **kw):
        raise NotImplementedError("CascadeEngine.forward_stream: streaming across stages is not built (a document's answer is final only when "
                                  "its last stage has decided); stream the stages' engines themselves")

    def capture(self, *args, **kw):
        raise NotImplementedError("CascadeEngine.capture: a later stage's batch size depends on the data, and a captured launch list has its "
                                  "shapes bound; capture the stages' engines themselves")

    def forward_vision_first(self, *args, **kw):
        raise NotImplementedError("CascadeEngine.forward_vision_first: a vision-first stage inside a cascade is not built (a stage's forward "
                                  "takes its whole inputs at once); run EarlyExitEngine.forward_vision_first on the stage's engine, or put an "
                                  "image-only stage in front and hand the next stage a callable")

    forward_vision = forward_vision_first

    # ---- arguments -----------------------------------------------------------------------------------------------------------------------
    def _per_stage(self, v, what):
        """None, one vector per stage, or the flat (SE1,) vector -> a list of S entries (None: the stage's default)."""
        if v is None:
            return [None] * self.S
        if isinstance(v, (list, tuple)) and len(v) == self.S and all(x is None or np.ndim(x) >= 1 for x in v):
            out = []
            for s, x in enumerate(v):
                if x is not None and np.asarray(x).reshape(-1).shape[0] != self.E1[s]:
                    raise ValueError(f"{what}: stage {s} has {self.E1[s]} exits, got {np.asarray(x).reshape(-1).shape[0]} entries")
                out.append(None if x is None else np.asarray(x, dtype=np.float64).reshape(-1))
            return out
        a = np.asarray(v, dtype=np.float64).reshape(-1) if np.ndim(v) == 1 else None
        if a is None or a.shape[0] != self.num_exits:
            raise ValueError(f"{what}: one ({', '.join(map(str, self.E1))}) vector per stage, or one flat ({self.num_exits},) vector")
        return split_thresholds(a, self.E1)

    def _stage_inputs(self, inputs):
        if isinstance(inputs, dict):
            return [inputs] * self.S
        inputs = list(inputs)
        if len(inputs) != self.S:
            raise ValueError(f"inputs: one dict, or one entry per stage ({self.S}), got {len(inputs)}")
        if callable(inputs[0]):
            raise ValueError("inputs: stage 0 runs on every document, its entry is a dict (a callable is for a stage documents are deferred to)")
        return inputs

    def _arrays(self, s, entry):
        """The arrays stage s reads out of a dict, as contiguous device tensors of the dtypes its forward takes (no copy when they are already)."""
        eng = self.stages[s]
        out = {}
        for k in (_IMAGE_KEYS if eng.beit else _LAYOUT_KEYS):
            x = entry.get(k)
            if x is not None:
                out[k] = eng._dev(x, torch.float32 if k == "pixel_values" else torch.int64, k)
        if "pixel_values" not in out or (not eng.beit and "input_ids" not in out):
            raise ValueError(f"stage {s}: inputs need pixel_values" + ("" if eng.beit else " and input_ids"))
        return out

    def _run_stage(self, s, arrays, n, out, thr, tmp, flags):
        """Stage s on n documents in consecutive chunks of at most its max_docs (documents are independent), results into row slices of `out`."""
        eng = self.stages[s]
        if getattr(eng, "has_deadline", None) and eng.has_deadline():
            raise ValueError(f"stage {s} has a deadline set: deadlines on cascade stages are not built (a stage runs in chunks, each of which "
                             "would start a clock of its own, and the cascade's budget spans its stages); set_deadline(None) on the stage's engine")
        if getattr(eng, "has_controller", None) and eng.has_controller():
            raise ValueError(f"stage {s} has a controller set: online exit control on cascade stages is not built (a stage's calls are the deferred "
                             "documents of another); set_controller(None) on the stage's engine")
        if eng.has_audit():
            raise ValueError(f"stage {s} has an audit set: audited exits on cascade stages are not built (a stage sees deferred documents under "
                             "new slots, and a shadow's final row is not a deferral); set_audit(None) on the stage's engine")
        if n > eng.max_docs and eng.has_quotas:
            raise ValueError(f"stage {s} has quotas set and {n} documents for max_docs = {eng.max_docs}: the chunks would each rank alone "
                             "(set_quotas(None), or a handle that takes the stage whole)")
        for a in range(0, n, eng.max_docs):
            b = min(n, a + eng.max_docs)
            eng.forward(**{k: v[a:b] for k, v in arrays.items()}, thresholds=thr, temperatures=tmp, out=tuple(t[a:b] for t in out), **flags)

    # ---- the cascade ---------------------------------------------------------------------------------------------------------------------
    def forward(self, inputs, thresholds=None, temperatures=None, **per_call_flags) -> CascadeOutput:
        """``inputs``: one dict from which every stage takes the arrays it needs (an image-only stage ``pixel_values``; a LayoutLMv3 stage
        ``input_ids`` / ``attention_mask`` / ``bbox`` / ``pixel_values`` / ``token_type_ids`` / ``position_ids``), all over the B documents of the
        call; or one entry per stage.  The entry of a stage behind the first may be a callable ``f(slots: np.ndarray) -> dict``: called only
        when somebody is deferred, with the deferred documents' original slots (one more small download, on this route only), it returns
        that stage's inputs already in deferred order and the gather is skipped -- OCR only for the pages the image model is unsure about.
        ``thresholds`` / ``temperatures``: None (every stage's defaults), one ``(E1_s,)`` vector per stage, or one flat ``(SE1,)`` vector;
        entry ``E_s`` of stage s < S-1 is its deferral threshold.  ``per_call_flags``: ``dense_rows``, ``validate``, ``whole_layers``,
        ``probe_always``, ``xprobe``, ``one_term``, ``low_latency``, handed to every stage's forward."""
        for k in per_call_flags:
            if k in _DUMP_FLAGS:
                raise ValueError(f"CascadeEngine.forward: {k} belongs to a dump-all call, where nobody is deferred; use CascadeEngine.dump")
            if k not in _FORWARD_FLAGS:
                raise ValueError(f"CascadeEngine.forward: {k} is an argument of one handle's forward (a cascade passes on {', '.join(_FORWARD_FLAGS)})")
        entries = self._stage_inputs(inputs)
        thr, tmp = self._per_stage(thresholds, "thresholds"), self._per_stage(temperatures, "temperatures")
        for s, eng in enumerate(self.stages):
            if thr[s] is None:
                thr[s] = np.full((self.E1[s],), float(eng.exit_config.global_threshold))
        dev, K = self.device, self.K
        arrays0 = self._arrays(0, entries[0])
        B = int(arrays0["pixel_values"].shape[0])
        with torch.cuda.device(dev):
            out = (torch.empty((B, K), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev),
                   torch.empty((B,), dtype=torch.float32, device=dev))
            stage = torch.zeros((B,), dtype=torch.int32, device=dev)      # stage 0 writes the cascade's tensors itself (out=): off_0 = 0
            self._run_stage(0, arrays0, B, out, thr[0], tmp[0], per_call_flags)
            stage_docs = [B] + [0] * (self.S - 1)
            cur, orig, n = out, None, B
            if self._count_host is None:
                self._count_host = torch.empty((1,), dtype=torch.int32).pin_memory()
            for s in range(self.S - 1):
                if n == 0:
                    break
                nxt = torch.empty((n,), dtype=torch.int32, device=dev)
                count = torch.empty((1,), dtype=torch.int32, device=dev)
                stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                capi.check(self.lib.ee_cascade_select(_ptr(cur[0]), _ptr(cur[1]), _ptr(orig), n, K, self.E1[s] - 1, self.defer_criterion[s].code,
                                                      float(thr[s][-1]), _ptr(nxt), _ptr(count), None, stream), None, "ee_cascade_select")
                # the one host read of the boundary: 4 bytes behind one stream wait (the next ee_forward takes its batch size by value)
                self._count_host.copy_(count, non_blocking=True)
                torch.cuda.current_stream().synchronize()
                m = int(self._count_host[0])
                if m == 0:
                    break
                nxt = nxt[:m]
                entry = entries[s + 1]
                if callable(entry):
                    arrays = self._arrays(s + 1, entry(nxt.cpu().numpy()))
                    if any(int(v.shape[0]) != m for v in arrays.values()):
                        raise ValueError(f"stage {s + 1}: the callable returned {[int(v.shape[0]) for v in arrays.values()]} rows for {m} deferred documents")
                else:
                    arrays = self._gather(s + 1, entry, nxt, count, B)
                res = (torch.empty((m, K), dtype=torch.float32, device=dev), torch.empty((m,), dtype=torch.int32, device=dev),
                       torch.empty((m,), dtype=torch.float32, device=dev))
                self._run_stage(s + 1, arrays, m, res, thr[s + 1], tmp[s + 1], per_call_flags)
                stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                capi.check(self.lib.ee_cascade_merge(_ptr(res[0]), _ptr(res[1]), _ptr(res[2]), _ptr(nxt), m, K, self.offsets[s + 1], s + 1,
                                                     _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(stage), stream), None, "ee_cascade_merge")
                stage_docs[s + 1] = m
                cur, orig, n = res, nxt, m
        return CascadeOutput(out[0], out[1], out[2], stage, stage_docs)

    __call__ = forward

    def _gather(self, s, entry, slots, count, B):
        """Rows `slots` of the caller's arrays for stage s, all arrays in one launch (ee_cascade_gather; the count stays on the device)."""
        src = self._arrays(s, entry)
        m = int(slots.shape[0])
        dst, descs = {}, (capi.CascadeDesc * capi.CASCADE_MAX_ARRAYS)()
        for i, (k, v) in enumerate(src.items()):
            if int(v.shape[0]) != B:
                raise ValueError(f"stage {s}: {k} has {int(v.shape[0])} rows for a call of {B} documents")
            dst[k] = torch.empty((m,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device)
            descs[i].src, descs[i].dst = v.data_ptr(), dst[k].data_ptr()
            descs[i].row_bytes = (v.numel() // B) * v.element_size()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        capi.check(self.lib.ee_cascade_gather(descs, len(src), _ptr(slots), _ptr(count), m, stream), None, "ee_cascade_gather")
        self._keepalive = src               # borrowed by the enqueued launch until the stream drains
        return dst

    def dump(self, inputs, temperatures=None) -> "torch.Tensor":
        """Every stage in dump-all mode over ALL documents, concatenated: ``(SE1, B, K) float32`` on the device, the array the dumped-array
        tools take.  ``inputs`` as in ``forward`` (no callables: every stage sees every document)."""
        entries = self._stage_inputs(inputs)
        tmp = self._per_stage(temperatures, "temperatures")
        parts = []
        for s, eng in enumerate(self.stages):
            if callable(entries[s]):
                raise ValueError(f"dump: stage {s} runs on every document, its entry is a dict")
            arrays = self._arrays(s, entries[s])
            B = int(arrays["pixel_values"].shape[0])
            chunks = [eng.forward(**{k: v[a:a + eng.max_docs] for k, v in arrays.items()}, temperatures=tmp[s], dump_all=True,
                                  want_all=True).all_logits for a in range(0, B, eng.max_docs)]
            parts.append(torch.cat(chunks, dim=1))
        return torch.cat(parts, dim=0)
