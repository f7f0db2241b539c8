"""Host-side driver of the HIP path: owns an ``ee_handle`` and moves pointers across the C-ABI.

PyTorch is used for device memory (input / output tensors), streams and nothing else; all arithmetic of the path
runs in libmmee_hip.so.  ``EarlyExitEngine.forward`` is the (logits, exit_layer, confidence) contract of the north
star; ``LayoutLMv3EEForSequenceClassification`` (modeling.py) wraps it behind the reference's ``forward`` signature.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from dataclasses import dataclass
from typing import Dict, Mapping, Optional, Sequence, Union

import numpy as np

from . import capi
from .config import EMBEDDING_EXITS, ExitRule, ModelConfig, check_patience_spec

try:  # torch is plumbing (device tensors / streams); importing it must not be the reason the product "works"
    import torch
except Exception as _e:  # pragma: no cover
    torch = None
    _torch_err = _e


@dataclass
class EngineOutput:
    logits: "torch.Tensor"                  # (B,K) float32 — logits at the exit each document left through
    exit_layer: "torch.Tensor"              # (B,)  int32   — index into the exit list, E = final classifier
    confidence: "torch.Tensor"              # (B,)  float32 — criterion at that exit
    all_logits: Optional["torch.Tensor"] = None   # (E+1,B,K) policy logits of every evaluated exit (NaN = not reached)
    all_crit: Optional["torch.Tensor"] = None     # (E+1,B)
    head_logits: Optional["torch.Tensor"] = None  # (E,B,Kh) raw exit-head logits (exit_states[j][0])
    head_crit: Optional["torch.Tensor"] = None    # (E,B)    (exit_states[j][1])
    hidden_cls: Optional["torch.Tensor"] = None   # (L+1,B,H)
    hidden_states: Optional["torch.Tensor"] = None   # (L+1,B,T+Pv,H): the state entering every layer and the last layer's output
    attentions: Optional["torch.Tensor"] = None      # (L,B,heads,T+Pv,T+Pv): attention probabilities of every layer (after the head mask)
    audit_mask: Optional["torch.Tensor"] = None      # (B,) bool: the documents an audited call ran on to the final exit (set_audit); None without an audit


@dataclass
class VisionPhase:
    """Phase 1 of a vision-first call (``EarlyExitEngine.forward_vision``; the definition is in include/mmee.h at ee_forward_vision)."""
    output: EngineOutput                    # logits / exit_layer (= 0) / confidence written at the slots that left at exit 0, nothing elsewhere
    survivors: "torch.Tensor"               # (B,) int32 on the device: the slots that stay, ascending; entries from ``count`` on are not written
    count: "torch.Tensor"                   # (1,) int32 on the device: how many stay


@dataclass
class VisionFirstOutput:
    """What ``EarlyExitEngine.forward_vision_first`` returns: the three outputs of ``forward`` on the full inputs, bit for bit."""
    logits: "torch.Tensor"                  # (B,K) float32
    exit_layer: "torch.Tensor"              # (B,)  int32
    confidence: "torch.Tensor"              # (B,)  float32
    stage: "torch.Tensor"                   # (B,)  int32: 0 = answered from the pixels, 1 = ran with text
    text_docs: int                          # how many documents needed text (the survivors of exit 0)


_TEXT_KEYS = ("input_ids", "attention_mask", "bbox", "token_type_ids", "position_ids")


@dataclass
class ResultChunk:
    """The documents that left at one exit (``EarlyExitEngine.forward_stream``): host numpy arrays, copies of the handle's pinned segment."""
    exit_index: int                         # the exit, in the path's order; E = final classifier
    doc_index: np.ndarray                   # (n,)  int32   -- the documents' slots in the call, ascending
    logits: np.ndarray                      # (n,K) float32 -- bit-equal to output.logits[doc_index]
    exit_layer: np.ndarray                  # (n,)  int32   -- exit_index, n times
    confidence: np.ndarray                  # (n,)  float32 -- bit-equal to output.confidence[doc_index]


def unpack_stream_rows(words, K: int):
    """(n, K + 3) int32 rows of ee_stream_next -> (doc_index int32 (n,), logits float32 (n,K), exit_layer int32 (n,), confidence float32 (n,)).
    The first K + 2 words of a row are the row of ``dist.pack_results`` (floats as their bit patterns: views, never conversions), the last
    one is the document's slot in the call.  Pure: numpy in, numpy copies out."""
    from .dist import unpack_results
    if not isinstance(words, np.ndarray) or words.dtype != np.int32:
        raise TypeError(f"streamed result rows are int32 words, got {getattr(words, 'dtype', type(words))}")
    if words.ndim != 2 or words.shape[1] != K + 3:
        raise ValueError(f"streamed result rows are (n, K + 3) = (n, {K + 3}) words, got {words.shape}")
    w = np.ascontiguousarray(words)
    lg, ex, cf = unpack_results(torch.from_numpy(w[:, :K + 2].copy()))
    return w[:, K + 2].copy(), lg.numpy().reshape(-1, K), ex.numpy(), cf.numpy()


class ResultStream:
    """What ``EarlyExitEngine.forward_stream`` returns: iterate it for one ``ResultChunk`` per evaluated exit, in the path's order, each as soon
    as the device has decided that exit (the iterator blocks in ee_stream_next, on an event; deeper layers keep running meanwhile).
    ``output`` is the forward's usual ``EngineOutput`` of device tensors, complete once the stream has drained (or after a synchronise).
    A later ``forward_stream`` on the engine drops the chunks not read yet: iterating the older stream then raises ``MMEEError``."""

    def __init__(self, engine: "EarlyExitEngine", output: Optional[EngineOutput] = None):
        self.engine, self.output = engine, output
        self._generation = engine._stream_generation

    def __iter__(self):
        return self

    def __next__(self) -> ResultChunk:
        eng = self.engine
        if self._generation != eng._stream_generation:
            raise capi.MMEEError("this result stream was dropped by a later forward_stream() on the engine (its output tensors stay complete)")
        e, n, rows = C.c_int32(), C.c_int32(), C.POINTER(C.c_int32)()
        capi.check(eng.lib.ee_stream_next(eng._h, C.byref(e), C.byref(rows), C.byref(n)), eng._h, "ee_stream_next")
        if e.value < 0:
            raise StopIteration
        W = eng.K + 3
        words = np.ctypeslib.as_array(rows, shape=(n.value, W)).copy() if n.value else np.zeros((0, W), dtype=np.int32)
        return ResultChunk(e.value, *unpack_stream_rows(words, eng.K))


@dataclass
class ControllerLog:
    """The log of a controller (``EarlyExitEngine.controller_log``) or of its replay (``risk.rolling_control``): one row per call (per group),
    numpy on the host.  ``loss = disagree / sampled`` of the rows that sampled anybody is what the promise of include/mmee.h bounds."""
    call: np.ndarray                        # (T,) int64
    p_before: np.ndarray                    # (T,) float64: the position the call ran at
    p_after: np.ndarray                     # (T,) float64
    sampled: np.ndarray                     # (T,) int64: audited documents of the call
    disagree: np.ndarray                    # (T,) int64: of those, delivered early with another answer than the full model's
    delivered: np.ndarray                   # (T,E) int64: audited documents delivered at exit e
    agree: np.ndarray                       # (T,E) int64
    thresholds: np.ndarray                  # (T,E1) float64: the thresholds the call ran with

    @staticmethod
    def from_rows(rows, E1: int) -> "ControllerLog":
        """From (T, controller_log_words(E1)) int64 words as the device writes them (include/mmee.h)."""
        r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, capi.controller_log_words(E1))
        E = E1 - 1
        f = lambda a: np.ascontiguousarray(a).view(np.float64)
        return ControllerLog(r[:, 0].copy(), f(r[:, 1]), f(r[:, 2]), r[:, 3].copy(), r[:, 4].copy(), r[:, 5:5 + E].copy(),
                             r[:, 5 + E:5 + 2 * E].copy(), f(r[:, 5 + 2 * E:]).reshape(-1, E1))

    @property
    def loss(self) -> np.ndarray:
        """(T,) disagree / sampled, NaN where nobody was sampled."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.sampled > 0, self.disagree / np.maximum(self.sampled, 1), np.nan)

    def excess(self, alpha: float) -> np.ndarray:
        """(T,) running sum of ``loss - alpha`` over the rows that sampled anybody: what stays at or below ``start / gamma + 1 - alpha``."""
        return np.cumsum(np.where(self.sampled > 0, np.nan_to_num(self.loss) - float(alpha), 0.0))


@dataclass
class DeadlineLog:
    """The device log of a deadline (``EarlyExitEngine.deadline_log``): one row per deadline call, numpy on the host.  ``elapsed_ns[t, e]`` is
    the device time from the call's begin launch to the check in front of exit ``e``'s decision: the rows are a per-exit device timeline of
    the forward, and ``elapsed_ns[:, -1] - elapsed_ns[t, cut_exit[t]]`` is the tail of empty launches behind a cut."""
    call: np.ndarray                        # (T,) int64: the handle's deadline call number, from 1
    budget_ns: np.ndarray                   # (T,) uint64 (2^64 - 1: stamps only)
    cut_exit: np.ndarray                    # (T,) int64, -1: not cut
    cut_by: np.ndarray                      # (T,) int64: 0 nobody, 1 the clock, 2 the host
    elapsed_ns: np.ndarray                  # (T,E1) uint64

    @staticmethod
    def from_rows(rows, E1: int) -> "DeadlineLog":
        """From (T, deadline_log_words(E1)) int64 words as the device writes them (include/mmee.h)."""
        r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, capi.deadline_log_words(E1))
        return DeadlineLog(r[:, 0].copy(), r[:, 1].copy().view(np.uint64), r[:, 2].copy(), r[:, 3].copy(),
                           np.ascontiguousarray(r[:, 4:]).view(np.uint64).reshape(-1, E1))


def _require_torch_cuda(device=None):
    if torch is None:
        raise capi.MMEEUnavailable(f"PyTorch-ROCm is required for device tensors: {_torch_err}")
    if not torch.cuda.is_available():
        raise capi.MMEEUnavailable("no MI355X visible (torch.cuda.is_available() is False); the HIP path has no CPU fallback")
    return torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")


class EarlyExitEngine:
    """One handle on one GPU.  Not thread-safe (same as the reference's one-model-per-process use)."""

    def __init__(self, cfg: ModelConfig, max_docs: int = 64, max_text_len: int = 512, precision: str = "auto",
                 device=None, xprobe: Optional[bool] = None):
        """``xprobe``: what ``forward(xprobe=None)`` runs at probe-first exit layers.  ``None`` (default): the X-space CLS probe
        (MMEE_FLAG_XPROBE, csrc/xprobe.hip) wherever the library has it -- split precision, LayoutLMv3-base / -large shapes; the C side
        falls back to the K | V probe elsewhere.  It is the faster valid schedule and the one ``bench.py`` measures: exit indices equal,
        logits within the 1e-4 bar, but an exit's row is a re-association of the whole-layer arithmetic, NOT bit-identical to the dump-all
        row.  ``False`` pins the K | V probe, whose rows are bit-identical to whole layers (the parity suite's bit-identity tests ask
        for that)."""
        self.lib = capi.load()
        self.device = _require_torch_cuda(device)
        self.cfg = cfg
        self.exit_config = cfg.exit_config
        ec = self.exit_config
        self.max_docs, self.max_text_len = int(max_docs), int(max_text_len)
        self.E = ec.num_exits
        self.K = cfg.num_labels
        self.Kh = cfg.num_labels if str(ec.encoder_layer_strategy) == "ramp" else 2
        c = capi.EEConfig()
        c.abi_version = capi.ABI_VERSION
        for f in ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "vocab_size",
                  "max_position_embeddings", "type_vocab_size", "pad_token_id", "max_2d_position_embeddings",
                  "coordinate_size", "shape_size", "rel_pos_bins", "max_rel_pos", "rel_2d_pos_bins", "max_rel_2d_pos",
                  "input_size", "patch_size", "num_channels", "num_labels"):
            setattr(c, f, int(getattr(cfg, f)))
        c.layer_norm_eps = float(cfg.layer_norm_eps)
        emb = ec.embedding_exits
        c.n_embedding_exits = len(emb)
        for i, e in enumerate(emb):
            c.embedding_exits[i] = capi.EXIT_KIND[e]
        enc = ec.encoder_exit_layers
        if len(enc) > capi.MAX_ENCODER_EXITS:
            raise ValueError("too many encoder exits")
        c.n_encoder_exits = len(enc)
        for i, l in enumerate(enc):
            c.encoder_exit_layers[i] = int(l)
        c.exit_head_num_layers = int(ec.exit_head_num_layers)
        c.strategy = 0 if str(ec.encoder_layer_strategy) == "ramp" else 1
        c.criterion = ec.inference_strategy.code
        c.max_docs, c.max_text_len = self.max_docs, self.max_text_len
        if precision == "auto":      # split-f16 GEMMs where the shapes allow it (hidden / intermediate sizes multiples of 256)
            precision = "split" if (cfg.hidden_size % 256 == 0 and cfg.intermediate_size % 256 == 0) else "fp32"
        c.precision = {"fp32": 0, "f32": 0, "bf16": 1, "split": 2, "f32_split": 2}[precision]
        self.beit = cfg.arch == "beit"
        self.xprobe_default = (precision in ("split", "f32_split") and not self.beit) if xprobe is None else bool(xprobe)
        c.arch = 1 if self.beit else 0
        c.use_abs_pos = int(cfg.use_absolute_position_embeddings)
        c.layer_scale = int(cfg.layer_scale_init_value > 0)
        c.use_mean_pooling = int(cfg.use_mean_pooling)
        self.use_lte = bool(ec.use_lte)     # bound at ee_create: two more parameters, the LTE score as the exit test (include/mmee.h)
        c.use_lte = int(self.use_lte)
        if self.beit:
            c.max_text_len = self.max_text_len = 0
        self.precision = precision          # resolved: "fp32" or "split"
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            capi.check(self.lib.ee_create(C.byref(c), C.byref(self._h)), None, "ee_create")
        self._finalized = False
        self._stream_generation = 0         # forward_stream() calls so far: a ResultStream belongs to one of them
        self.ensemble = None                # set_ensemble(): the host copies of (weights, bias), or None
        self.quotas, self.quota_mode = None, None      # set_quotas(): the per-exit quotas and "exact" / "at_least", or None
        self.audit = None                   # set_audit(): (fraction, seed, slot_base), or None
        self.controller = None              # set_controller(): dict(path, alpha, gamma, start, seed, log_cap), or None
        self._ctl_calls = 0                 # controlled calls since set_controller: call t audits under seed + t
        self.deadline = None                # set_deadline(): dict(budget_ns, eta_ns, log_cap), or None
        self._dl_last_cap = 0               # the log_cap of the deadline that was removed last: its log stays readable
        self.patience = None
        if ec.patience is not None:
            self.set_patience(ec.patience)
        self.exit_rule = ExitRule.PLAIN
        if ec.exit_rule != ExitRule.PLAIN:
            self.set_exit_rule(ec.exit_rule)

    # ---- lifetime ------------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.ee_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- parameters ----------------------------------------------------------------------------------------------
    def expected_tensors(self):
        n = self.lib.ee_num_expected_tensors(self._h)
        return [self.lib.ee_expected_tensor_name(self._h, i).decode() for i in range(n)]

    def load_weights(self, weights: Mapping[str, Union[np.ndarray, "torch.Tensor"]], strict: bool = True):
        """Copy parameters (HF names) into the handle.  Extra entries are ignored unless ``strict`` finds one missing."""
        expected = self.expected_tensors()
        missing = [n for n in expected if n not in weights]
        if missing and strict:
            raise KeyError(f"{len(missing)} parameter(s) missing from the checkpoint, e.g. {missing[:4]}")
        with torch.cuda.device(self.device):
            for name in expected:
                if name not in weights:
                    continue
                t = weights[name]
                if torch is not None and isinstance(t, torch.Tensor):
                    t = t.detach()
                    if t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
                        t = t.float()
                    t = t.contiguous()
                    dt = {torch.float32: capi.DT_F32, torch.float16: capi.DT_F16, torch.bfloat16: capi.DT_BF16}[t.dtype]
                    if t.is_cuda:
                        if dt != capi.DT_F32:
                            t = t.float()
                            dt = capi.DT_F32
                        # ee_load_tensor copies on the null stream: whatever produced ``t`` on torch's current stream (the
                        # cast above, or the caller's own kernels) must have finished first
                        torch.cuda.current_stream(t.device).synchronize()
                    shape = (C.c_int64 * t.dim())(*t.shape)
                    rc = self.lib.ee_load_tensor(self._h, name.encode(), C.c_void_p(t.data_ptr()), shape, t.dim(), dt,
                                                 1 if t.is_cuda else 0)
                else:
                    a = np.ascontiguousarray(np.asarray(t), dtype=np.float32)
                    shape = (C.c_int64 * a.ndim)(*a.shape)
                    rc = self.lib.ee_load_tensor(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim,
                                                 capi.DT_F32, 0)
                capi.check(rc, self._h, f"ee_load_tensor({name})")
            capi.check(self.lib.ee_finalize(self._h), self._h, "ee_finalize")
        self._finalized = True

    @classmethod
    def from_pretrained(cls, path: str, max_docs: int = 64, max_text_len: int = 512, precision: str = "auto",
                        device=None, ee_config: Optional[dict] = None) -> "EarlyExitEngine":
        """Load a local HF-format checkpoint directory (config.json with ``EE_config`` + safetensors / .bin), the
        counterpart of ``LayoutLMv3EEForSequenceClassification.from_pretrained`` at EE/configs.py:404-411."""
        cfg = ModelConfig.from_pretrained(path)
        if ee_config:
            cfg.EE_config.update(ee_config)
        eng = cls(cfg, max_docs=max_docs, max_text_len=max_text_len, precision=precision, device=device)
        eng.load_weights(load_checkpoint_tensors(path))
        return eng

    # ---- the hot path --------------------------------------------------------------------------------------------
    def _dev(self, x, dtype, name, required=True):
        if x is None:
            if required:
                raise ValueError(f"{name} is required")
            return None
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(x)
        if not x.is_cuda or x.device != self.device:
            x = x.to(self.device, non_blocking=True)
        if x.dtype != dtype:
            x = x.to(dtype)
        return x.contiguous()

    def forward(self, input_ids=None, attention_mask=None, bbox=None, pixel_values=None, token_type_ids=None,
                position_ids=None, thresholds: Optional[Union[float, Sequence[float]]] = None,
                temperatures: Optional[Sequence[float]] = None, dump_all: bool = False, dense_rows: bool = False,
                want_all: bool = False, want_head: bool = False, want_hidden_cls: bool = False,
                validate: bool = False, whole_layers: bool = False, probe_always: bool = False, xprobe: Optional[bool] = None,
                one_term: bool = False, inputs_embeds=None, want_hidden_states: bool = False, out=None, head_mask=None,
                want_attentions: bool = False, patience: Optional[Union[int, Sequence[int]]] = None, exit_rule=None,
                low_latency: bool = False, quotas: Optional[Sequence[int]] = None, quota_mode: Optional[str] = None,
                quota_fractions: Optional[Sequence[float]] = None, audit_fraction: Optional[float] = None,
                audit_seed: Optional[int] = None, deadline_ms: Optional[float] = None, _capture: bool = False,
                _stream: bool = False) -> EngineOutput:
        """``out``: optional preallocated ``(logits (B,K) f32, exit_layer (B,) i32, confidence (B,) f32)`` device tensors (contiguous; row
        slices of larger tensors qualify) the kernels write into instead of fresh allocations -- MicroBatchedEngine hands each half its slice.
        ``patience``: when given, ``set_patience(patience)`` before the call (an int, or one entry per exit; it matters under the "patience"
        criterion and under the two combined exit rules); under the patience criterion ``thresholds`` are ignored.  ``exit_rule``: when
        given, ``set_exit_rule(exit_rule)`` before the call.  Both stay set for later calls; a capture binds the rule.
        ``low_latency``: MMEE_FLAG_LOW_LATENCY, for batches of a few documents (the reference's ``eval_batch_size = 1``): the attention-output and
        FFN-down GEMMs of every layer run as split-K wherever ``capi`` ``ee_low_latency_k_splits`` allows it for this (B, T) -- see
        ``last_k_splits()``.  Same exits, logits within the 1e-4 bar, not the bits of the call without it; split precision, LayoutLMv3 only.
        ``quotas`` / ``quota_fractions`` / ``quota_mode``: when given, ``set_quotas(...)`` before the call (budgeted exits: every exit releases
        the most confident documents of THIS call, a chosen number of them; ``set_quotas``).  ``quota_fractions`` is the convenience: the share
        of the call's B documents per exit, turned into integers by ``sweep.quotas_from_fractions``.  They stay set for later calls, like the
        patience; ``set_quotas(None)`` switches them off.  Under ``quota_mode="exact"`` the thresholds are not read.
        ``audit_fraction`` / ``audit_seed``: when given, ``set_audit(audit_fraction, seed=audit_seed)`` before the call (audited exits: a hashed
        sample of the call's documents is delivered where it leaves and runs on to the final exit; with ``want_all=True`` its columns come
        back complete, ``output.audit_mask`` says which).  ``audit_seed`` alone re-seeds the audit that is set (vary it per call).  Both stay
        set for later calls; ``set_audit(None)`` switches the audit off.
        ``deadline_ms``: the budget of THIS call on an engine that has a deadline (``set_deadline``), in place of the engine's; the engine's
        ``eta`` table and log are used, nothing is synchronised, and the engine's own budget is back for the next call.  The override sets
        and restores the handle's budget around the enqueue: an engine is driven by one thread, and this is not safe next to another thread's
        ``forward`` or ``set_deadline`` on the same engine (``request_cut`` is).  Refused with ``capture``."""
        if not self._finalized:
            raise capi.MMEEError("load_weights() has not been called")
        if patience is not None:
            self.set_patience(patience)
        if exit_rule is not None:
            self.set_exit_rule(exit_rule)
        R = self.cfg.input_size
        px = self._dev(pixel_values, torch.float32, "pixel_values")
        emb = None
        if self.beit:                                   # image-only: (B,3,R,R) is the whole input
            if inputs_embeds is not None:
                raise ValueError("inputs_embeds: an image-only model has no text embeddings")
            ids = am = bb = tt = ps = None
            B, T = px.shape[0], 0
            if tuple(px.shape) != (B, self.cfg.num_channels, R, R):
                raise ValueError(f"pixel_values must be (B,{self.cfg.num_channels},{R},{R})")
        else:
            if inputs_embeds is not None:
                # EE/models/LayoutLMv3.py:414-417 -> HF:160-199: the rows replace word_embeddings(input_ids).  Without input_ids the position
                # ids are the sequential ones of HF:148-158 (nothing says which position is padding); the C-ABI still wants token ids for
                # its validation, so it gets pad-free dummies.  With BOTH, HF takes the position ids from input_ids and the rows from here.
                emb = self._dev(inputs_embeds, torch.float32, "inputs_embeds")
                if emb.dim() != 3 or emb.shape[2] != self.cfg.hidden_size:
                    raise ValueError(f"inputs_embeds must be (B,T,{self.cfg.hidden_size})")
                if input_ids is None:
                    Bq, Tq = emb.shape[:2]
                    pad = self.cfg.pad_token_id
                    input_ids = torch.full((Bq, Tq), 0 if pad != 0 else 1, dtype=torch.int64, device=self.device)
                    if position_ids is None:
                        position_ids = torch.arange(pad + 1, Tq + pad + 1, dtype=torch.int64, device=self.device).unsqueeze(0).expand(Bq, Tq)
            ids = self._dev(input_ids, torch.int64, "input_ids")
            B, T = ids.shape
            if emb is not None and tuple(emb.shape[:2]) != (B, T):
                raise ValueError("inputs_embeds and input_ids disagree on (B,T)")
            if bbox is None:
                bbox = torch.zeros((B, T, 4), dtype=torch.int64, device=self.device)   # EE/models/LayoutLMv3.py:433-436
            am = self._dev(attention_mask, torch.int64, "attention_mask", required=False)
            bb = self._dev(bbox, torch.int64, "bbox")
            tt = self._dev(token_type_ids, torch.int64, "token_type_ids", required=False)
            ps = self._dev(position_ids, torch.int64, "position_ids", required=False)
            if tuple(bb.shape) != (B, T, 4) or tuple(px.shape) != (B, self.cfg.num_channels, R, R):
                raise ValueError(f"bbox must be (B,T,4) and pixel_values (B,{self.cfg.num_channels},{R},{R}); got "
                                 f"{tuple(bb.shape)} / {tuple(px.shape)}")
        for t, n in ((am, "attention_mask"), (tt, "token_type_ids"), (ps, "position_ids")):
            if t is not None and tuple(t.shape) != (B, T):
                raise ValueError(f"{n} must be (B,T)")
        E, K = self.E, self.K
        if quotas is not None and quota_fractions is not None:
            raise ValueError("quotas and quota_fractions are two ways to say the same thing: pass one")
        if quota_fractions is not None:
            from .sweep import quotas_from_fractions
            quotas = quotas_from_fractions(B, quota_fractions, E)
        if quotas is not None:
            self.set_quotas(quotas, mode=quota_mode or self.quota_mode or "exact")
        elif quota_mode is not None:
            raise ValueError("quota_mode= goes with quotas= or quota_fractions= (set_quotas(None) switches quotas off)")
        if audit_fraction is not None or audit_seed is not None:
            self.forward_audit_args(audit_fraction, audit_seed)
        controlled = self.controller is not None and not dump_all      # the library's own rule: a dump-all call ignores the controller
        if controlled and thresholds is not None:
            raise ValueError("forward(thresholds=) on a controlled engine: the controller's position decides the thresholds "
                             "(controller_state()[\"thresholds\"] shows them; set_controller(None) switches it off)")
        if thresholds is None:
            thresholds = self.exit_config.global_threshold
        thr = np.broadcast_to(np.asarray(thresholds, dtype=np.float64).reshape(-1), (E + 1,)).copy() \
            if np.ndim(thresholds) else np.full((E + 1,), float(thresholds))
        thr_c = None if controlled else (C.c_double * (E + 1))(*thr.tolist())
        tmp_c = None
        if temperatures is not None:
            tm = np.asarray(temperatures, dtype=np.float64).reshape(-1)
            if tm.shape[0] != E + 1:
                raise ValueError(f"temperatures must have {E + 1} entries")
            tmp_c = (C.c_double * (E + 1))(*tm.tolist())
        dev = self.device
        if out is not None:
            out_logits, out_exit, out_conf = out
            for t, shp, dt in ((out_logits, (B, K), torch.float32), (out_exit, (B,), torch.int32), (out_conf, (B,), torch.float32)):
                if tuple(t.shape) != shp or t.dtype != dt or not t.is_contiguous() or t.device != dev:
                    raise ValueError(f"out: expected a contiguous {dt} tensor of shape {shp} on {dev}")
        else:
            out_logits = torch.empty((B, K), dtype=torch.float32, device=dev)
            out_exit = torch.empty((B,), dtype=torch.int32, device=dev)
            out_conf = torch.empty((B,), dtype=torch.float32, device=dev)
        nan = float("nan")
        all_logits = torch.full((E + 1, B, K), nan, dtype=torch.float32, device=dev) if want_all else None
        all_crit = torch.full((E + 1, B), nan, dtype=torch.float32, device=dev) if want_all else None
        head_logits = torch.full((E, B, self.Kh), nan, dtype=torch.float32, device=dev) if want_head else None
        head_crit = torch.full((E, B), nan, dtype=torch.float32, device=dev) if want_head else None
        hidden = torch.full((self.cfg.num_hidden_layers + 1, B, self.cfg.hidden_size), nan, dtype=torch.float32,
                            device=dev) if want_hidden_cls else None
        if xprobe is None:
            xprobe = self.xprobe_default
        hs = None
        if want_hidden_states:
            # output_hidden_states of the reference (EE/models/LayoutLMv3.py:182-183, 284-285): dump-all, whole layers; dense rows so that
            # the positions the mask drops hold what the reference computes for them
            if not dump_all:
                raise ValueError("want_hidden_states needs dump_all=True (nobody may leave early)")
            whole_layers, dense_rows, xprobe = True, True, False
            S = T + (self.cfg.input_size // self.cfg.patch_size) ** 2 + 1
            hs = torch.empty((self.cfg.num_hidden_layers + 1, B, S, self.cfg.hidden_size), dtype=torch.float32, device=dev)
        hm = att = None
        if head_mask is not None or want_attentions:
            # head_mask / output_attentions of the reference signature (EE/models/LayoutLMv3.py:382-385, 631-641): side kernels of the dump-all,
            # whole-layers forward (csrc/attention_maps.hip); the fused attention kernels of the hot path never see either
            if self.beit:
                raise NotImplementedError("head_mask / attention maps are built for the LayoutLMv3 layers only")
            if not dump_all:
                raise ValueError("head_mask / want_attentions need dump_all=True (they belong to model.forward, not to the early-exit path)")
            whole_layers, xprobe = True, False
            L_, nh = self.cfg.num_hidden_layers, self.cfg.num_attention_heads
            if head_mask is not None:
                # get_head_mask (transformers 4.26 modeling_utils): (heads,) is broadcast over the layers, (L, heads) is taken as is
                hm = self._dev(head_mask, torch.float32, "head_mask")
                if hm.dim() == 1:
                    hm = hm.unsqueeze(0).expand(L_, -1)
                if tuple(hm.shape) != (L_, nh):
                    raise ValueError(f"head_mask must be ({nh},) or ({L_}, {nh})")
                hm = hm.contiguous()
            if want_attentions:
                dense_rows = True
                S = T + (self.cfg.input_size // self.cfg.patch_size) ** 2 + 1
                att = torch.empty((L_, B, nh, S, S), dtype=torch.float32, device=dev)
        flags = ((capi.FLAG_NO_EXIT if dump_all else 0) | (capi.FLAG_DENSE_ROWS if dense_rows else 0) |
                 (capi.FLAG_WHOLE_LAYERS if whole_layers else 0) | (capi.FLAG_PROBE_ALWAYS if probe_always else 0) |
                 (capi.FLAG_XPROBE if xprobe else 0) | (capi.FLAG_ONE_TERM if one_term else 0) |
                 (capi.FLAG_LOW_LATENCY if low_latency else 0) | (capi.FLAG_STREAM_RESULTS if _stream else 0))
        # one_term: REPORTED low-precision mode (one f16 MFMA term per MAC instead of three in the layer GEMMs and the attention); outside the
        # 1e-4 bar by construction, exit indices may flip -- bench.py's `lowprec` field, never a result to rely on
        # xprobe: probe-first layers take the CLS context in X space (no Q | K | V for documents that leave); same exits, logits within
        # tolerance, not bit-identical to whole layers
        # whole_layers / probe_always override the handle's schedule for this call (default: every decision layer probed first, or the mask pin_schedule() set)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        if deadline_ms is not None and _capture:
            raise ValueError("capture(deadline_ms=): deadline calls are eager, a captured graph carries no deadline")
        if _capture:
            # ee_graph_capture: the same call eagerly (the outputs hold its results), then its launch list as a hipGraph bound to THESE tensors
            if emb is not None or hs is not None or hm is not None or att is not None or validate:
                raise ValueError("capture(): inputs_embeds / hidden states / head_mask / attention maps / validate belong to eager calls")
            gid = C.c_int32(-1)
            with torch.cuda.device(dev):
                cur = torch.cuda.current_stream()
                if getattr(self, "_cap_stream", None) is None:
                    self._cap_stream = torch.cuda.Stream(device=dev)      # the legacy null stream (torch's default) cannot be captured
                self._cap_stream.wait_stream(cur)
                rc = self.lib.ee_graph_capture(self._h, p(ids), p(am), p(bb), p(px), p(tt), p(ps), B, T, thr_c, tmp_c, flags,
                                               p(out_logits), p(out_exit), p(out_conf), p(all_logits), p(all_crit),
                                               p(head_logits), p(head_crit), p(hidden), C.c_void_p(self._cap_stream.cuda_stream), C.byref(gid))
                capi.check(rc, self._h, "ee_graph_capture")
                cur.wait_stream(self._cap_stream)
            res = EngineOutput(out_logits, out_exit, out_conf, all_logits, all_crit, head_logits, head_crit, hidden, None, None)
            ins = dict(input_ids=ids, attention_mask=am, bbox=bb, pixel_values=px, token_type_ids=tt, position_ids=ps)
            return CapturedForward(self, gid.value, {k: v for k, v in ins.items() if v is not None}, res)
        if deadline_ms is not None and self.deadline is None:
            raise ValueError("forward(deadline_ms=) overrides the budget of an engine that has a deadline: set_deadline(...) first "
                             "(set_deadline(None, stamps_only=True) for an engine whose calls are otherwise not cut)")
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            if emb is not None:
                capi.check(self.lib.ee_set_inputs_embeds(self._h, p(emb)), self._h, "ee_set_inputs_embeds")
            if hs is not None:
                capi.check(self.lib.ee_set_hidden_states_out(self._h, p(hs)), self._h, "ee_set_hidden_states_out")
            if hm is not None:
                capi.check(self.lib.ee_set_head_mask(self._h, p(hm)), self._h, "ee_set_head_mask")
            if att is not None:
                capi.check(self.lib.ee_set_attentions_out(self._h, p(att)), self._h, "ee_set_attentions_out")
            if deadline_ms is not None:                # budget and eta are arguments of this call's launches: set for it, put back behind it
                self._apply_deadline(self._budget_ns(deadline_ms), self.deadline["eta_ns"])
            rc = self.lib.ee_forward(self._h, p(ids), p(am), p(bb), p(px), p(tt), p(ps), B, T, thr_c, tmp_c, flags,
                                     p(out_logits), p(out_exit), p(out_conf), p(all_logits), p(all_crit),
                                     p(head_logits), p(head_crit), p(hidden), stream)
            if deadline_ms is not None:
                self._apply_deadline(self.deadline["budget_ns"], self.deadline["eta_ns"])
        capi.check(rc, self._h, "ee_forward")
        ctl_call = self._ctl_calls
        if controlled:                                 # the library has used this call's seed: count it before anything else can raise
            self._ctl_calls += 1
        self._keepalive = (ids, am, bb, px, tt, ps, emb, hm)   # borrowed by the enqueued kernels until the stream drains
        if validate:
            self.stage_counts()                        # synchronises; raises on out-of-range inputs
        mask = None
        if self.audit and not dump_all:                # the library's own rule: a dump-all call ignores the audit
            fraction, seed, slot_base = self.audit
            if controlled:                             # call t of a controller audits under seed + t
                seed = (self.controller["seed"] + ctl_call) & 0xFFFFFFFF
            mask = torch.from_numpy(self.audit_mask(B, fraction, seed, slot_base)).to(dev, non_blocking=True)
        return EngineOutput(out_logits, out_exit, out_conf, all_logits, all_crit, head_logits, head_crit, hidden, hs, att, mask)

    __call__ = forward

    def embedding_inputs(self, input_ids=None, attention_mask=None, bbox=None, pixel_values=None, token_type_ids=None, position_ids=None,
                         kinds: Optional[Sequence[str]] = None) -> Dict[str, "torch.Tensor"]:
        """The rows the embedding-level exit heads read, from stage 0 of the forward alone (``ee_embedding_inputs``, include/mmee.h): no
        encoder layer runs.  Returns ``{kind: (B,H) float32 device tensor}`` for ``kinds``, any non-empty subset of
        ``config.EMBEDDING_EXITS``, in the reference's order (vision, text, concat); default: the configuration's embedding exits.  Works
        on every LayoutLMv3 engine, whichever embedding exits it names; the bits are those a ``forward`` of this engine feeds the heads.
        The text and concat means run over all T positions of the call, padding included (the reference pads to ``max_length``): call at
        the T that deployment runs.  Inputs are converted as in ``forward``; the call only enqueues on the current stream, and out-of-range
        inputs are reported as after ``forward`` (by the next call, or ``check()`` once a forward has run)."""
        if not self._finalized:
            raise capi.MMEEError("load_weights() has not been called")
        if self.beit:
            raise ValueError("embedding_inputs: embedding-level exits belong to LayoutLMv3; an image-only model has none")
        kinds = list(self.exit_config.embedding_exits) if kinds is None else [str(k) for k in kinds]
        unknown = [k for k in kinds if k not in EMBEDDING_EXITS]
        if unknown:
            raise ValueError(f"embedding_inputs: {unknown} not among {list(EMBEDDING_EXITS)}")
        kinds = [k for k in EMBEDDING_EXITS if k in kinds]
        if not kinds:
            raise ValueError("embedding_inputs: no kinds (the configuration names no embedding-level exit: pass kinds=)")
        R, H = self.cfg.input_size, self.cfg.hidden_size
        px = self._dev(pixel_values, torch.float32, "pixel_values")
        ids = self._dev(input_ids, torch.int64, "input_ids")
        if ids.dim() != 2:
            raise ValueError("input_ids must be (B,T)")
        B, T = ids.shape
        if bbox is None:
            bbox = torch.zeros((B, T, 4), dtype=torch.int64, device=self.device)       # EE/models/LayoutLMv3.py:433-436
        am = self._dev(attention_mask, torch.int64, "attention_mask", required=False)
        bb = self._dev(bbox, torch.int64, "bbox")
        tt = self._dev(token_type_ids, torch.int64, "token_type_ids", required=False)
        ps = self._dev(position_ids, torch.int64, "position_ids", required=False)
        if tuple(bb.shape) != (B, T, 4) or tuple(px.shape) != (B, self.cfg.num_channels, R, R):
            raise ValueError(f"bbox must be (B,T,4) and pixel_values (B,{self.cfg.num_channels},{R},{R}); got "
                             f"{tuple(bb.shape)} / {tuple(px.shape)}")
        for t, n in ((am, "attention_mask"), (tt, "token_type_ids"), (ps, "position_ids")):
            if t is not None and tuple(t.shape) != (B, T):
                raise ValueError(f"{n} must be (B,T)")
        out = {k: torch.empty((B, H), dtype=torch.float32, device=self.device) for k in kinds}
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            rc = self.lib.ee_embedding_inputs(self._h, p(ids), p(am), p(bb), p(px), p(tt), p(ps), B, T, *[p(out.get(k)) for k in EMBEDDING_EXITS],
                                              stream)
        capi.check(rc, self._h, "ee_embedding_inputs")
        self._keepalive = (ids, am, bb, px, tt, ps)   # borrowed by the enqueued kernels until the stream drains
        return out

    # ---- vision first: OCR only for the documents the image keeps (the definition is in include/mmee.h at ee_forward_vision) ----------------
    def _exit_vectors(self, thresholds, temperatures):
        """thresholds (a scalar, or one entry per exit; None: the configuration's) and temperatures as the (E + 1,) C arrays of ee_forward."""
        E = self.E
        if thresholds is None:
            thresholds = self.exit_config.global_threshold
        thr = np.broadcast_to(np.asarray(thresholds, dtype=np.float64).reshape(-1), (E + 1,)).copy() \
            if np.ndim(thresholds) else np.full((E + 1,), float(thresholds))
        tmp_c = None
        if temperatures is not None:
            tm = np.asarray(temperatures, dtype=np.float64).reshape(-1)
            if tm.shape[0] != E + 1:
                raise ValueError(f"temperatures must have {E + 1} entries")
            tmp_c = (C.c_double * (E + 1))(*tm.tolist())
        return (C.c_double * (E + 1))(*thr.tolist()), tmp_c

    def forward_vision(self, pixel_values, thresholds: Optional[Union[float, Sequence[float]]] = None,
                       temperatures: Optional[Sequence[float]] = None, out=None) -> VisionPhase:
        """Phase 1 of a vision-first call (``ee_forward_vision``): from ``pixel_values`` (B,C,R,R) alone, the vision_avg exit -- exit 0 of an
        engine whose exit list names it -- exactly as ``forward`` decides it.  The documents that leave there get ``logits`` / ``exit_layer``
        = 0 / ``confidence`` with the bits of the one-call ``forward``; the others have nothing written and their slots come back in
        ``survivors`` (ascending) with their number in ``count``, both on the device.  ``thresholds`` / ``temperatures`` as in ``forward``
        (entry 0 is read).  ``out``: as in ``forward``.  The call only enqueues, keeps no state a later call needs and leaves
        ``stage_counts()`` / ``flops()`` / ``profile_read()`` describing the last ``forward``: phase 1 of the next batch may run while OCR
        works on this one.  Refused by the library with a message: image-only engines, no vision_avg, quotas, an audit, a controller."""
        if not self._finalized:
            raise capi.MMEEError("load_weights() has not been called")
        R = self.cfg.input_size
        px = self._dev(pixel_values, torch.float32, "pixel_values")
        if px.dim() != 4 or tuple(px.shape[1:]) != (self.cfg.num_channels, R, R):
            raise ValueError(f"pixel_values must be (B,{self.cfg.num_channels},{R},{R})")
        B, K, dev = int(px.shape[0]), self.K, self.device
        thr_c, tmp_c = self._exit_vectors(thresholds, temperatures)
        if out is not None:
            out_logits, out_exit, out_conf = out
            for t, shp, dt in ((out_logits, (B, K), torch.float32), (out_exit, (B,), torch.int32), (out_conf, (B,), torch.float32)):
                if tuple(t.shape) != shp or t.dtype != dt or not t.is_contiguous() or t.device != dev:
                    raise ValueError(f"out: expected a contiguous {dt} tensor of shape {shp} on {dev}")
        else:
            out_logits = torch.empty((B, K), dtype=torch.float32, device=dev)
            out_exit = torch.empty((B,), dtype=torch.int32, device=dev)
            out_conf = torch.empty((B,), dtype=torch.float32, device=dev)
        survivors = torch.empty((max(B, 1),), dtype=torch.int32, device=dev)
        count = torch.empty((1,), dtype=torch.int32, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            rc = self.lib.ee_forward_vision(self._h, p(px), B, thr_c, tmp_c, 0, p(out_logits), p(out_exit), p(out_conf), p(survivors), p(count),
                                            stream)
        capi.check(rc, self._h, "ee_forward_vision")
        self._keepalive = (px,)             # borrowed by the enqueued kernels until the stream drains
        return VisionPhase(EngineOutput(out_logits, out_exit, out_conf), survivors, count)

    def forward_vision_first(self, pixel_values, text, thresholds: Optional[Union[float, Sequence[float]]] = None,
                             temperatures: Optional[Sequence[float]] = None, low_latency: bool = False, xprobe: Optional[bool] = None,
                             whole_layers: bool = False, probe_always: bool = False, **not_built) -> VisionFirstOutput:
        """The vision-first call: ``forward_vision`` on all B documents, then an ordinary ``forward`` on the survivors of exit 0 with text
        that is supplied only now.  Returns, bit for bit, the ``logits`` / ``exit_layer`` / ``confidence`` of ``forward`` on the full inputs,
        ``stage`` (0 = answered from the pixels, 1 = ran with text) and ``text_docs``, the number of documents that needed text.
        ``text`` is either a dict of the caller's full arrays (``input_ids``, ``attention_mask``, ``bbox``, optional ``token_type_ids`` /
        ``position_ids``, B rows each): the survivors' rows and their pixel rows are gathered in one launch and the count stays on the
        device; or a callable ``f(slots: np.ndarray) -> dict`` as in ``CascadeEngine``: called once, only when somebody survives, with the
        survivors' slots (ascending), it returns their rows in that order -- OCR only for the pages the image keeps.  The text and concat
        exits average over all T positions of the call, padding included: the callable must pad to the T deployment runs, or the bits
        (and the decisions) are those of another T.  One 4-byte host read (the count) behind one stream wait; the callable route also
        downloads the slots.  ``low_latency`` / ``xprobe`` / ``whole_layers`` / ``probe_always`` go to phase 2 (they concern the layers, and
        the equality above is with ``forward`` under the same ones); under ``low_latency=True`` the bits are those of
        ``forward(low_latency=True)`` on the survivors' sub-batch, not of the one-call forward.
        Not built, refused: ``want_all`` / ``want_head`` / ``want_hidden_cls`` / ``dump_all`` outputs, a result stream, a captured graph,
        quotas, audits, controllers (the library's messages), ``MicroBatchedEngine`` and a vision-first stage of a ``CascadeEngine``."""
        for k in not_built:
            if k in ("want_all", "want_head", "want_hidden_cls", "want_hidden_states", "want_attentions", "dump_all", "head_mask"):
                raise ValueError(f"forward_vision_first: {k} belongs to a dump-all forward, where nobody leaves at exit 0 (not built)")
            if k in ("_stream", "stream", "_capture", "capture"):
                raise ValueError(f"forward_vision_first: {k}: a vision-first call under a result stream or a captured graph is not built (phase 2's "
                                 "batch size depends on the data)")
            raise ValueError(f"forward_vision_first: {k} is not an argument of a vision-first call")
        if not (callable(text) or isinstance(text, Mapping)):
            raise ValueError("forward_vision_first: text is a dict of the caller's full arrays or a callable f(slots) -> dict")
        px = self._dev(pixel_values, torch.float32, "pixel_values")
        dev, K = self.device, self.K
        arrays = None
        if not callable(text):
            arrays = {k: self._dev(text[k], torch.int64, k) for k in _TEXT_KEYS if text.get(k) is not None}
            if "input_ids" not in arrays:
                raise ValueError("forward_vision_first: text needs input_ids")
            for k, v in arrays.items():
                if int(v.shape[0]) != int(px.shape[0]):
                    raise ValueError(f"forward_vision_first: {k} has {int(v.shape[0])} rows for a call of {int(px.shape[0])} documents")
        with torch.cuda.device(dev):
            phase = self.forward_vision(px, thresholds, temperatures)
            B = int(px.shape[0])
            out = phase.output
            stage = torch.zeros((B,), dtype=torch.int32, device=dev)
            if getattr(self, "_vf_count_host", None) is None:
                self._vf_count_host = torch.empty((1,), dtype=torch.int32).pin_memory()
            # the one host read of the seam: 4 bytes behind one stream wait (phase 2's ee_forward takes its batch size by value)
            self._vf_count_host.copy_(phase.count, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            m = int(self._vf_count_host[0])
            if m == 0:
                return VisionFirstOutput(out.logits, out.exit_layer, out.confidence, stage, 0)
            slots = phase.survivors[:m]
            src = {"pixel_values": px}
            if callable(text):
                rows = text(slots.cpu().numpy())
                sub = {k: self._dev(rows[k], torch.int64, k) for k in _TEXT_KEYS if rows.get(k) is not None}
                if "input_ids" not in sub:
                    raise ValueError("forward_vision_first: the callable's dict needs input_ids")
                bad = {k: int(v.shape[0]) for k, v in sub.items() if int(v.shape[0]) != m}
                if bad:
                    raise ValueError(f"forward_vision_first: the callable returned {bad} rows for {m} surviving documents")
            else:
                sub = {}
                src.update(arrays)
            descs = (capi.CascadeDesc * capi.CASCADE_MAX_ARRAYS)()
            for i, (k, v) in enumerate(src.items()):
                sub[k] = torch.empty((m,) + tuple(v.shape[1:]), dtype=v.dtype, device=dev)
                descs[i].src, descs[i].dst = v.data_ptr(), sub[k].data_ptr()
                descs[i].row_bytes = (v.numel() // B) * v.element_size()
            ptr = lambda t: C.c_void_p(t.data_ptr())
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            capi.check(self.lib.ee_cascade_gather(descs, len(src), ptr(slots), ptr(phase.count), m, stream), None, "ee_cascade_gather")
            res = self.forward(**sub, thresholds=thresholds, temperatures=temperatures, low_latency=low_latency, xprobe=xprobe,
                               whole_layers=whole_layers, probe_always=probe_always)
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            capi.check(self.lib.ee_cascade_merge(ptr(res.logits), ptr(res.exit_layer), ptr(res.confidence), ptr(slots), m, K, 0, 1,
                                                 ptr(out.logits), ptr(out.exit_layer), ptr(out.confidence), ptr(stage), stream), None,
                       "ee_cascade_merge")
            self._keepalive = (self._keepalive, src, sub, res, phase)      # borrowed by the enqueued launches until the stream drains
        return VisionFirstOutput(out.logits, out.exit_layer, out.confidence, stage, m)

    def forward_stream(self, *args, **kw) -> ResultStream:
        """``forward`` with MMEE_FLAG_STREAM_RESULTS (include/mmee.h): same arguments, same device outputs (``.output``), and the returned
        ``ResultStream`` yields the documents to the host as they leave -- one ``ResultChunk`` per evaluated exit, E + 1 in all, the first ones
        while the deeper layers still run for the documents that stay.  Costs one small launch per exit.  Nobody leaves early in dump-all mode
        and the side outputs of ``model.forward`` belong to it, so ``dump_all``, ``want_hidden_states``, ``head_mask``, ``want_attentions`` and
        ``_capture`` raise ``ValueError``.  One stream per engine at a time: the next ``forward_stream`` drops what was not read."""
        for k in ("dump_all", "want_hidden_states", "want_attentions", "_capture"):
            if kw.get(k):
                raise ValueError(f"forward_stream: {k} does not go with a result stream (nobody leaves early in dump-all mode; captured graphs "
                                 "carry no events)")
        if kw.get("head_mask") is not None:
            raise ValueError("forward_stream: head_mask belongs to the dump-all forward")
        out = self.forward(*args, _stream=True, **kw)
        self._stream_generation += 1
        return ResultStream(self, out)

    def capture(self, *args, **kw) -> "CapturedForward":
        """The forward as a captured launch list (ee_graph_capture; round 6): same arguments as ``forward``.  The call runs once eagerly --
        the returned object's ``outputs`` hold its results -- and its launch list is instantiated as a hipGraph bound to the device tensors
        of THIS call: ``captured.inputs`` are static buffers (``captured.inputs["input_ids"].copy_(next_batch)``), ``captured.outputs`` are
        rewritten by every ``captured.launch(thresholds=..., temperatures=...)``.  Thresholds and temperatures are arguments of the launch,
        everything else ((B, T), flags, which optional outputs exist, the pinned exit-layer schedule) is part of the capture.  For the
        reference's operating point (eval_batch_size = 1, EE/configs.py:36; EE/utils.py:169-193): ~185 kernel launches per forward become
        one graph launch.  Replays return the bits of the eager call on the same inputs.  Device tensors of the right dtype are BORROWED as they are
        (no copy, as in ``forward``): hand in clones when the caller's own tensors must not become the graph's buffers."""
        return self.forward(*args, _capture=True, **kw)

    def check(self):
        """Synchronise and raise ``MMEEError`` if the last forward flagged out-of-range inputs or a split-precision overflow
        (``forward`` itself only enqueues; an unchecked error is also reported by the next ``forward`` call)."""
        self.stage_counts()

    # ---- statistics of the last forward (both synchronise) ----------------------------------------------------------
    def stage_counts(self):
        n = self.E + 1
        docs, rows, ns = (C.c_int32 * n)(), (C.c_int32 * n)(), C.c_int32()
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            capi.check(self.lib.ee_last_stage_counts(self._h, docs, rows, n, C.byref(ns), stream), self._h,
                       "ee_last_stage_counts")
        return {"docs": list(docs)[:ns.value], "rows": list(rows)[:ns.value]}

    def last_k_splits(self):
        """(attention-output, FFN-down): the split-K parts the layers' two residual GEMMs ran with in the last forward or graph launch
        (ee_last_k_splits); (1, 1) without ``low_latency`` or where the rule declined.  Does not synchronise."""
        a, d = C.c_int32(), C.c_int32()
        capi.check(self.lib.ee_last_k_splits(self._h, C.byref(a), C.byref(d)), self._h, "ee_last_k_splits")
        return a.value, d.value

    def profile(self, enable: bool = True):
        """Arm / disarm per-kernel HIP-event timing of the following forward calls."""
        capi.check(self.lib.ee_profile(self._h, 1 if enable else 0), self._h, "ee_profile")

    def profile_read(self):
        """{role: {"symbol", "ms", "launches"}} of the last forward run with profiling armed (synchronises)."""
        out = {}
        buf = C.create_string_buffer(160)
        idx = 0
        while True:
            ms, n = C.c_double(), C.c_int32()
            rc = self.lib.ee_profile_read(self._h, idx, buf, 160, C.byref(ms), C.byref(n))
            if rc != 0:
                break
            role, _, sym = buf.value.decode().partition("|")
            out[role] = {"symbol": sym, "ms": ms.value, "launches": n.value}
            idx += 1
        return out

    def flops(self):
        g, a = C.c_double(), C.c_double()
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            capi.check(self.lib.ee_last_flops(self._h, C.byref(g), C.byref(a), stream), self._h, "ee_last_flops")
        plan = self.layer_plan()
        return {"gemm": g.value, "attention": a.value, "probe": plan["probe_flops"],
                "total": g.value + a.value + plan["probe_flops"]}

    def pin_schedule(self, probe_layers=None, xprobe: Optional[bool] = None):
        """Pin which exit layers are probed first (ee_set_probe_mask).  The DEFAULT schedule probes every layer that ends in a decision and
        never changes by itself: the same call always issues the same launches and returns the same bits (round 5; rounds 2-4 let the
        library choose from whichever earlier forward had finished, a timing-dependent decision).  ``probe_layers``: iterable of 0-based layer
        indices; ``None`` asks the library's cost model which layers pay, judged from the stage populations of the LAST forward, which must
        have been a thresholded one (ee_suggest_probe_mask; synchronises), and pins that; ``False`` returns to the default.  Returns the
        pinned list (None for the default).  The mask is part of the handle's state until changed."""
        if probe_layers is False:
            capi.check(self.lib.ee_set_probe_mask(self._h, 0, 0), self._h, "ee_set_probe_mask")
            self._pinned = False
            return None
        if probe_layers is None:
            xp = self.xprobe_default if xprobe is None else bool(xprobe)
            m = C.c_uint64()
            with torch.cuda.device(self.device):
                stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                capi.check(self.lib.ee_suggest_probe_mask(self._h, capi.FLAG_XPROBE if xp else 0, C.byref(m), stream), self._h,
                           "ee_suggest_probe_mask")
            probe_layers = [l for l in range(self.cfg.num_hidden_layers) if (m.value >> l) & 1]
        layers = sorted(int(l) for l in probe_layers)
        mask = 0
        for l in layers:
            mask |= 1 << l
        capi.check(self.lib.ee_set_probe_mask(self._h, 1, mask), self._h, "ee_set_probe_mask")
        self._pinned = True
        return layers

    def set_criterion(self, strategy):
        """Exit criterion of every later forward ("max_confidence" / "entropy" / "margin" / "patience" / "gate", the last on gate handles
        only; ee_set_criterion).  The reference's driver overrides
        ``model.config.exit_config["inference_strategy"]`` after construction (EE/utils.py:62-78); modeling.py forwards that write here."""
        from .config import EarlyExitInference
        st = strategy if isinstance(strategy, EarlyExitInference) else EarlyExitInference(str(strategy))
        capi.check(self.lib.ee_set_criterion(self._h, st.code), self._h, "ee_set_criterion")
        self.exit_config.inference_strategy = st
        return st

    def set_patience(self, t: Union[int, Sequence[int]]):
        """Patience of every later forward and graph launch under the "patience" criterion (ee_set_patience): a document leaves at the first
        exit where its argmax has stayed the same for ``t`` exits in a row (include/mmee.h).  Captured graphs read the current value at every
        launch.  A sequence is a per-exit patience, one entry per exit and the final classifier (ee_set_patience_vector).  The same value
        serves the exit rules "patient_confident" and "patience_or_threshold" (``set_exit_rule``)."""
        t = check_patience_spec(t, self.E + 1)
        if isinstance(t, list):
            capi.check(self.lib.ee_set_patience_vector(self._h, (C.c_int32 * len(t))(*t), len(t)), self._h, "ee_set_patience_vector")
        else:
            capi.check(self.lib.ee_set_patience(self._h, t), self._h, "ee_set_patience")
        self.patience = t
        return t

    def set_exit_rule(self, rule) -> ExitRule:
        """Exit rule of every later forward and capture (ee_set_exit_rule; include/mmee.h MMEE_RULE_*): "plain" (the criterion / LTE test
        alone), "patient_confident" (the test has held at ``patience`` exits in a row) or "patience_or_threshold" (the test fires, or the
        prediction has been stable for ``patience`` exits).  Refused under the "patience" criterion, which has no threshold test."""
        r = rule if isinstance(rule, ExitRule) else ExitRule(str(rule))
        capi.check(self.lib.ee_set_exit_rule(self._h, r.code), self._h, "ee_set_exit_rule")
        self.exit_rule = r
        return r

    def set_ensemble(self, ensemble=None):
        """The exit ensemble of every later forward and capture (ee_set_ensemble; the definition is in include/mmee.h): the decision at exit m
        sees ``y_m = float32(bias[m] + sum_{j <= m} weights[m][j] * logsoftmax(scaled row of exit j))`` instead of exit m's scaled row alone,
        and ``logits`` / ``all_logits`` / ``confidence`` / ``all_crit`` and the result stream carry it; ``head_logits`` / ``head_crit`` stay the
        head's own.  ``ensemble``: an ``EnsembleFit`` (``heads.fit_exit_ensemble``), a ``(weights (E+1,E+1), bias (E+1,K) | None)`` pair (numpy
        or tensors; weights lower triangular), or ``None`` to clear it -- the engine then issues the launches and returns the bits it did
        before.  One small launch per exit, no backbone work.  Refused under the "gate" criterion and ``use_lte``, and, while the engine
        holds captured graphs, when the call would switch the ensemble on or off.  Synchronises the device."""
        if ensemble is None:
            capi.check(self.lib.ee_set_ensemble(self._h, None, None), self._h, "ee_set_ensemble")
            self.ensemble = None
            return None
        w, b = (ensemble.weights, ensemble.bias) if hasattr(ensemble, "weights") else ensemble
        host = lambda v: np.ascontiguousarray(v.detach().cpu().numpy() if (torch is not None and isinstance(v, torch.Tensor)) else np.asarray(v),
                                              dtype=np.float64)
        E1, K = self.E + 1, self.K
        w = host(w)
        b = None if b is None else host(b)
        if w.shape != (E1, E1) or (b is not None and b.shape != (E1, K)):
            raise ValueError(f"set_ensemble: weights must be (E+1,E+1) = {(E1, E1)} and bias (E+1,K) = {(E1, K)} or None")
        dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
        with torch.cuda.device(self.device):
            capi.check(self.lib.ee_set_ensemble(self._h, dp(w), dp(b)), self._h, "ee_set_ensemble")
        self.ensemble = (w, b)
        return self.ensemble

    @property
    def has_ensemble(self) -> bool:
        return bool(self.lib.ee_has_ensemble(self._h))

    def set_quotas(self, quotas: Optional[Sequence[int]] = None, mode: str = "exact"):
        """Budgeted exits of every later forward, capture and graph launch (ee_set_quotas; the definition is in include/mmee.h): ``quotas``, one
        non-negative integer per exit below the final classifier, is how many documents OF EACH CALL leave at that exit -- the most confident
        ones by the engine's criterion, ties to the lower slot.  ``mode="exact"``: exactly those (fewer when fewer arrive), thresholds are not
        read, so the size of every stage is ``n_{e+1} = max(0, n_e - q_e)`` whatever the pages are.  ``mode="at_least"``: those, and whoever
        passes the threshold test as well -- an upper bound on compute that holds for any data.  A document's logits still do not depend on
        its batch mates; only where it leaves does.  ``None`` switches quotas off: the engine then issues the launches and returns the bits
        it did before.  Two small launches per exit.  Refused under the "patience" criterion, the exit rules other than "plain" and
        ``use_lte``, and, while the engine holds captured graphs, when the call would switch quotas on or off or change the mode (new
        values under the same mode are read by the next replay)."""
        if quotas is None:
            capi.check(self.lib.ee_set_quotas(self._h, None, 0, 0), self._h, "ee_set_quotas")
            self.quotas, self.quota_mode = None, None
            return None
        if str(mode) not in capi.QUOTA_MODES:
            raise ValueError(f'set_quotas: mode "{mode}" is neither "exact" nor "at_least"')
        q = [int(v) for v in np.asarray(quotas).reshape(-1)]
        if any(float(a) != float(b) for a, b in zip(q, np.asarray(quotas).reshape(-1))):
            raise ValueError("set_quotas: quotas are whole numbers of documents (quota_fractions= takes shares)")
        capi.check(self.lib.ee_set_quotas(self._h, (C.c_int32 * max(len(q), 1))(*q), len(q), capi.QUOTA_MODES[str(mode)]), self._h, "ee_set_quotas")
        self.quotas, self.quota_mode = q, str(mode)
        return q

    @property
    def has_quotas(self) -> bool:
        return bool(self.lib.ee_has_quotas(self._h))

    def set_audit(self, fraction: Optional[float] = None, seed: int = 0, slot_base: int = 0):
        """Audited exits of every later forward (ee_set_audit; the definition is in include/mmee.h): a deterministic, content-blind sample of each
        call's documents -- chosen by hashing ``(seed, slot_base + index in the call)``, the share ``fraction`` of them on average -- gets its
        result exactly where and as the plain forward gives it and then runs on to the final exit as a shadow.  ``logits`` / ``exit_layer`` /
        ``confidence`` are bit for bit those of the call without the audit; with ``want_all=True`` (``want_head=True``) the sampled columns
        of ``all_logits`` / ``all_crit`` (``head_*``) come back complete, and ``output.audit_mask`` says which they are (``audit.sample``,
        ``audit.consistency``).  ``stage_counts()`` and ``flops()`` report what ran, shadows included.  Vary ``seed`` per call: slot 0 is
        always selected under seed 0.  ``None`` or 0 switches the audit off: the engine then issues the launches and returns the bits it did
        before.  No launch is added.  Refused together with quotas, with ``forward_stream``, with ``capture`` and while the engine holds
        captured graphs; dump-all calls ignore it.  Returns ``(fraction, seed, slot_base)`` or None."""
        if fraction is None or float(fraction) == 0.0:
            capi.check(self.lib.ee_set_audit(self._h, 0, 0, 0), self._h, "ee_set_audit")
            self.audit = None
            return None
        cut = capi.audit_cut(fraction)
        seed, slot_base = int(seed), int(slot_base)
        if not 0 <= seed < 2 ** 32:
            raise ValueError(f"set_audit: seed {seed} is not a 32-bit unsigned value")
        if not 0 <= slot_base < 2 ** 31:
            raise ValueError(f"set_audit: slot_base {slot_base} outside [0, 2^31)")
        capi.check(self.lib.ee_set_audit(self._h, cut, seed, slot_base), self._h, "ee_set_audit")
        self.audit = (float(fraction), seed, slot_base) if cut else None
        return self.audit

    def has_audit(self) -> bool:
        return bool(self.lib.ee_has_audit(self._h))

    def forward_audit_args(self, audit_fraction=None, audit_seed=None):
        """``forward(audit_fraction=, audit_seed=)`` as a ``set_audit`` call: the seed and the slot base that are set are kept where the call
        names none; ``audit_seed`` alone re-seeds the audit that is set."""
        cur = self.audit
        if audit_fraction is not None:
            return self.set_audit(audit_fraction, seed=cur[1] if audit_seed is None and cur else int(audit_seed or 0), slot_base=cur[2] if cur else 0)
        if audit_seed is not None:
            if not cur:
                raise ValueError("audit_seed= goes with audit_fraction= or an audit that is set (set_audit)")
            return self.set_audit(cur[0], seed=audit_seed, slot_base=cur[2])
        return cur

    @staticmethod
    def audit_mask(B: int, fraction: float, seed: int = 0, slot_base: int = 0) -> np.ndarray:
        """(B,) bool: which documents of a call of B an audit of (fraction, seed, slot_base) selects -- include/mmee.h's hash in numpy, the
        bits of ``ee_audit_selected``.  Needs no GPU and no library."""
        cut = capi.audit_cut(fraction)
        x = (np.arange(int(B), dtype=np.uint64) + np.uint64(int(slot_base))) & np.uint64(0xFFFFFFFF)
        m = np.uint64(0xFFFFFFFF)
        x = ((x * np.uint64(0x9E3779B1)) & m) ^ np.uint64(int(seed) & 0xFFFFFFFF)
        x ^= x >> np.uint64(16)
        x = (x * np.uint64(0x85EBCA6B)) & m
        x ^= x >> np.uint64(13)
        x = (x * np.uint64(0xC2B2AE35)) & m
        x ^= x >> np.uint64(16)
        return x < np.uint64(cut)

    def set_controller(self, path=None, *, alpha: Optional[float] = None, gamma: Optional[float] = None, start: Optional[float] = None,
                       seed: int = 0, log_cap: int = 1024):
        """Online exit control of every later forward (ee_set_controller; the definition, its promise and its limit are in include/mmee.h): the
        thresholds follow the disagreement the engine's own audit observes, between forwards, on the device.  ``path``: a ``(V,E1)`` array
        of threshold vectors, most conservative first; a ``RiskResult`` (its candidates are the path, ``start`` defaults to its selected
        index); or a ``SearchResult`` / ``RefineResult`` (through ``risk.path_from_front``).  ``alpha``: the level the audited disagreement
        rate is held to on average; ``gamma``: the step of the position per unit of excess loss; ``start``: the position of the first call
        (default 0, the most conservative vector); ``seed``: call t audits under ``seed + t``; ``log_cap``: rows of the device ring log
        ``controller_log()`` downloads.  Needs ``set_audit`` first.  ``None`` switches the controller off: the engine then issues the launches
        and returns the bits it did before.  Refused under the patience criterion, the combined exit rules, learning-to-exit and quotas, with
        ``forward_stream`` and ``capture``; ``forward(thresholds=)`` raises while it is set; dump-all calls ignore it."""
        if path is None:
            capi.check(self.lib.ee_set_controller(self._h, None, 0, 0.0, 0.0, 0.0, 0, 0), self._h, "ee_set_controller")
            self.controller = None
            return None
        from .risk import RiskResult, path_from_front
        from .sweep import RefineResult, SearchResult
        if isinstance(path, RiskResult):
            if start is None and path.selected >= 0:
                start = float(path.selected)
            path = path.thresholds
        elif isinstance(path, (SearchResult, RefineResult)):
            path = path_from_front(path)
        if alpha is None or gamma is None:
            raise ValueError("set_controller: alpha= (the risk level) and gamma= (the step) are required")
        th = np.ascontiguousarray(np.asarray(path, dtype=np.float64))
        E1 = self.E + 1
        if th.ndim != 2 or th.shape[1] != E1 or th.shape[0] < 2:
            raise ValueError(f"set_controller: path is an array (V,{E1}), V >= 2, most conservative first")
        sign = -1.0 if self.exit_config.inference_strategy.value == "entropy" else 1.0
        if E1 > 1 and not np.all(sign * np.diff(th[:, :E1 - 1], axis=0) <= 0):
            raise ValueError("set_controller: path must move towards the aggressive side at every exit, never back: falling for max_confidence / "
                             "margin / gate, rising for entropy")
        start = 0.0 if start is None else float(start)
        seed, log_cap = int(seed), int(log_cap)
        if not 0 <= seed < 2 ** 32:
            raise ValueError(f"set_controller: seed {seed} is not a 32-bit unsigned value")
        V = int(th.shape[0])
        capi.check(self.lib.ee_set_controller(self._h, th.ctypes.data_as(C.POINTER(C.c_double)), V, float(alpha), float(gamma), start, seed, log_cap),
                   self._h, "ee_set_controller")
        self.controller = dict(path=th, alpha=float(alpha), gamma=float(gamma), start=start, seed=seed, log_cap=log_cap)
        self._ctl_calls = 0
        return self.controller

    def has_controller(self) -> bool:
        return bool(self.lib.ee_has_controller(self._h))

    def controller_state(self) -> dict:
        """The controller's position and sums (ee_controller_state; synchronises the stream): ``position``, ``calls``, ``steps`` (calls that
        sampled anybody), ``sampled``, ``disagree`` (sums over them) and ``thresholds`` (E1,), the vector the NEXT call runs with."""
        p = C.c_double()
        n = [C.c_int64() for _ in range(4)]
        thr = (C.c_double * (self.E + 1))()
        with torch.cuda.device(self.device):
            capi.check(self.lib.ee_controller_state(self._h, C.byref(p), *[C.byref(x) for x in n], thr,
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), self._h, "ee_controller_state")
        return dict(position=p.value, calls=n[0].value, steps=n[1].value, sampled=n[2].value, disagree=n[3].value,
                    thresholds=np.array(list(thr), dtype=np.float64))

    def controller_log(self) -> "ControllerLog":
        """The device ring log, oldest row first (ee_controller_log; synchronises the stream): one row per controlled call, the latest
        ``log_cap`` of them.  The one download."""
        if self.controller is None:
            raise capi.MMEEError("controller_log: no controller is set (set_controller)")
        W, cap = capi.controller_log_words(self.E + 1), self.controller["log_cap"]
        rows = np.zeros((max(cap, 1), W), dtype=np.int64)
        n = C.c_int32(0)
        with torch.cuda.device(self.device):
            capi.check(self.lib.ee_controller_log(self._h, rows.ctypes.data_as(C.c_void_p), cap, C.byref(n),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)), self._h, "ee_controller_log")
        return ControllerLog.from_rows(rows[:n.value], self.E + 1)

    @staticmethod
    def _budget_ns(budget_ms) -> int:
        ns = int(round(float(budget_ms) * 1e6))
        if not 0 <= ns < capi.DEADLINE_OFF:
            raise ValueError(f"a deadline budget of {budget_ms} ms is not a number of ns in [0, 2^64 - 2)")
        return ns

    def _apply_deadline(self, budget_ns: int, eta_ns):
        eta_c = None if eta_ns is None else (C.c_uint64 * (self.E + 1))(*[int(x) for x in eta_ns])
        capi.check(self.lib.ee_set_deadline(self._h, C.c_uint64(budget_ns), eta_c), self._h, "ee_set_deadline")

    def set_deadline(self, budget_ms: Optional[float] = None, eta_ms=None, stamps_only: bool = False, log_cap: int = 1024):
        """Deadline exits of every later forward (ee_set_deadline; the definition is in include/mmee.h): anytime prediction.  A clock on the
        device starts with the call's first launch; in front of every exit's decision a small launch looks at it, and once
        ``elapsed + eta_ms[e] >= budget_ms`` -- or once ``request_cut()`` has asked -- everybody still in the batch leaves at that exit, with
        that exit's ordinary row.  The result is, bit for bit, ``forward`` under thresholds that fire for everybody from ``cut_exit`` on;
        ``deadline_log()`` says where the cut fell.  ``eta_ms``: per exit, the time from the decision at that exit to the end of the call if
        nobody is cut there (``deadline.eta_from_logs`` measures it; ``None``: zeros, the cut then falls at the first exit after the budget has
        passed).  ``stamps_only=True`` (``budget_ms`` must be ``None``): the clock never cuts; calls are logged and obey ``request_cut()`` only.
        ``log_cap``: rows of the device ring log.  The first deadline of an engine, one after ``set_deadline(None)`` and one with another
        ``log_cap`` restart the log (and synchronise the device); a new budget or ``eta_ms`` on an engine that has a deadline does neither,
        the log runs on.  ``set_deadline(None)`` removes the deadline (its log stays readable): the
        engine then issues the launches and returns the bits it did before.  Refused under the patience criterion, the combined exit rules,
        learning-to-exit, quotas, an audit or a controller, with ``capture`` and ``forward_vision``; dump-all calls ignore it.  A document
        whose criterion is a NaN is not cut: it runs to the final exit."""
        if budget_ms is None and not stamps_only:
            self._apply_deadline(capi.DEADLINE_OFF, None)
            if self.deadline is not None:
                self._dl_last_cap = self.deadline["log_cap"]
            self.deadline = None
            return None
        if budget_ms is not None and stamps_only:
            raise ValueError("set_deadline: stamps_only=True goes with budget_ms=None (the clock then never cuts)")
        budget_ns = capi.DEADLINE_NONE if stamps_only else self._budget_ns(budget_ms)
        eta_ns = None
        if eta_ms is not None:
            eta = np.asarray(eta_ms, dtype=np.float64).reshape(-1)
            if eta.shape[0] != self.E + 1 or not np.all(np.isfinite(eta)) or np.any(eta < 0):
                raise ValueError(f"set_deadline: eta_ms has {self.E + 1} finite entries >= 0, one per exit")
            eta_ns = [min(int(round(x * 1e6)), capi.DEADLINE_NONE) for x in eta.tolist()]
        if self.deadline is None or self.deadline["log_cap"] != int(log_cap):
            # the ring at its size, once; the entry point refuses what ee_set_deadline refuses, before anything is allocated
            capi.check(self.lib.ee_set_deadline_log(self._h, int(log_cap)), self._h, "ee_set_deadline_log")
        self._apply_deadline(budget_ns, eta_ns)
        self.deadline = dict(budget_ns=budget_ns, eta_ns=eta_ns, log_cap=int(log_cap))
        return self.deadline

    def has_deadline(self) -> bool:
        return bool(self.lib.ee_has_deadline(self._h))

    def request_cut(self) -> bool:
        """Cut every deadline forward enqueued on this engine so far at its next check, none enqueued later (ee_request_cut): one store to a
        pinned word the check launches read.  Any thread, no device call.  False on an engine that never had a deadline."""
        return self.lib.ee_request_cut(self._h) == 0

    def deadline_log(self) -> "DeadlineLog":
        """The device ring log, oldest row first (ee_deadline_log; synchronises the stream): one row per deadline call since ``set_deadline``,
        the latest ``log_cap`` of them.  It stays readable after ``set_deadline(None)``."""
        cap = self.deadline["log_cap"] if self.deadline else self._dl_last_cap
        W = capi.deadline_log_words(self.E + 1)
        rows = np.zeros((max(cap, 1), W), dtype=np.int64)
        n = C.c_int32(0)
        with torch.cuda.device(self.device):
            capi.check(self.lib.ee_deadline_log(self._h, rows.ctypes.data_as(C.c_void_p), cap, C.byref(n),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), self._h, "ee_deadline_log")
        return DeadlineLog.from_rows(rows[:min(n.value, cap)], self.E + 1)

    def clock_stamp(self):
        """Device tensor of capi.CLOCK_STAMP_WORDS int64: one (s_memtime, s_memrealtime) pair per CU as seen by one-wave workgroups enqueued on
        the current stream (ee_clock_stamp).  ``clock_ghz(a, b)`` turns two stamps into the shader clock held between them."""
        t = torch.zeros(capi.CLOCK_STAMP_WORDS, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            capi.check(self.lib.ee_clock_stamp(C.c_void_p(t.data_ptr()), stream), None, "ee_clock_stamp")
        return t

    @staticmethod
    def clock_ghz(stamp_a, stamp_b):
        """(mean GHz, per-XCD mean GHz list) between two ``clock_stamp()`` results (synchronises through .cpu()): d(s_memtime) /
        d(s_memrealtime) x 0.1 GHz of every CU slot filled in BOTH stamps (the CUs' counters are not aligned with each other, so only
        same-CU differences are taken), averaged per XCD and over the chip."""
        a = stamp_a.cpu().numpy().reshape(8, -1, 2).astype(np.float64)
        b = stamp_b.cpu().numpy().reshape(8, -1, 2).astype(np.float64)
        ok = (a[..., 1] > 0) & (b[..., 1] > a[..., 1])
        if not ok.any():
            return None, []
        ghz = np.where(ok, 0.1 * (b[..., 0] - a[..., 0]) / np.where(ok, b[..., 1] - a[..., 1], 1.0), 0.0)
        per = [float(ghz[x][ok[x]].mean()) for x in range(8) if ok[x].any()]
        return float(ghz[ok].mean()), per

    def layer_plan(self):
        """How the last forward ran each encoder layer (ee_last_layer_plan): rows through Q|K|V, rows through the rest of
        the layer, documents whose CLS row was probed before the layer's decision."""
        L = self.cfg.num_hidden_layers
        q, m, p = (C.c_int32 * L)(), (C.c_int32 * L)(), (C.c_int32 * L)()
        pf = C.c_double()
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            capi.check(self.lib.ee_last_layer_plan(self._h, q, m, p, L, C.byref(pf), stream), self._h, "ee_last_layer_plan")
        return {"rows_qkv": list(q), "rows_main": list(m), "docs_probe": list(p), "probe_flops": pf.value}


class CapturedForward:
    """One captured configuration of ``EarlyExitEngine.forward`` (see ``EarlyExitEngine.capture``)."""

    def __init__(self, engine: EarlyExitEngine, graph_id: int, inputs: Dict[str, "torch.Tensor"], outputs: EngineOutput):
        self.engine, self.graph_id, self.inputs, self.outputs = engine, graph_id, inputs, outputs

    def launch(self, thresholds: Optional[Union[float, Sequence[float]]] = None, temperatures: Optional[Sequence[float]] = None,
               validate: bool = False, patience: Optional[Union[int, Sequence[int]]] = None,
               quotas: Optional[Sequence[int]] = None) -> EngineOutput:
        """Replay on torch's current stream with this launch's thresholds / temperatures; returns ``self.outputs`` (the same tensors every
        time: copy what must outlive the next launch).  ``patience``: ``engine.set_patience(patience)`` first (an int or one entry per exit); a
        graph captured under the patience criterion or a combined exit rule replays with the engine's current patience either way.
        ``quotas``: ``engine.set_quotas(quotas, mode=<the engine's mode>)`` first; a graph captured with quotas set replays with the engine's
        current quotas either way (whether quotas are on, and the mode, are the capture's)."""
        eng = self.engine
        if patience is not None:
            eng.set_patience(patience)
        if quotas is not None:
            if eng.quota_mode is None:
                raise ValueError("launch(quotas=): the graph was captured without quotas (whether they are on is bound at capture)")
            eng.set_quotas(quotas, mode=eng.quota_mode)
        E = eng.E
        if thresholds is None:
            thresholds = eng.exit_config.global_threshold
        thr = np.broadcast_to(np.asarray(thresholds, dtype=np.float64).reshape(-1), (E + 1,)) if np.ndim(thresholds) else np.full((E + 1,), float(thresholds))
        thr_c = (C.c_double * (E + 1))(*thr.tolist())
        tmp_c = None
        if temperatures is not None:
            tm = np.asarray(temperatures, dtype=np.float64).reshape(-1)
            if tm.shape[0] != E + 1:
                raise ValueError(f"temperatures must have {E + 1} entries")
            tmp_c = (C.c_double * (E + 1))(*tm.tolist())
        with torch.cuda.device(eng.device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            capi.check(eng.lib.ee_graph_launch(eng._h, self.graph_id, thr_c, tmp_c, stream), eng._h, "ee_graph_launch")
        if validate:
            eng.stage_counts()
        return self.outputs

    __call__ = launch

    def close(self):
        if self.graph_id >= 0 and getattr(self.engine, "_h", None) is not None and self.engine._h.value:
            self.engine.lib.ee_graph_destroy(self.engine._h, self.graph_id)
        self.graph_id = -1


def load_checkpoint_tensors(path: str) -> Dict[str, "torch.Tensor"]:
    """Read every tensor of a local HF checkpoint directory (safetensors preferred, then pytorch_model.bin)."""
    st = [f for f in sorted(os.listdir(path)) if f.endswith(".safetensors")]
    out: Dict[str, "torch.Tensor"] = {}
    if st:
        from safetensors import safe_open
        for f in st:
            with safe_open(os.path.join(path, f), framework="pt", device="cpu") as fh:
                for k in fh.keys():
                    out[k] = fh.get_tensor(k)
        return out
    bins = [f for f in sorted(os.listdir(path)) if f.endswith(".bin") or f.endswith(".pt")]
    if not bins:
        raise FileNotFoundError(f"no *.safetensors / *.bin under {path}")
    for f in bins:
        out.update(torch.load(os.path.join(path, f), map_location="cpu", weights_only=True))
    return out


def save_checkpoint(path: str, cfg: ModelConfig, weights: Mapping[str, np.ndarray]):
    """Write an HF-format checkpoint directory (config.json with EE_config + model.safetensors)."""
    from safetensors.numpy import save_file
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cfg.to_hf_dict(), f, indent=2)
    save_file({k: np.ascontiguousarray(v) for k, v in weights.items()}, os.path.join(path, "model.safetensors"))
