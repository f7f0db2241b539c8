"""One-layer ramp exit heads fitted on the device from a frozen backbone's CLS rows (``ee_head_fit``, include/mmee.h).

The reference's two-stage strategies train only the heads on a frozen backbone (EE/models/EE_modules.py:91, 108-113;
EE/IC_only.py:189-207).  Then the training set of the head at encoder layer l is the CLS row leaving that layer, which a dump-all
forward already returns (``hidden_cls``), and for ``exit_head_num_layers = 1`` (one Linear, EE/models/LayoutLMv3.py:84-93) the fit is
L2-regularised softmax regression: strongly convex, one optimum.  ``collect_exit_features`` gathers the rows, ``fit_exit_heads``
solves the regression per exit with L-BFGS in float64 on the device, and ``HeadFit.state_dict`` names the result the way
``EarlyExitEngine.load_weights`` expects it.  This is not a trainer: two-layer heads, gates, the LTE classifier, embedding-level
exits, mini-batches and an unfrozen backbone are out of scope.

Reloading heads into an engine that holds captured graphs does not re-capture them: capture again after ``load_weights``.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Iterable, Mapping

import numpy as np

from . import capi
from .config import ModelConfig
from .engine import _require_torch_cuda, torch

STATUS = {0: "converged", 1: "max_evals", 2: "line_search"}


def _check_fittable(cfg: ModelConfig):
    ec = cfg.exit_config
    if str(ec.encoder_layer_strategy) != "ramp":
        raise ValueError("exit heads are fitted for the ramp strategy only: a gate shows the policy the final classifier's logits, "
                         "there is no head to fit")
    if ec.exit_head_num_layers != 1:
        raise ValueError("exit heads are fitted for exit_head_num_layers == 1 only (a two-layer head is not a convex problem)")
    if ec.embedding_exits:
        raise ValueError(f"embedding-level exits {ec.embedding_exits} cannot be fitted: the forward does not return their pooled inputs")
    if not ec.encoder_exit_layers:
        raise ValueError("the configuration has no encoder exits")


def collect_exit_features(engine, batches: Iterable[Mapping]):
    """Dump-all forwards of ``engine`` over ``batches`` (dicts of ``engine.forward`` keyword inputs: ``input_ids``, ``attention_mask``,
    ``bbox``, ``pixel_values``, ...; ``pixel_values`` alone for the image-only DiT handle).  Returns the device tensor (E,N,H) float32
    of the CLS rows leaving the configured encoder exit layers -- the inputs of the heads ``encoder.early_exits.0 .. E-1``."""
    _check_fittable(engine.cfg)
    layers = torch.tensor(engine.cfg.exit_config.encoder_exit_layers, dtype=torch.int64, device=engine.device)
    keys = ("input_ids", "attention_mask", "bbox", "pixel_values", "token_type_ids", "position_ids")
    rows = []
    for b in batches:
        out = engine.forward(**{k: b[k] for k in keys if k in b and b[k] is not None}, dump_all=True, want_hidden_cls=True)
        rows.append(out.hidden_cls.index_select(0, layers))
    if not rows:
        raise ValueError("no batches")
    return torch.cat(rows, dim=1).contiguous()


@dataclass
class HeadFit:
    weight: "torch.Tensor"       # (E,K,H) float32, device
    bias: "torch.Tensor"         # (E,K)   float32
    weight64: "torch.Tensor"     # the float64 solution the float32 pair is rounded from
    bias64: "torch.Tensor"
    loss: "torch.Tensor"         # (E,) float64: the objective at the returned point
    grad_norm: "torch.Tensor"    # (E,) float64
    evals: "torch.Tensor"        # (E,) int32: loss / gradient evaluations used
    status: "torch.Tensor"       # (E,) int32: 0 converged (grad_norm <= gtol), 1 max_evals, 2 the line search made no progress
    l2: float

    def logits(self, features) -> "torch.Tensor":
        """(E,N,K) float64 logits of the float32 heads on ``features`` (E,N,H), on the device."""
        X = _to_device(features, torch.float32, self.weight.device).to(torch.float64)
        if X.dim() == 2:
            X = X.unsqueeze(0)
        return torch.baddbmm(self.bias.to(torch.float64).unsqueeze(1), X, self.weight.to(torch.float64).transpose(1, 2))

    def state_dict(self, cfg: ModelConfig) -> Dict[str, np.ndarray]:
        """``{prefix}encoder.early_exits.{k}.out_proj.weight / .bias`` (host float32), ready for ``engine.load_weights`` next to the
        backbone's tensors."""
        _check_fittable(cfg)
        E, K, H = self.weight.shape
        if E != len(cfg.exit_config.encoder_exit_layers) or K != cfg.num_labels or H != cfg.hidden_size:
            raise ValueError(f"the fit is (E,K,H) = {(E, K, H)}, the configuration wants "
                             f"{(len(cfg.exit_config.encoder_exit_layers), cfg.num_labels, cfg.hidden_size)}")
        p = "beit." if cfg.arch == "beit" else "layoutlmv3."
        w, b = self.weight.cpu().numpy(), self.bias.cpu().numpy()
        out = {}
        for k in range(E):
            out[f"{p}encoder.early_exits.{k}.out_proj.weight"] = np.ascontiguousarray(w[k])
            out[f"{p}encoder.early_exits.{k}.out_proj.bias"] = np.ascontiguousarray(b[k])
        return out


def _to_device(x, dtype, dev):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x) if x.flags.writeable else np.array(x))
    return x.to(dev, dtype).contiguous()


def fit_exit_heads(features, labels, l2: float = 1e-2, gtol: float = 1e-9, max_evals: int = 2000, history: int = 8, device=None,
                   num_labels: int = None) -> HeadFit:
    """``features`` (E,N,H) float32 (numpy or device tensor; (N,H) is one exit), ``labels`` (N,) integers in [0,K) with
    K = ``num_labels`` (default: ``labels.max() + 1``; state it when a class may be absent).  Minimises, per exit, mean cross-entropy +
    (l2 / 2)(||W||^2 + ||b||^2) in float64 (include/mmee.h).  Features and parameters stay on the device.

    ``status`` says how each exit stopped.  Unit-variance, uncorrelated features converge to ``gtol = 1e-9`` in 40 - 60 evaluations; the CLS
    rows of a real backbone share a large common component (the condition number grows with it) and need several hundred to a thousand:
    hence the default budget of 2000 (the C entry point has no default) -- a stopped exit costs nothing more, so a generous budget is only
    paid by the exits that use it.  Raise ``max_evals`` when ``status`` is 1.

    Host synchronisation: the call waits for its stream once, after the last launch, to read the error word (a label outside [0,K) fails
    the call); with ``num_labels=None`` reading ``labels.max()`` is a second wait, before the first launch."""
    lib = capi.load()
    dev = features.device if (torch is not None and isinstance(features, torch.Tensor) and features.is_cuda and device is None) \
        else _require_torch_cuda(device)
    X = _to_device(features, torch.float32, dev)
    if X.dim() == 2:
        X = X.unsqueeze(0)
    y = _to_device(labels, torch.int64, dev).view(-1)
    E, N, H = X.shape
    K = int(y.max()) + 1 if num_labels is None else int(num_labels)
    if y.shape[0] != N:
        raise ValueError("labels must have one entry per feature row")
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    fit = HeadFit(torch.zeros((E, K, H), dtype=torch.float32, device=dev), torch.zeros((E, K), dtype=torch.float32, device=dev),
                  f64(E, K, H), f64(E, K), f64(E), f64(E), torch.zeros((E,), dtype=torch.int32, device=dev),
                  torch.full((E,), -1, dtype=torch.int32, device=dev), float(l2))
    need = int(lib.ee_head_fit_workspace_bytes(E, N, H, K, history))
    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        capi.check(lib.ee_head_fit(p(X), p(y), E, N, H, K, float(l2), float(gtol), int(max_evals), int(history), p(ws), need, p(fit.weight),
                                   p(fit.bias), p(fit.weight64), p(fit.bias64), p(fit.loss), p(fit.grad_norm), p(fit.evals), p(fit.status),
                                   stream), None, "ee_head_fit")
    return fit
