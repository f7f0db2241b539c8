"""Ramp exit heads fitted on the device from a frozen backbone's CLS rows (``ee_head_fit`` and ``ee_mlp_head_fit``, include/mmee.h).

The reference's two-stage strategies train only the heads on a frozen backbone (EE/models/EE_modules.py:91, 108-113;
EE/IC_only.py:189-207).  Then the training set of the head at encoder layer l is the CLS row leaving that layer, which a dump-all
forward already returns (``hidden_cls``).  ``collect_exit_features`` gathers the rows.

For ``exit_head_num_layers = 1`` (one Linear, EE/models/LayoutLMv3.py:84-93) the fit is L2-regularised softmax regression: strongly
convex, one optimum.  ``fit_exit_heads`` solves it per exit with L-BFGS in float64 on the device, and ``HeadFit.state_dict`` names the
result the way ``EarlyExitEngine.load_weights`` expects it.

For ``exit_head_num_layers = 2``, the reference's default (dense -> tanh -> out_proj, EE/models/LayoutLMv3.py:70-93),
``fit_mlp_exit_heads`` runs the same L-BFGS on the two-layer objective from a stated start (``init="identity"``: the one-layer head on
tanh(x)), and ``MlpHeadFit.state_dict`` names the four tensors per exit.  That objective is not convex: the fit returns a stationary
point reached by descent from the start (``status`` 0: gradient norm <= gtol), reproducible bit for bit, not a unique optimum.

Neither fit needs labels: with a fine-tuned checkpoint and unlabelled documents, ``collect_distill_features`` returns the final classifier's
logits next to the CLS rows, and ``fit_distilled_exit_heads`` / ``fit_distilled_mlp_exit_heads`` fit the same heads to reproduce its
distribution (``ee_head_fit_distill``, ``ee_mlp_head_fit_distill``: KL at a temperature, optionally mixed with the label loss by ``alpha``;
the reference declares ``alpha = 1, temperature = 1`` in EETrainingArguments, EE/models/EE_modules.py:288-298, and builds nothing on them).

All four head fits take ``sample_weight``: one weight per document, or one per (exit, document) (``ee_head_fit_weighted``,
``ee_mlp_head_fit_weighted``: the weighted mean of the same row losses).  ``reach_weights`` turns a policy scan's ``exits`` into the table
"exit e is asked about document n" (cascade-aware heads), ``balanced_class_weights`` weighs every class alike, and a 0/1 row is a held-out
mask over features that stay where they are.

The learning-to-exit classifier (``use_lte``: ONE ``nn.Linear(H, 1)`` + sigmoid shared by every encoder exit, scored on the CLS row leaving
the exit's layer) is fitted from the same dump-all forwards (``ee_lte_fit``): ``collect_lte_features`` gathers the CLS rows and the exits'
policy logits, ``lte_targets`` turns logits and labels into the targets "this exit is wrong here", ``fit_lte_classifier`` minimises the
reference's summed per-exit MSE (or the convex BCE) and ``LteFit.state_dict`` names ``encoder.lte_classifier.weight / .bias``.  The MSE
objective is not convex: ``status`` 0 is a stationary point reached by descent from the start.

The 2-way gate heads of the gate strategy -- the heads ``inference_strategy="gate"`` lets decide (include/mmee.h MMEE_CRIT_GATE) -- are fitted
from the same forwards too (``ee_head_fit_gate``): ``collect_gate_features`` gathers the CLS rows and the gated logits ``classifier(gate
input)``, ``gate_targets`` turns those and labels into "the classifier is right here", ``fit_gate_heads`` minimises the reference's
``BCEWithLogitsLoss`` against the one-hot of that (strongly convex: one optimum) and ``GateFit.state_dict`` names the heads.  That is the
one-layer gate (``exit_head_num_layers = 1``).  For the default depth of two, ``fit_mlp_gate_heads`` minimises the same loss on
W2 tanh(W1 x + b1) + b2 (``ee_mlp_head_fit_gate``: the two-layer ramp fit's launches with one row kernel exchanged) from a stated start, and
``MlpGateFit.state_dict`` names the four tensors per exit.  Like the two-layer ramp objective it is not convex: ``status`` 0 is a stationary
point reached by descent from the start.  It takes ``sample_weight`` (``ee_mlp_head_fit_gate_weighted``): with ``reach_weights`` gate e is fitted
on the documents no earlier exit released, the only ones it is ever asked about.

The embedding-level exit heads (``vision_exit_embeddings``, ``text_exit_embeddings``, ``concat_exit_embeddings``; EE/models/LayoutLMv3.py:320-340)
are heads of the same kind on other rows: the (B,H) means over every position of the visual embeddings, the text embeddings and the
LayerNorm of both (:466, 520, 582), which do not depend on the encoder.  ``engine.embedding_inputs`` (``ee_embedding_inputs``) returns them
from stage 0 of the forward alone, ``collect_embedding_features`` gathers them without running a layer, and ``embedding_exits=True`` on
``collect_exit_features`` / ``collect_distill_features`` / ``collect_gate_features`` puts them in front of the CLS rows, in the forward's exit
order.  The fits take that as any (E,N,H); ``state_dict(cfg, embedding_exits=True)`` of the four fit classes names the first heads by their
modules; a policy scan's exit index is then the feature row, which is all ``reach_weights`` needs.  Without the flag a configuration that
names an embedding-level exit is refused, as before.  The text and concat means run over all T positions of the call, padding included:
the same page padded to another T has another feature, so collect at the T that deployment runs (the reference pads to ``max_length``).

This is not a trainer: distilled gates, sample weights for one-layer gates, the LTE classifier at embedding-level exits, the final
classifier, per-exit LTE loss weights, mini-batches and an unfrozen backbone are out of scope.

Reloading heads into an engine that holds captured graphs does not re-capture them: capture again after ``load_weights``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Iterable, Mapping

import numpy as np

from . import capi
from .config import ModelConfig
from .engine import _require_torch_cuda, torch

STATUS = {0: "converged", 1: "max_evals", 2: "line_search"}
LTE_MAX_EVALS = 1000           # fit_lte_classifier's default budget; its docstring says where it comes from
_KEYS = ("input_ids", "attention_mask", "bbox", "pixel_values", "token_type_ids", "position_ids")
# checkpoint module of each embedding-level exit head (EE/models/LayoutLMv3.py:320-340)
_EMB_HEAD = {"vision_avg": "vision_exit_embeddings", "text_avg": "text_exit_embeddings", "text_visual_concat": "concat_exit_embeddings"}


def _dump_all(engine, batches, embedding_exits=False, **want):
    """Per batch: the CLS rows (E,n,H) leaving the configured encoder exit layers, and the dump-all forward's whole output.  With
    ``embedding_exits`` the (n_emb,n,H) pooled rows of ``engine.embedding_inputs`` stand in front of the CLS rows: the forward's exit order."""
    ec = engine.cfg.exit_config
    layers = torch.tensor(ec.encoder_exit_layers, dtype=torch.int64, device=engine.device)
    n_emb = len(ec.embedding_exits) if embedding_exits else 0
    for b in batches:
        out = engine.forward(**{k: b[k] for k in _KEYS if k in b and b[k] is not None}, dump_all=True, want_hidden_cls=True, **want)
        rows = out.hidden_cls.index_select(0, layers)
        yield (torch.cat([_embedding_rows(engine, b), rows]) if n_emb else rows), out


def _cat_batches(per_batch):
    """The batches' tensors joined along the document axis, one result per position."""
    cols = list(zip(*per_batch))
    if not cols:
        raise ValueError("no batches")
    return [torch.cat(c, dim=1).contiguous() for c in cols]


def _check_embedding_exits(cfg: ModelConfig, embedding_exits: bool):
    """What the ramp and the gate checks say about a configuration's embedding-level exits.  -> True when the configuration needs no
    encoder exit (it has embedding-level ones and they are being fitted)."""
    ec = cfg.exit_config
    if embedding_exits and cfg.arch == "beit":
        raise ValueError("embedding_exits=True: embedding-level exits belong to LayoutLMv3; a BEiT / DiT configuration has none")
    if ec.embedding_exits and not embedding_exits:
        raise ValueError(f"embedding-level exits {ec.embedding_exits} cannot be fitted by this call: the forward does not return their pooled "
                         "inputs.  Pass embedding_exits=True to the collector and to state_dict (collect_embedding_features gathers the rows)")
    return bool(embedding_exits and ec.embedding_exits)


def _check_fittable(cfg: ModelConfig, head_layers: int = 1, embedding_exits: bool = False):
    ec = cfg.exit_config
    if str(ec.encoder_layer_strategy) != "ramp":
        raise ValueError("ramp exit heads are fitted for the ramp strategy only: the 2-way heads of a gate configuration are fitted by "
                         "fit_gate_heads, or fit_mlp_gate_heads for two layers (collect_gate_features, gate_targets)")
    if head_layers == 2:
        if ec.exit_head_num_layers != 2:
            raise ValueError("two-layer exit heads are fitted for exit_head_num_layers == 2 only (fit_exit_heads fits the one-layer head)")
    elif head_layers != 1:
        raise ValueError(f"head_layers = {head_layers}: the heads of the reference have one or two layers")
    elif ec.exit_head_num_layers != 1:
        raise ValueError("exit heads are fitted for exit_head_num_layers == 1 only (a two-layer head is not a convex problem: "
                         "fit_mlp_exit_heads fits it, collect_exit_features(..., head_layers=2) gathers its rows)")
    if not _check_embedding_exits(cfg, embedding_exits) and not ec.encoder_exit_layers:
        raise ValueError("the configuration has no encoder exits")


def _embedding_rows(engine, batch, kinds=None):
    """(n_emb,n,H): the pooled rows of one batch from ``engine.embedding_inputs``, stacked in the reference's order"""
    rows = engine.embedding_inputs(**{k: batch[k] for k in _KEYS if k in batch and batch[k] is not None}, kinds=kinds)
    return torch.stack(list(rows.values()))


def collect_embedding_features(engine, batches: Iterable[Mapping], kinds=None):
    """The inputs of the embedding-level exit heads over ``batches`` (dicts of ``engine.forward`` keyword inputs), from
    ``engine.embedding_inputs`` alone: stage 0 of the forward, no encoder layer.  Returns the device tensor (n_emb,N,H) float32, one slab
    per kind in the reference's order (vision, text, concat) -- ``kinds`` defaults to the configuration's embedding exits; any non-empty
    subset of ``config.EMBEDDING_EXITS`` is allowed on any LayoutLMv3 engine.  Batches are concatenated in order.

    The text and concat rows are means over all T positions of the call, padding included: the same page padded to another T has another
    feature.  Collect at the T that deployment runs (the reference pads to ``max_length``)."""
    if engine.cfg.arch == "beit":
        raise ValueError("collect_embedding_features: embedding-level exits belong to LayoutLMv3; a BEiT / DiT engine has none")
    return _cat_batches((_embedding_rows(engine, b, kinds),) for b in batches)[0]


def collect_exit_features(engine, batches: Iterable[Mapping], head_layers: int = 1, embedding_exits: bool = False):
    """Dump-all forwards of ``engine`` over ``batches`` (dicts of ``engine.forward`` keyword inputs: ``input_ids``, ``attention_mask``,
    ``bbox``, ``pixel_values``, ...; ``pixel_values`` alone for the image-only DiT handle).  Returns the device tensor (E,N,H) float32
    of the CLS rows leaving the configured encoder exit layers -- the inputs of the heads ``encoder.early_exits.0 .. E-1``.
    ``head_layers`` states which heads the rows are for: 1 (``fit_exit_heads``) or 2 (``fit_mlp_exit_heads``); the configuration must agree.

    ``embedding_exits=True`` (LayoutLMv3): the configuration's embedding-level exits are fitted too.  The result is (n_emb + E,N,H) in the
    forward's exit order -- the pooled rows of the embedding exits first, in the reference's order (vision, text, concat), then the encoder
    exits -- from one dump-all forward plus one ``engine.embedding_inputs`` call per batch; a configuration without an encoder exit is then
    allowed.  Without it a configuration that names an embedding-level exit is refused.  The pitfall of ``collect_embedding_features``
    holds: the text and concat rows depend on the T the batch is padded to."""
    _check_fittable(engine.cfg, head_layers, embedding_exits)
    return _cat_batches((rows,) for rows, _ in _dump_all(engine, batches, embedding_exits))[0]


def _rows_and_logits(engine, batches, embedding_exits=False):
    """-> (the heads' input rows (E,N,H), those exits' policy logits (E,N,K) float32): the encoder exits, behind the embedding-level exits
    when ``embedding_exits`` (else those are skipped)"""
    ec = engine.cfg.exit_config
    n_emb, n_enc = len(ec.embedding_exits), len(ec.encoder_exit_layers)
    first = 0 if embedding_exits else n_emb
    return tuple(_cat_batches((rows, out.all_logits[first:n_emb + n_enc].to(torch.float32))
                              for rows, out in _dump_all(engine, batches, embedding_exits, want_all=True)))


def collect_distill_features(engine, batches: Iterable[Mapping], head_layers: int = 1, embedding_exits: bool = False):
    """``collect_exit_features`` for documents without labels.  Returns two device tensors from the same dump-all forwards: ``features``
    (E,N,H) float32 as above ((n_emb + E,N,H) with ``embedding_exits=True``), and ``teacher_logits`` (N,K) float32, the final classifier's
    logits on the same documents (the last row of ``all_logits``) -- the targets of ``fit_distilled_exit_heads`` /
    ``fit_distilled_mlp_exit_heads``.  Refusals and inputs are those of ``collect_exit_features``; LayoutLMv3 handles and the image-only DiT
    handle are supported."""
    _check_fittable(engine.cfg, head_layers, embedding_exits)
    feats, teacher = _cat_batches((rows, out.all_logits[-1:].to(torch.float32))
                                  for rows, out in _dump_all(engine, batches, embedding_exits, want_all=True))
    return feats, teacher[0]


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
    alpha: float = 0.0           # weight of the distillation term (fit_distilled_exit_heads); 0: fitted against labels alone
    temperature: float = 1.0     # the distillation temperature

    def logits(self, features) -> "torch.Tensor":
        """(E,N,K) float64 logits of the float32 heads on ``features`` (E,N,H), on the device."""
        return _linear_logits(self, features)

    def state_dict(self, cfg: ModelConfig, embedding_exits: bool = False) -> Dict[str, np.ndarray]:
        """``{prefix}encoder.early_exits.{k}.out_proj.weight / .bias`` (host float32), ready for ``engine.load_weights`` next to the
        backbone's tensors.  ``embedding_exits=True``: the fit's leading axis is n_emb + E (``collect_exit_features(...,
        embedding_exits=True)``) and its first n_emb heads are named ``layoutlmv3.vision_exit_embeddings`` / ``.text_exit_embeddings`` /
        ``.concat_exit_embeddings``, whichever the configuration has."""
        _check_fittable(cfg, 1, embedding_exits)
        return _out_proj_state(self, _head_stems(self, cfg, cfg.num_labels, "K", embedding_exits))


def _linear_logits(fit, features):
    """(E,N,K) float64 logits of the float32 one-layer heads ``fit.weight`` (E,K,H), ``fit.bias`` (E,K) on ``features`` (E,N,H)"""
    X = _rows(features, on=fit.weight.device)[1].to(torch.float64)
    return torch.baddbmm(fit.bias.to(torch.float64).unsqueeze(1), X, fit.weight.to(torch.float64).transpose(1, 2))


def _out_proj_state(fit, stems):
    """``{stem}.out_proj.weight / .bias`` of the one-layer heads ``fit.weight``, ``fit.bias``, as host float32; ``stems``: ``_head_stems``"""
    w, b = fit.weight.cpu().numpy(), fit.bias.cpu().numpy()
    out = {}
    for k, stem in enumerate(stems):
        out[f"{stem}.out_proj.weight"] = np.ascontiguousarray(w[k])
        out[f"{stem}.out_proj.bias"] = np.ascontiguousarray(b[k])
    return out


def _mlp_state(fit, stems):
    """``{stem}.dense.weight / .dense.bias / .out_proj.weight / .out_proj.bias`` of the two-layer heads of ``fit``, as host float32"""
    blocks = [t.cpu().numpy() for t in (fit.dense_weight, fit.dense_bias, fit.weight, fit.bias)]
    return {f"{stem}.{name}": np.ascontiguousarray(a[k]) for k, stem in enumerate(stems) for name, a in zip(_MLP_BLOCKS, blocks)}


def _to_device(x, dtype, dev):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x) if x.flags.writeable else np.array(x))
    return x.to(dev, dtype).contiguous()


def _rows(x, device=None, on=None):
    """``x`` (E,N,H), or (N,H) for one exit -> (dev, the (E,N,H) float32 tensor on it).  dev: ``on``, else ``x``'s own CUDA device unless
    ``device`` names one."""
    dev = on if on is not None else x.device if (torch is not None and isinstance(x, torch.Tensor) and x.is_cuda and device is None) \
        else _require_torch_cuda(device)
    X = _to_device(x, torch.float32, dev)
    return dev, X.unsqueeze(0) if X.dim() == 2 else X


def _labels(labels, dev, N, num_labels):
    """-> (y (N,) int64 on dev, K)"""
    y = _to_device(labels, torch.int64, dev).view(-1)
    K = int(y.max()) + 1 if num_labels is None else int(num_labels)
    if y.shape[0] != N:
        raise ValueError("labels must have one entry per feature row")
    return y, K


def _weight_shape(features, sample_weight):
    """The refusal of a ``sample_weight`` of the wrong shape, from shapes alone (nothing touches the library or a device)."""
    if sample_weight is None:
        return
    fs, ws = tuple(features.shape), tuple(np.shape(sample_weight))
    if len(fs) not in (2, 3):
        raise ValueError(f"features are {fs}, need (E,N,H), or (N,H) for one exit")
    E, N = (1 if len(fs) == 2 else fs[0]), fs[-2]
    if ws != (N,) and ws != (E, N):
        raise ValueError(f"sample_weight is {ws}, need (N,) = {(N,)} (the same for every exit) or (E,N) = {(E, N)}")


def _weights(sample_weight, dev, E, N):
    """``sample_weight`` (N,) or (E,N), numpy or tensor of any real dtype -> the (E,N) float32 table on dev"""
    w = _to_device(sample_weight, torch.float32, dev)
    return (w.unsqueeze(0).expand(E, N) if w.dim() == 1 else w).contiguous()


def reach_weights(exits, num_exits: int, device=None) -> "torch.Tensor":
    """The weight table of cascade-aware heads.  ``exits`` (N,): the exit index at which each document leaves under a policy, as a policy
    scan returns it (``criterion_scan_device``, ``early_exit``; a document no exit releases has index ``num_exits`` or more).  Returns
    (num_exits, N) float32 on the device: 1.0 where ``exits[n] >= e`` -- exit e is asked about document n because no earlier exit released
    it -- else 0.0.  The scan's exit index is the row of features collected in exit order: encoder head e without
    embedding-level exits, row e of ``collect_exit_features(..., embedding_exits=True)`` (embedding-level heads first) with them.  Plain torch, no host
    synchronisation; a device tensor stays on its device."""
    dev = exits.device if (torch is not None and isinstance(exits, torch.Tensor) and exits.is_cuda and device is None) \
        else _require_torch_cuda(device)
    x = _to_device(exits, torch.int64, dev).view(1, -1)
    return (x >= torch.arange(int(num_exits), dtype=torch.int64, device=dev).view(-1, 1)).to(torch.float32)


def balanced_class_weights(labels, num_labels: int, device=None) -> "torch.Tensor":
    """(N,) float32 on the device: w_n = N / (K count[y_n]) with K = ``num_labels`` and count[k] the documents of class k, so that every
    class present weighs N / K in total (scikit-learn's "balanced").  ``labels`` (N,) integers in [0,K).  Plain torch, no host
    synchronisation."""
    dev = labels.device if (torch is not None and isinstance(labels, torch.Tensor) and labels.is_cuda and device is None) \
        else _require_torch_cuda(device)
    y = _to_device(labels, torch.int64, dev).view(-1)
    K, N = int(num_labels), y.shape[0]
    count = torch.zeros((K,), dtype=torch.float64, device=dev).scatter_add_(0, y, torch.ones((N,), dtype=torch.float64, device=dev))
    return (N / (K * count[y])).to(torch.float32)


def _workspace(query, dev, *dims):
    """-> (a device buffer of the bytes ``ee_*_workspace_bytes`` symbol ``query`` asks for ``dims``, their count)"""
    need = int(getattr(capi.load(), query)(*dims))
    return torch.empty((max(need, 1),), dtype=torch.uint8, device=dev), need


def _call(name, dev, *args):
    """The library's ``name`` on ``dev``'s current stream (its last argument); tensors go as their addresses, ``None`` as NULL."""
    fn = getattr(capi.load(), name)
    with torch.cuda.device(dev):
        capi.check(fn(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], torch.cuda.current_stream().cuda_stream), None, name)


def _named(init, suffix, shape):
    """The one tensor of the mapping ``init`` whose key ends in ``suffix``; it must have ``shape``."""
    found = [v for key, v in init.items() if key.endswith(suffix)]
    if len(found) != 1:
        raise ValueError(f"init names {len(found)} tensors ending in {suffix}, need one")
    if tuple(np.shape(found[0])) != shape:
        raise ValueError(f"{suffix} is {tuple(np.shape(found[0]))}, need {shape}")
    return found[0]


def _head_stems(fit, cfg: ModelConfig, K: int, k_name: str, embedding_exits: bool = False):
    """``fit.weight`` (E,K,H) against the configuration (``k_name``: how the message writes K) -> the checkpoint name of every head of the
    fit without its tensor suffix, in the fit's row order: the forward's exit order.  With ``embedding_exits`` the configuration's
    embedding-level heads come first, in the reference's order, then ``encoder.early_exits.{k}``."""
    ec = cfg.exit_config
    n_emb, n_enc = (len(ec.embedding_exits) if embedding_exits else 0), len(ec.encoder_exit_layers)
    E, Kf, H = fit.weight.shape
    if (E, Kf, H) != (n_emb + n_enc, K, cfg.hidden_size):
        count = f"{n_emb} embedding-level + {n_enc} encoder exits: " if embedding_exits else ""
        raise ValueError(f"the fit is (E,{k_name},H) = {(E, Kf, H)}, the configuration wants {count}{(n_emb + n_enc, K, cfg.hidden_size)}")
    p = "beit." if cfg.arch == "beit" else "layoutlmv3."
    return [p + _EMB_HEAD[kind] for kind in ec.embedding_exits[:n_emb]] + [f"{p}encoder.early_exits.{k}" for k in range(n_enc)]


def fit_exit_heads(features, labels, l2: float = 1e-2, gtol: float = 1e-9, max_evals: int = 2000, history: int = 8, device=None,
                   num_labels: int = None, sample_weight=None) -> HeadFit:
    """``features`` (E,N,H) float32 (numpy or device tensor; (N,H) is one exit), ``labels`` (N,) integers in [0,K) with
    K = ``num_labels`` (default: ``labels.max() + 1``; state it when a class may be absent).  Minimises, per exit, mean cross-entropy +
    (l2 / 2)(||W||^2 + ||b||^2) in float64 (include/mmee.h).  Features and parameters stay on the device.

    ``status`` says how each exit stopped.  Unit-variance, uncorrelated features converge to ``gtol = 1e-9`` in 40 - 60 evaluations; the CLS
    rows of a real backbone share a large common component (the condition number grows with it) and need several hundred to a thousand:
    hence the default budget of 2000 (the C entry point has no default) -- a stopped exit costs nothing more, so a generous budget is only
    paid by the exits that use it.  Raise ``max_evals`` when ``status`` is 1.

    ``sample_weight``: ``None`` (every row counts once: ``ee_head_fit``, unchanged), (N,) for every exit alike, or (E,N), one row per exit
    (``reach_weights``, ``balanced_class_weights``, a 0/1 mask of held-out rows); numpy or device tensor of any real dtype, taken as float32.
    The mean becomes the weighted mean (1 / W_e) sum_n w[e][n] l_n (``ee_head_fit_weighted``); the problem stays strongly convex.  A row of
    weight zero is not looked at beyond its features, which must be finite: its label may be anything.  A weight that is negative or not
    finite, or an exit whose weights sum to zero, fails the call.

    Host synchronisation: the call waits for its stream once, after the last launch, to read the error word (a label outside [0,K) fails
    the call); with ``num_labels=None`` reading ``labels.max()`` is a second wait, before the first launch."""
    return _fit_heads(features, labels, None, l2, gtol, max_evals, history, device, num_labels, sample_weight)


def _new_head_fit(cls, dev, E, K, H, l2, *more):
    """The outputs of a one-layer fit on ``dev`` as a ``cls`` (HeadFit, GateFit): zeros, status -1; more: the fields behind ``l2``."""
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    return cls(torch.zeros((E, K, H), dtype=torch.float32, device=dev), torch.zeros((E, K), dtype=torch.float32, device=dev),
               f64(E, K, H), f64(E, K), f64(E), f64(E), torch.zeros((E,), dtype=torch.int32, device=dev),
               torch.full((E,), -1, dtype=torch.int32, device=dev), float(l2), *more)


def _ramp_problem(features, labels, soft, num_labels, device, sample_weight):
    """What the ramp fits are handed, on the device.  soft: None (the labelled objective), or (teacher_logits, alpha, temperature).  The
    refusals from shapes and scalars alone come first, before anything touches the library or a device.
    -> (dev, X (E,N,H) float32, y (N,) int64 or None, teacher (N,K) float32 or None, alpha, temperature, K)"""
    if soft is not None:
        K = _distill_check(features, soft[0], labels, soft[1], soft[2], num_labels)
    _weight_shape(features, sample_weight)
    capi.load()
    dev, X = _rows(features, device)
    if soft is None:
        y, K = _labels(labels, dev, X.shape[1], num_labels)
        return dev, X, y, None, 0.0, 1.0, K
    y = None if labels is None else _labels(labels, dev, X.shape[1], K)[0]
    return dev, X, y, _to_device(soft[0], torch.float32, dev), soft[1], soft[2], K


def _run_ramp_fit(stem, dev, X, y, teacher, alpha, temperature, sample_weight, start, K, l2, gtol, max_evals, history, outs):
    """One call of the C fit of the family ``stem`` ("ee_head_fit", "ee_mlp_head_fit"): ``stem`` itself against labels, ``stem_distill`` with a
    teacher, ``stem_weighted`` (either objective; teacher None: alpha 0) with a ``sample_weight``.  start: () or (theta0,); outs: the
    entry point's output tensors, in its order."""
    E, N, H = X.shape
    mix = (float(alpha), float(temperature))
    if sample_weight is not None:
        name, lead = f"{stem}_weighted", (X, y, teacher, _weights(sample_weight, dev, E, N))
    elif teacher is not None:
        name, lead = f"{stem}_distill", (X, teacher, y)
    else:
        name, lead, mix = stem, (X, y), ()
    query = f"{stem}_weighted_workspace_bytes" if sample_weight is not None else f"{stem}_workspace_bytes"
    ws, need = _workspace(query, dev, E, N, H, K, history)
    _call(name, dev, *lead, *start, E, N, H, K, *mix, float(l2), float(gtol), int(max_evals), int(history), ws, need, *outs)


def _fit_heads(features, labels, soft, l2, gtol, max_evals, history, device, num_labels, sample_weight) -> HeadFit:
    """The one-layer ramp fits' body; soft: as for _ramp_problem"""
    dev, X, y, teacher, alpha, temperature, K = _ramp_problem(features, labels, soft, num_labels, device, sample_weight)
    E, _, H = X.shape
    fit = _new_head_fit(HeadFit, dev, E, K, H, l2, float(alpha), float(temperature))
    _run_ramp_fit("ee_head_fit", dev, X, y, teacher, alpha, temperature, sample_weight, (), K, l2, gtol, max_evals, history,
                  (fit.weight, fit.bias, fit.weight64, fit.bias64, fit.loss, fit.grad_norm, fit.evals, fit.status))
    return fit


# ---- distillation from the final classifier: no labels needed ----------------------------------------------------------------------------
def _distill_check(features, teacher_logits, labels, alpha, temperature, num_labels) -> int:
    """The refusals of the distilled fits, from shapes and scalars alone (nothing touches a device) -> K"""
    fs, ts = tuple(features.shape), tuple(teacher_logits.shape)
    if len(fs) not in (2, 3):
        raise ValueError(f"features are {fs}, need (E,N,H), or (N,H) for one exit")
    N = fs[-2]
    if len(ts) != 2 or ts[0] != N:
        raise ValueError(f"teacher_logits are {ts}, need (N,K) with N = {N}: one row of the final classifier's logits per feature row")
    K = ts[1]
    if num_labels is not None and int(num_labels) != K:
        raise ValueError(f"num_labels = {num_labels}, but teacher_logits have K = {K} classes")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha = {alpha}, need 0 <= alpha <= 1")
    if not 0.0 < temperature < float("inf"):
        raise ValueError(f"temperature = {temperature}, need a finite temperature > 0")
    if alpha < 1.0 and labels is None:
        raise ValueError(f"labels are required at alpha = {alpha} < 1: only alpha = 1 (pure distillation) does without them")
    return K


def fit_distilled_exit_heads(features, teacher_logits, labels=None, alpha: float = 1.0, temperature: float = 1.0, l2: float = 1e-2,
                             gtol: float = 1e-9, max_evals: int = 2000, history: int = 8, device=None, num_labels: int = None,
                             sample_weight=None) -> HeadFit:
    """``fit_exit_heads`` against the final classifier instead of (or mixed with) labels: ``features`` (E,N,H) float32, ``teacher_logits``
    (N,K) float32 (``collect_distill_features``), K = ``teacher_logits.shape[1]`` (``num_labels``, when given, must agree).  Minimises, per
    exit, the mean of (1 - alpha) CE(z, y) + alpha T^2 KL(softmax(t / T) || softmax(z / T)) plus (l2 / 2)(||W||^2 + ||b||^2) in float64
    (include/mmee.h, ee_head_fit_distill).  The defaults ``alpha = 1, temperature = 1`` are the reference's declared ones
    (EETrainingArguments): pure self-distillation, and then ``labels`` are not needed and not looked at.  ``alpha < 1`` needs ``labels`` (N,)
    in [0,K); ``alpha = 0`` is ``fit_exit_heads``' objective.  For 0 <= alpha <= 1 the problem stays strongly convex: one optimum.

    A teacher logit that is not finite (dump-all marks the rows a document never reached with NaN) fails the call, as a label out of range
    does.  Budget, ``status`` and the one host wait after the last launch are ``fit_exit_heads``'; no wait is spent on ``labels.max()``.
    ``sample_weight`` is ``fit_exit_heads``': it weighs the whole mixed row loss, and neither the label nor the teacher row of a row of weight
    zero is looked at."""
    return _fit_heads(features, labels, (teacher_logits, alpha, temperature), l2, gtol, max_evals, history, device, num_labels, sample_weight)


# ---- two-layer heads: dense + tanh + out_proj -----------------------------------------------------------------------------------------
_MLP_BLOCKS = ("dense.weight", "dense.bias", "out_proj.weight", "out_proj.bias")


def mlp_param_count(H: int, K: int) -> int:
    return H * H + H + K * H + K


@dataclass
class MlpHeadFit:
    dense_weight: "torch.Tensor"  # (E,H,H) float32, device: W1 [out,in]
    dense_bias: "torch.Tensor"    # (E,H)
    weight: "torch.Tensor"        # (E,K,H): out_proj
    bias: "torch.Tensor"          # (E,K)
    theta64: "torch.Tensor"       # (E,P) float64: W1 row-major, b1, W2 row-major, b2 -- the point the float32 tensors are rounded from
    loss: "torch.Tensor"          # (E,) float64: the objective at the returned point
    grad_norm: "torch.Tensor"     # (E,) float64
    evals: "torch.Tensor"         # (E,) int32
    status: "torch.Tensor"        # (E,) int32: 0 stationary (grad_norm <= gtol), 1 max_evals, 2 the line search made no progress
    l2: float
    alpha: float = 0.0            # weight of the distillation term (fit_distilled_mlp_exit_heads); 0: fitted against labels alone
    temperature: float = 1.0      # the distillation temperature

    def logits(self, features) -> "torch.Tensor":
        """(E,N,K) float64 logits of the float32 heads on ``features`` (E,N,H), on the device."""
        return _mlp_logits(self, features)

    def state_dict(self, cfg: ModelConfig, embedding_exits: bool = False) -> Dict[str, np.ndarray]:
        """``{prefix}encoder.early_exits.{k}.dense.weight / .bias`` and ``.out_proj.weight / .bias`` (host float32), ready for
        ``engine.load_weights`` next to the backbone's tensors.  ``embedding_exits=True``: as ``HeadFit.state_dict``, the first n_emb of the
        fit's n_emb + E heads are the configuration's embedding-level heads."""
        _check_fittable(cfg, 2, embedding_exits)
        return _mlp_state(self, _head_stems(self, cfg, cfg.num_labels, "K", embedding_exits))


def _mlp_logits(fit, features):
    """(E,N,K) float64 logits of the float32 two-layer heads ``fit.dense_weight`` (E,H,H), ``fit.dense_bias`` (E,H), ``fit.weight`` (E,K,H),
    ``fit.bias`` (E,K) on ``features`` (E,N,H)"""
    f64 = torch.float64
    X = _rows(features, on=fit.weight.device)[1].to(f64)
    A = torch.tanh(torch.baddbmm(fit.dense_bias.to(f64).unsqueeze(1), X, fit.dense_weight.to(f64).transpose(1, 2)))
    return torch.baddbmm(fit.bias.to(f64).unsqueeze(1), A, fit.weight.to(f64).transpose(1, 2))


def _mlp_theta0(init, E, H, K, dev):
    """The start as a device tensor (E,P) float64."""
    P = mlp_param_count(H, K)
    if isinstance(init, str):
        if init != "identity":
            raise ValueError(f"init = {init!r}: 'identity', an (E,P) array or a mapping of head tensors")
        th = torch.zeros((E, P), dtype=torch.float64, device=dev)
        th[:, :H * H].view(E, H, H).diagonal(dim1=1, dim2=2).fill_(1.0)
        return th
    if isinstance(init, Mapping):
        shapes = ((H, H), (H,), (K, H), (K,))
        rows = []
        for k in range(E):
            rows.append(torch.cat([_to_device(_named(init, f"encoder.early_exits.{k}.{name}", shape), torch.float64, dev).reshape(-1)
                                   for name, shape in zip(_MLP_BLOCKS, shapes)]))
        return torch.stack(rows).contiguous()
    th = _to_device(init, torch.float64, dev)
    if th.dim() == 1:
        th = th.unsqueeze(0)
    if tuple(th.shape) != (E, P):
        raise ValueError(f"init is {tuple(th.shape)}, need (E,P) = {(E, P)}")
    return th


def fit_mlp_exit_heads(features, labels, l2: float = 1e-2, gtol: float = 1e-6, max_evals: int = 4000, history: int = 8, init="identity",
                       device=None, num_labels: int = None, sample_weight=None) -> MlpHeadFit:
    """Two-layer heads (dense + tanh + out_proj) per exit.  ``features`` (E,N,H) float32 (numpy or device tensor; (N,H) is one exit),
    ``labels`` (N,) integers in [0,K) with K = ``num_labels`` (default: ``labels.max() + 1``).  Minimises, per exit, mean cross-entropy of
    W2 tanh(W1 x + b1) + b2 plus (l2 / 2) ||theta||^2 over all four blocks, in float64 (include/mmee.h), by the L-BFGS of ``fit_exit_heads``.

    ``init``: ``"identity"`` (W1 = I, everything else 0: the one-layer head on tanh(x); zero itself is a saddle the iteration never
    leaves), an (E,P) array or tensor in the layout W1 row-major, b1, W2 row-major, b2, or a mapping holding, per exit k, the tensors
    ``...encoder.early_exits.{k}.dense.weight / .dense.bias / .out_proj.weight / .out_proj.bias`` of a checkpoint (a warm start).

    The objective is not convex.  ``status`` 0 says the gradient norm of the returned point is <= ``gtol``: a stationary point reached by
    descent from ``init``.  Unit-variance features of a few hundred rows need 600 - 1800 evaluations to ``gtol = 1e-6``: hence the default
    budget of 4000; a stopped exit costs nothing more.

    ``sample_weight`` is ``fit_exit_heads``' (``ee_mlp_head_fit_weighted``).

    Host synchronisation: as for ``fit_exit_heads``, one wait after the last launch (plus one for ``labels.max()`` without ``num_labels``)."""
    return _fit_mlp_heads(features, labels, None, l2, gtol, max_evals, history, init, device, num_labels, sample_weight)


def _fit_mlp_heads(features, labels, soft, l2, gtol, max_evals, history, init, device, num_labels, sample_weight) -> MlpHeadFit:
    """The two-layer ramp fits' body: _fit_heads' with a start and MlpHeadFit's outputs (zeros, status -1)"""
    dev, X, y, teacher, alpha, temperature, K = _ramp_problem(features, labels, soft, num_labels, device, sample_weight)
    E, _, H = X.shape
    theta0 = _mlp_theta0(init, E, H, K, dev)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    fit = MlpHeadFit(z((E, H, H), torch.float32), z((E, H), torch.float32), z((E, K, H), torch.float32), z((E, K), torch.float32),
                     z((E, mlp_param_count(H, K)), torch.float64), z((E,), torch.float64), z((E,), torch.float64), z((E,), torch.int32),
                     torch.full((E,), -1, dtype=torch.int32, device=dev), float(l2), float(alpha), float(temperature))
    _run_ramp_fit("ee_mlp_head_fit", dev, X, y, teacher, alpha, temperature, sample_weight, (theta0,), K, l2, gtol, max_evals, history,
                  (fit.dense_weight, fit.dense_bias, fit.weight, fit.bias, fit.theta64, fit.loss, fit.grad_norm, fit.evals, fit.status))
    return fit


def fit_distilled_mlp_exit_heads(features, teacher_logits, labels=None, alpha: float = 1.0, temperature: float = 1.0, l2: float = 1e-2,
                                 gtol: float = 1e-6, max_evals: int = 4000, history: int = 8, init="identity", device=None,
                                 num_labels: int = None, sample_weight=None) -> MlpHeadFit:
    """``fit_mlp_exit_heads`` against the final classifier: the objective of ``fit_distilled_exit_heads`` on the two-layer head
    (include/mmee.h, ee_mlp_head_fit_distill), from the start ``init`` (``"identity"`` needs no labels either).  Inputs, ``alpha``,
    ``temperature`` and the failures are those of ``fit_distilled_exit_heads``; budget, ``status`` (a stationary point reached by descent from
    ``init``: the objective is not convex) and ``init`` are ``fit_mlp_exit_heads``'; ``sample_weight`` is ``fit_distilled_exit_heads``'."""
    return _fit_mlp_heads(features, labels, (teacher_logits, alpha, temperature), l2, gtol, max_evals, history, init, device, num_labels,
                          sample_weight)


# ---- the learning-to-exit classifier: one Linear(H, 1) for all encoder exits ---------------------------------------------------------------------
LTE_LOSSES = {"mse": capi.LTE_LOSS_MSE, "bce": capi.LTE_LOSS_BCE}
_LTE_W, _LTE_B = "encoder.lte_classifier.weight", "encoder.lte_classifier.bias"


def _check_lte_cfg(cfg: ModelConfig):
    if cfg.arch == "beit":
        raise ValueError("the LTE classifier is fitted for LayoutLMv3 configurations only: use_lte is refused on BEiT / DiT handles")
    if not cfg.exit_config.encoder_exit_layers:
        raise ValueError("the configuration has no encoder exits: the LTE classifier scores the CLS rows leaving encoder exit layers")


def collect_lte_features(engine, batches: Iterable[Mapping]):
    """Dump-all forwards of ``engine`` over ``batches`` (dicts of ``engine.forward`` keyword inputs).  Returns two device tensors from the
    same forwards: ``features`` (E,N,H) float32, the CLS rows leaving the E configured encoder exit layers, and ``logits`` (E,N,K) float32,
    those exits' policy logits (``all_logits``: ramps the head's logits, gates ``classifier(gate input)``).  Any LayoutLMv3 engine with an
    encoder exit will do -- ramp or gate, 1- or 2-layer heads, with or without ``use_lte``; embedding-level exits are skipped."""
    _check_lte_cfg(engine.cfg)
    return _rows_and_logits(engine, batches)


def lte_targets(logits, labels, device=None) -> "torch.Tensor":
    """(E,N) float64 device tensor: 1 where the argmax (first maximum) of ``logits`` (E,N,K) float32 differs from ``labels`` (N,), else 0 --
    the reference's ``1 - lte_gold``.  A label outside [0,K) or a NaN logit (a row its document never reached) fails the call."""
    capi.load()
    dev, Z = _rows(logits, device)
    y = _to_device(labels, torch.int64, dev).view(-1)
    E, N, K = Z.shape
    if y.shape[0] != N:
        raise ValueError("labels must have one entry per document")
    out = torch.zeros((E, N), dtype=torch.float64, device=dev)
    _call("ee_lte_targets", dev, Z, y, E, N, K, out)
    return out


@dataclass
class LteFit:
    weight: "torch.Tensor"       # (1,H) float32, device
    bias: "torch.Tensor"         # (1,)  float32
    theta64: "torch.Tensor"      # (H+1,) float64: w then b, the point the float32 pair is rounded from
    loss: "torch.Tensor"         # (1,) float64: the objective at the returned point
    grad_norm: "torch.Tensor"    # (1,) float64
    evals: "torch.Tensor"        # (1,) int32
    status: "torch.Tensor"       # (1,) int32: 0 stationary (grad_norm <= gtol), 1 max_evals, 2 the line search made no progress
    l2: float
    loss_kind: str

    def scores(self, features) -> "torch.Tensor":
        """(E,N) float64 scores sigmoid(w . x + b) of the float32 classifier on ``features`` (E,N,H), on the device, in the forward's
        summation order: the rows ``sweep.lte_sweep`` and ``lte_scan_device`` take."""
        dev, X = _rows(features, on=self.weight.device)
        E, N, H = X.shape
        if H != self.weight.shape[1]:
            raise ValueError(f"features have H = {H}, the classifier {self.weight.shape[1]}")
        out = torch.empty((E, N), dtype=torch.float64, device=dev)
        _call("ee_lte_scores", dev, X, self.weight, self.bias, E, N, H, out)
        return out

    def state_dict(self, cfg: ModelConfig) -> Dict[str, np.ndarray]:
        """``layoutlmv3.encoder.lte_classifier.weight`` (1,H) and ``.bias`` (1,) (host float32), ready for ``engine.load_weights`` of a
        ``use_lte`` engine next to the other tensors."""
        _check_lte_cfg(cfg)
        if tuple(self.weight.shape) != (1, cfg.hidden_size):
            raise ValueError(f"the fit has weight {tuple(self.weight.shape)}, the configuration wants {(1, cfg.hidden_size)}")
        return {f"layoutlmv3.{_LTE_W}": np.ascontiguousarray(self.weight.cpu().numpy()).reshape(1, -1),
                f"layoutlmv3.{_LTE_B}": np.ascontiguousarray(self.bias.cpu().numpy()).reshape(1)}


def _lte_theta0(init, H):
    """The start as a host (H+1,) float64 array, or None for zero."""
    if init is None:
        return None
    host = lambda v: v.detach().cpu().numpy() if (torch is not None and isinstance(v, torch.Tensor)) else np.asarray(v)
    if isinstance(init, Mapping):
        return np.concatenate([host(_named(init, name, shape)).astype(np.float64).reshape(-1)
                               for name, shape in ((_LTE_W, (1, H)), (_LTE_B, (1,)))])
    a = host(init)
    if tuple(a.shape) != (H + 1,):
        raise ValueError(f"init is {tuple(a.shape)}, need (H+1,) = {(H + 1,)}: w then b")
    return a.astype(np.float64)


def fit_lte_classifier(features, targets, loss: str = "mse", l2: float = 1e-2, gtol: float = 1e-9, max_evals: int = LTE_MAX_EVALS,
                       history: int = 8, init=None, device=None) -> LteFit:
    """``features`` (E,N,H) float32 (numpy or device tensor; (N,H) is one exit), ``targets`` (E,N) in [0,1] (``lte_targets``; soft targets
    are allowed).  Minimises sum_e mean_n l(w . x + b, t) + (l2 / 2)(||w||^2 + b^2) over ONE (w, b) in float64 (include/mmee.h), by the
    L-BFGS of ``fit_exit_heads``.  ``loss="mse"`` is the reference's (sigmoid + MSE per exit, summed; not convex: ``status`` 0 is a stationary
    point reached by descent from ``init``); ``loss="bce"`` is the strongly convex alternative with one optimum.

    ``init``: ``None`` (zero), an (H+1,) array (w then b), or a mapping holding ``...encoder.lte_classifier.weight`` (1,H) and ``.bias`` (1,)
    of a checkpoint (a warm start).

    ``status`` says how the fit stopped.  Evaluations to ``gtol = 1e-9`` as tests/test_gpu_lte_fit.py prints them: unit-variance features
    19 - 72 (MSE 22 / 40 / 32 / 55 / 72, BCE 19 / 34 / 25 / 56 / 72 on its five problems), the CLS rows of the synthetic backbones, which share a
    large common component, 130 (H = 128) and 283 (H = 256, split precision); 40 000 well-conditioned rows an exit need 12 - 13.  Hence the
    default budget of 1000, 3.5 times the largest count seen (the C entry point has no default).  The launch list is fixed, so every unused tick
    still costs its three empty launches (about 9 microseconds): raise ``max_evals`` when ``status`` is 1, lower it when the call's latency matters.

    Host synchronisation: one wait after the last launch, to read the error word (a target outside [0,1] or NaN fails the call)."""
    if loss not in LTE_LOSSES:
        raise ValueError(f"loss = {loss!r}: 'mse' (the reference's) or 'bce'")
    H_in = int(features.shape[-1])
    theta0 = _lte_theta0(init, H_in)
    capi.load()
    dev, X = _rows(features, device)
    E, N, H = X.shape
    T = _to_device(targets, torch.float64, dev)
    if T.dim() == 1:
        T = T.unsqueeze(0)
    if tuple(T.shape) != (E, N):
        raise ValueError(f"targets are {tuple(targets.shape)}, need (E,N) = {(E, N)}")
    th0 = None if theta0 is None else _to_device(theta0, torch.float64, dev)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    fit = LteFit(z((1, H), torch.float32), z((1,), torch.float32), z((H + 1,), torch.float64), z((1,), torch.float64), z((1,), torch.float64),
                 z((1,), torch.int32), torch.full((1,), -1, dtype=torch.int32, device=dev), float(l2), loss)
    ws, need = _workspace("ee_lte_fit_workspace_bytes", dev, E, N, H, history)
    _call("ee_lte_fit", dev, X, T, th0, E, N, H, LTE_LOSSES[loss], float(l2), float(gtol), int(max_evals), int(history), ws, need, fit.weight,
          fit.bias, fit.theta64, fit.loss, fit.grad_norm, fit.evals, fit.status)
    return fit


# ---- 2-way gate heads: the heads inference_strategy = "gate" lets decide ---------------------------------------------------------------------
def _check_gate_cfg(cfg: ModelConfig, head_layers: int = 1, embedding_exits: bool = False):
    ec = cfg.exit_config
    if cfg.arch == "beit":
        raise ValueError("gate heads are fitted for LayoutLMv3 configurations only")
    if str(ec.encoder_layer_strategy) != "gate":
        raise ValueError("gate heads are fitted for the gate strategy only (encoder_layer_strategy = 'gate'): fit_exit_heads fits ramps")
    if head_layers == 2:
        if ec.exit_head_num_layers != 2:
            raise ValueError("two-layer gate heads are fitted for exit_head_num_layers == 2 only (fit_gate_heads fits the one-layer gate)")
    elif ec.exit_head_num_layers != 1:
        raise ValueError("gate heads are fitted for exit_head_num_layers == 1 only: a two-layer gate is not a convex problem, "
                         "fit_mlp_gate_heads fits it")
    if not _check_embedding_exits(cfg, embedding_exits) and not ec.encoder_exit_layers:
        raise ValueError("the configuration has no encoder exits")


def collect_gate_features(engine, batches: Iterable[Mapping], embedding_exits: bool = False):
    """Dump-all forwards of a gate-strategy ``engine`` over ``batches`` (dicts of ``engine.forward`` keyword inputs).  Returns two device
    tensors from the same forwards: ``features`` (E,N,H) float32, the CLS rows leaving the E configured encoder exit layers -- the inputs of
    the gates ``encoder.early_exits.0 .. E-1`` --, and ``gated_logits`` (E,N,K) float32, ``classifier(gate input)`` at those exits (the
    policy logits, ``all_logits``).  By default encoder exits only: embedding-level exits are skipped, as ``collect_lte_features`` skips them.
    ``embedding_exits=True``: the features are ``collect_exit_features(..., embedding_exits=True)``'s, (n_emb + E,N,H) with the pooled rows
    of the embedding-level gates first, and ``gated_logits`` is (n_emb + E,N,K), ``all_logits[:n_emb + E]``; the same pitfall holds (the text
    and concat rows depend on the T the batch is padded to)."""
    ec = engine.cfg.exit_config
    if engine.cfg.arch == "beit" or str(ec.encoder_layer_strategy) != "gate":
        raise ValueError("collect_gate_features needs a LayoutLMv3 engine of the gate strategy (encoder_layer_strategy = 'gate')")
    if not ec.encoder_exit_layers and not (embedding_exits and ec.embedding_exits):
        raise ValueError("the configuration has no encoder exits")
    return _rows_and_logits(engine, batches, embedding_exits)


def gate_targets(gated_logits, labels, device=None) -> "torch.Tensor":
    """(E,N) float64 device tensor: 1 where the argmax (first maximum) of ``gated_logits`` (E,N,K) float32 equals ``labels`` (N,), else 0 --
    the reference's ``correctly_gated`` (EE/models/LayoutLMv3.py:770-773), and ``1 - lte_targets``: the launch of ``ee_lte_targets`` and one
    subtraction on the device (exact).  A label outside [0,K) or a NaN logit fails the call."""
    return 1.0 - lte_targets(gated_logits, labels, device)


def _gate_scores(logits):
    """(E,N) float64 gate scores of the float32 roundings of ``logits`` (E,N,2), by the device function the forward decides with"""
    from .sweep import gate_table
    h = logits.to(torch.float32).contiguous()
    dummy = torch.zeros((h.shape[1], 1), dtype=torch.float64, device=h.device)
    return gate_table(h, dummy, device=h.device)[:-1]


@dataclass
class GateFit:
    weight: "torch.Tensor"       # (E,2,H) float32, device
    bias: "torch.Tensor"         # (E,2)   float32
    weight64: "torch.Tensor"     # the float64 solution the float32 pair is rounded from
    bias64: "torch.Tensor"
    loss: "torch.Tensor"         # (E,) float64: the objective at the returned point
    grad_norm: "torch.Tensor"    # (E,) float64
    evals: "torch.Tensor"        # (E,) int32: loss / gradient evaluations used
    status: "torch.Tensor"       # (E,) int32: 0 converged (grad_norm <= gtol), 1 max_evals, 2 the line search made no progress
    l2: float

    def logits(self, features) -> "torch.Tensor":
        """(E,N,2) float64 gate logits of the float32 heads on ``features`` (E,N,H), on the device."""
        return _linear_logits(self, features)

    def scores(self, features) -> "torch.Tensor":
        """(E,N) float64 gate scores 1 / (1 + exp(h0 - h1)) of the float32 heads' float32 logits on ``features`` (E,N,H), on the device, by the
        device function the forward decides with (``sweep.gate_table``'s rows)."""
        return _gate_scores(self.logits(features))

    def state_dict(self, cfg: ModelConfig, embedding_exits: bool = False) -> Dict[str, np.ndarray]:
        """``layoutlmv3.encoder.early_exits.{k}.out_proj.weight`` (2,H) / ``.bias`` (2,) (host float32), ready for ``engine.load_weights`` next
        to the backbone's tensors.  ``embedding_exits=True``: as ``HeadFit.state_dict``, the first n_emb of the fit's n_emb + E gates are the
        configuration's embedding-level heads."""
        _check_gate_cfg(cfg, 1, embedding_exits)
        return _out_proj_state(self, _head_stems(self, cfg, 2, "2", embedding_exits))


def fit_gate_heads(features, targets, l2: float = 1e-2, gtol: float = 1e-9, max_evals: int = 2000, history: int = 8, device=None,
                   sample_weight=None) -> GateFit:
    """``features`` (E,N,H) float32 (numpy or device tensor; (N,H) is one exit; ``collect_gate_features``), ``targets`` (E,N) in [0,1]
    (``gate_targets``; soft targets are allowed).  Minimises, per exit, (1 / (2N)) sum_n [bce(z_1, c) + bce(z_0, 1 - c)] +
    (l2 / 2)(||W||^2 + ||b||^2) over W (2,H), b (2,) in float64 (include/mmee.h, ee_head_fit_gate): ``nn.BCEWithLogitsLoss()`` on the (N,2)
    gate logits against the one-hot of the target, the reference's gate loss.  Strongly convex: one optimum.  The kernels, the L-BFGS and the
    budget are ``fit_exit_heads``' at K = 2.  Limits: H <= 1024 and a multiple of 4; ``sample_weight`` is not built for one-layer gates and is
    refused (``fit_mlp_gate_heads``, the two-layer gates' fit, takes it).

    Host synchronisation: one wait after the last launch, to read the error word (a target outside [0,1] or not finite fails the call)."""
    if sample_weight is not None:
        raise ValueError("fit_gate_heads: sample_weight is not built for one-layer gate heads (the ramp fits and fit_mlp_gate_heads take it)")
    fs = tuple(features.shape)
    if len(fs) not in (2, 3):
        raise ValueError(f"features are {fs}, need (E,N,H), or (N,H) for one exit")
    E, N, H = (1,) + fs if len(fs) == 2 else fs
    if H > 1024 or H % 4:
        raise ValueError(f"fit_gate_heads: H = {H}, need H <= 1024 and a multiple of 4")
    ts = tuple(np.shape(targets))
    if ts != (E, N) and not (E == 1 and ts == (N,)):
        raise ValueError(f"targets are {ts}, need (E,N) = {(E, N)}")
    if not l2 > 0.0:
        raise ValueError(f"fit_gate_heads: l2 = {l2}, need l2 > 0 (the objective is strongly convex only then)")
    capi.load()
    dev, X = _rows(features, device)
    T = _to_device(targets, torch.float64, dev).view(E, N)
    fit = _new_head_fit(GateFit, dev, E, 2, H, l2)
    ws, need = _workspace("ee_head_fit_workspace_bytes", dev, E, N, H, 2, history)
    _call("ee_head_fit_gate", dev, X, T, E, N, H, float(l2), float(gtol), int(max_evals), int(history), ws, need, fit.weight, fit.bias,
          fit.weight64, fit.bias64, fit.loss, fit.grad_norm, fit.evals, fit.status)
    return fit


# ---- two-layer 2-way gate heads: dense + tanh + out_proj (2,H), the default depth --------------------------------------------------------------
@dataclass
class MlpGateFit:
    dense_weight: "torch.Tensor"  # (E,H,H) float32, device: W1 [out,in]
    dense_bias: "torch.Tensor"    # (E,H)
    weight: "torch.Tensor"        # (E,2,H): out_proj; row 1 is "correctly gated"
    bias: "torch.Tensor"          # (E,2)
    theta64: "torch.Tensor"       # (E,P) float64: W1 row-major, b1, W2 row-major, b2 -- the point the float32 tensors are rounded from
    loss: "torch.Tensor"          # (E,) float64: the objective at the returned point
    grad_norm: "torch.Tensor"     # (E,) float64
    evals: "torch.Tensor"         # (E,) int32
    status: "torch.Tensor"        # (E,) int32: 0 stationary (grad_norm <= gtol), 1 max_evals, 2 the line search made no progress
    l2: float

    def logits(self, features) -> "torch.Tensor":
        """(E,N,2) float64 gate logits of the float32 heads on ``features`` (E,N,H), on the device."""
        return _mlp_logits(self, features)

    def scores(self, features) -> "torch.Tensor":
        """(E,N) float64 gate scores of the float32 heads' float32 logits on ``features`` (E,N,H), as ``GateFit.scores``."""
        return _gate_scores(self.logits(features))

    def state_dict(self, cfg: ModelConfig, embedding_exits: bool = False) -> Dict[str, np.ndarray]:
        """``layoutlmv3.encoder.early_exits.{k}.dense.weight`` (H,H) / ``.dense.bias`` (H,) / ``.out_proj.weight`` (2,H) / ``.out_proj.bias`` (2,)
        (host float32), ready for ``engine.load_weights`` next to the backbone's tensors.  ``embedding_exits=True``: as
        ``HeadFit.state_dict``, the first n_emb of the fit's n_emb + E gates are the configuration's embedding-level heads."""
        _check_gate_cfg(cfg, 2, embedding_exits)
        return _mlp_state(self, _head_stems(self, cfg, 2, "2", embedding_exits))


def fit_mlp_gate_heads(features, targets, l2: float = 1e-2, gtol: float = 1e-6, max_evals: int = 4000, history: int = 8, init="identity",
                       device=None, sample_weight=None) -> MlpGateFit:
    """Two-layer gate heads (dense + tanh + out_proj (2,H)) per exit.  ``features`` (E,N,H) float32 (numpy or device tensor; (N,H) is one exit;
    ``collect_gate_features``), ``targets`` (E,N) in [0,1] (``gate_targets``; soft targets are allowed).  Minimises, per exit,
    (1 / (2N)) sum_n [bce(z_1, c) + bce(z_0, 1 - c)] + (l2 / 2) ||theta||^2 with z = W2 tanh(W1 x + b1) + b2, in float64 (include/mmee.h,
    ee_mlp_head_fit_gate): ``fit_gate_heads``' loss on ``fit_mlp_exit_heads``' head at K = 2, by the same L-BFGS.  Limits: H <= 1024 and a
    multiple of 4.

    ``init`` is ``fit_mlp_exit_heads``' at K = 2: ``"identity"`` (W1 = I, everything else 0: the one-layer gate on tanh(x)), an (E,P) array or
    tensor, or a mapping holding a checkpoint's four tensors per exit (a warm start).  The objective is not convex: ``status`` 0 says the
    gradient norm of the returned point is <= ``gtol``, a stationary point reached by descent from ``init``; budget as ``fit_mlp_exit_heads``.

    ``sample_weight``: ``None`` (``ee_mlp_head_fit_gate``), (N,) or (E,N) as for the ramp fits (``ee_mlp_head_fit_gate_weighted``): the mean
    becomes the weighted mean.  ``reach_weights(exits, E)`` of a policy scan fits gate e on the documents that reach it.  The target of a row of
    weight zero is not looked at; a weight that is negative or not finite, or an exit whose weights sum to zero, fails the call.

    Host synchronisation: one wait after the last launch, to read the error word (a target outside [0,1] or not finite fails the call)."""
    fs = tuple(features.shape)
    if len(fs) not in (2, 3):
        raise ValueError(f"features are {fs}, need (E,N,H), or (N,H) for one exit")
    E, N, H = (1,) + fs if len(fs) == 2 else fs
    if H > 1024 or H % 4:
        raise ValueError(f"fit_mlp_gate_heads: H = {H}, need H <= 1024 and a multiple of 4")
    ts = tuple(np.shape(targets))
    if ts != (E, N) and not (E == 1 and ts == (N,)):
        raise ValueError(f"targets are {ts}, need (E,N) = {(E, N)}")
    if not l2 > 0.0:
        raise ValueError(f"fit_mlp_gate_heads: l2 = {l2}, need l2 > 0")
    _weight_shape(features, sample_weight)
    capi.load()
    dev, X = _rows(features, device)
    T = _to_device(targets, torch.float64, dev).view(E, N)
    theta0 = _mlp_theta0(init, E, H, 2, dev)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    fit = MlpGateFit(z((E, H, H), torch.float32), z((E, H), torch.float32), z((E, 2, H), torch.float32), z((E, 2), torch.float32),
                     z((E, mlp_param_count(H, 2)), torch.float64), z((E,), torch.float64), z((E,), torch.float64), z((E,), torch.int32),
                     torch.full((E,), -1, dtype=torch.int32, device=dev), float(l2))
    if sample_weight is None:
        name, query, lead = "ee_mlp_head_fit_gate", "ee_mlp_head_fit_workspace_bytes", (X, T)
    else:
        name, query, lead = "ee_mlp_head_fit_gate_weighted", "ee_mlp_head_fit_weighted_workspace_bytes", (X, T, _weights(sample_weight, dev, E, N))
    ws, need = _workspace(query, dev, E, N, H, 2, history)
    _call(name, dev, *lead, theta0, E, N, H, float(l2), float(gtol), int(max_evals), int(history), ws, need, fit.dense_weight, fit.dense_bias,
          fit.weight, fit.bias, fit.theta64, fit.loss, fit.grad_norm, fit.evals, fit.status)
    return fit


# ---- the exit ensemble: earlier heads' predictions join each decision --------------------------------------------------------------------------
@dataclass
class EnsembleFit:
    weights: "torch.Tensor"      # (E1,E1) float64, device: lower triangular, row m = the weights of exit m over exits 0 .. m
    bias: "torch.Tensor"         # (E1,K)  float64
    loss: "torch.Tensor"         # (E1,) float64: the objective at the returned point; never above the plain exit's mean NLL
    grad_norm: "torch.Tensor"    # (E1,) float64
    evals: "torch.Tensor"        # (E1,) int32
    status: "torch.Tensor"       # (E1,) int32: 0 converged (grad_norm <= gtol), 1 max_evals, 2 the line search made no progress
    l2: float

    def apply(self, logits) -> "torch.Tensor":
        """``sweep.ensemble_logits(logits, self.weights, self.bias)``: the ensembled (E1,N,K) float64 array of un-ensembled dumped ``logits``,
        with the bits a forward returns after ``engine.set_ensemble(self)``."""
        from .sweep import ensemble_logits
        return ensemble_logits(logits, self.weights, self.bias, device=self.weights.device)


def fit_exit_ensemble(logits, labels, l2: float = 1e-2, gtol: float = 1e-9, max_evals: int = 1000, history: int = 8, init=None,
                      device=None) -> EnsembleFit:
    """The weights of the exit ensemble (include/mmee.h, at ee_set_ensemble; Zero Time Waste's weighted geometric ensemble of the exits seen so
    far) from a dumped array, on the device (``ee_ensemble_fit``).  ``logits`` (E1,N,K): the UN-ensembled scaled rows of a dump-all forward
    (``all_logits``; numpy or device tensor, taken as float64); ``labels`` (N,) integers in [0,K).  Per exit m it minimises, in float64,
    mean cross-entropy of the ensemble row + (l2 / 2)(||w_m - e_m||^2 + ||b_m||^2): the penalty pulls toward the plain exit, where the fit
    starts (``init=None``), so ``loss[m]`` never exceeds the plain exit's mean NLL.  Strongly convex: one optimum, reached by the L-BFGS of
    ``fit_exit_heads``; deterministic to the bit.  ``init``: an ``EnsembleFit`` or a ``(weights, bias)`` pair to start from.

    The result goes to ``engine.set_ensemble(fit)`` and, through ``fit.apply(logits)``, to every dumped-array tool (``sweep.csf_table``,
    ``threshold_search``, ``metrics.exit_report``, ``Policy``) -- fit on one split, search thresholds on the ensembled array of another.

    Not built: ``sample_weight`` and reach weights, per-class weights, and the ensemble under the "gate" criterion or ``use_lte``.
    Host synchronisation: one wait after the last launch, to read the error word (a label outside [0,K) or a logit that is not finite -- a
    NaN row is an exit the document never reached -- fails the call)."""
    if not (l2 > 0):
        raise ValueError(f"fit_exit_ensemble: l2 = {l2}, need l2 > 0")
    capi.load()
    dev = logits.device if (torch is not None and isinstance(logits, torch.Tensor) and logits.is_cuda and device is None) \
        else _require_torch_cuda(device)
    L = _to_device(logits, torch.float64, dev)
    if L.dim() != 3:
        raise ValueError("logits must have shape (num_exits + 1, num_samples, num_labels)")
    E1, N, K = L.shape
    y = _to_device(labels, torch.int64, dev).view(-1)
    if y.shape[0] != N:
        raise ValueError("labels must have one entry per document")
    w0 = b0 = None
    if init is not None:
        iw, ib = (init.weights, init.bias) if isinstance(init, EnsembleFit) else init
        w0 = _to_device(iw, torch.float64, dev)
        b0 = None if ib is None else _to_device(ib, torch.float64, dev)
        if tuple(w0.shape) != (E1, E1) or (b0 is not None and tuple(b0.shape) != (E1, K)):
            raise ValueError(f"init must be weights (E1,E1) = {(E1, E1)} and bias (E1,K) = {(E1, K)}")
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    fit = EnsembleFit(z((E1, E1), torch.float64), z((E1, K), torch.float64), z((E1,), torch.float64), z((E1,), torch.float64),
                      z((E1,), torch.int32), torch.full((E1,), -1, dtype=torch.int32, device=dev), float(l2))
    ws, need = _workspace("ee_ensemble_fit_workspace_bytes", dev, E1, N, K, history)
    _call("ee_ensemble_fit", dev, L, y, w0, b0, E1, N, K, float(l2), float(gtol), int(max_evals), int(history), ws, need, fit.weights, fit.bias,
          fit.loss, fit.grad_norm, fit.evals, fit.status)
    return fit
