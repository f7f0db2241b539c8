"""The vision-first call (include/mmee.h at ee_forward_vision) on the MI355X.

1. vision_pool_kernel alone through ee_debug_vision_pool against float64 at every NV / FULL route and chunk edge, held to the bound
   tests/test_gpu_rows.py holds the pooled visual mean to (per row max|got - ref64| <= max(2 err32, 1e-6), err32 = torch float32 on the CPU), and,
   exactly, against ee_embedding_inputs' out_vision on the same pixels.
2. Phase 1 (forward_vision) against the one-call forward: the leavers' bits, the survivors' list, sentinels where nothing may be written.
3. The whole call on the dict route and on the callable route, bit for bit against forward on the full inputs, under the plain setting and
   under the margin criterion, a combined exit rule, an ensemble and temperatures; low_latency against the hand composition.
4. A handle that used the feature behaves as one that never did.  5. Every refusal, by message.

thresholds[0] is a midpoint of two adjacent sorted exit-0 criteria of the device's own dump-all call, more than 1e-9 apart (asserted on the CPU),
so that exactly 0, 5 or 12 of the 12 documents leave at exit 0."""
import ctypes as C

import numpy as np
import pytest

from . import rows_ref as R
from . import vision_first_ref as VR
from .conftest import DIT_EE, H256_KW, MATRIX_CASES, TINY_CASES, report_measured
from .hook_util import SENTINEL, _dev, _f32, _ptr, _stream, _torch

pytestmark = pytest.mark.gpu

GUARD = 4
B_DOCS = 12
LEAVE = (0, 5, 12)
H256_GATE_VISION = dict(exits=["vision_avg", "text_visual_concat", 1, 2], encoder_layer_strategy="gate", inference_strategy="max_confidence")
CASES = {      # name -> (tiny(**kw) keyword arguments, EE_config, precision, T)
    "tiny_ramp": ({}, TINY_CASES["tiny_ramp"], "fp32", 40),
    "h256_entropy_1layer": (H256_KW, MATRIX_CASES["h256_entropy_1layer"][1], "split", 48),
    "h256_gate_vision": (H256_KW, H256_GATE_VISION, "split", 48),
}
TEXT_KEYS = ("input_ids", "attention_mask", "bbox")


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _sent(*shape):
    torch = _torch()
    return torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel alone
# ---------------------------------------------------------------------------------------------------------------------------------------
def _pool_case(H, Pv, B, seed=0):
    """Inputs on rows_ref's grid (sums exact in float32 in any order); patches 0, 1 and the last one of every document have a mean 50 times
    their deviation."""
    rng = np.random.default_rng([seed, H, Pv, B])
    tab = lambda *shape: R.on_grid(0.02 * rng.standard_normal(shape))
    vis_raw = R.on_grid(0.05 * rng.standard_normal((B, Pv - 1, H)))
    large = sorted({0, min(1, Pv - 2), Pv - 2})
    vis_raw[:, large] = R.on_grid(2.0 + 0.04 * rng.standard_normal((B, len(large), H)))
    g, b = (1 + .1 * rng.standard_normal(H)).astype(np.float32), (.05 * rng.standard_normal(H)).astype(np.float32)
    return dict(vis_raw=vis_raw, cls_token=tab(H), pos_embed=tab(Pv, H), g=g, b=b)


def _pool_refs(c):
    """(float64 pooled (B,H), the same in torch float32 on the CPU)."""
    torch = _torch()
    B, H = c["vis_raw"].shape[0], c["vis_raw"].shape[2]
    v = np.concatenate([np.broadcast_to(c["cls_token"].astype(np.float64), (B, 1, H)), c["vis_raw"].astype(np.float64)], 1) + c["pos_embed"].astype(np.float64)
    ref = R.layer_norm(v, c["g"], c["b"], R.VIS_EPS).mean(1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    v32 = torch.cat([t(c["cls_token"]).expand(B, 1, H), t(c["vis_raw"])], 1) + t(c["pos_embed"])
    y32 = R._torch_ln(v32, c["g"], c["b"], R.VIS_EPS).mean(1).numpy()
    assert y32.dtype == np.float32
    return ref, y32


def _vision_pool(pkg, vis_raw, cls_token, pos_embed, g, b, B, Pv, H, eps=R.VIS_EPS):
    """One ee_debug_vision_pool call on device tensors: the pooled words (B,H), the guards behind both buffers checked."""
    torch = _torch()
    nch = (Pv + 31) // 32
    part, pooled = _sent(B * nch + GUARD, H), _sent(B + GUARD, H)
    pkg.capi.check(pkg.capi.load().ee_debug_vision_pool(_ptr(vis_raw), _ptr(cls_token), _ptr(pos_embed), _ptr(g), _ptr(b), eps, B, Pv, H,
                                                       _ptr(part), _ptr(pooled), _stream()), None, "ee_debug_vision_pool")
    torch.cuda.synchronize()
    assert torch.equal(part[B * nch:], torch.full_like(part[B * nch:], SENTINEL)), "a write behind the partial sums"
    assert torch.equal(pooled[B:], torch.full_like(pooled[B:], SENTINEL)), "a write behind the pooled rows"
    assert not torch.equal(part[:B * nch], torch.full_like(part[:B * nch], SENTINEL))
    return pooled[:B]


@pytest.mark.parametrize("Pv", [5, 33, 65, 197])
@pytest.mark.parametrize("H", [64, 256, 320, 512, 640, 768, 896, 1024])
def test_vision_pool_alone_against_float64(pkg, H, Pv):
    """Every NV (1 .. 4), FULL (768, 1024) and not; one chunk (5), a last chunk of one row (33, 65) or five rows (197); B = 1 and 3."""
    torch = _torch()
    for B in (1, 3):
        c = _pool_case(H, Pv, B)
        ref, y32 = _pool_refs(c)
        dev = {k: _dev(v, torch.float32) for k, v in c.items()}
        got = _f32(_vision_pool(pkg, dev["vis_raw"], dev["cls_token"], dev["pos_embed"], dev["g"], dev["b"], B, Pv, H))
        err, err32 = R.per_row_max(got - ref), R.per_row_max(y32.astype(np.float64) - ref)
        tol = R.tolerance(err32)
        w = int(np.argmax(err / tol))
        report_measured(f"vision_pool[H{H} Pv{Pv} B{B}]", f"max|err| pooled (worst row {w}: err32 {err32[w]:.3e}, err / tol {err[w] / tol[w]:.2f})",
                        float(err.max()))
        assert not np.isnan(got).any() and (err <= tol).all(), (H, Pv, B, err.tolist(), tol.tolist())


def test_the_hook_refuses_what_the_launcher_cannot_take(pkg):
    torch = _torch()
    c = {k: _dev(v, torch.float32) for k, v in _pool_case(64, 5, 1).items()}
    args = (c["vis_raw"], c["cls_token"], c["pos_embed"], c["g"], c["b"])
    for kw, msg in ((dict(H=66), "multiple of 4"), (dict(H=1028), "multiple of 4"), (dict(B=0), "bad shape"), (dict(Pv=1), "bad shape"),
                    (dict(eps=0.0), "eps must be positive")):
        with pytest.raises(pkg.capi.MMEEError, match=msg):
            _vision_pool(pkg, *args, **{**dict(B=1, Pv=5, H=64), **kw})
    with pytest.raises(pkg.capi.MMEEError, match="must not be NULL"):
        _vision_pool(pkg, None, *args[1:], 1, 5, 64)


def _patch_project(pkg, cfg, pix, W, form):
    """vis_raw of the handle's own pixels and weights through ee_debug_patch_project, in the form the handle runs (1: f32, 2: split)."""
    torch = _torch()
    H, P, R_, Cn = cfg.hidden_size, cfg.patch_size, cfg.input_size, cfg.num_channels
    B = pix.shape[0]
    M = B * (R_ // P) ** 2
    out = torch.empty((M, H), dtype=torch.float32, device="cuda")
    a = pkg.capi.DebugPatchProjectArgs()
    hold = [_dev(pix, torch.float32), _dev(np.ascontiguousarray(W["layoutlmv3.patch_embed.proj.weight"].reshape(H, -1)), torch.float32),
            _dev(W["layoutlmv3.patch_embed.proj.bias"], torch.float32)]
    a.pixel_values, a.weight, a.bias = (t.data_ptr() for t in hold)
    a.B, a.C, a.R, a.P, a.H, a.form = B, Cn, R_, P, H, form
    a.out, a.a_split_out = out.data_ptr(), None
    err = C.c_int32(-1)
    a.err_flag_out = C.pointer(err)
    pkg.capi.check(pkg.capi.load().ee_debug_patch_project(C.byref(a), _stream()), None, "ee_debug_patch_project")
    torch.cuda.synchronize()
    assert err.value == 0
    return out


@pytest.mark.parametrize("case,precision", [("tiny_ramp", "fp32"), ("h256_entropy_1layer", "fp32"), ("h256_entropy_1layer", "split")])
def test_the_pooled_row_has_the_bits_of_embedding_inputs(pkg, case, precision):
    torch = _torch()
    kw, ee, _, T = CASES[case]
    cfg = pkg.ModelConfig.tiny(EE_config=dict(ee), **kw)
    W = pkg.synth.make_weights(cfg, seed=71)
    d = pkg.synth.make_documents(cfg, 5, seed=72, text_len=T, min_words=2)
    eng = pkg.EarlyExitEngine(cfg, max_docs=8, max_text_len=T, precision=precision, xprobe=False)
    eng.load_weights(W)
    want = eng.embedding_inputs(d["input_ids"], d["attention_mask"], d["bbox"], d["pixel_values"], kinds=["vision_avg"])["vision_avg"]
    vis_raw = _patch_project(pkg, cfg, d["pixel_values"], W, 2 if precision == "split" else 1)
    f = lambda n: _dev(W[n].reshape(-1, cfg.hidden_size) if W[n].ndim > 1 else W[n], torch.float32)
    Pv = (cfg.input_size // cfg.patch_size) ** 2 + 1
    got = _vision_pool(pkg, vis_raw, f("layoutlmv3.cls_token"), f("layoutlmv3.pos_embed"), f("layoutlmv3.norm.weight"), f("layoutlmv3.norm.bias"),
                       5, Pv, cfg.hidden_size)
    torch.cuda.synchronize()
    assert torch.equal(got, want.view(torch.int32)), "vision_pool + pool_finish is not bit-equal to ee_embedding_inputs' out_vision"
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the handles of parts 2 - 5
# ---------------------------------------------------------------------------------------------------------------------------------------
class World:
    """One configuration: its weights, 12 documents, an engine per setting, and per setting the device's own criteria of a dump-all call
    (computed once, never written to)."""

    def __init__(self, pkg, case):
        self.pkg, self.case = pkg, case
        kw, ee, self.precision, self.T = CASES[case]
        self.cfg = pkg.ModelConfig.tiny(EE_config=dict(ee), **kw)
        self.W = pkg.synth.make_weights(self.cfg, seed=81, head_gain=4.0)
        d = pkg.synth.make_documents(self.cfg, B_DOCS, seed=82, text_len=self.T, min_words=2)
        torch = _torch()
        self.inputs = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in TEXT_KEYS + ("pixel_values",)}
        self._eng, self._crit = {}, {}

    def new_engine(self):
        eng = self.pkg.EarlyExitEngine(self.cfg, max_docs=B_DOCS, max_text_len=self.T, precision=self.precision, xprobe=False)
        eng.load_weights(self.W)
        return eng

    def engine(self, setting="plain"):
        if setting not in self._eng:
            eng = self.new_engine()
            E1 = eng.E + 1
            if setting == "margin":
                eng.set_criterion("margin")
            elif setting == "patient_confident":
                eng.set_patience([1] + [2] * (E1 - 1))
                eng.set_exit_rule("patient_confident")
            elif setting == "ensemble":
                eng.set_ensemble((np.tril(np.ones((E1, E1))) / np.arange(1, E1 + 1)[:, None], None))      # w = the running mean
            self._eng[setting] = eng
        return self._eng[setting]

    def temperatures(self, setting):
        return np.linspace(0.7, 1.6, self.engine(setting).E + 1) if setting == "temperatures" else None

    def text(self):
        return {k: self.inputs[k] for k in TEXT_KEYS}

    def thresholds(self, setting, n_leave):
        """thresholds[0]: exactly n_leave documents leave at exit 0; the later exits: the middle gap of the dump's criteria."""
        eng = self.engine(setting)
        if setting not in self._crit:
            out = eng.forward(**self.inputs, dump_all=True, want_all=True, temperatures=self.temperatures(setting))
            crit = _np(out.all_crit).astype(np.float64)
            assert np.isfinite(crit).all()
            self._crit[setting] = crit
        crit = self._crit[setting]
        sign = -1 if str(eng.exit_config.inference_strategy.value) == "entropy" else +1
        srt = np.sort(crit, axis=1)
        thr = 0.5 * (srt[:, B_DOCS // 2 - 1] + srt[:, B_DOCS // 2])
        thr[0] = VR.threshold_for(crit[0], n_leave, sign)      # asserts the gap of more than 1e-9
        assert (VR.exit0_leaves(crit[0], thr[0], sign).sum()) == n_leave
        return thr


@pytest.fixture(scope="module")
def worlds(pkg):
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = World(pkg, case)
        return cache[case]
    yield get
    for w in cache.values():
        for eng in w._eng.values():
            eng.close()


def _forward(w, setting, thr, xprobe=False, **kw):
    return w.engine(setting).forward(**w.inputs, thresholds=thr, temperatures=w.temperatures(setting), xprobe=xprobe, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. phase 1 against the forward
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xprobe", [False, True], ids=["kv_probe", "xprobe"])
@pytest.mark.parametrize("n_leave", LEAVE)
@pytest.mark.parametrize("case", list(CASES))
def test_phase_one_against_the_forward(worlds, case, n_leave, xprobe):
    torch = _torch()
    w = worlds(case)
    eng = w.engine()
    thr = w.thresholds("plain", n_leave)
    ref = _forward(w, "plain", thr, xprobe)
    ex = _np(ref.exit_layer)
    assert (ex == 0).sum() == n_leave
    out = (_sent(B_DOCS, eng.K).view(torch.float32), _sent(B_DOCS), _sent(B_DOCS).view(torch.float32))
    ph = eng.forward_vision(w.inputs["pixel_values"], thresholds=thr, out=out)
    torch.cuda.synchronize()
    left = ex == 0
    for name, got, want in (("logits", out[0], ref.logits), ("exit_layer", out[1], ref.exit_layer), ("confidence", out[2], ref.confidence)):
        g, r = _bits(_np(got)), _bits(_np(want))
        assert np.array_equal(g[left], r[left]), (name, "a leaver's bits differ from the one-call forward's")
        assert (g[~left] == SENTINEL).all(), (name, "a slot of a document that stays was written")
    m = int(_np(ph.count)[0])
    assert m == B_DOCS - n_leave and np.array_equal(_np(ph.survivors)[:m], np.nonzero(ex > 0)[0].astype(np.int32))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. the whole call
# ---------------------------------------------------------------------------------------------------------------------------------------
class TextSource:
    """The callable route's f(slots) -> dict: the survivors' rows of the full arrays, and a record of the calls."""

    def __init__(self, w, extra_rows=0):
        self.w, self.calls, self.extra = w, [], extra_rows
        self.torch = _torch()

    def __call__(self, slots):
        self.calls.append(np.array(slots))
        idx = self.torch.from_numpy(np.concatenate([slots, slots[:self.extra]]).astype(np.int64)).cuda()
        return {k: v.index_select(0, idx) for k, v in self.w.text().items()}


def _same_as_forward(got, ref, n_leave, tag):
    ex = _np(ref.exit_layer)
    for f in ("logits", "exit_layer", "confidence"):
        g, r = _np(getattr(got, f)), _np(getattr(ref, f))
        assert g.dtype == r.dtype and np.array_equal(_bits(g), _bits(r)), (tag, f)
    assert np.array_equal(_np(got.stage), (ex > 0).astype(np.int32)) and got.stage.dtype == _torch().int32, tag
    assert got.text_docs == B_DOCS - n_leave == int((ex > 0).sum()), tag


def _whole_call(w, setting, n_leave, xprobe):
    eng = w.engine(setting)
    thr, tm = w.thresholds(setting, n_leave), w.temperatures(setting)
    ref = _forward(w, setting, thr, xprobe)
    assert (_np(ref.exit_layer) == 0).sum() == n_leave
    px = w.inputs["pixel_values"]
    got = eng.forward_vision_first(px, w.text(), thresholds=thr, temperatures=tm, xprobe=xprobe)
    _same_as_forward(got, ref, n_leave, (setting, n_leave, "dict"))
    src = TextSource(w)
    got = eng.forward_vision_first(px, src, thresholds=thr, temperatures=tm, xprobe=xprobe)
    _same_as_forward(got, ref, n_leave, (setting, n_leave, "callable"))
    if n_leave == B_DOCS:
        assert src.calls == [], "the text source was asked although nobody survived"
    else:
        assert len(src.calls) == 1 and np.array_equal(src.calls[0], np.nonzero(_np(ref.exit_layer) > 0)[0]), "asked for other than the survivors, once"


@pytest.mark.parametrize("xprobe", [False, True], ids=["kv_probe", "xprobe"])
@pytest.mark.parametrize("n_leave", LEAVE)
@pytest.mark.parametrize("case", list(CASES))
def test_the_whole_call_is_the_forward_bit_for_bit(worlds, case, n_leave, xprobe):
    _whole_call(worlds(case), "plain", n_leave, xprobe)


@pytest.mark.parametrize("n_leave", LEAVE)
@pytest.mark.parametrize("setting", ["margin", "patient_confident", "ensemble", "temperatures"])
def test_the_whole_call_under_other_decisions(worlds, setting, n_leave):
    _whole_call(worlds("tiny_ramp"), setting, n_leave, False)


def test_wrong_row_counts_raise(worlds):
    w = worlds("tiny_ramp")
    eng, px = w.engine(), w.inputs["pixel_values"]
    thr = w.thresholds("plain", 5)
    with pytest.raises(ValueError, match="rows for 7 surviving documents"):
        eng.forward_vision_first(px, TextSource(w, extra_rows=1), thresholds=thr)
    short = {k: v[:B_DOCS - 1] for k, v in w.text().items()}
    with pytest.raises(ValueError, match=f"{B_DOCS - 1} rows for a call of {B_DOCS} documents"):
        eng.forward_vision_first(px, short, thresholds=thr)


@pytest.mark.parametrize("n_leave", LEAVE)
def test_low_latency_is_the_hand_composition(worlds, n_leave):
    """Phase 1, then forward(low_latency=True) on the index_selected survivors, merged by hand: bit for bit."""
    torch = _torch()
    w = worlds("h256_entropy_1layer")
    eng = w.engine()
    thr = w.thresholds("plain", n_leave)
    got = eng.forward_vision_first(w.inputs["pixel_values"], w.text(), thresholds=thr, low_latency=True)
    ph = eng.forward_vision(w.inputs["pixel_values"], thresholds=thr)
    torch.cuda.synchronize()
    m = int(_np(ph.count)[0])
    assert m == B_DOCS - n_leave
    want = [_np(ph.output.logits).copy(), _np(ph.output.exit_layer).copy(), _np(ph.output.confidence).copy()]
    stage = np.zeros(B_DOCS, np.int32)
    if m:
        idx = ph.survivors[:m].long()
        sub = eng.forward(**{k: v.index_select(0, idx) for k, v in w.inputs.items()}, thresholds=thr, low_latency=True)
        s = _np(idx)
        want[0][s], want[1][s], want[2][s], stage[s] = _np(sub.logits), _np(sub.exit_layer), _np(sub.confidence), 1
    for f, r in zip(("logits", "exit_layer", "confidence"), want):
        assert np.array_equal(_bits(_np(getattr(got, f))), _bits(r)), f
    assert np.array_equal(_np(got.stage), stage) and got.text_docs == m


def test_the_model_wrapper_takes_the_reference_style_inputs(pkg, worlds):
    w = worlds("tiny_ramp")
    model = pkg.LayoutLMv3EEForSequenceClassification(w.cfg, w.W, max_docs=B_DOCS, max_text_len=w.T, precision="fp32")
    thr = w.thresholds("plain", 5)
    ref = model.early_exit(**w.inputs, thresholds=thr)
    got = model.early_exit_vision_first(**w.inputs, thresholds=thr)
    for f in ("logits", "exit_layer", "confidence"):
        assert np.array_equal(_bits(_np(getattr(got, f))), _bits(_np(getattr(ref, f)))), f
    src = TextSource(w)
    got = model.early_exit_vision_first(pixel_values=w.inputs["pixel_values"], text=src, thresholds=thr)
    assert np.array_equal(_np(got.exit_layer), _np(ref.exit_layer)) and len(src.calls) == 1
    with pytest.raises(ValueError, match="pass one"):
        model.early_exit_vision_first(**w.inputs, text=src, thresholds=thr)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. nothing else moved
# ---------------------------------------------------------------------------------------------------------------------------------------
def _launches(eng, **kw):
    eng.profile(True)
    out = eng.forward(**kw)
    prof = {k: v["launches"] for k, v in eng.profile_read().items()}
    eng.profile(False)
    return out, prof


def test_a_handle_that_used_the_feature_is_one_that_never_did(worlds):
    w = worlds("tiny_ramp")
    thr = w.thresholds("plain", 5)
    used, fresh = w.new_engine(), w.new_engine()
    used.forward(**w.inputs, thresholds=thr)
    before = used.stage_counts()
    used.forward_vision(w.inputs["pixel_values"], thresholds=w.thresholds("plain", 12))
    assert used.stage_counts() == before, "forward_vision moved the stage counts of the last forward"
    used.forward_vision_first(w.inputs["pixel_values"], w.text(), thresholds=w.thresholds("plain", 0))
    for kw in (dict(thresholds=thr), dict(dump_all=True, want_all=True)):
        a, pa = _launches(used, **w.inputs, **kw)
        b, pb = _launches(fresh, **w.inputs, **kw)
        assert pa == pb, (kw.keys(), "launch counts per role differ")
        for f in ("logits", "exit_layer", "confidence") + (("all_logits", "all_crit") if "dump_all" in kw else ()):
            assert np.array_equal(_bits(_np(getattr(a, f))), _bits(_np(getattr(b, f)))), f
        assert used.stage_counts() == fresh.stage_counts()
    used.close()
    fresh.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def _raw(pkg, eng, px, B, flags=0, thr=True, **null):
    """ee_forward_vision itself; `null` names the pointers handed in as NULL.  The outputs are sentinels and must stay so."""
    torch = _torch()
    E1 = eng.E + 1
    bufs = dict(pixel_values=px, out_logits=_sent(max(B, 1), eng.K), out_exit=_sent(max(B, 1)), out_conf=_sent(max(B, 1)),
                survivors=_sent(max(B, 1)), count=_sent(1))
    p = {k: (None if null.get(k) else _ptr(v)) for k, v in bufs.items()}
    thr_c = (C.c_double * E1)(*([0.5] * E1)) if thr else None
    rc = eng.lib.ee_forward_vision(eng._h, p["pixel_values"], B, thr_c, None, flags, p["out_logits"], p["out_exit"], p["out_conf"], p["survivors"],
                                   p["count"], _stream())
    torch.cuda.synchronize()
    for k in ("out_logits", "out_exit", "out_conf", "survivors", "count"):
        assert torch.equal(bufs[k], torch.full_like(bufs[k], SENTINEL)), (k, "written by a refused call")
    pkg.capi.check(rc, eng._h, "ee_forward_vision")


def test_the_library_refuses_with_a_message_and_writes_nothing(pkg, worlds):
    torch = _torch()
    w = worlds("tiny_ramp")
    eng, px = w.new_engine(), w.inputs["pixel_values"]
    E = pkg.capi.MMEEError
    for null in ("pixel_values", "out_exit", "survivors", "count"):
        with pytest.raises(E, match="are required"):
            _raw(pkg, eng, px, B_DOCS, **{null: True})
    for B in (0, B_DOCS + 1):
        with pytest.raises(E, match="outside \\[1, max_docs"):
            _raw(pkg, eng, px, B)
    for flag in (pkg.capi.FLAG_NO_EXIT, pkg.capi.FLAG_STREAM_RESULTS, pkg.capi.FLAG_DENSE_ROWS):
        with pytest.raises(E, match="do not go with a vision-first call"):
            _raw(pkg, eng, px, B_DOCS, flags=flag)
    with pytest.raises(E, match="thresholds required"):
        _raw(pkg, eng, px, B_DOCS, thr=False)
    eng.set_quotas([1] * eng.E)
    with pytest.raises(E, match="quotas are set"):
        _raw(pkg, eng, px, B_DOCS)
    eng.set_quotas(None)
    eng.set_audit(0.5, seed=3)
    with pytest.raises(E, match="an audit is set"):
        _raw(pkg, eng, px, B_DOCS)
    path = np.linspace(0.99, 0.5, 4)[:, None] * np.ones((1, eng.E + 1))
    eng.set_controller(path, alpha=0.1, gamma=0.5)
    with pytest.raises(E, match="a controller is set"):
        _raw(pkg, eng, px, B_DOCS)
    eng.set_controller(None)
    eng.set_audit(None)
    mask = torch.ones((w.cfg.num_hidden_layers, w.cfg.num_attention_heads), dtype=torch.float32, device="cuda")
    pkg.capi.check(eng.lib.ee_set_head_mask(eng._h, _ptr(mask)), eng._h, "ee_set_head_mask")
    with pytest.raises(E, match="one-shot side input / output is armed"):
        _raw(pkg, eng, px, B_DOCS)
    with pytest.raises(E, match="dump-all mode"):                          # it stayed armed: the next forward consumes (and here refuses) it
        eng.forward(**w.inputs, thresholds=0.5)
    eng.forward_vision(px, thresholds=0.5)                                 # and the handle is in order again
    torch.cuda.synchronize()
    eng.close()


def test_handles_without_the_exit_are_refused(pkg):
    torch = _torch()
    cfg = pkg.ModelConfig.tiny(EE_config=dict(TINY_CASES["tiny_gate"]))
    eng = pkg.EarlyExitEngine(cfg, max_docs=4, max_text_len=40, precision="fp32")
    eng.load_weights(pkg.synth.make_weights(cfg, seed=5))
    px = torch.zeros((2, cfg.num_channels, cfg.input_size, cfg.input_size), device="cuda")
    with pytest.raises(pkg.capi.MMEEError, match="no vision_avg exit"):
        eng.forward_vision(px, thresholds=0.5)
    eng.close()
    dcfg = pkg.ModelConfig.dit_tiny(EE_config=dict(DIT_EE))
    dit = pkg.EarlyExitEngine(dcfg, max_docs=4)
    dit.load_weights(pkg.synth.make_weights_beit(dcfg, seed=6))
    px = torch.zeros((2, dcfg.num_channels, dcfg.input_size, dcfg.input_size), device="cuda")
    with pytest.raises(pkg.capi.MMEEError, match="MMEE_ARCH_BEIT"):
        dit.forward_vision(px, thresholds=0.5)
    dit.close()


def test_the_python_layer_refuses_what_is_not_built(pkg, worlds):
    w = worlds("tiny_ramp")
    eng, px = w.engine(), w.inputs["pixel_values"]
    for k in ("want_all", "want_head", "dump_all"):
        with pytest.raises(ValueError, match="belongs to a dump-all forward"):
            eng.forward_vision_first(px, w.text(), thresholds=0.5, **{k: True})
    for k in ("_stream", "_capture"):
        with pytest.raises(ValueError, match="result stream or a captured graph is not built"):
            eng.forward_vision_first(px, w.text(), thresholds=0.5, **{k: True})
    with pytest.raises(ValueError, match="a dict of the caller's full arrays or a callable"):
        eng.forward_vision_first(px, None, thresholds=0.5)
    with pytest.raises(NotImplementedError, match="no vision-first call"):
        pkg.MicroBatchedEngine.forward_vision_first(None, px, w.text())
    with pytest.raises(NotImplementedError, match="inside a cascade is not built"):
        pkg.CascadeEngine.forward_vision_first(None, px, w.text())
