"""Audited exits (include/mmee.h, behind the cascades) on the MI355X against the numpy restatement of tests/audit_ref.py: the AUDIT form of the
decide kernels alone through ee_debug_exit_audit at the wave and decide-chunk edges; the forward on ``tiny_ramp``, the ``h256`` ramp and gate
configurations, every combination the header claims (patience, the two exit rules, learning-to-exit, the gate criterion, an ensemble, the
low-latency mode, the tiny DiT, a MicroBatchedEngine); the reading side (``audit.sample`` / ``audit.consistency``); and the refusals.

The device's exp may differ from numpy's in the last place of float64.  So the launch's criteria are compared with numpy's within 1e-12
relative plus the rounding to the float32 they are stored as, and every threshold sits at the midpoint of two adjacent sorted criteria more
than 1e-9 apart with no criterion within 1e-12 of it (asserted on the CPU): what is DECIDED cannot differ, and is compared exactly.  The
forward is compared with the same handle's own unaudited and dump-all calls, bit for bit.

The dumped-array tools score against references and refuse a call without them (tests/test_host_search.py, test_host_exit_metrics.py,
test_host_threshold_refine.py pin that), so the label-free runs here hand them ``AuditSample.references()``, the final exit's predictions."""
import ctypes as C

import numpy as np
import pytest

from . import audit_ref as A
from . import csf_ref
from . import ensemble_ref as ER
from . import exit_stage_ref as R
from .conftest import DIT_EE, H256_KW, MATRIX_CASES, TINY_CASES
from .hook_util import SENTINEL, _stream, _torch

pytestmark = pytest.mark.gpu

GUARD = 4
STAGE_N = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
KS = (2, 16, 17)
TEMPS = (1.0, 3.0, 0.5)
FORMS = ("max_confidence", "entropy", "margin", "gate", "patience", "streak")          # four criteria of the threshold kernel, two stateful kernels
KERNEL = {"patience": (R.PATIENCE, R.PLAIN), "streak": (R.THRESHOLD, R.STREAK)}
CRIT_CODE = dict(R.CRIT_CODE, gate=4)
MIN_GAP, MIN_DIST = 1e-9, 1e-12
PATIENCE_T = 2
SENT32 = np.int32(SENTINEL)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the launch alone
# ---------------------------------------------------------------------------------------------------------------------------------------
def _i32(a, pad=1):
    a = np.asarray(a, np.int64).reshape(-1)
    return _torch().from_numpy(np.concatenate([a, np.full(pad, SENTINEL, np.int64)]).astype(np.int32)).cuda()


def _sent(words):
    torch = _torch()
    return torch.full((int(words) + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")


def _counts(stage):
    sq = stage["sum_len_sq"]
    return [stage["n"], stage["n_rows"], sq & 0xFFFFFFFF, sq >> 32]


def gate_score(h):
    h = np.asarray(h, np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(h[:, 0] - h[:, 1]))


def _gap_threshold(crit, position=0.5):
    """The midpoint of a gap of more than MIN_GAP between adjacent sorted criteria, nearest the median; every criterion more than MIN_DIST away."""
    v = np.sort(crit)
    if len(v) < 2:
        return float(v[0] - 0.125)
    gaps = np.diff(v)
    ok = np.nonzero(gaps > MIN_GAP)[0]
    assert ok.size, "no gap wider than 1e-9"
    i = ok[np.abs(ok + 1 - position * len(v)).argmin()]
    thr = 0.5 * (v[i] + v[i + 1])
    assert np.abs(crit - thr).min() > MIN_DIST
    return float(thr)


def _hook_case(n, form, K, temp, exit_index, seed=0):
    """One stage, its logits and state, this exit's decision by exit_stage_ref (the gate criterion: by its definition, here) and the audit's
    inputs: about 40 % of the slots selected, and at a later exit a mixed `delivered` among them."""
    rng = np.random.default_rng(9000 + 13 * n + 101 * FORMS.index(form) + K + seed)
    B = n + 37
    stage = R.make_stage(n, B, seed=n + K + seed)
    o = stage["doc_orig"]
    z = (rng.standard_normal((n, K)) * 2.0 * temp).astype(np.float32)
    head = rng.uniform(-3.0, 3.0, (n, 2)).astype(np.float32) if form == "gate" else None
    x = csf_ref.scaled(z[None], [temp])[0]
    s32 = x.astype(np.float32)
    criterion = form if form in CRIT_CODE else "max_confidence"
    mode, rule = KERNEL.get(form, (R.THRESHOLD, R.PLAIN))
    prev, run = np.full(B, R.DIRTY, np.int64), np.full(B, R.DIRTY, np.int64)
    if exit_index > 0:                                                           # state as earlier exits leave it: half the documents agree / hold a streak
        am = R.argmax_first(s32)
        agree = rng.random(n) < 0.5
        prev[o] = np.where(agree, am, (am + 1) % K)
        run[o] = rng.integers(0, 3, n)
    with np.errstate(invalid="ignore", over="ignore"):
        crit = gate_score(head) if form == "gate" else csf_ref.csf(x, criterion)
    thr = 0.5 if form == "patience" else _gap_threshold(crit)
    if form == "gate":
        leave, state = crit > thr, (prev, run)
    else:
        r = R.decide_ref(stage, z, mode=mode, rule=rule, criterion=criterion, thr=thr, temp=temp, patience=PATIENCE_T, exit_index=exit_index, B=B,
                         state=(prev, run))
        leave, state = r["leave"], r["state"]
        assert np.array_equal(r["scaled32"].view(np.int32), s32.view(np.int32))
    cut, aseed, base = A.cut_of(0.4), 11 + seed, 5
    sel = A.selected(cut, aseed, o + base)
    delivered = np.full(B, SENTINEL, np.int64)                                   # exit 0: must be overwritten for the stage's slots, never read
    if exit_index > 0:
        delivered[o] = sel & (rng.random(n) < 0.5)
    return dict(n=n, B=B, K=K, form=form, criterion=criterion, mode=mode, rule=rule, temp=temp, thr=thr, stage=stage, z=z, head=head, s32=s32,
                crit=crit, leave=leave, state_in=(prev, run), state_out=state, cut=cut, seed=aseed, slot_base=base, delivered=delivered,
                exit_index=exit_index)


def _call(pkg, c, by_pointer=0, is_final=0, null=(), **over):
    """One ee_debug_exit_audit call; `over`: fields of the argument block set last, as they are.  Returns every buffer, raw (numpy)."""
    torch = _torch()
    st, n, B, K, e = c["stage"], c["n"], c["B"], c["K"], c["exit_index"]
    keep = dict(z=torch.from_numpy(np.ascontiguousarray(c["z"])).cuda(), head=None if c["head"] is None else torch.from_numpy(np.ascontiguousarray(c["head"])).cuda(),
                counts=_i32(_counts(st), 0), doc_orig=_i32(st["doc_orig"]), doc_off=_i32(st["doc_off"]), x_phys=_i32(st["x_phys"]))
    b = dict(n_counts=_sent(4), n_doc_orig=_sent(n), n_doc_off=_sent(n + 1), n_x_src=_sent(n), n_meta_src=_sent(n), out_logits=_sent(B * K), out_exit=_sent(B),
             out_conf=_sent(B), out_all_logits=_sent((e + 1) * B * K), out_all_crit=_sent((e + 1) * B), out_head_logits=_sent((e + 1) * B * 2),
             out_head_crit=_sent((e + 1) * B))
    b["prev"], b["run"], b["delivered"] = _i32(c["state_in"][0], GUARD), _i32(c["state_in"][1], GUARD), _i32(c["delivered"], GUARD)
    a = pkg.capi.DebugExitAuditArgs()
    d = a.decide
    for k, v in dict(mode=c["mode"], rule=c["rule"], criterion=CRIT_CODE[c["criterion"]], K=K, Kh=2, thr=float(c["thr"]), temp=float(c["temp"]),
                     patience=PATIENCE_T, by_pointer=by_pointer, exit_index=e, is_final=is_final, no_exit=0, B=B).items():
        setattr(d, k, v)
    d.pol_logits, d.head_logits = keep["z"].data_ptr(), None if keep["head"] is None else keep["head"].data_ptr()
    for k in ("counts", "doc_orig", "doc_off", "x_phys"):
        setattr(d, k, keep[k].data_ptr())
    for k, t in b.items():
        if k != "delivered":
            setattr(d, k, None if k in null else t.data_ptr())
    a.cut, a.seed, a.slot_base, a.delivered = c["cut"], c["seed"], c["slot_base"], b["delivered"].data_ptr()
    for k, v in over.items():
        setattr(a if k in ("cut", "seed", "slot_base", "delivered") else d, k, v)
    pkg.capi.check(pkg.capi.load().ee_debug_exit_audit(C.byref(a), _stream()), None, "ee_debug_exit_audit")
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in b.items()}


def _rows(words, rows, width):
    idx = (np.asarray(rows, np.int64)[:, None] * width + np.arange(width)[None]).reshape(-1)
    return idx, words[idx]


def _only(words, idx, what):
    rest = words.copy()
    rest[idx] = SENTINEL
    assert (rest == SENTINEL).all(), (what, "a write outside the documents' slots")


def _close_f32(got_words, want64, tag):
    """Stored float32 criteria: the rounding of a float64 within 1e-12 relative of numpy's."""
    g = got_words.view(np.float32).astype(np.float64)
    assert (np.abs(g - want64) <= (2.0 ** -24 + 1e-12) * np.maximum(np.abs(want64), 1e-30)).all(), tag


def _check(tag, c, b, is_final=False):
    st, n, B, K, e = c["stage"], c["n"], c["B"], c["K"], c["exit_index"]
    o = st["doc_orig"]
    leave = np.ones(n, bool) if is_final else c["leave"]
    r = A.audit_decide(st, leave, c["delivered"], cut=c["cut"], seed=c["seed"], slot_base=c["slot_base"], exit_index=e, is_final=is_final)
    nx, w = r["next"], r["writes"]
    got_counts = [int(x) & 0xFFFFFFFF for x in b["n_counts"]]
    assert got_counts == _counts(nx) + [SENTINEL] * GUARD, (tag, got_counts, _counts(nx))
    for k, extra in (("n_doc_orig", 0), ("n_doc_off", 1), ("n_x_src", 0), ("n_meta_src", 0)):
        want = nx[k][:n + extra + GUARD]
        assert np.array_equal(b[k], want), (tag, k, np.nonzero(b[k] != want)[0][:6].tolist())
    # delivered: the restatement's array, the guard behind it and the slots outside the stage intact
    assert np.array_equal(b["delivered"][:B], r["delivered"].astype(np.int32)) and (b["delivered"][B:] == SENT32).all(), (tag, "delivered")
    # the results: written for `writes` only -- a delivered document's slots still hold the sentinel
    idx, got = _rows(b["out_exit"], o[w], 1)
    assert (got == e).all(), tag
    _only(b["out_exit"], idx, (tag, "out_exit"))
    idx, got = _rows(b["out_logits"], o[w], K)
    assert np.array_equal(got, c["s32"][w].view(np.int32).reshape(-1)), (tag, "out_logits")
    _only(b["out_logits"], idx, (tag, "out_logits"))
    idx, got = _rows(b["out_conf"], o[w], 1)
    _close_f32(got, c["crit"][w], (tag, "out_conf"))
    _only(b["out_conf"], idx, (tag, "out_conf"))
    # the dump rows: every document of the stage, delivered or not
    idx, got = _rows(b["out_all_logits"], e * B + o, K)
    assert np.array_equal(got, c["s32"].view(np.int32).reshape(-1)), (tag, "out_all_logits")
    _only(b["out_all_logits"], idx, (tag, "out_all_logits"))
    idx, got = _rows(b["out_all_crit"], e * B + o, 1)
    _close_f32(got, c["crit"], (tag, "out_all_crit"))
    _only(b["out_all_crit"], idx, (tag, "out_all_crit"))
    if c["head"] is None:
        assert (b["out_head_logits"] == SENTINEL).all() and (b["out_head_crit"] == SENTINEL).all(), tag
    else:
        idx, got = _rows(b["out_head_logits"], e * B + o, 2)
        assert np.array_equal(got, _bits(c["head"]).reshape(-1)), (tag, "out_head_logits")
        _only(b["out_head_logits"], idx, (tag, "out_head_logits"))
        idx, got = _rows(b["out_head_crit"], e * B + o, 1)
        assert (np.abs(got.view(np.float32).astype(np.float64) - gate_score(c["head"])) <= 1e-6).all(), (tag, "out_head_crit")
        _only(b["out_head_crit"], idx, (tag, "out_head_crit"))
    # the per-document state: updated for every document of the stage, delivered ones included; untouched where the kernel keeps none
    stateful = c["form"] in KERNEL
    for k, before, after in (("prev", c["state_in"][0], c["state_out"][0]), ("run", c["state_in"][1], c["state_out"][1])):
        want = (after if stateful else before).astype(np.int64)
        if c["form"] == "streak" and k == "prev":
            want = before.astype(np.int64)
        assert np.array_equal(b[k][:B].astype(np.int64), want.astype(np.int32).astype(np.int64)) and (b[k][B:] == SENT32).all(), (tag, k)
    return r


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", STAGE_N)
def test_launch_alone_delivers_keeps_and_marks_as_the_restatement(pkg, n, form):
    """Exit 0 on a `delivered` full of sentinels (written, not read) and exit 2 on a mixed one; K, the temperature and by-value / by-pointer
    cycled against the sizes and forms so that the matrix meets every value of each."""
    ni, fi = STAGE_N.index(n), FORMS.index(form)
    K, temp = KS[(ni + fi) % 3], TEMPS[(ni + 2 * fi + ni // 3) % 3]
    for exit_index in (0, 2):
        c = _hook_case(n, form, K, temp, exit_index)
        by_pointer = (ni + fi + exit_index // 2) % 2
        tag = f"audit.launch[n={n} {form} K={K} T={temp} exit={exit_index} ptr={by_pointer}]"
        r = _check(tag, c, _call(pkg, c, by_pointer=by_pointer), False)
        o = c["stage"]["doc_orig"]
        if exit_index == 0:
            assert set(np.unique(r["delivered"][o])) <= {0, 1}
        elif n >= 63:                                                            # the case is a case: shadows, new deliveries, plain leavers, stayers
            was = c["delivered"][o] != 0
            assert was.any() and (r["writes"] & r["keep"]).any() and (r["writes"] & ~r["keep"]).any() and (~r["writes"] & r["keep"] & ~was).any(), tag
            assert (c["leave"] & was).any() and not r["writes"][was].any() and r["keep"][was].all(), tag


@pytest.mark.parametrize("n", [65, 1025])
def test_launch_at_the_final_exit_writes_for_the_undelivered_only_and_keeps_nobody(pkg, n):
    for form in ("max_confidence", "patience"):
        for exit_index in (0, 2):
            c = _hook_case(n, form, 16, 3.0, exit_index, seed=1)
            r = _check(f"audit.final[n={n} {form} exit={exit_index}]", c, _call(pkg, c, is_final=1), True)
            was = np.zeros(n, bool) if exit_index == 0 else c["delivered"][c["stage"]["doc_orig"]] != 0
            assert not r["keep"].any() and np.array_equal(r["writes"], ~was) and r["next"]["n"] == 0
            assert exit_index == 0 or was.any()


def test_launch_fraction_one_keeps_everybody_and_the_refusals(pkg):
    c = dict(_hook_case(257, "margin", 17, 0.5, 0), cut=1 << 32)
    r = _check("audit.all", c, _call(pkg, c))
    assert r["keep"].all() and np.array_equal(r["writes"], c["leave"]) and c["leave"].any() and not c["leave"].all()
    null = ("out_logits", "out_conf", "out_all_logits", "out_all_crit", "out_head_logits", "out_head_crit")
    b = _call(pkg, c, null=null)
    for k in null:
        assert (b[k] == SENTINEL).all(), k
    assert np.array_equal(b["delivered"][:c["B"]], r["delivered"].astype(np.int32))
    for over, match in ((dict(cut=0), r"outside \[1, 2\^32\]"), (dict(cut=(1 << 32) + 1), r"outside \[1, 2\^32\]"), (dict(slot_base=-1), "negative"),
                        (dict(delivered=None), "delivered must not be NULL"), (dict(no_exit=1), "no_exit must be 0"), (dict(mode=1, rule=1), "no kernel for mode"),
                        (dict(criterion=2), "criterion"), (dict(B=100), "n_docs")):
        with pytest.raises(pkg.capi.MMEEError, match=match):
            _call(pkg, c, **over)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. / 3. the forward
# ---------------------------------------------------------------------------------------------------------------------------------------
H256_RAMP = dict(MATRIX_CASES["h256_entropy_1layer"][1], inference_strategy="max_confidence")
LTE_EE = dict(exits=[1, 2], encoder_layer_strategy="ramp", use_lte=True)
# name -> (shape, EE_config, precision, documents, text length, seed of the weights and of the documents, exit heads share the classifier).
# Half of an exit's documents leave at its median, so with independent random heads nobody is left for the final exit after seven of them.
# The ramp cases take the classifier's parameters for every encoder exit head (a model whose exits share one classifier, as in PABEE and in
# tests/test_gpu_patience.py): a page that is hard at one exit is then hard at the next.  The seeds were chosen on the CPU oracle's table for
# the three properties test 2 asserts on the device's.
CASES = {
    "tiny_ramp": ("tiny", dict(TINY_CASES["tiny_ramp"]), "fp32", 64, 16, 21, True),
    "h256_ramp": ("h256", H256_RAMP, "split", 24, 48, 61, True),
    "h256_gate": ("h256", dict(MATRIX_CASES["h256_gate"][1]), "split", 24, 48, 21, False),
    "h256_lte": ("h256", LTE_EE, "split", 24, 48, 91, False),
    "dit_tiny": ("dit", dict(DIT_EE), None, 24, 0, 91, False),
}
FIELDS = ("logits", "exit_layer", "confidence")
DUMPS = ("all_logits", "all_crit", "head_logits", "head_crit")
FRACTION, SEED = 0.25, 1


def _shared_heads(W):
    W = dict(W)
    for k in list(W):
        if ".early_exits." in k:
            src = "classifier" + k[k.index(".", k.index(".early_exits.") + len(".early_exits.")):]
            if src in W and W[src].shape == W[k].shape:
                W[k] = W[src].copy()
    return W


class Case:
    """One configuration: the documents, an engine with the K | V probe pinned (its rows are the dump-all rows bit for bit), and the thresholds
    of a criterion from the engine's own dump-all table."""

    def __init__(self, pkg, name):
        torch = _torch()
        shape, ee, precision, B, T, seed, shared = CASES[name]
        self.pkg, self.name, self.B, self.T, self.dit, self.precision = pkg, name, B, T, shape == "dit", precision
        mk = {"tiny": lambda **kw: pkg.ModelConfig.tiny(**kw), "h256": lambda **kw: pkg.ModelConfig.tiny(**kw, **H256_KW),
              "dit": lambda **kw: pkg.ModelConfig.dit_tiny(**kw)}[shape]
        self.cfg = mk(EE_config=dict(ee))
        if self.dit:
            self.W = pkg.synth.make_weights_beit(self.cfg, seed=seed, head_gain=4.0)
            docs = {"pixel_values": pkg.synth.make_documents(self.cfg, B, seed=seed + 1, text_len=8)["pixel_values"]}
        else:
            self.W = pkg.synth.make_weights(self.cfg, seed=seed, head_gain=4.0)
            if shared:
                self.W = _shared_heads(self.W)
            d = pkg.synth.make_documents(self.cfg, B, seed=seed + 1, text_len=T, min_words=2)
            docs = {k: d[k] for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}
        self.dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in docs.items()}
        self.E, self.K = self.cfg.exit_config.num_exits, self.cfg.num_labels
        self.eng = self.engine()

    def size(self):
        return dict(max_docs=self.B) if self.dit else dict(max_docs=self.B, max_text_len=self.T, precision=self.precision)

    def engine(self):
        eng = self.pkg.EarlyExitEngine(self.cfg, xprobe=False, **self.size())
        eng.load_weights(self.W)
        return eng

    def inputs(self):
        return {k: v.contiguous() for k, v in self.dev.items()}

    def thresholds(self, eng, criterion, **kw):
        """Midpoints of adjacent sorted values, more than 1e-9 apart, of the handle's own dump-all table, nearest each exit's median."""
        o = eng.forward(**self.inputs(), dump_all=True, want_all=True, want_head=True, **kw)
        eng.check()
        if criterion == "gate":
            t = _np(self.pkg.sweep.gate_table(o.head_logits, o.all_logits[self.E]))
        elif criterion == "lte":
            t = _np(o.all_crit).astype(np.float64)
        else:
            t = _np(self.pkg.sweep.csf_table(o.all_logits, criterion=criterion)[0])
        assert t.shape == (self.E + 1, self.B) and np.isfinite(t).all()
        n_emb = len(self.cfg.exit_config.embedding_exits) if criterion == "lte" else 0      # embedding exits have no LTE score: a constant row
        thr, width = csf_ref.gap_thresholds(t[n_emb:], 0.5, MIN_GAP)
        thr = np.concatenate([np.full(n_emb, 0.5), thr])
        assert (width[:-1] > MIN_GAP).all() and np.abs(t[n_emb:-1] - thr[n_emb:-1, None]).min() > MIN_DIST
        return thr


@pytest.fixture(scope="module")
def cases(pkg):
    built = {}

    def get(name):
        if name not in built:
            built[name] = Case(pkg, name)
        c = built[name]
        c.eng.set_audit(None)
        c.eng.set_ensemble(None)
        c.eng.set_exit_rule("plain")
        if name not in ("h256_lte",):
            c.eng.set_criterion("max_confidence")
        return c

    yield get
    for c in built.values():
        c.eng.close()


def _three_calls(c, eng, fraction=FRACTION, seed=SEED, **kw):
    """The handle's dump-all call, its unaudited call and its audited call under the same arguments; the audit is left set."""
    eng.set_audit(None)
    dump = eng.forward(**c.inputs(), dump_all=True, want_all=True, want_head=True, **{k: v for k, v in kw.items() if k != "thresholds"})
    plain = eng.forward(**c.inputs(), want_all=True, want_head=True, **kw)
    plain_counts = eng.stage_counts()["docs"]
    assert plain.audit_mask is None and not eng.has_audit()
    aud = eng.forward(**c.inputs(), want_all=True, want_head=True, audit_fraction=fraction, audit_seed=seed, **kw)
    counts = eng.stage_counts()["docs"]
    eng.check()
    assert eng.has_audit() and eng.audit == (fraction, seed, 0)
    return dump, plain, aud, plain_counts, counts


def _check_forward(c, dump, plain, aud, plain_counts, counts, tag, fraction=FRACTION, seed=SEED, slot_base=0, final_too=True):
    B, E = c.B, c.E
    m = A.mask(B, fraction, seed, slot_base)
    ex = _np(plain.exit_layer)
    # the case is a case (an assertion on the unaudited call, which does not need the feature): a selected document leaves early and becomes a
    # shadow, an unselected one leaves early and is gone, and (final_too) a selected one reaches the final exit by itself
    assert (m & (ex < E)).any() and (~m & (ex < E)).any(), (tag, ex.tolist(), np.nonzero(m)[0].tolist())
    assert not final_too or (m & (ex == E)).any(), (tag, ex.tolist(), np.nonzero(m)[0].tolist())
    for f in FIELDS:
        assert np.array_equal(_np(getattr(aud, f)).view(np.int32), _np(getattr(plain, f)).view(np.int32)), (tag, f)
    assert aud.audit_mask is not None and aud.audit_mask.is_cuda and np.array_equal(_np(aud.audit_mask), m), tag
    for f in DUMPS:
        d, p, a = (getattr(o, f) for o in (dump, plain, aud))
        if d is None:
            continue
        d, p, a = _np(d), _np(p), _np(a)
        n_e = d.shape[0]                                                         # E + 1 (all_*) or E (head_*)
        assert np.array_equal(_bits(a[:, m]), _bits(d[:, m])) and not np.isnan(d[:, m]).any(), (tag, f, "selected columns")
        reached = np.arange(n_e)[:, None] <= ex[None, :]
        for got in (a[:, ~m], p):                                                # unselected columns are the unaudited call's: the dump up to exit_layer, NaN behind it
            r = reached[:, ~m] if got is not p else reached
            want = d[:, ~m] if got is not p else d
            assert np.array_equal(_bits(got[r]), _bits(want[r])) and np.isnan(got[~r]).all(), (tag, f, "unselected columns")
    assert plain_counts == A.active_at_exit(ex, np.zeros(B, bool), E + 1), tag
    assert counts == A.active_at_exit(ex, m, E + 1), (tag, counts)
    return m, ex


FORWARD = [("tiny_ramp", "max_confidence"), ("tiny_ramp", "entropy"), ("tiny_ramp", "margin"), ("h256_ramp", "max_confidence"), ("h256_gate", "max_confidence")]


@pytest.mark.parametrize("name,criterion", FORWARD)
def test_forward_results_are_the_unaudited_bits_and_the_sample_is_the_dump(cases, name, criterion):
    c = cases(name)
    c.eng.set_criterion(criterion)
    thr = c.thresholds(c.eng, criterion)
    calls = _three_calls(c, c.eng, thresholds=thr)
    m, ex = _check_forward(c, *calls, (name, criterion))
    if name == "tiny_ramp":
        assert c.B == 64 and m.sum() == 17
    # fraction 1: everybody runs to the end, every stage holds B documents, the results are still the early-exit ones
    dump, plain = calls[0], calls[1]
    o = c.eng.forward(**c.inputs(), want_all=True, want_head=True, thresholds=thr, audit_fraction=1.0)
    assert c.eng.stage_counts()["docs"] == [c.B] * (c.E + 1)
    assert np.array_equal(_bits(_np(o.all_logits)), _bits(_np(dump.all_logits))) and np.array_equal(_bits(_np(o.all_crit)), _bits(_np(dump.all_crit)))
    assert np.array_equal(_bits(_np(o.head_logits)), _bits(_np(dump.head_logits))) and _np(o.audit_mask).all()
    for f in FIELDS:
        assert np.array_equal(_np(getattr(o, f)).view(np.int32), _np(getattr(plain, f)).view(np.int32)), f
    assert len(np.unique(ex)) >= 3
    # another seed is another sample; a dump-all call ignores the audit
    o2 = c.eng.forward(**c.inputs(), thresholds=thr, audit_fraction=FRACTION, audit_seed=2)
    assert np.array_equal(_np(o2.audit_mask), A.mask(c.B, FRACTION, 2)) and not np.array_equal(_np(o2.audit_mask), m)
    o3 = c.eng.forward(**c.inputs(), dump_all=True, want_all=True)
    assert o3.audit_mask is None and c.eng.stage_counts()["docs"] == [c.B] * (c.E + 1) and c.eng.has_audit()
    assert np.array_equal(_bits(_np(o3.all_logits)), _bits(_np(dump.all_logits)))
    c.eng.check()


def test_a_handle_without_an_audit_issues_the_parent_s_launches_and_bits(cases):
    c = cases("h256_ramp")
    thr = c.thresholds(c.eng, "max_confidence")

    def run(eng, **kw):
        eng.profile(True)
        o = eng.forward(**c.inputs(), thresholds=thr, **kw)
        prof = eng.profile_read()
        eng.profile(False)
        return {f: _np(getattr(o, f)) for f in FIELDS}, {role: v["launches"] for role, v in prof.items()}

    never, other = c.engine(), c.engine()
    out_never, n_never = run(never)
    assert n_never["exit_decide"] == c.E + 1
    out_aud, n_aud = run(other, audit_fraction=FRACTION, audit_seed=SEED)
    assert other.has_audit() and n_aud == n_never                                # an audited handle issues exactly as many launches
    other.set_audit(None)
    out_none, n_none = run(other)
    assert not other.has_audit() and other.audit is None
    out_zero, n_zero = run(other, audit_fraction=0.0)
    assert not other.has_audit() and n_none == n_never and n_zero == n_never
    for f in FIELDS:
        for got in (out_aud, out_none, out_zero):
            assert np.array_equal(got[f].view(np.int32), out_never[f].view(np.int32)), f
    never.close()
    other.close()


def test_patience_criterion(cases):
    c = cases("tiny_ramp")
    c.eng.set_criterion("patience")
    calls = _three_calls(c, c.eng, patience=1)
    _check_forward(c, *calls, "patience", final_too=False)
    c.eng.set_criterion("max_confidence")


@pytest.mark.parametrize("rule", ["patient_confident", "patience_or_threshold"])
def test_exit_rules(cases, rule):
    c = cases("tiny_ramp")
    thr = c.thresholds(c.eng, "max_confidence")
    c.eng.set_exit_rule(rule)
    calls = _three_calls(c, c.eng, thresholds=thr, patience=2)
    _check_forward(c, *calls, rule, final_too=False)
    c.eng.set_exit_rule("plain")


def test_learning_to_exit(cases):
    c = cases("h256_lte")
    thr = c.thresholds(c.eng, "lte")
    calls = _three_calls(c, c.eng, thresholds=thr)
    _check_forward(c, *calls, "use_lte", final_too=False)


def test_gate_criterion(cases):
    c = cases("h256_gate")
    c.eng.set_criterion("gate")
    thr = c.thresholds(c.eng, "gate")
    calls = _three_calls(c, c.eng, thresholds=thr)
    _check_forward(c, *calls, "gate", final_too=False)
    c.eng.set_criterion("max_confidence")


def test_an_ensemble_set(cases):
    c = cases("tiny_ramp")
    c.eng.set_ensemble(ER.random_weights(c.E + 1, c.K, seed=3))
    thr = c.thresholds(c.eng, "max_confidence")                                  # the table of the ensemble rows y_e, which all_logits carries
    calls = _three_calls(c, c.eng, thresholds=thr)
    _check_forward(c, *calls, "ensemble", final_too=False)
    c.eng.set_ensemble(None)


def test_low_latency(cases):
    """Whole layers in all three calls: the split-K parts are chosen from the call's static (B, T), the same in each."""
    c = cases("h256_ramp")
    thr = c.thresholds(c.eng, "max_confidence", low_latency=True, whole_layers=True)
    calls = _three_calls(c, c.eng, thresholds=thr, low_latency=True, whole_layers=True)
    _check_forward(c, *calls, "low_latency", final_too=False)
    assert max(c.eng.last_k_splits()) > 1


def test_tiny_dit(cases):
    c = cases("dit_tiny")
    thr = c.thresholds(c.eng, "max_confidence")
    calls = _three_calls(c, c.eng, thresholds=thr)
    _check_forward(c, *calls, "dit", final_too=False)


def test_micro_batched_engine_with_two_slices_is_the_single_handle(cases, pkg):
    c = cases("tiny_ramp")
    thr = c.thresholds(c.eng, "max_confidence")
    one = c.eng.forward(**c.inputs(), want_all=True, want_head=True, thresholds=thr, audit_fraction=FRACTION, audit_seed=SEED)
    one_counts = c.eng.stage_counts()["docs"]
    mb = pkg.MicroBatchedEngine(c.cfg, xprobe=False, micro_batches=2, **c.size())
    mb.load_weights(c.W)
    assert mb.set_audit(FRACTION, seed=SEED) == (FRACTION, SEED, 0) and mb.has_audit()
    two = mb.forward(**c.inputs(), want_all=True, want_head=True, thresholds=thr)
    assert mb.stage_counts()["docs"] == one_counts
    m = A.mask(c.B, FRACTION, SEED)
    assert np.array_equal(_np(two.audit_mask), m) and np.array_equal(_np(one.audit_mask), m)
    assert m[:c.B // 2].any() and m[c.B // 2:].any() and not np.array_equal(m[:c.B // 2], m[c.B // 2:])      # the second slice needs its slot base
    for f in FIELDS + DUMPS:
        assert np.array_equal(_np(getattr(two, f)).view(np.int32), _np(getattr(one, f)).view(np.int32)), f
    mb.set_audit(None)
    assert not mb.has_audit() and mb.forward(**c.inputs(), thresholds=thr).audit_mask is None
    mb.check()
    mb.close()


def test_model_wrapper_passes_the_audit_on_and_chunks_keep_the_caller_s_slots(cases, pkg):
    """``early_exit(audit_fraction=, audit_seed=)`` on a model whose engine holds fewer documents than the call: the chunks run under their own
    slot base, so the mask and every output are the single-handle ones, and the engine's audit is what the call set afterwards."""
    c = cases("tiny_ramp")
    thr = c.thresholds(c.eng, "max_confidence")
    one = c.eng.forward(**c.inputs(), want_all=True, want_head=True, thresholds=thr, audit_fraction=FRACTION, audit_seed=SEED)
    m = pkg.LayoutLMv3EEForSequenceClassification(c.cfg, weights=c.W, max_docs=24, max_text_len=c.T, precision=c.precision)
    out = m.early_exit(**c.inputs(), thresholds=thr, audit_fraction=FRACTION, audit_seed=SEED, want_all=True, want_head=True, xprobe=False)
    mask = A.mask(c.B, FRACTION, SEED)
    assert c.B > 2 * 24 and np.array_equal(_np(out.audit_mask), mask) and not np.array_equal(mask[24:48], mask[:24])
    for f in FIELDS + DUMPS:
        assert np.array_equal(_np(getattr(out, f)).view(np.int32), _np(getattr(one, f)).view(np.int32)), f
    assert m.engine.audit == (FRACTION, SEED, 0) and m.engine.has_audit()
    small = {k: v[:24].contiguous() for k, v in c.inputs().items()}                # a call that fits: passed straight through
    out2 = m.early_exit(**small, thresholds=thr, audit_seed=2, xprobe=False)
    assert np.array_equal(_np(out2.audit_mask), A.mask(24, FRACTION, 2)) and m.engine.audit == (FRACTION, 2, 0)
    m.engine.check()
    m.engine.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the tools
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_sample_feeds_the_dumped_array_tools_and_consistency_counts(cases, pkg):
    torch = _torch()
    c = cases("tiny_ramp")
    thr = c.thresholds(c.eng, "max_confidence")
    dump, plain, aud, _, _ = _three_calls(c, c.eng, thresholds=thr)
    s = pkg.audit.sample(aud)
    m = A.mask(c.B, FRACTION, SEED)
    idx = np.nonzero(m)[0]
    gathered = dump.all_logits[:, torch.from_numpy(idx).cuda()]
    assert np.array_equal(_np(s.index), idx) and np.array_equal(_bits(_np(s.logits)), _bits(_np(gathered)))
    assert np.array_equal(_bits(_np(s.crit)), _bits(_np(dump.all_crit)[:, idx])) and np.array_equal(_np(s.exit_layer), _np(plain.exit_layer)[idx])
    # label-free: the references are the final exit's own predictions
    al = _np(dump.all_logits)
    refs = s.references()
    assert np.array_equal(_np(refs), np.argmax(al[c.E][idx], -1))
    got, want = (pkg.sweep.threshold_search(z, references=refs, num_per_exit=3, mixtures=200, seed=5) for z in (s.logits, gathered))
    assert got.num_samples == len(idx) and np.array_equal(got.front_thresholds, want.front_thresholds) and np.array_equal(got.front_hits, want.front_hits)
    assert np.array_equal(got.front_exit_sum, want.front_exit_sum) and len(got.front_hits) >= 1
    ra, rb = (pkg.metrics.exit_report(z, refs, exits=s.exit_layer) for z in (s.logits, gathered))
    for f in ("accuracy", "brier_loss", "nll", "ece", "aurc", "average_confidence"):
        assert np.array_equal(getattr(ra, f), getattr(rb, f)), f
    assert ra.accuracy[c.E] == 1.0 and np.array_equal(ra.exit_hist, np.bincount(_np(s.exit_layer), minlength=c.E + 1))
    # consistency: numpy counts on the dump
    ex = _np(plain.exit_layer)[idx]
    am = np.argmax(al, -1)                                                       # numpy: the first maximum
    d = np.array([(ex == e).sum() for e in range(c.E)])
    a = np.array([((ex == e) & (am[ex, idx] == am[c.E, idx])).sum() for e in range(c.E)])
    for rep in (pkg.audit.consistency(aud), pkg.audit.consistency(s)):
        assert np.array_equal(rep.delivered, d) and np.array_equal(rep.agree, a) and rep.num_samples == len(idx)
        assert rep.pooled_delivered == d.sum() and rep.pooled_agree == a.sum() and d.sum() >= 1
    # the operating point of the report is the pooled agreement, the final-exit deliveries counted as agreeing
    assert ra.accuracy[c.E + 1] == (a.sum() + (ex == c.E).sum()) / len(idx)
    # two calls accumulate
    aud2 = c.eng.forward(**c.inputs(), want_all=True, thresholds=thr, audit_seed=2)
    both = pkg.AuditSample.concat([s, pkg.audit.sample(aud2)])
    assert both.num_samples == len(idx) + int(A.mask(c.B, FRACTION, 2).sum())
    assert pkg.audit.consistency(both).pooled_delivered >= d.sum()
    with pytest.raises(ValueError, match="not audited"):
        pkg.audit.sample(plain)
    with pytest.raises(ValueError, match="want_all"):
        pkg.audit.sample(c.eng.forward(**c.inputs(), thresholds=thr))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. the refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_say_why_and_leave_the_handle_usable(cases, pkg):
    c = cases("tiny_ramp")
    thr = c.thresholds(c.eng, "max_confidence")
    want = {f: _np(getattr(c.eng.forward(**c.inputs(), thresholds=thr), f)) for f in FIELDS}
    eng = c.engine()
    lib = pkg.capi.load()
    q = [1] * c.E

    def usable(audited):
        o = eng.forward(**c.inputs(), thresholds=thr)
        assert eng.has_audit() == audited and (o.audit_mask is not None) == audited
        for f in FIELDS:
            assert np.array_equal(_np(getattr(o, f)).view(np.int32), want[f].view(np.int32)), f
        eng.check()

    # quotas, in either order
    eng.set_audit(FRACTION, seed=SEED)
    with pytest.raises(pkg.capi.MMEEError, match="an audit is set: a rank would count"):
        eng.set_quotas(q)
    assert not eng.has_quotas
    usable(True)
    eng.set_audit(None)
    eng.set_quotas(q, mode="at_least")
    with pytest.raises(pkg.capi.MMEEError, match="quotas are set: a rank would count"):
        eng.set_audit(FRACTION)
    assert not eng.has_audit() and eng.audit is None
    eng.set_quotas(None)
    usable(False)
    # the result stream and captured graphs
    eng.set_audit(FRACTION, seed=SEED)
    with pytest.raises(pkg.capi.MMEEError, match="MMEE_FLAG_STREAM_RESULTS while an audit is set"):
        eng.forward_stream(**c.inputs(), thresholds=thr)
    usable(True)
    with pytest.raises(pkg.capi.MMEEError, match="ee_graph_capture: an audit is set"):
        eng.capture(**{k: v.clone() for k, v in c.inputs().items()}, thresholds=thr)
    usable(True)
    eng.set_audit(None)
    cap = eng.capture(**{k: v.clone() for k, v in c.inputs().items()}, thresholds=thr)
    with pytest.raises(pkg.capi.MMEEError, match="holds captured graphs"):
        eng.set_audit(FRACTION)
    assert not eng.has_audit()
    eng.set_audit(None)                                                          # off stays off: nothing to refuse
    out = cap.launch(thresholds=thr)
    assert np.array_equal(_np(out.exit_layer), want["exit_layer"])
    cap.close()
    eng.set_audit(FRACTION, seed=SEED)                                           # the graphs are gone
    usable(True)
    # the C entry point's own range checks (the Python side refuses them before the call)
    assert lib.ee_set_audit(eng._h, (1 << 32) + 1, 0, 0) != 0 and "above 2^32" in pkg.capi.last_error(eng._h)
    assert lib.ee_set_audit(eng._h, 1 << 31, 0, -1) != 0 and "slot_base -1 is negative" in pkg.capi.last_error(eng._h)
    usable(True)
    for bad in (-0.5, 1.5):
        with pytest.raises(ValueError, match="outside"):
            eng.set_audit(bad)
    with pytest.raises(ValueError, match="slot_base"):
        eng.set_audit(FRACTION, slot_base=-1)
    with pytest.raises(ValueError, match="32-bit"):
        eng.set_audit(FRACTION, seed=1 << 32)
    fresh = c.engine()
    with pytest.raises(ValueError, match="audit_seed= goes with"):
        fresh.forward(**c.inputs(), thresholds=thr, audit_seed=3)
    fresh.close()
    usable(True)
    # a cascade refuses a stage with an audit set
    other = c.engine()
    cascade = pkg.CascadeEngine([eng, other])
    with pytest.raises(ValueError, match="audited exits on cascade stages are not built"):
        cascade.forward(c.inputs())
    eng.set_audit(None)
    out = cascade.forward(c.inputs())
    assert out.logits.shape == (c.B, c.K)
    usable(False)
    cascade.close()
