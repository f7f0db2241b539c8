"""Model cascades (include/mmee.h, behind MMEE_QUOTA_*) on the MI355X against the numpy restatement of tests/cascade_ref.py: the three launches
of a stage boundary alone (ee_cascade_select / _gather / _merge) at the wave, workgroup and chunk edges with sentinel guards behind every
output, then ``CascadeEngine`` on synthetic weights against the composition done by hand in this file.

The device's exp may differ from numpy's in the last place of float64, so the select launch's float64 criteria are compared with numpy's within
1e-12 relative, and everything that is DECIDED on them -- the list, its order, the count -- is compared exactly with the restatement applied to
the device's own returned criteria.  The cascade is compared with the hand composition bit for bit: stage forward, the restatement's
selection on the device's own criteria (``csf_table`` of the delivered rows), ``index_select``, the next forward on that sub-batch with the
same chunking, a numpy merge.  Deferral thresholds sit at midpoints of adjacent sorted criteria more than 1e-9 apart, and a CPU assertion
checks that no criterion is within 1e-12 of its threshold."""
import numpy as np
import pytest

from . import cascade_ref as CR
from . import csf_ref
from . import metrics_ref
from .conftest import DIT_EE, H256_KW, TINY_CASES
from .hook_util import SENTINEL, _ptr, _stream, _torch

pytestmark = pytest.mark.gpu

GUARD = 4
SENT64 = np.int64(0x7FF5A5A57FA5A5A5)                  # a NaN bit pattern no kernel writes
MIN_GAP, MIN_DIST = 1e-9, 1e-12
CRIT_CODE = {"max_confidence": 0, "entropy": 1, "margin": 3}
SELECT_N = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
KS = (2, 16, 17)
PATTERNS = ("nobody", "everybody", "alternating", "random_third")


def _np(t):
    return t.detach().cpu().numpy()


def _sent(words):
    torch = _torch()
    return torch.full((int(words) + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")


def _cuda(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the three launches alone
# ---------------------------------------------------------------------------------------------------------------------------------------
def _select_case(n, K, criterion, pattern, with_orig, seed):
    """Rows whose criterion is far on one side of the threshold: small noise with one label 0.5 above the rest is unsure (max-softmax 0.62 at
    K = 2, 0.09 at K = 17), with one label 5 above the rest sure (0.99 / 0.90).  Neither closer nor further apart, so that the expressions
    stay well conditioned and a relative bound of 1e-12 means something: the entropy is log A - B / A without a max shift, which cancels on
    a peaked row (at a gap of 12 it is 8e-5 from two terms near 12, and one last-place difference between two exp implementations is 2e-11
    of it), and the margin's 1 - exp(m2 - m1) cancels where the two largest logits nearly tie."""
    rng = np.random.default_rng(seed)
    final_exit = 5
    want = {"nobody": np.zeros(n, bool), "everybody": np.ones(n, bool), "alternating": np.arange(n) % 2 == 1,
            "random_third": rng.random(n) < 1.0 / 3.0}[pattern]
    z = (rng.standard_normal((n, K)) * 0.05).astype(np.float32)
    z[np.arange(n), rng.integers(0, K, n)] += np.where(want, np.float32(0.5), np.float32(5.0))
    ex = np.full(n, final_exit, np.int32)
    early = rng.random(n) < 0.25                                           # left before the final exit: never selected, sure or not
    ex[early] = rng.integers(0, final_exit, n)[early]
    nan_row = n // 2 if n > 1 else None
    if nan_row is not None:
        z[nan_row, rng.integers(0, K)] = np.nan                            # never fires: selected whatever the pattern says
        ex[nan_row] = final_exit
    orig = np.sort(rng.choice(3 * n + 5, n, replace=False)).astype(np.int32) if with_orig else None
    c = CR.criteria(z, criterion)
    ok = ~np.isnan(c)
    up = csf_ref.SIGN[criterion] > 0
    unsure, sure = c[ok & want], c[ok & ~want]
    # between the unsure and the sure rows; with one kind only, beyond every value a criterion takes, on the side that kind needs
    if unsure.size and sure.size:
        lo, hi = (unsure.max(), sure.min()) if up else (sure.max(), unsure.min())
        assert lo + 1e-3 < hi
        thr = 0.5 * (lo + hi)
    elif unsure.size == 0:
        thr = -1.0 if up else 1e9                                          # every number fires
    else:
        thr = 2.0 if up else -1.0                                          # nothing fires
    expect = (want | np.isnan(c)) & (ex == final_exit)
    return dict(n=n, K=K, criterion=criterion, z=z, ex=ex, orig=orig, final_exit=final_exit, thr=float(thr), ref_crit=c, expect=expect)


def _run_select(pkg, c, with_crit=True):
    torch = _torch()
    n = c["n"]
    z, ex = _cuda(c["z"]), _cuda(c["ex"])
    orig = None if c["orig"] is None else _cuda(c["orig"])
    nxt, count = _sent(n), _sent(1)
    crit = torch.from_numpy(np.full(n + GUARD, SENT64, np.int64)).cuda()
    rc = pkg.capi.load().ee_cascade_select(_ptr(z), _ptr(ex), _ptr(orig), n, c["K"], c["final_exit"], CRIT_CODE[c["criterion"]], c["thr"],
                                           _ptr(nxt), _ptr(count), _ptr(crit) if with_crit else None, _stream())
    pkg.capi.check(rc, None, "ee_cascade_select")
    torch.cuda.synchronize()
    return _np(nxt), _np(count), _np(crit)


@pytest.mark.parametrize("criterion", list(CRIT_CODE))
@pytest.mark.parametrize("n", SELECT_N)
def test_select_alone(pkg, n, criterion):
    for K in KS:
        for pi, pattern in enumerate(PATTERNS):
            for with_orig in (False, True):
                tag = (n, K, criterion, pattern, with_orig)
                c = _select_case(n, K, criterion, pattern, with_orig, seed=1000 * n + 10 * K + pi + (5 if with_orig else 0))
                nxt, count, crit = _run_select(pkg, c)
                assert (crit[n:] == SENT64).all() and (count[1:] == SENTINEL).all(), tag
                dev, ref = crit[:n].view(np.float64), c["ref_crit"]
                assert np.array_equal(np.isnan(dev), np.isnan(ref)), tag
                with np.errstate(invalid="ignore"):
                    rel = np.where(np.isnan(ref), 0.0, np.abs(dev - ref) / np.maximum(np.abs(ref), 1e-300))
                assert (rel <= 1e-12).all(), (tag, float(rel.max()))
                want = CR.select(dev, c["ex"], c["final_exit"], c["thr"], criterion, c["orig"])
                m = int(count[0])
                assert m == len(want) and np.array_equal(nxt[:m], want), (tag, m, len(want))
                assert (nxt[m:] == SENTINEL).all(), (tag, "a write past the count")
                # the case is what it set out to be: exactly the intended documents, the NaN row among them, nobody who left early
                slots = np.arange(n) if c["orig"] is None else c["orig"]
                assert np.array_equal(want, slots[c["expect"]].astype(np.int32)), tag
                assert m == 0 or np.all(np.diff(nxt[:m]) > 0), tag
    # without the criteria output the decision is the same
    nxt2, count2, crit2 = _run_select(pkg, c, with_crit=False)
    assert np.array_equal(nxt2, nxt) and np.array_equal(count2, count) and (crit2 == SENT64).all()


def test_select_of_an_empty_stage_writes_a_zero_count(pkg):
    torch = _torch()
    count = _sent(1)
    pkg.capi.check(pkg.capi.load().ee_cascade_select(None, None, None, 0, 16, 3, 0, 0.5, None, _ptr(count), None, _stream()), None, "ee_cascade_select")
    torch.cuda.synchronize()
    assert _np(count).tolist() == [0] + [SENTINEL] * GUARD


GATHER_ROW_BYTES = (8, 24, 40, 4096, 49152, 49160)


@pytest.mark.parametrize("cap", [1, 255, 256, 257])
@pytest.mark.parametrize("row_bytes", GATHER_ROW_BYTES)
def test_gather_alone(pkg, row_bytes, cap):
    """Eight descriptors in one launch: the parametrised row size three times (aligned; destination 8 bytes off; source 4 bytes off, so rows
    of 4096 and 49152 bytes also take the 8- and 4-byte paths) and five small ones.  Compared on the device with index_select."""
    torch = _torch()
    lib = pkg.capi.load()
    rows_src = cap + 3
    gen = torch.Generator(device="cuda").manual_seed(row_bytes * 1000 + cap)
    rng = np.random.default_rng(row_bytes + cap)
    # (row_bytes, source offset in words, destination offset in words)
    plan = [(row_bytes, 0, 0), (row_bytes, 0, 2), (row_bytes, 1, 0), (8, 0, 0), (24, 0, 2), (40, 0, 0), (4096, 0, 0), (24, 1, 1)]
    srcs = []
    for rb, so, _ in plan:
        w = rb // 4
        buf = torch.randint(0, 1 << 30, (so + rows_src * w + GUARD,), dtype=torch.int32, device="cuda", generator=gen)
        srcs.append((buf, buf[so:so + rows_src * w].view(rows_src, w)))
    slots_np = np.sort(rng.choice(rows_src, cap, replace=False)).astype(np.int32)
    slots = torch.cat([_cuda(slots_np), torch.full((GUARD,), 1 << 28, dtype=torch.int32, device="cuda")])   # a slot past the count is never read as a row
    for count_v in sorted({0, 1, cap}):
        count = _cuda(np.array([count_v], np.int32))
        dsts = [_sent(do + cap * (rb // 4)) for rb, _, do in plan]
        descs = (pkg.capi.CascadeDesc * 8)()
        for i, (rb, so, do) in enumerate(plan):
            descs[i].src = srcs[i][1].data_ptr()
            descs[i].dst = dsts[i].data_ptr() + 4 * do
            descs[i].row_bytes = rb
            assert (descs[i].dst % 16 == 0) == (do == 0) and (descs[i].src % 16 == 0) == (so == 0)
        pkg.capi.check(lib.ee_cascade_gather(descs, 8, _ptr(slots), _ptr(count), cap, _stream()), None, "ee_cascade_gather")
        torch.cuda.synchronize()
        idx = slots[:count_v].long()
        for i, (rb, so, do) in enumerate(plan):
            w = rb // 4
            got = dsts[i]
            want = torch.full_like(got, SENTINEL)
            want[do:do + count_v * w] = srcs[i][1].index_select(0, idx).reshape(-1)
            assert torch.equal(got, want), (row_bytes, cap, count_v, i, "rows below the count are the source's, everything else keeps its sentinel")
    # fewer descriptors, and cap == 0: nothing is launched
    one = (pkg.capi.CascadeDesc * 8)()
    dst = _sent(cap * (row_bytes // 4))
    one[0].src, one[0].dst, one[0].row_bytes = srcs[0][1].data_ptr(), dst.data_ptr(), row_bytes
    pkg.capi.check(lib.ee_cascade_gather(one, 1, _ptr(slots), _ptr(_cuda(np.array([cap], np.int32))), 0, _stream()), None, "ee_cascade_gather")
    pkg.capi.check(lib.ee_cascade_gather(one, 0, None, None, cap, _stream()), None, "ee_cascade_gather")
    torch.cuda.synchronize()
    assert (dst == SENTINEL).all()


@pytest.mark.parametrize("n", [0, 1, 257])
@pytest.mark.parametrize("K", KS)
def test_merge_alone(pkg, K, n):
    torch = _torch()
    rng = np.random.default_rng(100 * K + n)
    B = n + 19
    prev = (rng.standard_normal((B, K)).astype(np.float32), rng.integers(0, 5, B).astype(np.int32), rng.random(B).astype(np.float32),
            rng.integers(0, 2, B).astype(np.int32))
    res = (rng.standard_normal((n, K)).astype(np.float32), rng.integers(0, 7, n).astype(np.int32), rng.random(n).astype(np.float32))
    if n:
        res[0][0, 0] = np.nan                                              # bit patterns travel, values are not looked at
    slots = np.sort(rng.choice(B, n, replace=False)).astype(np.int32)
    outs = [torch.cat([_cuda(a.reshape(-1).view(np.int32)), torch.full((GUARD,), SENTINEL, dtype=torch.int32, device="cuda")]) for a in prev]
    ins = [_cuda(a) for a in res] + [_cuda(slots)]
    rc = pkg.capi.load().ee_cascade_merge(*[_ptr(t) if n else None for t in ins], n, K, 11, 2, *[_ptr(t) for t in outs], _stream())
    pkg.capi.check(rc, None, "ee_cascade_merge")
    torch.cuda.synchronize()
    want = CR.merge(prev, res, slots, 11, 2)
    for name, got, w in zip(("logits", "exit_layer", "confidence", "stage"), outs, want):
        g = _np(got)
        assert (g[-GUARD:] == SENTINEL).all(), (name, "guard")
        assert np.array_equal(g[:-GUARD], np.ascontiguousarray(w).reshape(-1).view(np.int32)), (K, n, name)
    if n:
        assert np.array_equal(want[1][slots], res[1] + 11) and (want[3][slots] == 2).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the cascade on synthetic weights
# ---------------------------------------------------------------------------------------------------------------------------------------
B_DOCS, T_DOCS = 24, 48
CRITERION = "max_confidence"
H256_EE = dict(exits=["text_visual_concat", 1, 2], encoder_layer_strategy="ramp", inference_strategy="max_confidence")
FIELDS = ("logits", "exit_layer", "confidence", "stage")


class World:
    """The three models, one set of documents, and what is computed once: every model's dump-all table over all documents."""

    def __init__(self, pkg):
        self.pkg = pkg
        self.cfg = dict(dit=pkg.ModelConfig.dit_tiny(EE_config=dict(DIT_EE)), tiny=pkg.ModelConfig.tiny(EE_config=dict(TINY_CASES["tiny_ramp"])),
                        h256=pkg.ModelConfig.tiny(EE_config=dict(H256_EE), **H256_KW))
        self.W = dict(dit=pkg.synth.make_weights_beit(self.cfg["dit"], seed=91, head_gain=4.0),
                      tiny=pkg.synth.make_weights(self.cfg["tiny"], seed=92, head_gain=4.0),
                      h256=pkg.synth.make_weights(self.cfg["h256"], seed=93, head_gain=4.0))
        d = pkg.synth.make_documents(self.cfg["tiny"], B_DOCS, seed=94, text_len=T_DOCS, min_words=2)
        self.refs = d["labels"]
        self.inputs = {k: _cuda(d[k]) for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}
        self._eng, self._dump = {}, {}

    def engine(self, name, max_docs=B_DOCS):
        key = (name, max_docs)
        if key not in self._eng:
            kw = dict(max_docs=max_docs) if name == "dit" else dict(max_docs=max_docs, max_text_len=T_DOCS,
                                                                     precision="split" if name == "h256" else "fp32")
            eng = self.pkg.EarlyExitEngine(self.cfg[name], xprobe=False, **kw)
            eng.load_weights(self.W[name])
            self._eng[key] = eng
        return self._eng[key]

    def stage_inputs(self, eng, rows=None):
        keys = ("pixel_values",) if eng.beit else ("input_ids", "attention_mask", "bbox", "pixel_values")
        return {k: (self.inputs[k] if rows is None else self.inputs[k].index_select(0, rows)) for k in keys}

    def table(self, name):
        """numpy float64 criteria (E1,B) of the model's dump-all rows over all documents (the reference side of the thresholds)."""
        if name not in self._dump:
            eng = self.engine(name)
            al = _np(eng.forward(**self.stage_inputs(eng), dump_all=True, want_all=True).all_logits)
            assert np.isfinite(al).all()
            self._dump[name] = (al, csf_ref.csf(al.astype(np.float64), CRITERION))
        return self._dump[name][1]

    def thresholds(self, names, leave=0.05, defer=1.0 / 3.0):
        """Per-stage thresholds: below a stage's final exit about `leave` of the documents pass each exit; at the final exit of a stage that
        can defer about `defer` of the documents are below the threshold.  Every threshold is the midpoint of a gap wider than 1e-9."""
        out = []
        for s, name in enumerate(names):
            t = self.table(name)
            thr, width = csf_ref.gap_thresholds(t, 1.0 - leave, MIN_GAP)
            if s + 1 < len(names):
                last, w_last = csf_ref.gap_thresholds(np.stack([t[-1], t[-1]]), defer, MIN_GAP)
                thr[-1], width[-1] = last[0], w_last[0]
                assert np.abs(t - thr[:, None]).min() > MIN_DIST, (name, "a criterion within 1e-12 of its threshold")
            else:
                assert np.abs(t[:-1] - thr[:-1, None]).min() > MIN_DIST, (name, "a criterion within 1e-12 of its threshold")
            assert np.all(width > MIN_GAP)
            out.append(thr)
        return out


@pytest.fixture(scope="module")
def world(pkg):
    return World(pkg)


def _device_criteria(pkg, logits):
    """The device's own float64 criteria of delivered rows (n,K): csf_table's, the functions the select launch calls."""
    return _np(pkg.sweep.csf_table(logits.double().unsqueeze(0), None, CRITERION)[0])[0]


def hand_cascade(world, engines, thr):
    """The composition by hand: forward, the restatement's selection on the device's own criteria, index_select, the next forward on the
    sub-batch in chunks of the engine's max_docs, a numpy merge."""
    torch, pkg = _torch(), world.pkg
    e1 = [e.E + 1 for e in engines]
    off = CR.offsets(e1)
    K = engines[0].K
    out = (np.zeros((B_DOCS, K), np.float32), np.zeros(B_DOCS, np.int32), np.zeros(B_DOCS, np.float32), np.zeros(B_DOCS, np.int32))
    slots, stage_docs = np.arange(B_DOCS, dtype=np.int32), [0] * len(engines)
    for s, eng in enumerate(engines):
        n = len(slots)
        if n == 0:
            break
        stage_docs[s] = n
        ins = world.stage_inputs(eng, torch.from_numpy(slots.astype(np.int64)).cuda())
        parts = [eng.forward(**{k: v[a:a + eng.max_docs] for k, v in ins.items()}, thresholds=thr[s]) for a in range(0, n, eng.max_docs)]
        lg, ex, cf = (torch.cat([getattr(p, f) for p in parts]) for f in ("logits", "exit_layer", "confidence"))
        out = CR.merge(out, (_np(lg), _np(ex), _np(cf)), slots, off[s], s)
        if s + 1 == len(engines):
            break
        crit = _device_criteria(pkg, lg)
        slots = CR.select(crit, _np(ex), eng.E, thr[s][-1], CRITERION, slots)
    return dict(zip(FIELDS, out)), stage_docs


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, tag):
    for f in FIELDS:
        g = _np(getattr(got, f))
        assert g.dtype == want[f].dtype and np.array_equal(_bits(g), _bits(want[f])), (tag, f)


CASCADES = {"tiny_h256": ("tiny", "h256"), "dit_tiny": ("dit", "tiny"), "dit_tiny_h256": ("dit", "tiny", "h256")}


@pytest.mark.parametrize("name", list(CASCADES))
def test_cascade_is_the_hand_composition(world, pkg, name):
    names = CASCADES[name]
    engines = [world.engine(n) for n in names]
    casc = pkg.CascadeEngine(engines)
    assert casc.E1 == [e.E + 1 for e in engines] and casc.num_exits == sum(casc.E1)
    thr = world.thresholds(names)
    want, docs = hand_cascade(world, engines, thr)
    assert docs[1] > 0 and docs[1] < B_DOCS, ("about a third is deferred", docs)
    for how, arg in (("per stage", thr), ("flat", pkg.cascade.flat_thresholds(thr))):
        got = casc.forward(world.inputs, thresholds=arg)
        _same(got, want, (name, how))
        assert got.stage_docs == docs, (name, how, got.stage_docs, docs)
    # one dict per stage is the same call
    got = casc.forward([world.stage_inputs(e) for e in engines], thresholds=thr)
    _same(got, want, (name, "a dict per stage"))
    ex, st = _np(got.exit_layer), _np(got.stage)
    assert np.array_equal(ex, CR.global_exits(st, ex - CR.offsets(casc.E1)[st], casc.E1))
    assert [int((st >= s).sum()) if s else B_DOCS for s in range(len(names))][:2] == docs[:2]
    # nobody defers: the later stages never run
    lo = [t.copy() for t in thr]
    lo[0][-1] = -1.0
    for e in engines[1:]:
        e.profile(True)
    got = casc.forward(world.inputs, thresholds=lo)
    launches = [sum(v["launches"] for v in e.profile_read().values()) for e in engines[1:]]
    for e in engines[1:]:
        e.profile(False)
    assert launches == [0] * (len(names) - 1) and got.stage_docs == [B_DOCS] + [0] * (len(names) - 1)
    w0, d0 = hand_cascade(world, engines, lo)
    _same(got, w0, (name, "nobody defers"))
    assert d0 == got.stage_docs and (_np(got.stage) == 0).all()
    # everybody defers, all the way down
    hi = [np.full_like(t, 2.0) for t in thr]
    engines[-1].profile(True)
    got = casc.forward(world.inputs, thresholds=hi)
    ran = sum(v["launches"] for v in engines[-1].profile_read().values())
    engines[-1].profile(False)
    assert ran > 0 and got.stage_docs == [B_DOCS] * len(names)
    w1, d1 = hand_cascade(world, engines, hi)
    _same(got, w1, (name, "everybody defers"))
    assert (_np(got.stage) == len(names) - 1).all() and (_np(got.exit_layer) == casc.num_exits - 1).all()


def test_a_stage_smaller_than_its_batch_runs_in_chunks(world, pkg):
    """max_docs = 8 on the second stage, everybody deferred: chunks 8 / 8 / 8, the bits of the stage taken whole; and a third deferred."""
    big, small = world.engine("tiny"), world.engine("tiny", max_docs=8)
    dit = world.engine("dit")
    casc, whole = pkg.CascadeEngine([dit, small]), pkg.CascadeEngine([dit, big])
    thr = world.thresholds(("dit", "tiny"))
    hi = [np.full_like(thr[0], 2.0), thr[1]]
    got, ref = casc.forward(world.inputs, thresholds=hi), whole.forward(world.inputs, thresholds=hi)
    assert got.stage_docs == [B_DOCS, B_DOCS] == ref.stage_docs
    _same(got, {f: _np(getattr(ref, f)) for f in FIELDS}, "chunks of 8 against the stage whole")
    want, docs = hand_cascade(world, [dit, small], hi)
    _same(got, want, "chunks of 8 against the hand composition")
    got = casc.forward(world.inputs, thresholds=thr)
    want, docs = hand_cascade(world, [dit, small], thr)
    _same(got, want, "a third deferred, chunks of 8")
    assert got.stage_docs == docs
    # quotas rank a call's documents: a stage that runs in slices refuses them, a stage that takes the batch whole does not
    small.set_quotas([1] * small.E, mode="at_least")
    try:
        with pytest.raises(ValueError, match="quotas"):
            casc.forward(world.inputs, thresholds=hi)
    finally:
        small.set_quotas(None)
    _same(casc.forward(world.inputs, thresholds=thr), want, "after the quotas are cleared")


def test_callable_inputs_are_the_gather_route(world, pkg):
    torch = _torch()
    engines = [world.engine("dit"), world.engine("tiny")]
    casc = pkg.CascadeEngine(engines)
    thr = world.thresholds(("dit", "tiny"))
    calls = []

    def ocr(slots):
        assert isinstance(slots, np.ndarray) and slots.dtype == np.int32
        calls.append(slots.copy())
        return world.stage_inputs(engines[1], torch.from_numpy(slots.astype(np.int64)).cuda())

    ref = casc.forward(world.inputs, thresholds=thr)
    got = casc.forward([{"pixel_values": world.inputs["pixel_values"]}, ocr], thresholds=thr)
    _same(got, {f: _np(getattr(ref, f)) for f in FIELDS}, "callable against gather")
    assert got.stage_docs == ref.stage_docs and len(calls) == 1
    assert np.array_equal(calls[0], np.nonzero(_np(ref.stage) == 1)[0].astype(np.int32))
    lo = [thr[0].copy(), thr[1]]
    lo[0][-1] = -1.0
    got = casc.forward([{"pixel_values": world.inputs["pixel_values"]}, ocr], thresholds=lo)
    assert len(calls) == 1 and got.stage_docs == [B_DOCS, 0], "nobody is deferred: the callable is not called"


def test_the_dumped_array_tools_take_the_concatenated_dump(world, pkg):
    """The equivalence of the definition, at temperature 1 with xprobe=False engines under one criterion."""
    names = CASCADES["dit_tiny_h256"]
    engines = [world.engine(n) for n in names]
    casc = pkg.CascadeEngine(engines)
    thr = world.thresholds(names)
    flat = pkg.cascade.flat_thresholds(thr)
    D = casc.dump(world.inputs)
    assert tuple(D.shape) == (casc.num_exits, B_DOCS, casc.K) and D.dtype == _torch().float32
    Dn = _np(D)
    assert np.array_equal(_bits(Dn), _bits(np.concatenate([world._dump[n][0] for n in names])))
    table = csf_ref.csf(Dn.astype(np.float64), CRITERION)
    assert np.abs(table[:-1] - flat[:-1, None]).min() > MIN_DIST
    got = casc.forward(world.inputs, thresholds=flat)
    scan = _np(pkg.policy.criterion_scan_device(D, flat, CRITERION)[0])
    assert np.array_equal(scan, _np(got.exit_layer)), "criterion_scan_device(dump, flat) is the cascade's global exit_layer"
    assert np.array_equal(scan, csf_ref.exits(table, flat, +1))
    # what leaves is the dump's row at that exit
    assert np.array_equal(_bits(_np(got.logits)), _bits(Dn[scan, np.arange(B_DOCS)]))
    refs = world.refs
    rep = pkg.metrics.exit_report(D, refs, exits=got.exit_layer)
    want = metrics_ref.report(Dn.astype(np.float64), refs, exits=scan)
    assert np.array_equal(rep.accuracy, want["accuracy"])
    assert np.array_equal(np.asarray(rep.exit_hist), np.bincount(scan, minlength=casc.num_exits))
    # the searches take the table and hand back a flat vector the cascade takes
    res = pkg.sweep.threshold_search(D, refs, num_per_exit=3, mixtures=2000)
    pick = np.asarray(res.front_thresholds[0], dtype=np.float64)
    assert pick.shape == (casc.num_exits,) and [len(t) for t in pkg.cascade.split_thresholds(pick, engines)] == casc.E1
    assert casc.forward(world.inputs, thresholds=pick).stage_docs[0] == B_DOCS
    cost = pkg.cascade.exit_costs([e.cfg for e in engines], attention_mask=_np(world.inputs["attention_mask"]))
    assert cost.shape == (casc.num_exits, B_DOCS)
    assert len(pkg.sweep.threshold_search(D, refs, num_per_exit=3, mixtures=2000, cost=cost).front_thresholds) >= 1


def test_a_handle_used_in_a_cascade_is_unchanged_alone(world, pkg):
    eng = world.engine("tiny")
    thr = world.thresholds(("dit", "tiny"))
    call = dict(world.stage_inputs(eng), thresholds=thr[1])

    def run():
        eng.profile(True)
        o = eng.forward(**call)
        prof = {role: v["launches"] for role, v in eng.profile_read().items()}
        eng.profile(False)
        return {f: _np(getattr(o, f)) for f in FIELDS[:3]}, prof

    before, n_before = run()
    pkg.CascadeEngine([world.engine("dit"), eng]).forward(world.inputs, thresholds=thr)
    after, n_after = run()
    assert n_after == n_before
    for f in FIELDS[:3]:
        assert np.array_equal(_bits(after[f]), _bits(before[f])), f


def test_refusals_on_the_device(world, pkg):
    dit, tiny = world.engine("dit"), world.engine("tiny")
    other = pkg.ModelConfig.tiny(EE_config=dict(exits=[1], encoder_layer_strategy="ramp"), num_labels=tiny.K + 1)
    odd = pkg.EarlyExitEngine(other, max_docs=2, max_text_len=T_DOCS, xprobe=False)
    odd.load_weights(pkg.synth.make_weights(other, seed=3))
    with pytest.raises(ValueError, match="num_labels"):
        pkg.CascadeEngine([dit, odd])
    fresh = pkg.EarlyExitEngine(other, max_docs=2, max_text_len=T_DOCS, xprobe=False)
    with pytest.raises(pkg.capi.MMEEError, match="load_weights"):
        pkg.CascadeEngine([dit, fresh])
    casc = pkg.CascadeEngine([dit, tiny])
    with pytest.raises(NotImplementedError, match="streaming across stages"):
        casc.forward_stream(world.inputs)
    with pytest.raises(NotImplementedError, match="batch size depends on the data"):
        casc.capture(world.inputs)
    with pytest.raises(ValueError, match="CascadeEngine.dump"):
        casc.forward(world.inputs, dump_all=True)
    with pytest.raises(ValueError, match="input_ids"):
        casc.forward([{"pixel_values": world.inputs["pixel_values"]}] * 2, thresholds=[np.full(5, 2.0), np.full(8, 2.0)])
    odd.close()
    fresh.close()
