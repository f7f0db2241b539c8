"""The exit stage of csrc/exit_stage.hip alone, through ee_debug_head_out / ee_debug_exit_decide / ee_debug_rows_out, against the float64
restatement of tests/exit_stage_ref.py at every decision edge.  tests/test_host_exit_stage_ref.py shows without a GPU that the inputs used here
(built by exit_stage_ref, the same calls) force the leave patterns they name, keep every criterion half a MIN_GAP from its threshold, chain up to
the whole-store policies, and see each of sixteen subtle faults.

Acceptance:
  integer outputs (next stage, counts, sum_len_sq, state, exit indices) and every slot a kernel must not write   equality, no exclusions
  scaled logits (float)((double)z / temp), copied head logits, CLS rows, padded rows                              bit equality
  head_out logits, out_head_crit (float32 paths)     per row |got - ref64| <= max(2 err32, 1e-6), err32 = the same operation in float32 on the CPU
  out_all_crit, out_conf (float64 rounded)           np.float32(ref64) or the float32 next to it; the count of neighbours is recorded
  LTE score (float64)                                |got - ref| <= dt / 4 + 4 * 2^-53, dt = |np.dot - exact dot| of that row
Every output buffer starts as SENTINEL words and ends in GUARD entries that must survive; state arrays start as 0xA5 bytes outside the slots a
case sets."""
import ctypes as C

import numpy as np
import pytest

from . import csf_ref
from . import exit_stage_ref as R
from .conftest import report_measured
from .hook_util import SENTINEL, _encode_split, _stream, _torch

pytestmark = pytest.mark.gpu

GUARD = 4


# ---------------------------------------------------------------------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------------------------------------------------------------------
def _i32(a, pad=1):
    """An int array on the device, `pad` spare entries behind it (a stage of no documents still needs a pointer)."""
    torch = _torch()
    a = np.asarray(a, np.int64).reshape(-1)
    return torch.from_numpy(np.concatenate([a, np.full(pad, SENTINEL, np.int64)]).astype(np.int32)).cuda()


def _f(a, dtype=np.float32):
    torch = _torch()
    a = np.ascontiguousarray(a, dtype)
    if a.size == 0:
        a = np.zeros(4, dtype)
    return torch.from_numpy(a).cuda()


def _sent(words):
    torch = _torch()
    return torch.full((int(words) + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")


def _counts(stage):
    sq = stage["sum_len_sq"]
    return [stage["n"], stage["n_rows"], sq & 0xFFFFFFFF, sq >> 32]


def _words(t, n=None):
    return t.cpu().numpy()[:n]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _expect(words, want_rows, rows, width, what):
    """Rows `rows` of a [*, width] int32 buffer hold want_rows (bit patterns; a NaN matches any NaN), every other word is SENTINEL."""
    got = words.copy()
    want = np.full(len(got), SENTINEL, np.int32)
    idx = (np.asarray(rows, np.int64)[:, None] * width + np.arange(width)[None]).reshape(-1)
    want[idx] = np.asarray(want_rows, np.int32).reshape(-1)
    both_nan = np.zeros(len(got), bool)
    both_nan[idx] = np.isnan(got[idx].view(np.float32)) & np.isnan(want[idx].view(np.float32))
    bad = np.nonzero((got != want) & ~both_nan)[0]
    assert bad.size == 0, (what, bad[:6].tolist(), got[bad[:6]].tolist(), want[bad[:6]].tolist())


def _near_f32(tag, got_words, ref64, what):
    """np.float32(ref64) or the float32 next to it; a NaN for a NaN.  Returns how many took the neighbour."""
    got = np.asarray(got_words, np.int32).view(np.float32)
    want = np.asarray(ref64, np.float64).astype(np.float32)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(invalid="ignore"):
        near = (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))
    bad = np.nonzero(~(same | near))[0]
    assert bad.size == 0, (tag, what, bad[:6].tolist(), got[bad[:6]].tolist(), want[bad[:6]].tolist())
    return int((~same & near).sum())


# ---------------------------------------------------------------------------------------------------------------------------------------
# one ee_debug_exit_decide call
# ---------------------------------------------------------------------------------------------------------------------------------------
OPTIONAL = ("out_logits", "out_conf", "out_all_logits", "out_all_crit", "out_head_logits", "out_head_crit")


def _decide(pkg, c, by_pointer=0, null=(), stage_dev=None, meta=None, **over):
    """Runs one exit of case c (exit_stage_ref.single_case's dict).  stage_dev: the current stage as device tensors (a chained call), else
    built from c["stage"].  meta: (meta_old device [rows, 4], rows) switches the compaction on.  Returns every buffer, raw."""
    torch = _torch()
    p = dict(c)
    p.update(over)
    st, n, B, K, e = p["stage"], p["stage"]["n"], p["B"], p["K"], p["exit_index"]
    Kh = 2
    dev = stage_dev or dict(counts=_i32(_counts(st), 0), doc_orig=_i32(st["doc_orig"]), doc_off=_i32(st["doc_off"]), x_phys=_i32(st["x_phys"]))
    chained = isinstance(p["state"], dict)                              # a chained call: the caller's device state
    prev, run = (np.full(B, R.DIRTY, np.int64),) * 2 if p["state"] is None or chained else p["state"]
    b = dict(prev=_i32(prev, GUARD), run=_i32(run, GUARD), n_counts=_sent(4), n_doc_orig=_sent(n), n_doc_off=_sent(n + 1), n_x_src=_sent(n),
             n_meta_src=_sent(n), out_logits=_sent(B * K), out_exit=_sent(B), out_conf=_sent(B), out_all_logits=_sent((e + 1) * B * K),
             out_all_crit=_sent((e + 1) * B), out_head_logits=_sent((e + 1) * B * Kh), out_head_crit=_sent((e + 1) * B))
    if chained:
        b["prev"], b["run"] = p["state"]["prev"], p["state"]["run"]
    keep = [_f(p["logits"]), None if p["head_logits"] is None else _f(p["head_logits"]), None if p["lte_score"] is None else _f(p["lte_score"], np.float64)]
    a = pkg.capi.DebugExitDecideArgs()
    for k, v in dict(mode=p["mode"], rule=p["rule"], criterion=R.CRIT_CODE[p["criterion"]], K=K, Kh=Kh, thr=p["thr"], temp=p["temp"],
                     patience=p["patience"], by_pointer=by_pointer, exit_index=e, is_final=int(p.get("is_final", 0)), no_exit=int(p.get("no_exit", 0)),
                     B=B).items():
        setattr(a, k, v)
    a.pol_logits, a.head_logits, a.lte_score = (t.data_ptr() if t is not None else None for t in keep)
    for k, t in dev.items():
        setattr(a, k, t.data_ptr())
    for k, t in b.items():
        setattr(a, k, None if k in null else t.data_ptr())
    if meta is not None:
        b["meta_new"], b["row_src"] = _sent(meta[1] * 4), _sent(meta[1])
        a.meta_old, a.meta_new, a.row_src = meta[0].data_ptr(), b["meta_new"].data_ptr(), b["row_src"].data_ptr()
    pkg.capi.check(pkg.capi.load().ee_debug_exit_decide(C.byref(a), _stream()), None, "ee_debug_exit_decide")
    torch.cuda.synchronize()
    b["_null"] = tuple(null)
    return b


def _check_decide(tag, c, r, b, counters, **over):
    """Every buffer of one call against decide_ref's result r."""
    p = dict(c)
    p.update(over)
    st, n, B, K, e = p["stage"], p["stage"]["n"], p["B"], p["K"], p["exit_index"]
    o, lv, nx = st["doc_orig"], r["leave"], r["next"]
    null = b["_null"]
    got_counts = [int(w) & 0xFFFFFFFF for w in _words(b["n_counts"])]
    assert got_counts == _counts(nx) + [SENTINEL] * GUARD, (tag, got_counts, _counts(nx))
    for k, extra in (("n_doc_orig", 0), ("n_doc_off", 1), ("n_x_src", 0), ("n_meta_src", 0)):
        got, want = _words(b[k]), nx[k][:n + extra + GUARD]
        assert np.array_equal(got, want), (tag, k, np.nonzero(got != want)[0][:6].tolist())
    if not isinstance(p["state"], dict):
        for k, want in zip(("prev", "run"), r["state"]):
            assert np.array_equal(_words(b[k]), np.concatenate([want, [SENTINEL] * GUARD])), (tag, k)
    _expect(_words(b["out_exit"]), np.full(lv.sum(), e), o[lv], 1, (tag, "out_exit"))
    if "out_logits" not in null:
        _expect(_words(b["out_logits"]), _bits(r["scaled32"][lv]), o[lv], K, (tag, "out_logits"))
    if "out_all_logits" not in null:
        _expect(_words(b["out_all_logits"]), _bits(r["scaled32"]), e * B + o, K, (tag, "out_all_logits"))
    for k, rows, ref in (("out_conf", o[lv], r["crit"][lv]), ("out_all_crit", e * B + o, r["crit"])):
        if k in null:
            continue
        w = _words(b[k])
        counters["near"] += _near_f32(tag, w[rows], ref, k)
        counters["crit"] += len(rows)
        w[rows] = SENTINEL
        assert (w == SENTINEL).all(), (tag, k, "a write outside the documents' slots")
    heads = p["head_logits"] is not None
    for k, width in (("out_head_logits", 2), ("out_head_crit", 1)):
        if k in null:
            continue
        w = _words(b[k])
        if not heads:
            assert (w == SENTINEL).all(), (tag, k, "written without head logits")
        elif k == "out_head_logits":
            _expect(w, _bits(p["head_logits"]), e * B + o, 2, (tag, k))
        else:
            rows = e * B + o
            hc = "max_confidence" if p["mode"] == R.PATIENCE else p["criterion"]
            got, ref = w[rows].view(np.float32).astype(np.float64), r["head_crit"]
            err, err32 = np.abs(got - ref), np.abs(R.crit_f32(p["head_logits"], hc).astype(np.float64) - ref)
            tol = R.tolerance(err32)
            if n:
                counters["head_err"] = max(counters["head_err"], float(err.max()))
                counters["head_err32"] = max(counters["head_err32"], float(err32.max()))
                counters["head_ratio"] = max(counters["head_ratio"], float((err / tol).max()))
            if not (err <= tol).all():                                   # the figures of a miss are on record before the assertion
                worst = int(np.argmax(err / tol))
                report_measured(tag, f"out_head_crit max|err| (worst row {worst}: err32 {err32[worst]:.3e}, err / tol {err[worst] / tol[worst]:.2f})", float(err.max()))
            assert (err <= tol).all(), (tag, k, float(err.max()), float(tol.min()))
            w[rows] = SENTINEL
            assert (w == SENTINEL).all(), (tag, k, "a write outside the documents' slots")


def _new_counters():
    return dict(near=0, crit=0, head_err=0.0, head_err32=0.0, head_ratio=0.0)


def _report(tag, ct):
    report_measured(tag, f"criteria stored as the float32 next to np.float32(ref64), of {ct['crit']}", float(ct["near"]))
    if ct["head_err32"] or ct["head_err"]:
        report_measured(tag, f"out_head_crit max|err| (err32 {ct['head_err32']:.3e}, worst err / tol {ct['head_ratio']:.2f})", ct["head_err"])


def _same_bytes(tag, a, b):
    torch = _torch()
    for k in a:
        if k != "_null":
            assert torch.equal(a[k], b[k]), (tag, k, "by_pointer changes the bytes")


# ---------------------------------------------------------------------------------------------------------------------------------------
# decide, single exit
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ki", range(len(R.KERNELS)), ids=R.KERNEL_IDS)
@pytest.mark.parametrize("n", R.SINGLE_N)
def test_decide_single_exit(pkg, n, ki):
    """Every leave pattern at one stage size for one kernel, the criteria, K and the gate-style head cycled (exit_stage_ref.single_plan); the
    values by pointer give the same bytes as by value."""
    ct = _new_counters()
    for pattern, criterion, K, head in R.single_plan(n, ki):
        c = R.single_case(R.KERNELS[ki], criterion, n, pattern, K, seed=ki, head=head)
        tag = f"exit_stage.decide[{R.KERNEL_IDS[ki]} n={n} {pattern} {criterion} K={K}]"
        r = R.run_case(c)
        assert np.array_equal(r["leave"], c["want"])
        b = _decide(pkg, c)
        _check_decide(tag, c, r, b, ct)
        _same_bytes(tag, b, _decide(pkg, c, by_pointer=1))
    _report(f"exit_stage.decide[{R.KERNEL_IDS[ki]} n={n}]", ct)


def test_decide_long_documents_fill_sum_len_sq_past_32_bits(pkg):
    c = R.big_case()
    r = R.run_case(c)
    assert r["next"]["sum_len_sq"] > 1 << 32
    ct = _new_counters()
    for by_pointer in (0, 1):
        _check_decide("exit_stage.decide[2049 x 1500 rows]", c, r, _decide(pkg, c, by_pointer=by_pointer), ct)


@pytest.mark.parametrize("ki", range(len(R.KERNELS)), ids=R.KERNEL_IDS)
def test_decide_final_and_no_exit(pkg, ki):
    ct = _new_counters()
    c = R.single_case(R.KERNELS[ki], "margin", 1025, "random", 10, seed=ki, head=True)
    for flags in (dict(is_final=True), dict(no_exit=True), dict(is_final=True, no_exit=True)):
        r = R.run_case(c, **flags)
        assert r["leave"].all() == bool(flags.get("is_final")) and r["leave"].any() == bool(flags.get("is_final"))
        b = _decide(pkg, c, **flags)
        _check_decide(f"exit_stage.decide[{R.KERNEL_IDS[ki]} {flags}]", c, r, b, ct)
        _same_bytes(str(flags), b, _decide(pkg, c, by_pointer=1, **flags))
    _report(f"exit_stage.decide[{R.KERNEL_IDS[ki]} final / no_exit]", ct)


@pytest.mark.parametrize("null", OPTIONAL + ("head_logits",))
def test_decide_every_optional_output_null_once(pkg, null):
    ct = _new_counters()
    for ki in (0, 2, 3, 5):
        c = R.single_case(R.KERNELS[ki], "entropy", 65, "alternating", 17, seed=ki, head=True)
        if null == "head_logits":
            c = dict(c, head_logits=None)
        _check_decide(f"exit_stage.decide[{R.KERNEL_IDS[ki]} without {null}]", c, R.run_case(c), _decide(pkg, c, null=() if null == "head_logits" else (null,)), ct)


@pytest.mark.parametrize("ki", [i for i, k in enumerate(R.KERNELS) if k[0] == R.LTE], ids=lambda i: R.KERNEL_IDS[i])
def test_decide_lte_exit_without_a_score(pkg, ki):
    """An embedding exit under LTE has no score: the criterion written out is 1.0 and the event never fires (the agreement counter of EITHER
    still releases its documents, a streak is reset)."""
    ct = _new_counters()
    c = dict(R.single_case(R.KERNELS[ki], "max_confidence", 65, "random", 10, seed=ki, head=True), lte_score=None)
    r = R.run_case(c)
    assert (r["crit"] == 1.0).all() and r["leave"].any() == (R.KERNELS[ki][1] == R.EITHER) and not r["leave"].all()
    for by_pointer in (0, 1):
        _check_decide(f"exit_stage.decide[{R.KERNEL_IDS[ki]} no score]", c, r, _decide(pkg, c, by_pointer=by_pointer), ct)
    assert ct["near"] == 0


@pytest.mark.parametrize("ki", [i for i, k in enumerate(R.KERNELS) if k[0] == R.PATIENCE or k[1] != R.PLAIN], ids=lambda i: R.KERNEL_IDS[i])
def test_decide_exit_zero_does_not_read_the_state(pkg, ki):
    """State that would release everybody if exit 0 read it, and dirty state: the same decisions, the run counters rewritten."""
    ct = _new_counters()
    c = R.exit0_case(R.KERNELS[ki])
    r = R.run_case(c)
    _check_decide(f"exit_stage.decide[{R.KERNEL_IDS[ki]} exit 0, adversarial state]", c, r, _decide(pkg, c), ct)
    d = dict(c, state=None)
    _check_decide(f"exit_stage.decide[{R.KERNEL_IDS[ki]} exit 0, dirty state]", d, R.run_case(d), _decide(pkg, d, by_pointer=1), ct)


# ---------------------------------------------------------------------------------------------------------------------------------------
# decision edges
# ---------------------------------------------------------------------------------------------------------------------------------------
def _one_doc(mode, criterion, z, **kw):
    st = R.make_stage(1, 2)
    base = dict(kernel=(mode, R.PLAIN), mode=mode, rule=R.PLAIN, criterion=criterion, n=1, B=2, K=z.shape[1], stage=st, logits=z, head_logits=None,
                lte_score=None, thr=0.5, temp=1.0, patience=1, exit_index=0, state=None)
    base.update(kw)
    return base


def test_decide_strict_at_equality(pkg):
    """Criteria that are exact in float64; the threshold AT the value never fires, one float64 step to the firing side fires."""
    ct = _new_counters()
    for name, mode, criterion, z, score, val, steps in R.edge_cases():
        for thr, fires in steps:
            for by_pointer in (0, 1):
                c = _one_doc(mode, criterion, z, lte_score=score, thr=float(thr))
                r = R.run_case(c)
                assert bool(r["leave"][0]) == fires and r["crit"][0] == val
                _check_decide(f"exit_stage.edge[{name} thr={thr!r}]", c, r, _decide(pkg, c, by_pointer=by_pointer), ct)
    assert ct["near"] == 0                                              # 1, 0.5 and 0 are float32 values: stored exactly


def test_decide_a_nan_row_never_fires_and_leaves_at_the_final_exit(pkg):
    ct = _new_counters()
    z = np.array([[0.3, np.nan, 1.0]], np.float32)
    for criterion in csf_ref.CRITERIA:
        for thr in (-np.inf, 0.0, np.inf):
            for final in (False, True):
                c = _one_doc(R.THRESHOLD, criterion, z, thr=thr, is_final=final, exit_index=3 if final else 1, state=None)
                r = R.run_case(c, is_final=final)
                assert bool(r["leave"][0]) == final and np.isnan(r["crit"][0])
                b = _decide(pkg, c)
                _check_decide(f"exit_stage.edge[NaN row {criterion} thr={thr} final={final}]", c, r, b, ct, is_final=final)
                assert (_words(b["out_exit"])[c["stage"]["doc_orig"][0]] == 3) == final


def test_decide_first_maximum_of_the_scaled_logits(pkg):
    """Two float32 logits z0 < z1 that the temperature 3 rounds to one scaled value: the argmax is the first index; and patience 0 / 1 at exit 0."""
    ct = _new_counters()
    z0, z1 = R.collision_pair(3.0)
    assert z0 < z1 and np.float32(np.float64(z0) / 3.0) == np.float32(np.float64(z1) / 3.0)
    for z, first in ((np.array([[z0, z1]], np.float32), 0), (np.array([[-1.0, z0, 0.0, z1]], np.float32), 1), (np.array([[z1, z0]], np.float32), 0)):
        for mode, rule in ((R.PATIENCE, R.PLAIN), (R.THRESHOLD, R.EITHER), (R.LTE, R.EITHER)):
            for t, leaves in ((0, True), (1, False)):
                c = _one_doc(mode, "max_confidence", z, rule=rule, temp=3.0, patience=t, thr=2.0 if mode == R.THRESHOLD else -1.0,
                             lte_score=np.array([0.5]) if mode == R.LTE else None)
                r = R.run_case(c)
                slot = c["stage"]["doc_orig"][0]
                assert r["state"][0][slot] == first and r["state"][1][slot] == 0 and bool(r["leave"][0]) == leaves
                for by_pointer in (0, 1):
                    _check_decide(f"exit_stage.edge[collision {z.shape[1]} labels, mode {mode} rule {rule} t={t}]", c, r, _decide(pkg, c, by_pointer=by_pointer), ct)


# ---------------------------------------------------------------------------------------------------------------------------------------
# chained
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain():
    return R.chain_inputs()


CHAIN_CASES = [(k, c) for k in R.KERNELS for c in (csf_ref.CRITERIA if k == (R.THRESHOLD, R.PLAIN) else ("max_confidence",))]


@pytest.mark.parametrize("kernel,criterion", CHAIN_CASES, ids=[f"{R.KERNEL_IDS[R.KERNELS.index(k)]}-{c}" for k, c in CHAIN_CASES])
def test_chained_exits_reproduce_the_whole_store_policy(pkg, chain, kernel, criterion):
    """1025 documents through 5 exits, every call's n_* outputs the next call's stage (the device buffers themselves), state and metadata carried
    on the device, the row map expanded behind every decision."""
    torch = _torch()
    ct = _new_counters()
    mode, rule = kernel
    ref = R.chain_ref(chain, kernel, criterion)
    x, table, sign, thr, width = R.chain_tables(chain, kernel, criterion)
    want_exit = R.chain_whole_store(chain, kernel, criterion)
    B, K, E1, st0 = R.CHAIN_B, R.CHAIN_K, R.CHAIN_E1, chain["stage"]
    rows0 = st0["n_rows"]
    state = dict(prev=_i32(np.full(B, R.DIRTY), GUARD), run=_i32(np.full(B, R.DIRTY), GUARD))
    final = dict(out_logits=_sent(B * K), out_exit=_sent(B), out_conf=_sent(B))
    stage_dev, meta_dev, meta_np = None, _i32(chain["meta"], 0).view(rows0, 4), chain["meta"]
    for e, step in enumerate(ref["steps"]):
        st = step["stage"]
        o = st["doc_orig"]
        c = dict(mode=mode, rule=rule, criterion=criterion, B=B, K=K, stage=st, logits=chain["store"][e][o], head_logits=None,
                 lte_score=chain["scores"][e][o] if mode == R.LTE else None, thr=float(thr[e]), temp=float(R.CHAIN_TEMPS[e]), patience=R.CHAIN_T,
                 exit_index=e, state=state, is_final=e == E1 - 1)
        tag = f"exit_stage.chain[{R.KERNEL_IDS[R.KERNELS.index(kernel)]} {criterion} exit {e}]"
        b = _decide(pkg, c, by_pointer=e % 2, stage_dev=stage_dev, meta=(meta_dev, rows0))
        _check_decide(tag, c, step, b, ct)
        for k, want in zip(("prev", "run"), step["state"]):
            assert np.array_equal(_words(state[k]), np.concatenate([want, [SENTINEL] * GUARD])), (tag, k)
        nx = step["next"]
        row_src, meta_new = R.compact_ref(nx, meta_np, rows0)
        assert np.array_equal(_words(b["row_src"]), np.concatenate([row_src, [SENTINEL] * GUARD])), (tag, "row_src")
        assert np.array_equal(_words(b["meta_new"]), np.concatenate([meta_new.reshape(-1), [SENTINEL] * GUARD])), (tag, "meta_new")
        lv = step["leave"]                                               # what the leavers of this exit carry home; the final buffers collect them
        for k, width_ in (("out_logits", K), ("out_exit", 1), ("out_conf", 1)):
            idx = torch.from_numpy((o[lv][:, None] * width_ + np.arange(width_)).reshape(-1)).cuda()
            final[k][idx] = b[k][idx]
        stage_dev = dict(counts=b["n_counts"], doc_orig=b["n_doc_orig"], doc_off=b["n_doc_off"], x_phys=b["n_x_src"])
        meta_dev, meta_np = b["meta_new"][:rows0 * 4].view(rows0, 4), meta_new
    o = st0["doc_orig"]
    _expect(_words(final["out_exit"]), want_exit[o], o, 1, "final exits against the whole-store policy")
    _expect(_words(final["out_logits"]), _bits(x.astype(np.float32)[want_exit[o], o]), o, K, "final logits")
    w = _words(final["out_conf"])
    ct["near"] += _near_f32("chain", w[o], table[want_exit[o], o], "final confidences")
    _report(f"exit_stage.chain[{R.KERNEL_IDS[R.KERNELS.index(kernel)]} {criterion}]", ct)
    assert torch.equal(stage_dev["counts"][:4].cpu(), torch.zeros(4, dtype=torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------------------
# head_out
# ---------------------------------------------------------------------------------------------------------------------------------------
def _head_out(pkg, c, n_docs=None):
    torch = _torch()
    n = c["n"] if n_docs is None else n_docs
    H, Ko, md = c["H"], c["Ko"], c["max_docs"]
    t = dict(x=_f(c["x"]), W=_f(c["W"]), b=_f(c["b"]), n=_i32([n], 0), gather=None if c["gather"] is None else _i32(c["gather"]))
    out, score = _sent(md * Ko), None
    a = pkg.capi.DebugHeadOutArgs()
    a.in_, a.in_rows, a.ld, a.gather, a.W, a.b = t["x"].data_ptr(), c["in_rows"], c["ld"], t["gather"].data_ptr() if t["gather"] is not None else None, \
        t["W"].data_ptr(), t["b"].data_ptr()
    a.H, a.Ko, a.n_docs, a.max_docs, a.out = H, Ko, t["n"].data_ptr(), md, out.data_ptr()
    if "lte_x" in c:
        if c["split"]:
            words = np.full((c["lte_rows"], c["lte_ld"]), SENTINEL, np.int32)
            words[:, :H] = _encode_split(c["lte_x"][:, :H], R.LTE_SPLIT_SCALE)
            t["lx"] = torch.from_numpy(words).cuda()
        else:
            t["lx"] = _f(c["lte_x"])
        t.update(lw=_f(c["lte_w"]), lb=_f(c["lte_b"]), lg=None if c["lte_gather"] is None else _i32(c["lte_gather"]))
        score = _sent(2 * md)
        a.lte_in, a.lte_rows, a.lte_ld, a.lte_gather = t["lx"].data_ptr(), c["lte_rows"], c["lte_ld"], t["lg"].data_ptr() if t["lg"] is not None else None
        a.lte_split_inv, a.lte_w, a.lte_b, a.lte_out = 1.0 / R.LTE_SPLIT_SCALE if c["split"] else 0.0, t["lw"].data_ptr(), t["lb"].data_ptr(), score.data_ptr()
    pkg.capi.check(pkg.capi.load().ee_debug_head_out(C.byref(a), _stream()), None, "ee_debug_head_out")
    torch.cuda.synchronize()
    return _words(out), None if score is None else _words(score)


@pytest.mark.parametrize("lte", [0, 1, 2], ids=["no_lte", "lte_f32", "lte_split"])
@pytest.mark.parametrize("H", R.HEAD_H)
def test_head_out_against_float64(pkg, H, lte):
    for c in R.head_cases(H, lte):
        c = dict(c, split=lte == 2)
        n, Ko = c["n"], c["Ko"]
        tag = f"exit_stage.head_out[H={H} n={n} Ko={Ko} ld={c['ld']} gather={c['gather'] is not None} lte={lte}]"
        out, score = _head_out(pkg, c)
        ref = R.head_out_ref(c["x"], c["W"], c["b"], c["gather"], n)
        err32 = np.abs(R.head_out_f32(c["x"], c["W"], c["b"], c["gather"], n).astype(np.float64) - ref).max(-1)
        got = out[:n * Ko].view(np.float32).astype(np.float64).reshape(n, Ko)
        err, tol = np.abs(got - ref).max(-1), R.tolerance(err32)
        worst = int(np.argmax(err / tol))
        report_measured(tag, f"max|err| over {n} rows (worst row {worst}: err32 {err32[worst]:.3e}, err / tol {err[worst] / tol[worst]:.2f})", float(err.max()))
        assert (err <= tol).all(), (tag, float(err.max()))
        assert (out[n * Ko:] == SENTINEL).all(), (tag, "a write past the last document")
        if lte:
            want, dt = R.lte_score_ref(c["lte_x"], c["lte_w"], c["lte_b"], c["lte_gather"], n)
            s = score[:2 * n].view(np.float64)
            serr, stol = np.abs(s - want), dt / 4 + 4 * 2.0 ** -53
            worst = int(np.argmax(serr / stol))
            report_measured(tag, f"LTE score max|err| (worst row {worst}: dt {dt[worst]:.3e}, err / tol {serr[worst] / stol[worst]:.2f})", float(serr.max()))
            assert (serr <= stol).all(), (tag, float(serr.max()), float(stol[worst]))
            assert (score[2 * n:] == SENTINEL).all(), (tag, "a score past the last document")


def test_head_out_without_documents_writes_nothing(pkg):
    for lte in (0, 2):
        c = dict(R.head_cases(256, lte)[1], split=lte == 2)
        out, score = _head_out(pkg, c, n_docs=0)
        assert (out == SENTINEL).all() and (score is None or (score == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------------------------
# rows_out
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rows_x(X, split):
    torch = _torch()
    return torch.from_numpy(_encode_split(X, R.LTE_SPLIT_SCALE)).cuda() if split else _f(X)


def _rows_out(pkg, **kw):
    torch = _torch()
    a = pkg.capi.DebugRowsOutArgs()
    keep = []
    for k, v in kw.items():
        if hasattr(v, "data_ptr"):
            keep.append(v)
            v = v.data_ptr()
        setattr(a, k, v)
    pkg.capi.check(pkg.capi.load().ee_debug_rows_out(C.byref(a), _stream()), None, "ee_debug_rows_out")
    torch.cuda.synchronize()


@pytest.mark.parametrize("split", [False, True], ids=["f32", "split"])
@pytest.mark.parametrize("H", [128, 768, 1024])
def test_gather_cls_is_a_copy_of_the_rows(pkg, H, split):
    x_rows, out_rows, md = 100, 90, 80
    X = R.grid_rows(x_rows, H, seed=H)
    xd = _rows_x(X, split)
    for n in (0, 70):
        for with_orig in (False, True):
            rng = np.random.default_rng(n + with_orig)
            x_phys, doc_orig = rng.integers(0, x_rows, n), rng.permutation(out_rows)[:n] if with_orig else None
            out = _sent(out_rows * H)
            _rows_out(pkg, which=0, X=xd, x_rows=x_rows, H=H, split_inv=1.0 / R.LTE_SPLIT_SCALE if split else 0.0, x_phys=_i32(x_phys),
                      doc_orig=_i32(doc_orig) if with_orig else None, n_docs=_i32([n], 0), max_docs=md, out=out, out_rows=out_rows)
            want, written = R.gather_cls_ref(X, x_phys, doc_orig, out_rows)
            _expect(_words(out), _bits(want[written]), np.nonzero(written)[0], H, f"gather_cls H={H} split={split} n={n} doc_orig={with_orig}")


@pytest.mark.parametrize("split", [False, True], ids=["f32", "split"])
@pytest.mark.parametrize("T,Pv,text", [(1, 1, True), (1, 5, True), (9, 1, True), (9, 5, True), (0, 1, False), (0, 5, False)])
def test_rows_to_padded_is_the_reference_layout(pkg, T, Pv, text, split):
    """Split values are ones the planes hold exactly, so the float32 the kernel's load gives is the value itself: bit equality in both forms."""
    B = 3
    for H in (128, 1024):
        if text:
            text_dst, ntext, doc_off, rows = R.padded_case(T, Pv)
            assert (text_dst < 0).any()
        else:
            text_dst, ntext, doc_off, rows = None, None, np.arange(B) * Pv, B * Pv
        X = R.grid_rows(rows + 2, H, seed=T + Pv)
        out = _sent(B * (T + Pv) * H)
        _rows_out(pkg, which=1, X=_rows_x(X, split), x_rows=rows + 2, H=H, split_inv=1.0 / R.LTE_SPLIT_SCALE if split else 0.0, B=B, T=T, Pv=Pv,
                  text_dst=_i32(text_dst) if text else None, ntext=_i32(ntext) if text else None, doc_off=_i32(doc_off), out=out, out_rows=B * (T + Pv))
        want = R.rows_to_padded_ref(X, B, T, Pv, text_dst, ntext, doc_off)
        _expect(_words(out), _bits(want), np.arange(B * (T + Pv)), H, f"rows_to_padded T={T} Pv={Pv} H={H} split={split}")


def test_indices_outside_the_buffers_are_refused(pkg):
    """What the hooks can only decide on host copies of the caller's device arrays: refused with a message, nothing launched."""
    c = dict(R.head_cases(128, 0)[1], split=False)
    c["gather"] = np.array([0, 1, c["in_rows"], 2])
    with pytest.raises(Exception, match=r"gather\[2\] = 7 outside \[0, 7 rows\)"):
        _head_out(pkg, c)
    case = R.single_case(R.KERNELS[0], "max_confidence", 5, "random", 2)
    for change, text in ((dict(doc_orig=[0, 1, 2, 3, case["B"]]), f"doc_orig[4] = {case['B']} outside [0, B = {case['B']})"),
                         (dict(doc_off=[1, 2, 3, 4, 5, 6]), "doc_off[0] = 1, must be 0"),
                         (dict(doc_off=[0, 2, 2, 4, 5, 6]), "stage document 1 has 0 rows (or the stage more than 2^28)")):
        st = dict(case["stage"], **{k: np.asarray(v) for k, v in change.items()})
        st["n_rows"] = int(st["doc_off"][-1])
        with pytest.raises(Exception) as ei:
            _decide(pkg, dict(case, stage=st))
        assert text in str(ei.value), str(ei.value)
    X = _f(np.zeros((4, 128)))
    with pytest.raises(Exception, match=r"x_phys\[1\] = 4 outside \[0, 4 rows\)"):
        _rows_out(pkg, which=0, X=X, x_rows=4, H=128, split_inv=0.0, x_phys=_i32([0, 4]), doc_orig=None, n_docs=_i32([2], 0), max_docs=2,
                  out=_sent(4 * 128), out_rows=4)
