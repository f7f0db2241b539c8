"""Budgeted exits (include/mmee.h, at MMEE_QUOTA_*) on the MI355X against the numpy restatement of tests/quota_ref.py: the ranking step and
the quota decide alone through ee_debug_exit_quota at the wave, workgroup, decide-chunk and LDS-tile edges; the forward (eager, captured,
streamed, low-latency) on ``tiny_ramp``, the ``h256`` ramp and gate configurations, the tiny DiT and a handle with an ensemble set; and the
dumped-array tool ``quota_scan_device``.

The device's exp may differ from numpy's in the last place of float64, so the launch's float64 criteria are compared with numpy's within
1e-12 relative, and everything that is DECIDED on them -- ranks, exits, the next stage, the counts -- is compared exactly with the restatement
applied to the device's own returned criteria.  The forward is compared with the restatement on the device table (``csf_table`` / ``gate_table``)
of the same handle's dump-all forward at temperature 1; the test asserts that the table values on either side of every quota boundary differ
by more than 1e-9 (equal pages excepted, where the tie-break is the point).  Thresholds sit at midpoints of adjacent sorted criteria more than
1e-9 apart, and a CPU assertion checks that no criterion is within 1e-12 of its threshold."""
import ctypes as C

import numpy as np
import pytest

from . import csf_ref
from . import ensemble_ref as ER
from . import exit_stage_ref as R
from . import quota_ref as Q
from .conftest import DIT_EE, H256_KW, MATRIX_CASES, TINY_CASES, report_measured, sweep_ref_inputs
from .hook_util import SENTINEL, _stream, _torch

pytestmark = pytest.mark.gpu

GUARD = 4
STAGE_N = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
KS = (2, 16, 17)
TEMPS = (1.0, 3.0, 0.5)
CRITERIA = ("max_confidence", "entropy", "margin", "gate")
CRIT_CODE = dict(R.CRIT_CODE, gate=4)
SIGN = dict(csf_ref.SIGN, gate=+1)
SENT64 = np.int64(0x7FF5A5A57FA5A5A5)                  # a NaN bit pattern no kernel writes
MIN_GAP, MIN_DIST = 1e-9, 1e-12
EXIT_INDEX = 2


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


def _hook_case(n, criterion, K, temp, seed=0):
    rng = np.random.default_rng(7000 + 13 * n + 101 * CRITERIA.index(criterion) + K + seed)
    B = n + 37
    stage = R.make_stage(n, B, seed=n + K + seed)
    z = (rng.standard_normal((n, K)) * 2.0 * temp).astype(np.float32)
    head = rng.uniform(-3.0, 3.0, (n, 2)).astype(np.float32) if criterion == "gate" else None
    return dict(n=n, B=B, K=K, criterion=criterion, temp=temp, stage=stage, z=z, head=head)


def numpy_criteria(c):
    """(c_i (n,) by numpy, scaled rows (n,K) float32 = what leaves)."""
    x = csf_ref.scaled(c["z"][None], [c["temp"]])[0]
    with np.errstate(invalid="ignore", over="ignore"):
        crit = gate_score(c["head"]) if c["criterion"] == "gate" else csf_ref.csf(x, c["criterion"])
    return crit, x.astype(np.float32)


def _call(pkg, c, q, how, thr=0.0, by_pointer=0, null=(), **over):
    """One ee_debug_exit_quota call; `over`: fields of the argument block set last, as they are.  Returns every buffer, raw (numpy)."""
    torch = _torch()
    st, n, B, K, e = c["stage"], c["n"], c["B"], c["K"], EXIT_INDEX
    keep = dict(z=torch.from_numpy(np.ascontiguousarray(c["z"])).cuda(), head=None if c["head"] is None else torch.from_numpy(np.ascontiguousarray(c["head"])).cuda(),
                counts=_i32(_counts(st), 0), doc_orig=_i32(st["doc_orig"]), doc_off=_i32(st["doc_off"]), x_phys=_i32(st["x_phys"]))
    b = dict(n_counts=_sent(4), n_doc_orig=_sent(n), n_doc_off=_sent(n + 1), n_x_src=_sent(n), n_meta_src=_sent(n), out_logits=_sent(B * K), out_exit=_sent(B),
             out_conf=_sent(B), out_all_logits=_sent((e + 1) * B * K), out_all_crit=_sent((e + 1) * B), out_head_logits=_sent((e + 1) * B * 2),
             out_head_crit=_sent((e + 1) * B), rank=_sent(n))
    crit = torch.from_numpy(np.full(n + GUARD, SENT64, np.int64)).cuda()
    a = pkg.capi.DebugExitQuotaArgs()
    d = a.decide
    for k, v in dict(mode=0, rule=0, criterion=CRIT_CODE[c["criterion"]], K=K, Kh=2, thr=float(thr), temp=float(c["temp"]), patience=0, by_pointer=by_pointer,
                     exit_index=e, is_final=0, no_exit=0, B=B).items():
        setattr(d, k, v)
    d.pol_logits, d.head_logits = keep["z"].data_ptr(), None if keep["head"] is None else keep["head"].data_ptr()
    for k in ("counts", "doc_orig", "doc_off", "x_phys"):
        setattr(d, k, keep[k].data_ptr())
    for k, t in b.items():
        if k != "rank":
            setattr(d, k, None if k in null else t.data_ptr())
    a.quota, a.quota_mode, a.crit, a.rank = int(q), int(how), crit.data_ptr(), b["rank"].data_ptr()
    for k, v in over.items():
        setattr(a if k in ("quota", "quota_mode", "crit", "rank") else d, k, v)
    pkg.capi.check(pkg.capi.load().ee_debug_exit_quota(C.byref(a), _stream()), None, "ee_debug_exit_quota")
    torch.cuda.synchronize()
    out = {k: t.cpu().numpy() for k, t in b.items()}
    out["crit"] = crit.cpu().numpy()
    return out


def _rows(words, rows, width):
    idx = (np.asarray(rows, np.int64)[:, None] * width + np.arange(width)[None]).reshape(-1)
    return idx, words[idx]


def _only(words, idx, what):
    rest = words.copy()
    rest[idx] = SENTINEL
    assert (rest == SENTINEL).all(), (what, "a write outside the documents' slots")


def _check(tag, c, b, q, mode, thr, ref_crit, ref_rows):
    """Every buffer of one call: the criteria against numpy, everything decided on them against the restatement on the device's criteria."""
    st, n, B, K, e = c["stage"], c["n"], c["B"], c["K"], EXIT_INDEX
    o, sign = st["doc_orig"], SIGN[c["criterion"]]
    assert (b["crit"][n:] == SENT64).all() and (b["rank"][n:] == SENTINEL).all(), tag
    dev = b["crit"][:n].view(np.float64)
    both_nan = np.isnan(dev) & np.isnan(ref_crit)
    with np.errstate(invalid="ignore"):
        rel = np.where(both_nan, 0.0, np.abs(dev - ref_crit) / np.maximum(np.abs(ref_crit), 1e-300))
    assert np.array_equal(np.isnan(dev), np.isnan(ref_crit)) and (rel <= 1e-12).all(), (tag, float(np.nanmax(rel)) if n else 0.0)
    lv, rk, nx = Q.decide(st, dev, sign, q, mode, thr)
    assert np.array_equal(b["rank"][:n], rk), (tag, "rank", np.nonzero(b["rank"][:n] != rk)[0][:6].tolist())
    got_counts = [int(w) & 0xFFFFFFFF for w in b["n_counts"]]
    assert got_counts == _counts(nx) + [SENTINEL] * GUARD, (tag, got_counts, _counts(nx))
    for k, extra in (("n_doc_orig", 0), ("n_doc_off", 1), ("n_x_src", 0), ("n_meta_src", 0)):
        want = nx[k][:n + extra + GUARD]
        assert np.array_equal(b[k], want), (tag, k, np.nonzero(b[k] != want)[0][:6].tolist())
    idx, got = _rows(b["out_exit"], o[lv], 1)
    assert (got == e).all(), tag
    _only(b["out_exit"], idx, (tag, "out_exit"))
    # what leaves: the scaled row of exit_stage_ref, bit for bit; the confidence is (float) of the device's criterion
    idx, got = _rows(b["out_logits"], o[lv], K)
    assert np.array_equal(got, _bits(ref_rows[lv]).reshape(-1)) or np.isnan(ref_rows[lv]).any(), (tag, "out_logits")
    _only(b["out_logits"], idx, (tag, "out_logits"))
    idx, got = _rows(b["out_all_logits"], e * B + o, K)
    assert np.array_equal(got[~np.isnan(ref_rows).reshape(-1)], _bits(ref_rows).reshape(-1)[~np.isnan(ref_rows).reshape(-1)]), (tag, "out_all_logits")
    _only(b["out_all_logits"], idx, (tag, "out_all_logits"))
    want_conf = dev.astype(np.float32)
    for k, rows, want in (("out_conf", o[lv], want_conf[lv]), ("out_all_crit", e * B + o, want_conf)):
        idx, got = _rows(b[k], rows, 1)
        g = got.view(np.float32)
        assert np.array_equal(g[~np.isnan(want)], want[~np.isnan(want)]) and np.isnan(g[np.isnan(want)]).all(), (tag, k)
        _only(b[k], idx, (tag, k))
    if c["head"] is None:
        assert (b["out_head_logits"] == SENTINEL).all() and (b["out_head_crit"] == SENTINEL).all(), tag
    else:
        idx, got = _rows(b["out_head_logits"], e * B + o, 2)
        assert np.array_equal(got, _bits(c["head"]).reshape(-1)), (tag, "out_head_logits")
        _only(b["out_head_logits"], idx, (tag, "out_head_logits"))
        idx, got = _rows(b["out_head_crit"], e * B + o, 1)
        hc = gate_score(c["head"]) if c["criterion"] == "gate" else R.criterion64(c["head"].astype(np.float64), c["criterion"])
        assert (np.abs(got.view(np.float32).astype(np.float64) - hc) <= R.tolerance(np.abs(R.crit_f32(c["head"], c["criterion"]).astype(np.float64) - hc)
                                                                                      if c["criterion"] != "gate" else 1e-7)).all(), (tag, "out_head_crit")
        _only(b["out_head_crit"], idx, (tag, "out_head_crit"))
    return lv, rk, float(rel.max()) if n else 0.0


def _gap_threshold(crit, sign, position):
    """A threshold at the midpoint of a gap of more than MIN_GAP between adjacent sorted criteria, near `position` of the way up; every
    criterion more than MIN_DIST away (asserted)."""
    v = np.sort(crit[np.isfinite(crit)])
    if len(v) < 2:
        thr = (v[0] if len(v) else 0.5) - 0.125
    else:
        gaps = np.diff(v)
        ok = np.nonzero(gaps > MIN_GAP)[0]
        assert ok.size, "no gap wider than 1e-9"
        i = ok[np.abs(ok + 1 - position * len(v)).argmin()]
        thr = 0.5 * (v[i] + v[i + 1])
    assert np.abs(crit[np.isfinite(crit)] - thr).min() > MIN_DIST if len(v) else True
    return float(thr)


def _quota_values(n):
    return sorted({0, 1, max(n - 1, 0), n, n + 5, (2 * n) // 5})


@pytest.mark.parametrize("criterion", CRITERIA)
@pytest.mark.parametrize("n", STAGE_N)
def test_launch_alone_ranks_and_decides_as_the_restatement(pkg, n, criterion):
    """Every quota value at one stage size under one criterion, both modes; K, the temperature and by-value / by-pointer cycled against them so
    that the matrix meets every value of each."""
    ni, ci = STAGE_N.index(n), CRITERIA.index(criterion)
    K, temp = KS[(ni + ci) % 3], TEMPS[(ni + 2 * ci + ni // 3) % 3]
    c = _hook_case(n, criterion, K, temp)
    ref_crit, ref_rows = numpy_criteria(c)
    sign = SIGN[criterion]
    thr = _gap_threshold(ref_crit, sign, 0.6 if sign > 0 else 0.4)
    worst, seen = 0.0, set()
    for j, q in enumerate(_quota_values(n)):
        for mode in (Q.EXACT, Q.AT_LEAST):
            by_pointer = (j + mode + ni) % 2
            tag = f"quota.launch[n={n} {criterion} K={K} T={temp} q={q} {Q.MODE_NAME[mode]} ptr={by_pointer}]"
            b = _call(pkg, c, q, mode, thr=thr if mode == Q.AT_LEAST else float("nan"), by_pointer=by_pointer)
            lv, rk, rel = _check(tag, c, b, q, mode, thr, ref_crit, ref_rows)
            worst = max(worst, rel)
            seen.add(int(lv.sum()))
            if mode == Q.EXACT:
                assert lv.sum() == min(q, n)
            else:
                fired = Q.fires(ref_crit, sign, thr)
                assert lv.sum() == max(min(q, n), fired.sum()) and (lv | ~fired).all()
    assert len(seen) >= min(3, n + 1)
    report_measured(f"quota.launch[n={n},{criterion},K={K},T={temp}]", "max relative error of the float64 criteria against numpy", worst)


@pytest.mark.parametrize("n", [64, 256, 1024, 2050])
def test_launch_ties_straddling_the_quota_the_lower_slot_leaves(pkg, n):
    """Every row twice (equal rows give equal criteria, on the device and in numpy alike), at slots in no particular order: an odd quota cuts a
    pair, and the document at the lower original slot is the one that leaves."""
    for criterion in ("max_confidence", "entropy"):
        c = _hook_case(n, criterion, 16, 1.0, seed=1)
        c["z"][1::2] = c["z"][0::2]
        ref_crit, ref_rows = numpy_criteria(c)
        o = c["stage"]["doc_orig"]
        for q in (1, n // 2 + (n // 2 + 1) % 2, n - 1):
            assert q % 2 == 1
            for mode in (Q.EXACT, Q.AT_LEAST):
                thr = -1.0 if SIGN[criterion] > 0 else 1e9                       # AT_LEAST with a threshold everybody passes: nobody may stay
                b = _call(pkg, c, q, mode, thr=thr if mode == Q.AT_LEAST else 0.0, by_pointer=q % 2)
                lv, rk, _ = _check(f"quota.ties[n={n} {criterion} q={q} {Q.MODE_NAME[mode]}]", c, b, q, mode, thr, ref_crit, ref_rows)
                dev = b["crit"][:n].view(np.float64)
                assert np.array_equal(dev[0::2], dev[1::2])
                if mode == Q.AT_LEAST:
                    assert lv.all()
                    continue
                pair = lv[0::2] != lv[1::2]
                assert pair.sum() == 1                                           # exactly one pair is cut ...
                j = int(np.nonzero(pair)[0][0])
                lo, hi = (2 * j, 2 * j + 1) if o[2 * j] < o[2 * j + 1] else (2 * j + 1, 2 * j)
                assert lv[lo] and not lv[hi] and rk[lo] == q - 1 and rk[hi] == q      # ... and its lower slot leaves


@pytest.mark.parametrize("n", [65, 1025])
def test_launch_nan_rows_rank_last_and_leave_only_when_the_quota_reaches_them(pkg, n):
    for criterion in ("max_confidence", "entropy", "margin"):
        c = _hook_case(n, criterion, 17, 3.0, seed=2)
        bad = np.random.default_rng(n).permutation(n)[:5]
        c["z"][bad, 3] = np.nan
        ref_crit, ref_rows = numpy_criteria(c)
        assert np.isnan(ref_crit[bad]).all() and np.isnan(ref_crit).sum() == 5
        o = c["stage"]["doc_orig"]
        by_slot = bad[np.argsort(o[bad])]
        for q, gone in ((n - 5, 0), (n - 3, 2), (n, 5), (n + 5, 5)):
            for mode in (Q.EXACT, Q.AT_LEAST):
                thr = np.inf * SIGN[criterion]                                  # nobody fires
                b = _call(pkg, c, q, mode, thr=thr)
                lv, rk, _ = _check(f"quota.nan[n={n} {criterion} q={q} {Q.MODE_NAME[mode]}]", c, b, q, mode, thr, ref_crit, ref_rows)
                assert np.array_equal(rk[by_slot], np.arange(n - 5, n))          # last, by slot among themselves
                assert lv[by_slot].tolist() == [True] * gone + [False] * (5 - gone) and lv[~np.isnan(ref_crit)].all()


def test_launch_without_the_optional_outputs_and_its_refusals(pkg):
    c = _hook_case(257, "margin", 16, 0.5)
    ref_crit, ref_rows = numpy_criteria(c)
    null = ("out_logits", "out_conf", "out_all_logits", "out_all_crit", "out_head_logits", "out_head_crit")
    b = _call(pkg, c, 100, Q.EXACT, null=null)
    lv, rk, nx = Q.decide(c["stage"], b["crit"][:257].view(np.float64), +1, 100, Q.EXACT)
    assert np.array_equal(b["rank"][:257], rk) and np.array_equal(b["n_doc_orig"], nx["n_doc_orig"][:257 + GUARD])
    for k in null:
        assert (b[k] == SENTINEL).all(), k
    for over, match in ((dict(quota=-1), "negative"), (dict(quota_mode=0), "quota_mode"), (dict(mode=2), "mode must be 0"), (dict(rule=1), "mode must be 0"),
                        (dict(is_final=1), "is_final"), (dict(no_exit=1), "is_final"), (dict(crit=None), "crit and rank"), (dict(rank=None), "crit and rank"),
                        (dict(criterion=2), "criterion"), (dict(B=100), "n_docs")):
        with pytest.raises(pkg.capi.MMEEError, match=match):
            _call(pkg, c, 10, Q.EXACT, **over)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the forward
# ---------------------------------------------------------------------------------------------------------------------------------------
H256_RAMP = dict(MATRIX_CASES["h256_entropy_1layer"][1], inference_strategy="max_confidence")
# name -> (shape, EE_config, precision, documents, text length, ensemble)
CASES = {
    "tiny_ramp": ("tiny", dict(TINY_CASES["tiny_ramp"]), "fp32", 24, 16, False),
    "h256_ramp": ("h256", H256_RAMP, "split", 24, 48, False),
    "h256_gate": ("h256", dict(MATRIX_CASES["h256_gate"][1]), "split", 24, 48, False),
    "dit_tiny": ("dit", dict(DIT_EE), None, 24, 0, False),
    "tiny_ramp_ensemble": ("tiny", dict(TINY_CASES["tiny_ramp"]), "fp32", 24, 16, True),
}
FIELDS = ("logits", "exit_layer", "confidence")


class Case:
    """One configuration: the engine, the documents (``pairs``: documents 2j and 2j + 1 are the same page) and, per criterion, the device table
    of the engine's own dump-all forward at temperature 1."""

    def __init__(self, pkg, name, pairs=False):
        torch = _torch()
        shape, ee, precision, B, T, ens = CASES[name]
        self.pkg, self.name, self.B, self.T, self.dit, self.precision, self.ens = pkg, name, B, T, shape == "dit", precision, ens
        mk = {"tiny": lambda **kw: pkg.ModelConfig.tiny(**kw), "h256": lambda **kw: pkg.ModelConfig.tiny(**kw, **H256_KW),
              "dit": lambda **kw: pkg.ModelConfig.dit_tiny(**kw)}[shape]
        self.cfg = mk(EE_config=dict(ee))
        if self.dit:
            self.W = pkg.synth.make_weights_beit(self.cfg, seed=91, head_gain=4.0)
            docs = {"pixel_values": pkg.synth.make_documents(self.cfg, B, seed=92, text_len=8)["pixel_values"]}
        else:
            self.W = pkg.synth.make_weights(self.cfg, seed=91, head_gain=4.0)
            d = pkg.synth.make_documents(self.cfg, B, seed=92, text_len=T, min_words=2)
            docs = {k: d[k] for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}
        if pairs:
            docs = {k: np.repeat(np.ascontiguousarray(v)[:B // 2], 2, axis=0) for k, v in docs.items()}
        self.dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in docs.items()}
        self.E, self.K = self.cfg.exit_config.num_exits, self.cfg.num_labels
        self.eng = self.engine()
        self._tables = {}

    def engine(self):
        size = dict(max_docs=self.B) if self.dit else dict(max_docs=self.B, max_text_len=self.T, precision=self.precision)
        eng = self.pkg.EarlyExitEngine(self.cfg, **size)
        eng.load_weights(self.W)
        if self.ens:
            eng.set_ensemble(ER.random_weights(self.E + 1, self.K, seed=3))
        return eng

    def inputs(self):
        return {k: v.contiguous() for k, v in self.dev.items()}

    def fwd(self, eng=None, **kw):
        return (eng or self.eng).forward(**self.inputs(), whole_layers=True, **kw)

    def table(self, criterion):
        """(table (E1,B) float64 on the host, dump): the criterion of the dump-all rows by the device's table kernels."""
        if criterion not in self._tables:
            self.eng.set_quotas(None)
            self.eng.set_criterion(criterion)
            o = self.fwd(dump_all=True, want_all=True, want_head=True)
            self.eng.check()
            if criterion == "gate":
                t = self.pkg.sweep.gate_table(o.head_logits, o.all_logits[self.E])
            else:
                t = self.pkg.sweep.csf_table(o.all_logits, criterion=criterion)[0]
            t = _np(t)
            assert t.shape == (self.E + 1, self.B) and np.isfinite(t).all()
            self._tables[criterion] = (t, dict(al=_np(o.all_logits), ac=_np(o.all_crit)))
        self.eng.set_criterion(criterion)
        return self._tables[criterion]


@pytest.fixture(scope="module")
def cases(pkg):
    built = {}

    def get(name, pairs=False):
        key = (name, pairs)
        if key not in built:
            built[key] = Case(pkg, name, pairs)
        c = built[key]
        c.eng.set_quotas(None)
        c.eng.set_exit_rule("plain")
        c.eng.set_criterion("max_confidence")
        return c

    yield get
    for c in built.values():
        c.eng.close()


def quota_vectors(B, E, seed=0):
    """Three quota vectors: one with a zero, one that empties the batch before the final exit, one that leaves a rest for the final exit."""
    rng = np.random.default_rng(B + E + 1000 * seed)
    a = rng.integers(1, max(2, B // E), E)
    a[E // 2] = 0
    b = np.full(E, 1)
    b[:max(1, E - 1)] = -(-B // max(1, E - 1))                               # ceil(B / (E - 1)): everybody is gone before the last quota
    c = rng.integers(0, max(2, B // (E + 1)) + 1, E)
    c[0] = max(c[0], 1)
    return [a.tolist(), b.tolist(), c.tolist()]


def _check_rows(c, o, ex, dump, tag):
    rows = np.arange(c.B)
    got = _np(o.exit_layer)
    assert np.array_equal(got, ex), (tag, got.tolist(), ex.tolist())
    assert np.array_equal(_bits(_np(o.logits)), _bits(dump["al"][ex, rows])), tag
    assert np.array_equal(_bits(_np(o.confidence)), _bits(dump["ac"][ex, rows])), tag


FORWARD = [("tiny_ramp", "max_confidence"), ("tiny_ramp", "entropy"), ("tiny_ramp", "margin"), ("h256_ramp", "max_confidence"), ("h256_ramp", "entropy"),
           ("h256_gate", "gate"), ("h256_gate", "max_confidence"), ("dit_tiny", "max_confidence"), ("tiny_ramp_ensemble", "max_confidence"),
           ("tiny_ramp_ensemble", "margin")]


@pytest.mark.parametrize("name,criterion", FORWARD)
def test_exact_forward_stage_sizes_are_known_before_the_call(cases, name, criterion):
    c = cases(name)
    table, dump = c.table(criterion)
    sign = SIGN[criterion]
    emptied = 0
    for quotas in quota_vectors(c.B, c.E):
        sizes = Q.stage_sizes(c.B, quotas)                                       # on the host, BEFORE the call
        want_hist = [min(q, n) for q, n in zip(quotas, sizes)] + [sizes[-1]]
        gaps = Q.boundary_gaps(table, sign, quotas, Q.EXACT)
        assert (gaps > MIN_GAP).all(), (name, criterion, quotas, gaps.tolist())
        ex = Q.scan(table, sign, quotas, Q.EXACT)[0]
        o = c.fwd(quotas=quotas, quota_mode="exact")
        assert c.eng.stage_counts()["docs"] == sizes, (name, quotas)
        _check_rows(c, o, ex, dump, (name, criterion, quotas))
        assert np.bincount(_np(o.exit_layer), minlength=c.E + 1).tolist() == want_hist
        emptied += sizes[-1] == 0
        # thresholds are not read under EXACT: impossible ones change nothing
        o2 = c.fwd(thresholds=np.full(c.E + 1, -1e30 * sign))
        assert c.eng.has_quotas and np.array_equal(_np(o2.exit_layer), ex)
        c.eng.check()
    assert emptied >= 1
    c.eng.set_quotas(None)


@pytest.mark.parametrize("name", ["tiny_ramp", "h256_ramp", "dit_tiny"])
def test_equal_pages_straddling_a_quota_are_split_with_the_lower_slot_leaving(cases, name):
    c = cases(name, pairs=True)
    table, dump = c.table("max_confidence")
    assert np.array_equal(table[:, 0::2], table[:, 1::2])                        # equal pages give equal bits
    quotas = [3] * c.E if c.E * 3 < c.B else [5, 3] + [1] * (c.E - 2)
    assert all(q % 2 == 1 for q in quotas)
    ex = Q.scan(table, +1, quotas, Q.EXACT)[0]
    # the only ties are the pairs; every other neighbour across a boundary is more than 1e-9 away
    pairs_table = table[:, 0::2]
    for e in range(c.E):
        srt = np.sort(pairs_table[e])
        assert (np.diff(srt) > MIN_GAP).all(), (name, e)
    o = c.fwd(quotas=quotas)
    _check_rows(c, o, ex, dump, (name, "pairs"))
    got = _np(o.exit_layer)
    split = got[0::2] != got[1::2]
    assert split.sum() >= 1 and (got[0::2] <= got[1::2]).all()                   # a cut pair: the lower slot left first (exit 0 always cuts one)
    first = np.nonzero(split)[0]
    assert (got[1::2][first] > got[0::2][first]).all()
    assert c.eng.stage_counts()["docs"] == Q.stage_sizes(c.B, quotas)
    c.eng.check()


@pytest.mark.parametrize("name,criterion", [("tiny_ramp", "max_confidence"), ("tiny_ramp", "entropy"), ("h256_ramp", "margin"), ("h256_gate", "gate"),
                                            ("tiny_ramp_ensemble", "max_confidence")])
def test_at_least_forward(cases, name, criterion):
    c = cases(name)
    table, dump = c.table(criterion)
    sign = SIGN[criterion]
    thr, width = csf_ref.gap_thresholds(table, 0.7 if sign > 0 else 0.3, MIN_GAP)
    assert np.abs(table[:-1] - thr[:-1, None]).min() > MIN_DIST
    plain = c.fwd(thresholds=thr)
    want = {f: _np(getattr(plain, f)) for f in FIELDS}
    plain_counts = c.eng.stage_counts()["docs"]
    assert np.array_equal(want["exit_layer"], csf_ref.exits(table, thr, sign)) and len(np.unique(want["exit_layer"])) >= 2
    # all-zero quotas: the plain thresholded forward, bit for bit
    o = c.fwd(thresholds=thr, quotas=[0] * c.E, quota_mode="at_least")
    for f in FIELDS:
        assert np.array_equal(_np(getattr(o, f)), want[f]), f
    assert c.eng.stage_counts()["docs"] == plain_counts
    for quotas in quota_vectors(c.B, c.E):
        gaps = Q.boundary_gaps(table, sign, quotas, Q.AT_LEAST, thr)
        assert (gaps > MIN_GAP).all(), (name, quotas, gaps.tolist())
        ex = Q.scan(table, sign, quotas, Q.AT_LEAST, thr)[0]
        o = c.fwd(thresholds=thr, quotas=quotas, quota_mode="at_least")
        _check_rows(c, o, ex, dump, (name, criterion, quotas, "at_least"))
        docs = c.eng.stage_counts()["docs"]
        assert all(a <= b for a, b in zip(docs, Q.stage_sizes(c.B, quotas))) and all(a <= b for a, b in zip(docs, plain_counts))
        assert (ex <= Q.scan(table, sign, quotas, Q.EXACT)[0]).all() and (ex <= want["exit_layer"]).all()
    c.eng.check()
    c.eng.set_quotas(None)


@pytest.mark.parametrize("name", ["tiny_ramp", "h256_gate", "dit_tiny"])
def test_captured_replays_read_the_current_quotas_and_the_stream_carries_q_rows(cases, pkg, name):
    c = cases(name)
    table, dump = c.table("max_confidence")
    qa, qb, qc = quota_vectors(c.B, c.E)
    eng = c.engine()
    eager = {}
    for key, q in (("a", qa), ("c", qc)):
        assert (Q.boundary_gaps(table, +1, q, Q.EXACT) > MIN_GAP).all()
        o = eng.forward(**c.inputs(), whole_layers=True, quotas=q)
        eager[key] = {f: _np(getattr(o, f)) for f in FIELDS}
        assert np.array_equal(eager[key]["exit_layer"], Q.scan(table, +1, q, Q.EXACT)[0])
    assert not np.array_equal(eager["a"]["exit_layer"], eager["c"]["exit_layer"])
    eng.set_quotas(qa)
    cap = eng.capture(**{k: v.clone() for k, v in c.inputs().items()}, whole_layers=True)
    for f in FIELDS:
        assert np.array_equal(_np(getattr(cap.outputs, f)), eager["a"][f]), f
    out = cap.launch()
    for f in FIELDS:
        assert np.array_equal(_np(getattr(out, f)), eager["a"][f]), f
    eng.set_quotas(qc)                                                           # between two replays: the second one changes
    out = cap.launch()
    for f in FIELDS:
        assert np.array_equal(_np(getattr(out, f)), eager["c"][f]), f
    assert eng.stage_counts()["docs"] == Q.stage_sizes(c.B, qc)
    out = cap.launch(quotas=qa)
    assert np.array_equal(_np(out.exit_layer), eager["a"]["exit_layer"])
    # on / off and the mode are the capture's
    for args in ((None,), (qa, "at_least")):
        with pytest.raises(pkg.capi.MMEEError, match="captured graphs"):
            eng.set_quotas(*args)
    assert eng.has_quotas
    eng.check()
    cap.close()
    eng.set_quotas(None)
    cap2 = eng.capture(**{k: v.clone() for k, v in c.inputs().items()}, whole_layers=True, thresholds=2.0)
    with pytest.raises(pkg.capi.MMEEError, match="captured graphs"):
        eng.set_quotas(qa)
    with pytest.raises(ValueError, match="captured without quotas"):
        cap2.launch(quotas=qa)
    cap2.close()
    # the result stream: chunk e holds exactly q_e rows (what is left of them), known before the call
    sizes = Q.stage_sizes(c.B, qc)
    rs = eng.forward_stream(**c.inputs(), whole_layers=True, quotas=qc)
    chunks = list(rs)
    assert [len(ch.doc_index) for ch in chunks] == [min(q, n) for q, n in zip(qc, sizes)] + [sizes[-1]]
    for ch in chunks:
        assert np.all(eager["c"]["exit_layer"][ch.doc_index] == ch.exit_index)
        assert np.array_equal(ch.logits, eager["c"]["logits"][ch.doc_index]) and np.array_equal(ch.confidence, eager["c"]["confidence"][ch.doc_index])
    eng.check()
    eng.close()


def test_low_latency_and_the_probe_schedules_leave_the_same_exits(cases):
    c = cases("h256_ramp")
    table, dump = c.table("max_confidence")
    # The low-latency and X-space rows are re-associations inside the 1e-4 logit bar, and a max-softmax moves by less than the largest logit
    # change: quota vectors whose boundaries are 1e-3 wide ON THE REFERENCE TABLE (chosen by that table alone) cannot flip.  Seeds in order.
    clear = [q for seed in range(40) for q in quota_vectors(c.B, c.E, seed) if (Q.boundary_gaps(table, +1, q, Q.EXACT) > 1e-3).all()][:3]
    assert len(clear) == 3
    for quotas in clear:
        ex = Q.scan(table, +1, quotas, Q.EXACT)[0]
        o = c.fwd(quotas=quotas)
        assert np.array_equal(_np(o.exit_layer), ex)
        for kw in (dict(low_latency=True, whole_layers=True), dict(xprobe=False), dict(xprobe=True)):
            o2 = c.eng.forward(**c.inputs(), quotas=quotas, **kw)
            assert np.array_equal(_np(o2.exit_layer), ex), kw
            assert c.eng.stage_counts()["docs"] == Q.stage_sizes(c.B, quotas)
    c.eng.check()
    c.eng.set_quotas(None)


def test_quota_fractions_and_the_model_wrapper(cases, pkg):
    c = cases("tiny_ramp")
    table, dump = c.table("max_confidence")
    f = [0.1, 0.0, 0.2, 0.15, 0.05, 0.1, 0.2]
    quotas = pkg.sweep.quotas_from_fractions(c.B, f)
    o = c.fwd(quota_fractions=f)
    assert c.eng.quotas == quotas and c.eng.quota_mode == "exact"
    assert c.eng.stage_counts()["docs"] == Q.stage_sizes(c.B, quotas)
    with pytest.raises(ValueError, match="pass one"):
        c.fwd(quotas=quotas, quota_fractions=f)
    with pytest.raises(ValueError, match="quota_mode="):
        c.fwd(quota_mode="exact")
    with pytest.raises(ValueError, match="whole numbers"):
        c.eng.set_quotas([0.5] * c.E)
    with pytest.raises(ValueError, match="neither"):
        c.eng.set_quotas(quotas, mode="at_most")
    c.eng.set_quotas(None)
    assert not c.eng.has_quotas and c.eng.quotas is None


def test_refusals_say_why_and_change_nothing(cases, pkg):
    c = cases("tiny_ramp")
    eng = c.engine()
    E = c.E
    q = [2] * E
    for bad, match in (([2] * (E + 1), "exits below the final one"), ([2] * (E - 1), "exits below the final one"), ([2] * (E - 1) + [-1], r"quotas\[\d+\]=-1")):
        with pytest.raises(pkg.capi.MMEEError, match=match):
            eng.set_quotas(bad)
        assert not eng.has_quotas
    eng.set_criterion("patience")
    with pytest.raises(pkg.capi.MMEEError, match="MMEE_CRIT_PATIENCE"):
        eng.set_quotas(q)
    eng.set_criterion("max_confidence")
    for rule in ("patient_confident", "patience_or_threshold"):
        eng.set_exit_rule(rule)
        with pytest.raises(pkg.capi.MMEEError, match="MMEE_RULE_STREAK / MMEE_RULE_EITHER"):
            eng.set_quotas(q)
        eng.set_exit_rule("plain")
    assert not eng.has_quotas
    eng.set_quotas(q, mode="at_least")
    with pytest.raises(pkg.capi.MMEEError, match="while quotas are set"):
        eng.set_criterion("patience")
    with pytest.raises(pkg.capi.MMEEError, match="while quotas are set"):
        eng.set_exit_rule("patient_confident")
    assert eng.has_quotas and str(eng.exit_config.inference_strategy) == "max_confidence"
    o = eng.forward(**c.inputs(), whole_layers=True, thresholds=2.0)              # still works, as AT_LEAST with thresholds nobody passes
    assert np.bincount(_np(o.exit_layer), minlength=E + 1)[:E].tolist() == q
    eng.close()
    lte_cfg = pkg.ModelConfig.tiny(EE_config=dict(exits=[1, 2], encoder_layer_strategy="ramp", use_lte=True), **H256_KW)
    lte = pkg.EarlyExitEngine(lte_cfg, max_docs=4, max_text_len=16)
    with pytest.raises(pkg.capi.MMEEError, match="use_lte"):
        lte.set_quotas([1, 1])
    lte.close()
    mb = pkg.MicroBatchedEngine(c.cfg, max_docs=c.B, max_text_len=c.T, precision="fp32", micro_batches=2)
    with pytest.raises(ValueError, match="each rank alone"):
        mb.forward(**c.inputs(), quotas=q)
    with pytest.raises(ValueError, match="each rank alone"):
        mb.set_quotas(q)
    mb.close()


def test_a_handle_without_quotas_issues_the_launches_it_always_did(cases, pkg):
    c = cases("h256_ramp")
    table, dump = c.table("max_confidence")
    thr = np.median(table, axis=1)

    def run(eng, **kw):
        eng.profile(True)
        o = eng.forward(**c.inputs(), thresholds=thr, whole_layers=True, **kw)
        prof = eng.profile_read()
        eng.profile(False)
        return {f: _np(getattr(o, f)) for f in FIELDS}, {role: v["launches"] for role, v in prof.items()}

    never, cleared = c.engine(), c.engine()
    out_never, n_never = run(never)
    cleared.set_quotas(None)
    out_cleared, n_cleared = run(cleared)
    assert n_never == n_cleared and n_never["exit_quota_rank"] == 0 and n_never["exit_decide"] == c.E + 1
    quotas = quota_vectors(c.B, c.E)[2]
    out_q, n_q = run(cleared, quotas=quotas)
    assert n_q["exit_quota_rank"] == 2 * c.E and n_q["exit_decide"] == c.E + 1    # two launches per exit below the final one, none at it
    assert {k: v for k, v in n_q.items() if k != "exit_quota_rank"} == {k: v for k, v in n_never.items() if k != "exit_quota_rank"}
    cleared.set_quotas(None)
    out_after, n_after = run(cleared)
    assert n_after == n_never
    for f in FIELDS:
        assert np.array_equal(out_after[f], out_never[f]) and np.array_equal(out_cleared[f], out_never[f]), f
    never.close()
    cleared.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. the dumped-array tool
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic(pkg):
    store, refs = sweep_ref_inputs(seed=31, E1=7, N=5000, K=16)
    tables = {cr: _np(pkg.sweep.csf_table(store, criterion=cr)[0]) for cr in ("max_confidence", "entropy")}
    return store, refs, tables


def _same(a, b):
    return np.array_equal(a, b) or (a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]))


@pytest.mark.parametrize("mode", [Q.EXACT, Q.AT_LEAST], ids=["exact", "at_least"])
@pytest.mark.parametrize("G", [1, 7, 1024, 5000])
def test_tool_equals_the_restatement_exactly(pkg, synthetic, G, mode):
    store, refs, tables = synthetic
    for criterion in ("max_confidence", "entropy"):
        table, sign = tables[criterion], SIGN[criterion]
        thr = np.quantile(table, 0.8 if sign > 0 else 0.2, axis=1)
        frac = [0.05, 0.1, 0.0, 0.2, 0.1, 0.15]
        quotas = pkg.sweep.quotas_from_fractions(min(G, 5000), frac) if G > 1 else [0, 1, 0, 0, 1, 0]
        scan = pkg.policy.quota_scan_device(table, quotas, mode=Q.MODE_NAME[mode], thresholds=thr if mode == Q.AT_LEAST else None, group_size=G, sign=sign)
        ex, cuts = Q.scan(table, sign, quotas, mode, thr if mode == Q.AT_LEAST else None, G=G)
        assert np.array_equal(_np(scan.exits), ex), (criterion, G, int((_np(scan.exits) != ex).sum()))
        assert _same(_np(scan.cuts), cuts), (criterion, G)
        assert scan.counts().tolist() == np.bincount(ex, minlength=7).tolist()
    # the exits go unchanged into the report
    rep = pkg.metrics.exit_report(store, refs, exits=scan.exits)
    assert rep is not None


def test_tool_nan_criteria_a_short_last_group_and_the_policy(pkg, synthetic):
    store, refs, tables = synthetic
    table = tables["max_confidence"][:, :1031].copy()
    table[1, [5, 700, 1030]] = np.nan
    table[3, 5] = np.nan
    quotas = [100, 150, 0, 200, 1000, 3]
    for G in (300, 1031, 4096):
        scan = pkg.policy.quota_scan_device(table, quotas, group_size=G)
        ex, cuts = Q.scan(table, +1, quotas, Q.EXACT, G=G)
        assert np.array_equal(_np(scan.exits), ex) and _same(_np(scan.cuts), cuts), G
    pol = pkg.Policy(store[:, :1031], {"quotas": quotas, "exit_policy": "quota_policy"})
    exits_store, predictions, dist = pol.quota_policy()
    want = Q.scan(tables["max_confidence"][:, :1031], +1, quotas, Q.EXACT)[0]
    assert np.array_equal(exits_store, want) and abs(sum(dist.values()) - 1.0) < 1e-12
    assert np.array_equal(_np(predictions), store[want, np.arange(1031), :])
    with pytest.raises(ValueError, match="quotas"):
        pkg.policy.quota_scan_device(table, quotas[:-1])
    with pytest.raises(ValueError, match="needs thresholds"):
        pkg.policy.quota_scan_device(table, quotas, mode="at_least")


def test_tool_with_the_batch_as_the_group_reproduces_a_forward(cases, pkg):
    c = cases("h256_ramp")
    table, dump = c.table("max_confidence")
    quotas = quota_vectors(c.B, c.E)[2]
    o = c.fwd(quotas=quotas)
    scan = pkg.policy.quota_scan_device(table, quotas, group_size=c.B)
    assert np.array_equal(_np(scan.exits), _np(o.exit_layer))
    # ... and two batches in one table are two forwards
    both = np.concatenate([table, table[:, ::-1]], axis=1)
    scan2 = pkg.policy.quota_scan_device(both, quotas, group_size=c.B)
    assert np.array_equal(_np(scan2.exits)[:c.B], _np(o.exit_layer))
    assert np.array_equal(_np(scan2.exits)[c.B:], Q.scan(table[:, ::-1], +1, quotas, Q.EXACT)[0])
    c.eng.check()
    c.eng.set_quotas(None)


@pytest.mark.parametrize("criterion", ["max_confidence", "entropy"])
def test_thresholds_of_a_whole_table_scan_release_the_quotas_histogram(pkg, synthetic, criterion):
    """MSDNet's thresholds: the midpoints of the cuts of a one-group scan, fed to the plain thresholded scan, release exactly the scan's leavers."""
    store, refs, tables = synthetic
    table, sign = tables[criterion], SIGN[criterion]
    quotas, p, q = pkg.sweep.budget_quotas(np.arange(1.0, 8.0), 3.2, 5000)
    scan = pkg.policy.quota_scan_device(table, quotas, sign=sign)
    cuts = _np(scan.cuts)[0]
    assert (np.abs(cuts[:, 0] - cuts[:, 1]) > MIN_GAP).all()                     # no cut straddles a tie
    thr = scan.thresholds()
    assert thr.shape == (7,) and np.abs(table[:-1] - thr[:-1, None]).min() > MIN_DIST
    ex = _np(pkg.policy.criterion_scan_device(store, thr, criterion)[0])
    assert np.array_equal(ex, _np(scan.exits))
    hist = np.bincount(ex, minlength=7)
    assert hist[:6].tolist() == quotas and hist[6] == 5000 - sum(quotas)
    assert abs(float(hist @ np.arange(1.0, 8.0)) / 5000 - 3.2) < 7.0 / 5000 * 6  # the batch spends its budget up to the rounding of the quotas
