"""Online exit control (include/mmee.h, behind the audit's) on the MI355X against the numpy restatement of tests/controller_ref.py: the
tally and the step launches alone through their hooks; a controlled forward against the replay tool on its own concatenated dump-all table and
against the restatement, bit for bit in the position and the thresholds and equal in every count and every exit; each controlled call against
a plain audited forward given the logged thresholds; the promise on a model whose exit heads are confidently wrong; handle hygiene and the
refusals.

The hooks' inputs are integers and copies, so everything they return is compared exactly.  In the forward, the criterion of a document is
computed twice on the device -- by the decide launch and by the table kernel of the dumped-array tools -- from the same float32 row by the
same operations; a threshold is a lerp of gap midpoints of that table, so a last-place difference between the two could change a decision only
if a lerped threshold fell inside one ulp of a criterion."""
import ctypes as C

import numpy as np
import pytest

from . import audit_ref as A
from . import controller_ref as CR
from . import csf_ref
from . import ensemble_ref as ER
from . import exit_stage_ref as R
from .conftest import H256_KW, MATRIX_CASES, TINY_CASES
from .hook_util import SENTINEL, _stream, _torch

pytestmark = pytest.mark.gpu

GUARD = 4
STAGE_N = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
FIELDS = ("logits", "exit_layer", "confidence")
FRACTION = 0.5
MIN_GAP = 1e-9


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a.view(np.int32) if a.dtype == np.float32 else a


def _dev(a, dtype):
    return _torch().from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the tally launch alone
# ---------------------------------------------------------------------------------------------------------------------------------------
def _tally_case(n, seed=0, K=5, E1=4):
    """A final stage of n documents among B = n + 37 shuffled slots; rows of small integers (tied maxima are common), a NaN row on either side;
    marks that are set outside the stage too (never read there)."""
    rng = np.random.default_rng(700 + 3 * n + seed)
    B = n + 37
    stage = R.make_stage(n, B, seed=n + seed)
    o = np.asarray(stage["doc_orig"], np.int64)
    assert len(np.unique(o)) == n and (n < 3 or not np.array_equal(o, np.sort(o)))
    pol = rng.integers(-2, 3, (n, K)).astype(np.float32) * 3.0
    out_logits = rng.integers(-2, 3, (B, K)).astype(np.float32)
    delivered = (rng.random(B) < 0.6).astype(np.int64) * rng.integers(1, 9, B)
    if n >= 3:
        pol[0, 2] = np.nan                                                   # a row without a maximum counts as K - 1, on either side
        out_logits[o[1], 0] = np.nan
        delivered[o[:3]] = 1
        pol[2] = 6.0                                                         # all tied: index 0
        out_logits[o[2]] = [1.0, 1.0, 0.0, 1.0, -1.0][:K]
    out_exit = rng.integers(0, E1 - 1, B)
    return dict(n=n, B=B, K=K, E1=E1, temp=3.0, o=o, counts=[n, int(stage["n_rows"]), 0, 0], pol=pol, out_logits=out_logits, delivered=delivered,
                out_exit=out_exit, cut=A.cut_of(0.4), seed=11 + seed, slot_base=5)


def _tally(pkg, c, **over):
    torch = _torch()
    keep = dict(pol=_dev(c["pol"], np.float32), counts=_dev(c["counts"], np.int32), o=_dev(c["o"], np.int32), delivered=_dev(c["delivered"], np.int32),
                out_logits=_dev(c["out_logits"], np.float32), out_exit=_dev(c["out_exit"], np.int32))
    words = CR.log_words(c["E1"]) - 3 - c["E1"]
    tally = torch.full((words + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
    a = pkg.capi.DebugAuditTallyArgs()
    a.pol_logits, a.pol_rows, a.K, a.B, a.E1, a.temp = keep["pol"].data_ptr(), c["n"], c["K"], c["B"], c["E1"], c["temp"]
    a.counts, a.doc_orig, a.delivered = keep["counts"].data_ptr(), keep["o"].data_ptr(), keep["delivered"].data_ptr()
    a.out_logits, a.out_exit = keep["out_logits"].data_ptr(), keep["out_exit"].data_ptr()
    a.cut, a.seed, a.slot_base, a.tally = c["cut"], c["seed"], c["slot_base"], tally.data_ptr()
    for k, v in over.items():
        setattr(a, k, v)
    pkg.capi.check(pkg.capi.load().ee_debug_audit_tally(C.byref(a), _stream()), None, "ee_debug_audit_tally")
    torch.cuda.synchronize()
    got = tally.cpu().numpy()
    assert (got[words:] == SENTINEL).all(), "a write behind the tally"
    return got[:words]


def _tally_ref(c, **over):
    k = dict(cut=c["cut"], seed=c["seed"], slot_base=c["slot_base"])
    k.update(over)
    return CR.tally(c["o"], c["pol"], c["temp"], c["delivered"], c["out_logits"], c["out_exit"], B=c["B"], E1=c["E1"], **k)


@pytest.mark.parametrize("n", STAGE_N)
def test_tally_hook_counts_what_the_restatement_counts(pkg, n):
    c = _tally_case(n)
    want = _tally_ref(c)
    got = _tally(pkg, c)
    assert np.array_equal(got, want), (n, got.tolist(), want.tolist())
    if n >= 64:                                                              # the case is a case: shadows that agree and shadows that do not
        assert 0 < want[1] < want[2:2 + c["E1"] - 1].sum() and 0 < want[0] < c["B"]
    # everybody selected; and a cut and seed under which numpy selects nobody
    assert np.array_equal(_tally(pkg, c, cut=1 << 32), _tally_ref(c, cut=1 << 32)) and _tally_ref(c, cut=1 << 32)[0] == c["B"]
    assert not A.selected(1, 12345, np.arange(c["B"]) + c["slot_base"]).any()
    got0 = _tally(pkg, c, cut=1, seed=12345)
    assert got0[0] == 0 and np.array_equal(got0, _tally_ref(c, cut=1, seed=12345))


def test_tally_hook_refusals(pkg):
    c = _tally_case(65)
    for over, match in ((dict(cut=0), r"outside \[1, 2\^32\]"), (dict(slot_base=-1), "negative"), (dict(E1=1), "2 <= E1 <= 64"), (dict(E1=65), "2 <= E1 <= 64"),
                        (dict(B=10), "n_docs"), (dict(pol_rows=3), "leave the 3 rows"), (dict(tally=None), "must not be NULL"), (dict(temp=0.0), "temp")):
        with pytest.raises(pkg.capi.MMEEError, match=match):
            _tally(pkg, c, **over)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the step launch alone
# ---------------------------------------------------------------------------------------------------------------------------------------
PATH3 = np.array([[0.93, 0.91, 0.97, 0.5], [0.71, 0.64, 0.82, 0.5], [0.33, 0.12, 0.41, 0.25]])
ENT3 = np.array([[0.05, 0.11, 0.5], [0.45, 0.38, 0.5], [1.9, 2.3, 0.5]])
STEP_CASES = {
    # name: (path, sign, alpha, gamma, p, calls, (sampled, disagree))
    "nobody_sampled": (PATH3, 1.0, 0.1, 1.0, 1.37, 4, (0, 0)),
    "crosses_zero_downward": (PATH3, 1.0, 0.1, 1.0, 0.3, 2, (7, 7)),
    "crosses_zero_upward": (PATH3, 1.0, 0.1, 1.0, -0.05, 9, (5, 0)),
    "stays_below_zero": (PATH3, 1.0, 0.1, 1.0, -0.6, 3, (6, 0)),
    "clamped_at_the_top": (PATH3, 1.0, 0.3, 2.5, 1.9, 0, (8, 0)),
    "integer_position": (PATH3, 1.0, 0.25, 4.0, 1.0, 1, (4, 2)),
    "interior": (PATH3, 1.0, 0.1, 0.7, 1.3, 5, (3, 1)),
    "two_vectors": (PATH3[[0, 2]], 1.0, 0.2, 0.5, 0.4, 6, (9, 1)),
    "entropy_below_zero": (ENT3, -1.0, 0.1, 1.0, 0.2, 0, (2, 2)),
    "entropy_interior": (ENT3, -1.0, 0.05, 0.3, 1.5, 7, (16, 3)),
}


def _f64_words(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.int64)


def _step(pkg, path, sign, alpha, gamma, state, tal, thr, log_cap=3, over=None):
    torch = _torch()
    V, E1 = path.shape
    W = CR.log_words(E1)
    words = np.concatenate([_f64_words([state[0]]), np.asarray(state[1:], np.int64)])
    bufs = dict(path=_dev(path, np.float64), state=_dev(np.concatenate([words, [SENTINEL] * GUARD]), np.int64), tally=_dev(tal, np.int64),
                thr=_dev(np.concatenate([_f64_words(thr), [SENTINEL] * GUARD]), np.int64),
                log=torch.full((log_cap * W + GUARD,), SENTINEL, dtype=torch.int64, device="cuda"))
    a = pkg.capi.DebugControllerStepArgs()
    a.path, a.V, a.E1, a.sign, a.alpha, a.gamma = bufs["path"].data_ptr(), V, E1, sign, alpha, gamma
    a.state, a.tally, a.thr, a.log, a.log_cap = bufs["state"].data_ptr(), bufs["tally"].data_ptr(), bufs["thr"].data_ptr(), bufs["log"].data_ptr(), log_cap
    for k, v in (over or {}).items():
        setattr(a, k, v)
    pkg.capi.check(pkg.capi.load().ee_debug_controller_step(C.byref(a), _stream()), None, "ee_debug_controller_step")
    torch.cuda.synchronize()
    return {k: bufs[k].cpu().numpy() for k in ("state", "thr", "log")}


@pytest.mark.parametrize("name", list(STEP_CASES))
def test_step_hook_is_the_restatement_bit_for_bit(pkg, name):
    path, sign, alpha, gamma, p, calls, (sampled, disagree) = STEP_CASES[name]
    V, E1 = path.shape
    E, W = E1 - 1, CR.log_words(E1)
    tal = np.concatenate([[sampled, disagree], [sampled] + [0] * (E - 1), [sampled - disagree] + [0] * (E - 1)]).astype(np.int64)      # all delivered at exit 0
    state = (np.float64(p), calls, calls // 2, 5 * calls, calls)
    thr = CR.thresholds(path, p, sign)
    row, after, thr_next = CR.advance(path, sign, alpha, gamma, state, tal, thr)
    got = _step(pkg, path, sign, alpha, gamma, state, tal, thr)
    want_state = np.concatenate([_f64_words([after[0]]), np.asarray(after[1:], np.int64)])
    assert np.array_equal(got["state"][:5], want_state) and (got["state"][5:] == SENTINEL).all(), (name, got["state"], want_state)
    assert np.array_equal(got["thr"][:E1], _f64_words(thr_next)) and (got["thr"][E1:] == SENTINEL).all(), (name, got["thr"][:E1].view(np.float64), thr_next)
    want_row = np.concatenate([[row["call"]], _f64_words([row["p_before"], row["p_after"]]), tal, _f64_words(thr)])
    log = got["log"]
    at = (calls % 3) * W
    assert np.array_equal(log[at:at + W], want_row), name
    rest = log.copy()
    rest[at:at + W] = SENTINEL
    assert (rest == SENTINEL).all(), (name, "a write outside the call's row of the ring")
    # what the names promise
    if name == "nobody_sampled":
        assert after[0] == p and after[2] == state[2] and np.array_equal(_f64_words(thr_next), _f64_words(thr)) and after[1] == calls + 1
    if name in ("crosses_zero_downward", "stays_below_zero"):
        assert after[0] < 0 and (thr_next[:E] == np.inf).all()
    if name == "entropy_below_zero":
        assert after[0] < 0 <= p and (thr_next[:E] == -np.inf).all()
    if name == "crosses_zero_upward":
        assert p < 0 <= after[0] and np.isfinite(thr_next).all()
    if name == "clamped_at_the_top":
        assert after[0] == V - 1 and p - gamma * (0.0 - alpha) > V - 1 and np.array_equal(thr_next[:E], (path[V - 2] + (path[V - 1] - path[V - 2]) * 1.0)[:E])
    if name == "integer_position":
        assert float(p).is_integer() and np.array_equal(thr[:E], path[1, :E]) and after[0] == 0.0 and np.array_equal(thr_next[:E], path[0, :E])
    # no log given: the state and the thresholds all the same
    got2 = _step(pkg, path, sign, alpha, gamma, state, tal, thr, over=dict(log=None, log_cap=0))
    assert np.array_equal(got2["state"], got["state"]) and np.array_equal(got2["thr"], got["thr"]) and (got2["log"] == SENTINEL).all()


def test_step_hook_refusals(pkg):
    path, sign, alpha, gamma, p, calls, _ = STEP_CASES["interior"]
    state, tal, thr = (np.float64(p), calls, 0, 0, 0), np.zeros(8, np.int64), CR.thresholds(path, p, sign)
    for over, match in ((dict(V=1), "2 <= V"), (dict(E1=1), "2 <= E1 <= 64"), (dict(sign=0.0), r"sign is \+1 or -1"), (dict(alpha=1.0), "alpha"),
                        (dict(gamma=0.0), "gamma"), (dict(gamma=float("nan")), "gamma"), (dict(thr=None), "must not be NULL"), (dict(log=None), "without a log")):
        with pytest.raises(pkg.capi.MMEEError, match=match):
            _step(pkg, path, sign, alpha, gamma, state, tal, thr, over=over)
    with pytest.raises(pkg.capi.MMEEError, match="negative"):
        _step(pkg, path, sign, alpha, gamma, (np.float64(p), -1, 0, 0, 0), tal, thr)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. the forward
# ---------------------------------------------------------------------------------------------------------------------------------------
def _shared_heads(W):
    """Every encoder exit head takes the classifier's parameters (a model whose exits share one classifier, as in tests/test_gpu_audit.py): a
    page that is hard at one exit is hard at the next, so somebody reaches the final exit."""
    W = dict(W)
    for k in list(W):
        if ".early_exits." in k:
            src = "classifier" + k[k.index(".", k.index(".early_exits.") + len(".early_exits.")):]
            if src in W and W[src].shape == W[k].shape:
                W[k] = W[src].copy()
    return W


# name -> (shape, EE_config, precision, calls T, documents per call B, text length, seed, exit heads share the classifier)
CASES = {
    "tiny_ramp": ("tiny", dict(TINY_CASES["tiny_ramp"]), "fp32", 16, 16, 16, 21, True),
    "h256_gate": ("h256", dict(MATRIX_CASES["h256_gate"][1]), "split", 6, 16, 48, 21, False),
}


class Case:
    """T calls of B different documents, the weights, and engines of max_docs = B with the K | V probe (their rows are the dump-all rows bit for bit)."""

    def __init__(self, pkg, name, weights=None):
        torch = _torch()
        shape, ee, precision, T, B, text, seed, shared = CASES[name]
        self.pkg, self.name, self.T, self.B, self.text, self.precision = pkg, name, T, B, text, precision
        self.cfg = pkg.ModelConfig.tiny(EE_config=dict(ee)) if shape == "tiny" else pkg.ModelConfig.tiny(EE_config=dict(ee), **H256_KW)
        self.W = pkg.synth.make_weights(self.cfg, seed=seed, head_gain=4.0)
        if shared:
            self.W = _shared_heads(self.W)
        if weights is not None:
            self.W = weights(self.W)
        d = pkg.synth.make_documents(self.cfg, T * B, seed=seed + 1, text_len=text, min_words=2)
        self.dev = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}
        self.E, self.K = self.cfg.exit_config.num_exits, self.cfg.num_labels
        self.engines = []

    def engine(self):
        eng = self.pkg.EarlyExitEngine(self.cfg, xprobe=False, max_docs=self.B, max_text_len=self.text, precision=self.precision)
        eng.load_weights(self.W)
        self.engines.append(eng)
        return eng

    def call(self, t):
        return {k: v[t * self.B:(t + 1) * self.B].contiguous() for k, v in self.dev.items()}

    def dump(self, eng):
        """The concatenated dump-all arrays of the T calls: (all_logits (E1,N,K), head_logits (E,N,Kh)) on the device."""
        torch = _torch()
        outs = [eng.forward(**self.call(t), dump_all=True, want_all=True, want_head=True) for t in range(self.T)]
        eng.check()
        return torch.cat([o.all_logits for o in outs], 1), torch.cat([o.head_logits for o in outs], 1)

    def close(self):
        for e in self.engines:
            e.close()


@pytest.fixture(scope="module")
def cases(pkg):
    built = {}

    def get(name):
        if name not in built:
            built[name] = Case(pkg, name)
        return built[name]

    yield get
    for c in built.values():
        c.close()


def _table(pkg, c, criterion, all_logits, head_logits):
    """(criterion table (E1,N), bad (E1,N) uint8, sign) as numpy: the device's own table, and consistency against the final exit's argmax."""
    if criterion == "gate":
        t = _np(pkg.sweep.gate_table(head_logits, all_logits[c.E]))
    else:
        t = _np(pkg.sweep.csf_table(all_logits, criterion=criterion)[0])
    am = CR.first_argmax(_np(all_logits))
    return np.ascontiguousarray(t, np.float64), (am != am[c.E][None]).astype(np.uint8), -1.0 if criterion == "entropy" else 1.0


def _path(table, sign, positions=(0.9, 0.7, 0.5, 0.3, 0.12)):
    """V vectors of gap midpoints of the table, from the conservative end of every exit's criteria to the aggressive one."""
    pos = positions if sign > 0 else tuple(1.0 - q for q in positions)
    path = np.stack([csf_ref.gap_thresholds(table, q, MIN_GAP)[0] for q in pos])
    assert np.all(sign * np.diff(path[:, :-1], axis=0) < 0)
    return path


def _controlled_run(c, eng, path, *, alpha, gamma, start, seed, fraction=FRACTION, **fw):
    eng.set_audit(fraction, seed=99)                                       # the audit's own seed is not read while a controller is set
    eng.set_controller(path, alpha=alpha, gamma=gamma, start=start, seed=seed, log_cap=64)
    assert eng.has_controller() and eng.controller_state()["position"] == start
    outs = [eng.forward(**c.call(t), **fw) for t in range(c.T)]
    eng.check()
    return outs, eng.controller_log(), eng.controller_state()


def _same_log(got, want, tag):
    """got: a ControllerLog; want: a ControllerLog or the restatement's dict.  Bits of p and of the thresholds, every count."""
    for k in ("call", "p_before", "p_after", "sampled", "disagree", "delivered", "agree", "thresholds"):
        w = want[k] if isinstance(want, dict) else getattr(want, k)
        assert np.array_equal(_bits(np.asarray(getattr(got, k))), _bits(np.asarray(w))), (tag, k, getattr(got, k), w)


FORWARD = [("tiny_ramp", "max_confidence"), ("tiny_ramp", "entropy"), ("tiny_ramp", "margin"), ("h256_gate", "gate")]


@pytest.mark.parametrize("name,criterion", FORWARD)
def test_forward_is_the_replay_and_the_restatement(cases, pkg, name, criterion):
    c = cases(name)
    eng = c.engine()
    eng.set_criterion(criterion)
    all_logits, head_logits = c.dump(eng)
    table, bad, sign = _table(pkg, c, criterion, all_logits, head_logits)
    path = _path(table, sign)
    alpha, gamma, start, seed = 0.1, 1.0, 1.7, 7                            # a fractional start: ee_set_controller computes the first call's lerp on the host
    outs, log, state = _controlled_run(c, eng, path, alpha=alpha, gamma=gamma, start=start, seed=seed)
    N, E1 = c.T * c.B, c.E + 1
    ex = np.concatenate([_np(o.exit_layer) for o in outs])
    # the replay tool on the concatenated dump, and the restatement on the same table
    if criterion == "gate":
        replay = pkg.risk.rolling_control(table, path, alpha=alpha, gamma=gamma, group_size=c.B, fraction=FRACTION, seed=seed, start=start, bad=bad)
    else:
        replay = pkg.risk.rolling_control(all_logits, path, criterion=criterion, alpha=alpha, gamma=gamma, group_size=c.B, fraction=FRACTION, seed=seed,
                                          start=start)
    r_ex, r_log, r_p = CR.rolling(table, bad, path, sign=sign, cut=A.cut_of(FRACTION), seed=seed, alpha=alpha, gamma=gamma, p0=start, G=c.B)
    assert len(log.call) == c.T and log.call.tolist() == list(range(c.T))
    _same_log(log, replay.log, (name, criterion, "forward vs replay"))
    _same_log(log, r_log, (name, criterion, "forward vs restatement"))
    assert np.array_equal(ex, _np(replay.exits)) and np.array_equal(ex, r_ex), (name, criterion, np.nonzero(ex != r_ex)[0][:8].tolist())
    assert _bits(np.float64(state["position"])) == _bits(np.float64(r_p)) == _bits(np.float64(replay.position)) and state["calls"] == c.T
    assert state["sampled"] == log.sampled.sum() and state["disagree"] == log.disagree.sum() and state["steps"] == (log.sampled > 0).sum()
    assert np.array_equal(_bits(state["thresholds"]), _bits(CR.thresholds(path, r_p, sign)))
    # the run is a run: the position moved, somebody audited left early
    print(name, criterion, "p:", np.round(log.p_after, 3).tolist(), "exits:", np.bincount(ex, minlength=E1).tolist(), "disagree:", log.disagree.tolist())
    assert len(np.unique(log.p_after)) > 1 and (ex < c.E).any() and log.delivered.sum() > 0, (log.p_after, np.bincount(ex))
    assert (CR.excess(r_log, alpha) <= CR.bound(start, gamma, alpha) + 1e-10).all()
    # the mask an output carries is the call's own: seed + t
    for t, o in enumerate(outs):
        assert np.array_equal(_np(o.audit_mask), A.mask(c.B, FRACTION, seed + t)), t
        assert log.sampled[t] == A.mask(c.B, FRACTION, seed + t).sum()
    # RollingResult.exits goes unchanged into exit_report
    if criterion != "gate":
        rep = pkg.metrics.exit_report(all_logits, pkg.sweep.final_predictions(all_logits), exits=replay.exits)
        assert np.array_equal(rep.exit_hist, np.bincount(ex, minlength=E1)) and isinstance(rep.efficiency(), dict)
    # each controlled call is, bit for bit, a plain audited forward given the logged thresholds and the call's seed; its per-exit counts are
    # audit.consistency's of that forward run with want_all
    other = c.engine()
    other.set_criterion(criterion)
    for t in (0, 1, c.T // 2, c.T - 1):
        other.set_audit(FRACTION, seed=(seed + t) & 0xFFFFFFFF)
        o = other.forward(**c.call(t), thresholds=log.thresholds[t], want_all=True)
        for f in FIELDS:
            assert np.array_equal(_bits(_np(getattr(o, f))), _bits(_np(getattr(outs[t], f)))), (name, criterion, t, f)
        rep = pkg.audit.consistency(o)
        assert np.array_equal(rep.delivered, log.delivered[t]) and np.array_equal(rep.agree, log.agree[t]), (t, rep.delivered, log.delivered[t])
        assert rep.num_samples == log.sampled[t] and rep.pooled_delivered - rep.pooled_agree == log.disagree[t]
    other.check()
    # a dump-all call in between takes no step and uses no seed
    before = eng.controller_state()
    o = eng.forward(**c.call(0), dump_all=True, want_all=True)
    assert o.audit_mask is None
    after = eng.controller_state()
    assert after["calls"] == before["calls"] and after["position"] == before["position"] and np.array_equal(after["thresholds"], before["thresholds"])
    nxt = eng.forward(**c.call(1))
    assert np.array_equal(_np(nxt.audit_mask), A.mask(c.B, FRACTION, seed + c.T))
    eng.check()


def test_an_ensemble_and_temperatures_the_tally_reads_the_row_the_decision_read(cases, pkg):
    """Under an ensemble the final decide launch reads the ensemble's rows with temperature 1, under ``temperatures=`` it scales the head's: in
    both the tally must compare what that launch wrote.  Each controlled call against a plain audited forward given the logged thresholds, and its
    counts against ``audit.consistency`` of that forward's complete columns."""
    c = cases("tiny_ramp")
    temps = np.linspace(0.6, 2.0, c.E + 1)
    path = np.repeat(np.array([0.97, 0.8, 0.6, 0.4, 0.1])[:, None], c.E + 1, axis=1)
    for tag, ensemble in (("temperatures", None), ("ensemble and temperatures", ER.random_weights(c.E + 1, c.K, seed=3))):
        eng, other = c.engine(), c.engine()
        for e in (eng, other):
            e.set_ensemble(ensemble)
        alpha, gamma, start, seed = 0.1, 1.0, 2.4, 5
        outs, log, _ = _controlled_run(c, eng, path, alpha=alpha, gamma=gamma, start=start, seed=seed, temperatures=temps)
        assert log.delivered.sum() > 0, (tag, log.delivered.sum(0), log.sampled)
        assert np.array_equal(_bits(log.thresholds[0]), _bits(CR.thresholds(path, start, 1.0)))
        for t in range(c.T):
            other.set_audit(FRACTION, seed=seed + t)
            o = other.forward(**c.call(t), thresholds=log.thresholds[t], temperatures=temps, want_all=True)
            for f in FIELDS:
                assert np.array_equal(_bits(_np(getattr(o, f))), _bits(_np(getattr(outs[t], f)))), (tag, t, f)
            rep = pkg.audit.consistency(o)
            assert np.array_equal(rep.delivered, log.delivered[t]) and np.array_equal(rep.agree, log.agree[t]), (tag, t, rep.delivered, log.delivered[t])
            assert rep.num_samples == log.sampled[t] and rep.pooled_delivered - rep.pooled_agree == log.disagree[t], (tag, t)
            want_p = CR.step(log.p_before[t], int(log.sampled[t]), int(log.disagree[t]), alpha, gamma, len(path))
            assert _bits(np.float64(log.p_after[t])) == _bits(np.float64(want_p)), (tag, t)
        assert (CR.excess(dict(sampled=log.sampled, disagree=log.disagree), alpha) <= CR.bound(start, gamma, alpha) + 1e-10).all()
        eng.check()
        other.check()


def _wrong_heads(never_predicted):
    def change(W):
        W = dict(W)
        for k in list(W):
            if k.endswith("out_proj.bias") and not k.startswith("classifier"):
                b = W[k].copy()
                b[never_predicted] += 40.0
                W[k] = b
        return W
    return change


def test_the_promise_on_a_model_whose_exit_heads_are_confidently_wrong(cases, pkg):
    base = cases("tiny_ramp")
    eng0 = base.engine()
    all_logits, _ = base.dump(eng0)
    final = CR.first_argmax(_np(all_logits)[base.E])
    label = int(np.bincount(final, minlength=base.K).argmin())
    assert (final != label).all(), "the final classifier predicts every label somewhere: pick other weights"
    c = Case(pkg, "tiny_ramp", weights=_wrong_heads(label))
    try:
        eng = c.engine()
        al, hl = c.dump(eng)
        table, bad, sign = _table(pkg, c, "max_confidence", al, hl)
        assert bad[:c.E].all() and not bad[c.E].any() and (table[:c.E] > 0.999).all()
        path = np.repeat(np.array([0.99, 0.9, 0.8, 0.7])[:, None], c.E + 1, axis=1)
        alpha, gamma, start, seed = 0.1, 1.0, 2.0, 3
        # a condition on the fixture, checked on the CPU first: the restatement goes below 0 and comes back within the T calls
        _, r_log, _ = CR.rolling(table, bad, path, sign=sign, cut=A.cut_of(FRACTION), seed=seed, alpha=alpha, gamma=gamma, p0=start, G=c.B)
        first_below = int(np.nonzero(r_log["p_after"] < 0)[0][0])
        assert (r_log["p_after"][first_below:] >= 0).any() and (r_log["sampled"] > 0).all()
        outs, log, state = _controlled_run(c, eng, path, alpha=alpha, gamma=gamma, start=start, seed=seed)
        _same_log(log, r_log, "wrong heads")
        below = log.p_before < 0
        assert below.any() and (log.p_before[np.nonzero(below)[0][0]:] >= 0).any()
        for t, o in enumerate(outs):
            ex = _np(o.exit_layer)
            if below[t]:                                                   # nobody leaves early: every threshold is +inf
                assert (ex == c.E).all() and np.isinf(log.thresholds[t, :c.E]).all() and log.disagree[t] == 0 and log.delivered[t].sum() == 0
            else:                                                          # everybody leaves at exit 0 with the wrong answer
                assert (ex == 0).all() and log.disagree[t] == log.sampled[t] and log.delivered[t, 0] == log.sampled[t]
        ex_sum = log.excess(alpha)
        assert (ex_sum <= start / gamma + 1 - alpha + 1e-10).all() and ex_sum.max() > 0, ex_sum
        assert (log.p_after >= -gamma * (1 - alpha) - 1e-12).all()
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. hygiene and refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_handle_without_a_controller_issues_the_parent_s_launches_and_bits(cases, pkg):
    c = cases("tiny_ramp")
    eng = c.engine()
    al, hl = c.dump(eng)
    table, _, sign = _table(pkg, c, "max_confidence", al, hl)
    path = _path(table, sign)
    thr = path[2]

    def run(e, **kw):
        e.profile(True)
        o = e.forward(**c.call(0), **kw)
        prof = e.profile_read()
        e.profile(False)
        return {f: _np(getattr(o, f)) for f in FIELDS}, {role: v["launches"] for role, v in prof.items()}

    never, other = c.engine(), c.engine()
    out_never, n_never = run(never, thresholds=thr)
    assert n_never["exit_decide"] == c.E + 1 and n_never.get("controller", 0) == 0
    other.set_audit(FRACTION, seed=1)
    other.set_controller(path, alpha=0.1, gamma=1.0, start=2.0, seed=1)
    out_ctl, n_ctl = run(other)                                             # position 2.0: the thresholds are path[2]'s own bits
    assert n_ctl["controller"] == 2 and {k: v for k, v in n_ctl.items() if k != "controller"} == {k: v for k, v in n_never.items() if k != "controller"}
    other.set_controller(None)
    assert not other.has_controller() and other.controller is None and other.has_audit()
    out_aud, n_aud = run(other, thresholds=thr)
    other.set_audit(None)
    out_off, n_off = run(other, thresholds=thr)
    assert n_aud == n_never and n_off == n_never
    for f in FIELDS:
        for got in (out_ctl, out_aud, out_off):
            assert np.array_equal(_bits(got[f]), _bits(out_never[f])), f
    never.check()
    other.check()


def test_refusals_say_why_and_leave_the_handle_usable(cases, pkg):
    c = cases("tiny_ramp")
    eng = c.engine()
    al, hl = c.dump(eng)
    table, _, sign = _table(pkg, c, "max_confidence", al, hl)
    path = _path(table, sign)
    thr = path[2]
    want = {f: _np(getattr(eng.forward(**c.call(0), thresholds=thr), f)) for f in FIELDS}
    kw = dict(alpha=0.1, gamma=1.0, start=2.0, seed=1)
    Err = pkg.capi.MMEEError

    def usable(controlled):
        assert eng.has_controller() == controlled
        if controlled:
            eng.set_controller(path, **kw)                                  # back to position 2.0
        o = eng.forward(**c.call(0), thresholds=None if controlled else thr)
        for f in FIELDS:
            assert np.array_equal(_bits(_np(getattr(o, f))), _bits(want[f])), f
        eng.check()

    with pytest.raises(Err, match="no audit is set"):
        eng.set_controller(path, **kw)
    usable(False)
    eng.set_audit(FRACTION, seed=1)
    # the parameters
    for over, match in ((dict(alpha=0.0), "alpha"), (dict(alpha=1.0), "alpha"), (dict(gamma=0.0), "gamma"), (dict(gamma=float("inf")), "gamma"),
                        (dict(start=-0.5), "p0"), (dict(start=4.5), "p0")):
        with pytest.raises(Err, match=match):
            eng.set_controller(path, **dict(kw, **over))
    bad_path = path.copy()
    bad_path[-1, 0] = -np.inf                                               # still falling: the entry point's own check
    with pytest.raises(Err, match="is not finite"):
        eng.set_controller(bad_path, **kw)
    with pytest.raises(ValueError, match=r"V >= 2"):
        eng.set_controller(path[:1], **kw)
    with pytest.raises(ValueError, match="towards the aggressive side"):
        eng.set_controller(path[::-1], **kw)
    with pytest.raises(ValueError, match="alpha= .* and gamma="):
        eng.set_controller(path)
    lib = pkg.capi.load()
    flat = np.ascontiguousarray(path)
    assert lib.ee_set_controller(eng._h, flat.ctypes.data_as(C.POINTER(C.c_double)), 1, 0.1, 1.0, 0.0, 0, 8) != 0 and "2 <= V" in pkg.capi.last_error(eng._h)
    assert not eng.has_controller()
    usable(False)
    # the patience criterion, the exit rules, quotas
    eng.set_criterion("patience")
    with pytest.raises(Err, match="MMEE_CRIT_PATIENCE"):
        eng.set_controller(path, **kw)
    eng.set_criterion("max_confidence")
    eng.set_patience(2)
    eng.set_exit_rule("patient_confident")
    with pytest.raises(Err, match="MMEE_RULE_STREAK / MMEE_RULE_EITHER"):
        eng.set_controller(path, **kw)
    eng.set_exit_rule("plain")
    eng.set_controller(path, **kw)
    with pytest.raises(Err, match="while a controller is set"):
        eng.set_exit_rule("patience_or_threshold")
    with pytest.raises(Err, match="a controller is set"):
        eng.set_criterion("entropy")
    with pytest.raises(Err, match="an audit is set"):
        eng.set_quotas([1] * c.E)
    with pytest.raises(Err, match="ee_set_audit: a controller is set"):
        eng.set_audit(None)
    assert eng.has_audit() and eng.audit is not None
    usable(True)
    # the forward's own arguments
    with pytest.raises(ValueError, match="on a controlled engine"):
        eng.forward(**c.call(0), thresholds=thr)
    thr_c = (C.c_double * (c.E + 1))(*thr.tolist())
    torch = _torch()
    call = c.call(0)
    out_exit = torch.empty((c.B,), dtype=torch.int32, device="cuda")
    out_logits = torch.empty((c.B, c.K), dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def raw(thr_arg, logits, flags=0):
        rc = lib.ee_forward(eng._h, p(call["input_ids"]), p(call["attention_mask"]), p(call["bbox"]), p(call["pixel_values"]), None, None, c.B, c.text, thr_arg,
                            None, flags, p(logits), p(out_exit), None, None, None, None, None, None, _stream())
        assert rc != 0
        return pkg.capi.last_error(eng._h)

    assert "thresholds are given while a controller is set" in raw(thr_c, out_logits)
    assert "out_logits is NULL while a controller is set" in raw(None, None)
    with pytest.raises(Err, match="MMEE_FLAG_STREAM_RESULTS while a controller is set"):
        eng.forward_stream(**call)
    with pytest.raises(Err, match="ee_graph_capture: a controller is set"):
        eng.capture(**{k: v.clone() for k, v in call.items()})
    usable(True)
    # captured graphs held
    eng.set_controller(None)
    eng.set_audit(None)
    cap = eng.capture(**{k: v.clone() for k, v in call.items()}, thresholds=thr)
    with pytest.raises(Err, match="ee_set_controller: the handle holds captured graphs"):
        eng.set_controller(path, **kw)
    cap.close()
    usable(False)
    # micro-batches and cascades
    mb = pkg.MicroBatchedEngine(c.cfg, xprobe=False, micro_batches=2, max_docs=c.B, max_text_len=c.text, precision=c.precision)
    mb.load_weights(c.W)
    with pytest.raises(ValueError, match="over micro-batches is not built"):
        mb.set_controller(path, **kw)
    mb.engines[0].set_audit(FRACTION)
    mb.engines[0].set_controller(path, **kw)
    with pytest.raises(ValueError, match="over micro-batches is not built"):
        mb.forward(**call, thresholds=thr)
    mb.close()
    eng.set_audit(FRACTION, seed=1)
    eng.set_controller(path, **kw)
    other = c.engine()
    with pytest.raises(ValueError, match="online exit control on cascade stages is not built"):
        pkg.CascadeEngine([eng, other]).forward(call)
    with pytest.raises(Err, match="no controller is set"):
        other.controller_log()
    usable(True)
    # learning-to-exit: the controller's own refusal (an audit alone is fine on such a handle)
    lte_cfg = pkg.ModelConfig.tiny(EE_config=dict(exits=[1, 2], encoder_layer_strategy="ramp", use_lte=True), **H256_KW)
    lte = pkg.EarlyExitEngine(lte_cfg, xprobe=False, max_docs=4, max_text_len=48, precision="split")
    lte.load_weights(pkg.synth.make_weights(lte_cfg, seed=91, head_gain=4.0))
    lte.set_audit(FRACTION, seed=1)
    with pytest.raises(Err, match="ee_set_controller: a use_lte handle"):
        lte.set_controller(np.array([[0.3, 0.3, 0.5], [0.6, 0.6, 0.5]])[::-1], **dict(kw, start=0.0))
    assert not lte.has_controller() and lte.has_audit()
    lte.close()
    # a handle without an exit below the final one has nothing to steer
    flat_cfg = pkg.ModelConfig.tiny(EE_config=dict(exits=[], encoder_layer_strategy="ramp", inference_strategy="max_confidence"))
    flat = pkg.EarlyExitEngine(flat_cfg, xprobe=False, max_docs=4, max_text_len=c.text, precision=c.precision)
    flat.load_weights(pkg.synth.make_weights(flat_cfg, seed=3))
    flat.set_audit(FRACTION, seed=1)
    with pytest.raises(Err, match=r"E1 = 1 exits, need 2 <= E1 <= 64"):
        flat.set_controller(np.array([[0.5], [0.5]]), **dict(kw, start=0.0))
    assert not flat.has_controller()
    flat.close()
    # the model wrapper passes through
    m = pkg.LayoutLMv3EEForSequenceClassification(c.cfg, weights=c.W, max_docs=c.B, max_text_len=c.text, precision=c.precision)
    m.engine.set_audit(FRACTION, seed=1)
    assert m.set_controller(path, **kw)["start"] == 2.0 and m.engine.has_controller()
    o = m.early_exit(**call, xprobe=False)
    assert np.array_equal(_np(o.exit_layer), want["exit_layer"]) and np.array_equal(_np(o.audit_mask), A.mask(c.B, FRACTION, 1))
    assert m.engine.controller_state()["calls"] == 1
    assert m.set_controller(None) is None and not m.engine.has_controller()
    m.engine.close()
