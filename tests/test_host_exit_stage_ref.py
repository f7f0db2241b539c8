"""The float64 restatement of the exit stage (tests/exit_stage_ref.py), checked without a GPU: chained exit by exit it reproduces the whole-store
restatements the project already trusts (csf_ref.scan, patience_ref.patience_exits, rule_ref.rule_exits, lte_ref.lte_exits) for every
(mode, rule, criterion) tests/test_gpu_exit_stage.py runs; its inputs are what they promise (the forced leave patterns leave, every criterion
stays at least half a gap of MIN_GAP from its threshold, the edge criteria are exact); and they can SEE a subtly wrong kernel -- every mutation
of exit_stage_ref.MUTATIONS changes an integer output or moves a float output by at least 10 times the tolerance it is held to on the GPU."""
import numpy as np
import pytest

from . import csf_ref
from . import exit_stage_ref as R
from .hook_util import SENTINEL, _encode_split

MARGIN = 10.0
CHAIN_CASES = [(k, c) for k in R.KERNELS for c in (csf_ref.CRITERIA if k[0] == R.THRESHOLD else ("max_confidence",))]
CHAIN_IDS = [f"{R.KERNEL_IDS[R.KERNELS.index(k)]}-{c}" for k, c in CHAIN_CASES]


@pytest.fixture(scope="module")
def chain():
    return R.chain_inputs()


def _ints_differ(a, b):
    """Any integer output of two decide_ref results: the leavers, the state, the next stage."""
    if not np.array_equal(a["leave"], b["leave"]) or any(not np.array_equal(x, y) for x, y in zip(a["state"], b["state"])):
        return True
    return any(not np.array_equal(np.asarray(a["next"][k]), np.asarray(b["next"][k])) for k in a["next"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# chained = whole store
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,criterion", CHAIN_CASES, ids=CHAIN_IDS)
def test_the_chained_exits_are_the_whole_store_policy(chain, kernel, criterion):
    x, table, sign, thr, width = R.chain_tables(chain, kernel, criterion)
    assert np.all(width[:-1] >= R.MIN_GAP)
    assert np.abs(table[:-1] - thr[:-1, None]).min() >= 0.5 * R.MIN_GAP           # the reference alone keeps every criterion away from its threshold
    got = R.chain_ref(chain, kernel, criterion)
    want = R.chain_whole_store(chain, kernel, criterion)
    o = chain["stage"]["doc_orig"]
    assert np.array_equal(got["exit"][o], want[o])
    rest = np.setdiff1d(np.arange(R.CHAIN_B), o)
    assert (got["exit"][rest] == -1).all()                                         # slots outside the batch are never written
    assert np.array_equal(got["logits"][o], x.astype(np.float32)[want[o], o])
    assert np.array_equal(got["conf"][o], table[want[o], o])
    hist = np.bincount(want[o], minlength=R.CHAIN_E1)
    print(R.KERNEL_IDS[R.KERNELS.index(kernel)], criterion, "leavers per exit", hist.tolist())
    assert (hist >= 20).sum() >= 3 and hist[-1] >= 20                              # several exits release documents (a streak or a run of 2 cannot at exit 0) and the final exit is reached
    for e, st in enumerate(got["steps"]):                                          # the stage arrays stay a consistent document table
        nx = st["next"]
        n = nx["n"]
        assert nx["n_doc_off"][0] == 0 and nx["n_doc_off"][n] == nx["n_rows"] and (nx["n_doc_off"][n + 1:] == SENTINEL).all()
        assert nx["sum_len_sq"] == int((np.diff(nx["n_doc_off"][:n + 1]) ** 2).sum())
    assert got["steps"][-1]["next"]["n"] == 0


def test_the_chain_inputs_are_what_they_promise(chain):
    st = chain["stage"]
    lens = np.diff(st["doc_off"])
    assert st["n"] == 1025 and lens[7] == 257 and lens[1000] == 600 and lens.min() >= 1
    assert len(set(st["doc_orig"].tolist())) == 1025 and st["doc_orig"].max() < R.CHAIN_B and not np.array_equal(st["doc_orig"], np.arange(1025))
    assert (st["x_phys"] != st["doc_off"][:-1]).mean() > 0.99
    order = np.argsort(st["x_phys"])                                               # the physical documents do not overlap
    assert (st["x_phys"][order][1:] >= (st["x_phys"] + lens)[order][:-1]).all()
    z0, z1 = R.collision_pair(3.0)
    assert z0 < z1 and np.float32(np.float64(z0) / 3.0) == np.float32(np.float64(z1) / 3.0)
    s32 = csf_ref.scaled(chain["store"], R.CHAIN_TEMPS).astype(np.float32)
    planted = np.arange(0, R.CHAIN_B, 9)
    assert (s32[1, planted].argmax(-1) == 2).all() and (chain["store"][1, planted].argmax(-1) == 5).all()
    # two long documents survive exit 0 under every kernel of the GPU test: the stride loop of the row-map expansion runs
    for kernel, criterion in CHAIN_CASES:
        nx = R.chain_ref(chain, kernel, criterion)["steps"][0]["next"]
        assert np.diff(nx["n_doc_off"][:nx["n"] + 1]).max() > 256, (kernel, criterion)


# ---------------------------------------------------------------------------------------------------------------------------------------
# single exits: the patterns are forced, the thresholds sit in gaps
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ki", range(len(R.KERNELS)), ids=R.KERNEL_IDS)
@pytest.mark.parametrize("n", R.SINGLE_N)
def test_the_single_exit_cases_leave_as_their_pattern_says(n, ki):
    for pattern, criterion, K, head in R.single_plan(n, ki):
        c = R.single_case(R.KERNELS[ki], criterion, n, pattern, K, seed=ki, head=head)
        r = R.run_case(c)
        assert np.array_equal(r["leave"], c["want"]), (pattern, criterion, K)
        assert c["gap"] >= R.MIN_GAP
        if c["mode"] != R.PATIENCE and n:
            assert np.abs(r["crit"] - c["thr"]).min() >= 0.5 * R.MIN_GAP
        if K > 1:
            assert np.array_equal(c["want"], R.pattern_mask(pattern, n, ki))
        if head and n:                                                               # the float32 yardstick of out_head_crit stays inside the rule's floor
            assert np.abs(c["head_logits"]).max() <= 1.0
            for hc in csf_ref.CRITERIA:
                err32 = np.abs(R.crit_f32(c["head_logits"], hc).astype(np.float64) - R.criterion64(c["head_logits"].astype(np.float64), hc))
                assert err32.max() < 5e-7, (hc, err32.max())
        nx = r["next"]
        assert nx["n"] == int((~c["want"]).sum()) and np.array_equal(nx["n_doc_orig"][:nx["n"]], c["stage"]["doc_orig"][~c["want"]])


def test_the_single_exit_matrix_meets_every_value():
    seen = set()
    for n in R.SINGLE_N:
        for ki in range(len(R.KERNELS)):
            for pattern, criterion, K, head in R.single_plan(n, ki):
                seen |= {("p", ki, pattern), ("c", ki, criterion), ("K", ki, K), ("h", ki, head), ("nK", n, K), ("nc", n, criterion)}
    for ki in range(len(R.KERNELS)):
        assert all(("p", ki, p) in seen for p in R.PATTERNS) and all(("c", ki, c) in seen for c in csf_ref.CRITERIA)
        assert all(("K", ki, K) in seen for K in (1, 2, 10, 17)) and ("h", ki, True) in seen and ("h", ki, False) in seen
    assert all(("nK", n, K) in seen for n in R.SINGLE_N for K in (1, 2, 10, 17))
    w = R.pattern_mask("waves_3_15", 2049)
    assert w[3 * 64:4 * 64].all() and w[15 * 64:16 * 64].all() and w[1024 + 3 * 64:1024 + 4 * 64].all() and not w.all()
    f = R.pattern_mask("first_chunk", 2049)
    assert f[:1024].all() and not f[1024:].all() and f[1024:].any()
    big = R.big_case()
    r = R.run_case(big)
    assert r["next"]["sum_len_sq"] > 1 << 32 and r["next"]["n_rows"] > 3_000_000 and big["stage"]["n_rows"] == 2049 * 1500 < 1 << 28


def test_the_edge_criteria_are_exact():
    for name, mode, criterion, z, score, val, steps in R.edge_cases():
        if mode == R.THRESHOLD:
            for temp in (1.0, 3.0):
                assert R.criterion64(csf_ref.scaled(z[None], [temp])[0], criterion)[0] == val, (name, temp)
        st = R.make_stage(1, 2)
        for thr, fires in steps:
            r = R.decide_ref(st, z, mode=mode, rule=R.PLAIN, criterion=criterion, thr=thr, temp=1.0, patience=1, exit_index=0, B=2, lte_score=score)
            assert bool(r["leave"][0]) == fires, (name, thr)
    nan = np.array([[0.3, np.nan, 1.0]], np.float32)
    for criterion in csf_ref.CRITERIA:
        for thr in (-np.inf, 0.0, np.inf):
            r = R.decide_ref(R.make_stage(1, 2), nan, mode=R.THRESHOLD, rule=R.PLAIN, criterion=criterion, thr=thr, temp=1.0, patience=1, exit_index=0, B=2)
            assert not r["leave"][0] and np.isnan(r["crit"][0])


# ---------------------------------------------------------------------------------------------------------------------------------------
# every mutation is seen by the GPU test's own inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
SEEN_IN = {                                                                           # mutation -> the test below that shows it is seen
    "carry_dropped": "scan", "wave_inclusive": "scan", "off_all_lengths": "scan", "meta_from_xphys": "scan", "sumsq_32": "scan",
    "state_dense": "state", "streak_no_reset": "state", "state_read_exit0": "state", "argmax_last": "state", "argmax_unscaled": "state",
    "ge": "strictness", "lte_le": "strictness", "margin_skip_all_max": "strictness",
    "head_tail_dropped": "head_out", "gather_ignored": "head_out", "text_dst_copied": "padded",
}


def test_every_named_fault_has_a_check():
    assert set(SEEN_IN) == set(R.MUTATIONS) and len(R.MUTATIONS) == 16


def _single_sees(mut, kernels, ns, patterns=R.PATTERNS):
    hits = 0
    for ki in kernels:
        for n in ns:
            for pattern, criterion, K, head in R.single_plan(n, ki):
                if pattern in patterns:
                    c = R.single_case(R.KERNELS[ki], criterion, n, pattern, K, seed=ki, head=head)
                    hits += _ints_differ(R.run_case(c), R.run_case(c, mut))
    return hits


def test_the_scan_faults_are_seen():
    every = range(len(R.KERNELS))
    assert _single_sees("carry_dropped", every, (1025, 2049)) >= 7 and _single_sees("carry_dropped", every, (1023, 1024)) == 0
    assert _single_sees("wave_inclusive", every, (65, 1023)) >= 7 and _single_sees("wave_inclusive", every, (64,), ("nobody",)) == 7
    assert _single_sees("off_all_lengths", every, (63, 1025)) >= 7
    assert _single_sees("meta_from_xphys", every, (1, 64, 2049)) >= 7
    assert _single_sees("sumsq_32", every, R.SINGLE_N) == 0                           # only the long documents reach 2^32
    big = R.big_case()
    assert R.run_case(big)["next"]["sum_len_sq"] != R.run_case(big, "sumsq_32")["next"]["sum_len_sq"]


def test_the_state_faults_are_seen(chain):
    stateful = [i for i, k in enumerate(R.KERNELS) if k[0] == R.PATIENCE or k[1] != R.PLAIN]
    streak = [i for i, k in enumerate(R.KERNELS) if k[1] == R.STREAK]
    agree = [i for i in stateful if i not in streak]
    for ki in stateful:
        assert _single_sees("state_dense", [ki], (65, 1025)) >= 1, ki
    for ki in streak:
        assert _single_sees("streak_no_reset", [ki], (64, 1025), ("alternating", "random")) >= 1, ki
    # exit 0 on dirty state: the streak kernels see a read; the agreement kernels see it on the adversarial state of exit0_case
    for ki in stateful:
        c = R.exit0_case(R.KERNELS[ki])
        a, b = R.run_case(c), R.run_case(c, "state_read_exit0")
        assert _ints_differ(a, b), ki
        d = R.run_case(c, state=None)                                                 # and the true answer does not depend on the state
        assert np.array_equal(a["leave"], d["leave"]) and np.array_equal(a["state"][1], d["state"][1])
    for ki in agree:                                                                  # the planted pairs of the chain: first maximum of the SCALED logits
        for mut in ("argmax_last", "argmax_unscaled"):
            got = R.chain_ref(chain, R.KERNELS[ki], "max_confidence", mut)
            ref = R.chain_ref(chain, R.KERNELS[ki], "max_confidence")
            assert not np.array_equal(got["exit"], ref["exit"]) or any(_ints_differ(x, y) for x, y in zip(got["steps"], ref["steps"])), (ki, mut)
    z0, z1 = R.collision_pair(3.0)
    z = np.array([[z0, z1]], np.float32)
    for mut, prev in (("", 0), ("argmax_last", 1), ("argmax_unscaled", 1)):
        r = R.decide_ref(R.make_stage(1, 2), z, mode=R.PATIENCE, rule=R.PLAIN, criterion="max_confidence", thr=0.5, temp=3.0, patience=1, exit_index=0,
                         B=2, mut=mut)
        assert r["state"][0][R.make_stage(1, 2)["doc_orig"][0]] == prev


def test_the_strictness_and_margin_faults_are_seen():
    seen = dict(ge=0, lte_le=0, margin_skip_all_max=0)
    for name, mode, criterion, z, score, val, steps in R.edge_cases():
        st = R.make_stage(1, 2)
        kw = dict(mode=mode, rule=R.PLAIN, criterion=criterion, temp=1.0, patience=1, exit_index=0, B=2, lte_score=score)
        for mut in seen:
            for thr, _ in steps:
                a, b = R.decide_ref(st, z, thr=thr, **kw), R.decide_ref(st, z, thr=thr, mut=mut, **kw)
                moved = abs(float(b["crit"][0]) - float(a["crit"][0]))
                seen[mut] += _ints_differ(a, b) or moved >= MARGIN * 2.0 ** -24     # a stored criterion <= 1 is held to one float32 step
    print(seen)
    assert seen["ge"] >= 6 and seen["lte_le"] >= 3 and seen["margin_skip_all_max"] >= 2


@pytest.mark.parametrize("H", [128, 384, 1024])
def test_the_head_out_cases_see_a_subtle_fault(H):
    for lte in (0, 1, 2):
        for c in R.head_cases(H, lte):
            ref = R.head_out_ref(c["x"], c["W"], c["b"], c["gather"], c["n"])
            tol = R.tolerance(np.abs(R.head_out_f32(c["x"], c["W"], c["b"], c["gather"], c["n"]).astype(np.float64) - ref).max(-1))
            assert tol.max() < 1e-5
            for mut in ("head_tail_dropped", "gather_ignored"):
                if mut == "gather_ignored" and c["gather"] is None:
                    continue
                ratio = float((np.abs(R.head_out_ref(c["x"], c["W"], c["b"], c["gather"], c["n"], mut) - ref).max(-1) / tol).max())
                print(f"H={H} n={c['n']} Ko={c['Ko']} {mut}: a row moves by {ratio:.1f} x its tolerance")
                assert ratio >= MARGIN, (mut, c["n"], ratio)
            if lte:
                if lte == 2:
                    _encode_split(c["lte_x"][:, :H], R.LTE_SPLIT_SCALE)              # asserts that the planes hold the values exactly
                s, dt = R.lte_score_ref(c["lte_x"], c["lte_w"], c["lte_b"], c["lte_gather"], c["n"])
                tol = dt / 4 + 4 * 2.0 ** -53
                assert c["lte_gather"] is None or c["gather"] is None or not np.array_equal(c["lte_gather"], c["gather"])
                for mut in ("head_tail_dropped", "gather_ignored"):
                    if mut == "gather_ignored" and c["lte_gather"] is None:
                        continue
                    moved = np.abs(R.lte_score_ref(c["lte_x"], c["lte_w"], c["lte_b"], c["lte_gather"], c["n"], mut)[0] - s)
                    assert (moved / tol).max() >= MARGIN, (mut, c["n"])


def test_the_padded_cases_see_a_copied_dropped_position():
    for T in (1, 9):
        for Pv in (1, 5):
            text_dst, ntext, doc_off, rows = R.padded_case(T, Pv)
            assert (text_dst < 0).any() and (ntext >= 0).all() and rows == (ntext + Pv).sum()
            X = R.grid_rows(rows, 128, seed=T + Pv)
            assert (np.abs(X) > 0).all()
            a = R.rows_to_padded_ref(X, 3, T, Pv, text_dst, ntext, doc_off)
            b = R.rows_to_padded_ref(X, 3, T, Pv, text_dst, ntext, doc_off, "text_dst_copied")
            assert not np.array_equal(a, b) and (a[:, :T][text_dst < 0] == 0).all()         # held to bit equality
