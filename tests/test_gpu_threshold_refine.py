"""The threshold refinement on the GPU (ee_threshold_refine / sweep.threshold_refine): every integer and every bit pattern against the numpy
restatement (tests/refine_ref.py: every neighbour by a full walk), at the limits of E1, N and P and across the delta kernel's document chunk;
then against code that ships -- the final vectors and all neighbours of one of them through ``threshold_search(mixtures=)`` -- and end to end
into a forward.  The seeds are chosen so that the restatement itself meets the conditions each test asserts before it compares (moves made,
thresholds raised, every status): no case passes because nothing happened."""
import numpy as np
import pytest

from . import refine_ref as RR
from .conftest import TINY_CASES
from .test_gpu_search_cost import _ragged, _table

pytestmark = pytest.mark.gpu
CHUNK = 1024                     # kRefineChunk of csrc/threshold_refine.hip: the documents of one workgroup of the delta kernel
W_ALL = [0, 16, 64, 2 ** 32 - 1]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _starts(E1, P, seed=8):
    """nobody leaves early | everybody leaves at once | random digits"""
    return np.array([[P - 1] * E1, [0] * E1, np.random.default_rng(seed).integers(0, P, E1).tolist()])


def _chains(starts, ws):
    """The cross product as threshold_refine lays it out: chain s = (start s // W, value s % W)."""
    return [(st.tolist(), int(w)) for st in np.asarray(starts) for w in ws]


def _refs(conf, correct, cost, P, chains, budgets=None, max_rounds=64):
    return [RR.refine(conf, correct, cost, P, st, w, None if budgets is None else budgets[i], max_rounds) for i, (st, w) in enumerate(chains)]


def _check(res, refs, tag=""):
    assert len(res.hits) == len(refs), tag
    assert np.array_equal(_bits(res.table), _bits(refs[0]["table"])), tag
    for s, ref in enumerate(refs):
        t = (tag, s)
        assert res.digits[s].tolist() == ref["digits"], t
        assert np.array_equal(_bits(res.thresholds[s]), _bits(ref["thresholds"])), t
        assert (int(res.hits[s]), int(res.exit_sum[s]), int(res.cost_sum[s])) == (ref["hits"], ref["exit_sum"], ref["cost_sum"]), t
        assert (int(res.rounds[s]), int(res.status[s])) == (ref["rounds"], ref["status"]), t
        assert (int(res.start_hits[s]), int(res.start_cost_sum[s])) == (ref["start_hits"], ref["start_cost_sum"]), t
        assert res.J[s] == ref["J"] and res.start_J[s] == ref["start_J"], t
        assert res.J[s] >= res.start_J[s] and (res.J[s] == res.start_J[s]) == (int(res.rounds[s]) == 0), t
    assert res.cost_sum.dtype == np.uint64 and res.digits.dtype == np.uint8 and (res.digits[:, -1] == 0).all() and (res.thresholds[:, -1] == 0.0).all(), tag


def _something_happened(refs):
    """At least one chain makes three or more moves, and at least one move RAISES a threshold (it lands on the documents' own exit)."""
    assert max(r["rounds"] for r in refs) >= 3
    assert any(p_to > p_from for r in refs for _, p_from, p_to in r["moves"])


# ---- shapes: the limits, the chunk, both cost forms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E1,N,P", [(2, 1, 2), (3, 17, 2), (7, 300, 10), (7, CHUNK + 1, 4), (24, 500, 10), (64, 64, 64)])
def test_shapes_with_unit_and_ragged_costs(pkg, E1, N, P):
    conf, correct = _table(5, E1, N)
    starts = _starts(E1, P)
    ws = W_ALL if E1 < 24 else [0, 64]                                # the restatement walks (E1 - 1) P N documents per round: fewer chains
    chains = _chains(starts, ws)
    unit = np.ascontiguousarray(np.broadcast_to(np.arange(E1)[:, None], (E1, N)))
    refs = _refs(conf, correct, None, P, chains)
    if N >= 300:
        _something_happened(refs)
    a = pkg.sweep.threshold_refine((conf, correct), num_per_exit=P, start=starts, hit_value=ws, max_rounds=64)
    _check(a, refs, "cost=None")
    assert a.num_samples == N and a.hit_value.tolist() == [w for _, w in chains]
    for cost in (unit, np.arange(E1)):                                # the unit cost given explicitly, as (E1,N) and as (E1,)
        b = pkg.sweep.threshold_refine((conf, correct), num_per_exit=P, start=starts, hit_value=ws, max_rounds=64, cost=cost)
        for f in ("table", "digits", "thresholds", "hits", "exit_sum", "cost_sum", "rounds", "status", "start_hits", "start_cost_sum"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
    # ragged costs: sums pass 2^32 where N allows; the hit values in the costs' own scale
    rag = _ragged(E1, N)
    ws = [0, 10 ** 7, 10 ** 8, 2 ** 32 - 1] if E1 < 24 else [10 ** 8]
    chains = _chains(starts, ws)
    refs = _refs(conf, correct, rag, P, chains)
    if N >= 300:
        _something_happened(refs)
    if N >= 500:
        assert max(r["start_cost_sum"] for r in refs) > 2 ** 32
    _check(pkg.sweep.threshold_refine((conf, correct), num_per_exit=P, start=starts, hit_value=ws, max_rounds=64, cost=rag), refs, "ragged")


def test_default_start_is_nobody_leaves_early(pkg):
    conf, correct = _table(5, 7, 300)
    ref = RR.refine(conf, correct, None, 10, [9] * 7, 8)
    assert ref["rounds"] >= 3 and ref["start_cost_sum"] == 6 * 300    # every document runs to the final exit
    res = pkg.sweep.threshold_refine((conf, correct), hit_value=8)
    _check(res, [ref])


def test_strict_compare_on_a_rounded_table_with_a_constant_row_and_wild_costs(pkg):
    """Two decimals and 40 percentiles of 300 values: duplicated percentile values and many confidences EQUAL to a threshold; one exit row
    constant (all its percentiles equal, nobody beats them); a cost that is not monotone in e, over the whole 32 bits."""
    E1, N, P = 7, 300, 40
    conf, correct = _table(5, E1, N)
    conf = np.round(conf, 2)
    conf[3] = 0.5
    cost = np.random.default_rng(99).integers(0, 2 ** 32, (E1, N))
    table = RR.R.percentile_table(conf, P)
    assert any(len(set(table[e])) < P for e in (0, 1, 2, 4, 5)) and (conf[:E1 - 1, :, None] == table[:E1 - 1, None, :]).sum() > 50
    assert cost.max() >= 2 ** 31 and not (np.diff(cost.astype(np.int64), axis=0) >= 0).all()
    starts = np.concatenate([_starts(E1, P), _starts(E1, P, seed=9)[2:]])
    ws = [0, 1, 2 ** 28, 2 ** 31, 2 ** 32 - 1]
    chains = _chains(starts, ws)
    refs = _refs(conf, correct, cost, P, chains)
    _something_happened(refs)
    _check(pkg.sweep.threshold_refine((conf, correct), num_per_exit=P, start=starts, hit_value=ws, max_rounds=64, cost=cost), refs)
    # the same table with the plain exit-index cost
    ws = [0, 8, 16, 64]
    refs = _refs(conf, correct, None, P, _chains(starts, ws))
    _something_happened(refs)
    _check(pkg.sweep.threshold_refine((conf, correct), num_per_exit=P, start=starts, hit_value=ws, max_rounds=64), refs, "unit")


# ---- budgets, statuses, max_rounds ---------------------------------------------------------------------------------------------------------------
def test_budgets_and_every_status(pkg):
    E1, N, P = 7, 300, 10
    conf, correct = _table(5, E1, N)
    rag = _ragged(E1, N)
    UP, DOWN = 10 ** 8, 10 ** 7                                       # hit values at which the chains go up / come down for several rounds
    free_up = RR.refine(conf, correct, rag, P, [0] * E1, UP)          # wants to pay for accuracy
    free_down = RR.refine(conf, correct, rag, P, [P - 1] * E1, DOWN)
    assert free_up["rounds"] >= 3 and free_down["rounds"] >= 3 and free_up["cost_sum"] > free_up["start_cost_sum"]
    starts = np.array([[0] * E1, [0] * E1, [0] * E1, [P - 1] * E1, [P - 1] * E1, [P - 1] * E1])
    ws = np.array([UP] * 3 + [DOWN] * 3)
    budgets = [(free_up["start_cost_sum"] + free_up["cost_sum"]) // 2,         # in the way
               free_up["start_cost_sum"],                                       # equal to the start's cost_sum: the start is admissible
               free_up["start_cost_sum"] - 1,                                   # below it: status 2, the outputs are the start's
               free_down["start_cost_sum"], free_down["start_cost_sum"] - 1, 2 ** 62]
    chains = [(st.tolist(), int(w)) for st, w in zip(starts, ws)]
    refs = _refs(conf, correct, rag, P, chains, budgets)
    assert [r["status"] for r in refs] == [0, 0, 2, 0, 2, 0]
    assert refs[0]["cost_sum"] <= budgets[0] < free_up["cost_sum"] and refs[0]["rounds"] >= 1
    assert refs[3]["rounds"] >= 3 and refs[5]["digits"] == free_down["digits"]
    for s in (2, 4):
        assert refs[s]["rounds"] == 0 and refs[s]["digits"][:E1 - 1] == starts[s][:E1 - 1].tolist() and refs[s]["cost_sum"] == refs[s]["start_cost_sum"]
    # one call of four chains, two starts x two hit values, each with its own budget
    res = pkg.sweep.threshold_refine((conf, correct), num_per_exit=P, start=starts[[0, 3]], hit_value=[UP, DOWN], max_rounds=64, cost=rag,
                                     budget=[budgets[0], 2 ** 62, 2 ** 62, budgets[3]])
    _check(res, [refs[0], RR.refine(conf, correct, rag, P, [0] * E1, DOWN), RR.refine(conf, correct, rag, P, [P - 1] * E1, UP), refs[3]], "mixed")
    for s, (st, w) in enumerate(chains):
        one = pkg.sweep.threshold_refine((conf, correct), num_per_exit=P, start=np.array([st]), hit_value=w, max_rounds=64, cost=rag, budget=budgets[s])
        _check(one, [refs[s]], f"chain {s}")
    # budget_mean is the same budget divided by N
    bm = pkg.sweep.threshold_refine((conf, correct), num_per_exit=P, start=starts[:1], hit_value=UP, max_rounds=64, cost=rag,
                                    budget_mean=(budgets[0] + 0.5) / N)
    _check(bm, [refs[0]], "budget_mean")
    # status 1: max_rounds = 1 is exactly one step of the restatement
    first = RR.refine(conf, correct, rag, P, [P - 1] * E1, DOWN, max_rounds=1)
    assert first["status"] == 1 and first["rounds"] == 1 and first["moves"] == free_down["moves"][:1]
    res = pkg.sweep.threshold_refine((conf, correct), num_per_exit=P, hit_value=DOWN, max_rounds=1, cost=rag)
    _check(res, [first], "max_rounds=1")
    # ... and a chain that moved in every round ends with 1 even where nothing would follow
    last = RR.refine(conf, correct, rag, P, [P - 1] * E1, DOWN, max_rounds=free_down["rounds"])
    assert last["status"] == 1 and last["digits"] == free_down["digits"]
    _check(pkg.sweep.threshold_refine((conf, correct), num_per_exit=P, hit_value=DOWN, max_rounds=free_down["rounds"], cost=rag), [last], "exact")
    assert {r["status"] for r in refs} | {first["status"]} == {0, 1, 2}


# ---- a chain does not depend on its company, on the stream or on the unit ----------------------------------------------------------------------------
def test_one_chain_alone_and_among_65(pkg):
    E1, N, P = 24, 500, 10
    conf, correct = _table(5, E1, N)
    rng = np.random.default_rng(17)
    starts = rng.integers(0, P, (65, E1))
    starts[40] = starts[7]                                            # a duplicate chain
    ref = RR.refine(conf, correct, None, P, starts[7].tolist(), 64)
    assert ref["rounds"] >= 3
    alone = pkg.sweep.threshold_refine((conf, correct), num_per_exit=P, start=starts[7:8], hit_value=64, max_rounds=64)
    _check(alone, [ref], "alone")
    crowd = pkg.sweep.threshold_refine((conf, correct), num_per_exit=P, start=starts, hit_value=64, max_rounds=64)
    assert len(crowd.hits) == 65 and len(set(map(bytes, crowd.digits))) > 1 and len(set(crowd.rounds.tolist())) > 1       # the chains differ
    for f in ("digits", "thresholds", "hits", "exit_sum", "cost_sum", "rounds", "status", "start_hits", "start_cost_sum"):
        assert np.array_equal(getattr(crowd, f)[7], getattr(alone, f)[0]), f
        assert np.array_equal(getattr(crowd, f)[40], getattr(crowd, f)[7]), f
    front = crowd.front()
    assert front == sorted(front, key=lambda i: int(crowd.cost_sum[i])) and (np.diff(crowd.hits[front]) > 0).all()
    for i in range(65):                                               # nobody dominates a front entry; everybody else is dominated or tied
        dominated = any((crowd.cost_sum[j] <= crowd.cost_sum[i] and crowd.hits[j] >= crowd.hits[i]) and
                        (crowd.cost_sum[j] < crowd.cost_sum[i] or crowd.hits[j] > crowd.hits[i] or j < i) for j in range(65) if j != i)
        assert dominated == (i not in front), i


def test_scaling_the_unit_changes_nothing(pkg):
    E1, N, P = 7, 300, 10
    conf, correct = _table(5, E1, N)
    rag = _ragged(E1, N) % 1000 + np.arange(E1)[:, None] * 50
    starts = _starts(E1, P)
    ws = np.array([0, 1000, 10000])
    base_ref = _refs(conf, correct, rag, P, _chains(starts, ws))
    _something_happened(base_ref)
    budget = np.array([r["start_cost_sum"] + 2000 for r in base_ref])
    a = pkg.sweep.threshold_refine((conf, correct), num_per_exit=P, start=starts, hit_value=ws, cost=rag, budget=budget, max_rounds=64)
    _check(a, _refs(conf, correct, rag, P, _chains(starts, ws), budget.tolist()), "x1")
    b = pkg.sweep.threshold_refine((conf, correct), num_per_exit=P, start=starts, hit_value=ws * 1237, cost=rag * 1237, budget=budget * 1237, max_rounds=64)
    assert np.array_equal(a.digits, b.digits) and np.array_equal(a.rounds, b.rounds) and np.array_equal(a.status, b.status)
    assert np.array_equal(a.hits, b.hits) and np.array_equal(a.cost_sum * np.uint64(1237), b.cost_sum) and [j * 1237 for j in a.J] == b.J


def test_two_streams_give_equal_bits(pkg):
    import torch
    E1, N, P = 24, 500, 10
    conf, correct = _table(5, E1, N)
    starts = np.random.default_rng(4).integers(0, P, (16, E1))
    cf, cr = torch.from_numpy(conf).cuda(), torch.from_numpy(correct).cuda()
    torch.cuda.synchronize()
    out = []
    for _ in range(2):
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            out.append(pkg.sweep.threshold_refine((cf, cr), num_per_exit=P, start=starts, hit_value=[16, 64], max_rounds=64))
    assert max(out[0].rounds) >= 3
    for f in ("table", "digits", "thresholds", "hits", "exit_sum", "cost_sum", "rounds", "status", "start_hits", "start_cost_sum"):
        assert np.array_equal(getattr(out[0], f), getattr(out[1], f)), f


def test_entropy_runs_negated_and_comes_back_real(pkg):
    """The logits form with the '<' criterion: the chains run on the negated table and the thresholds come back negated, exactly."""
    rng = np.random.default_rng(12)
    E1, N, K = 5, 200, 6
    logits = rng.normal(size=(E1, N, K)) * np.linspace(1.0, 3.0, E1)[:, None, None]
    refs = rng.integers(0, K, N)
    table, correct = pkg.sweep.csf_table(logits, refs, criterion="entropy", as_csf=True)
    starts = _starts(E1, 6)
    a = pkg.sweep.threshold_refine(logits, refs, criterion="entropy", num_per_exit=6, start=starts, hit_value=[2, 8])
    b = pkg.sweep.threshold_refine((table, correct), num_per_exit=6, start=starts, hit_value=[2, 8])
    assert max(a.rounds) >= 1 and np.array_equal(a.digits, b.digits) and np.array_equal(a.hits, b.hits)
    assert np.array_equal(_bits(a.thresholds), _bits(-b.thresholds)) and np.array_equal(_bits(a.table), _bits(-b.table))
    _check(b, _refs(table.cpu().numpy(), correct.cpu().numpy(), None, 6, _chains(starts, [2, 8])))


# ---- against code that ships: the search scores the same vectors ---------------------------------------------------------------------------------------
def test_final_vectors_and_all_neighbours_through_the_search(pkg):
    E1, N, P = 7, 300, 10
    conf, correct = _table(5, E1, N)
    rag = _ragged(E1, N)
    starts = _starts(E1, P)
    ws = [10 ** 7, 10 ** 8]
    res = pkg.sweep.threshold_refine((conf, correct), num_per_exit=P, start=starts, hit_value=ws, max_rounds=64, cost=rag)
    assert max(res.rounds) >= 3 and (res.status == 0).all()
    got = pkg.sweep.threshold_search((conf, correct), num_per_exit=P, mixtures=res.digits, semantics="policy", cost=rag, want_all=True)
    assert np.array_equal(_bits(got.table), _bits(res.table))
    assert np.array_equal(np.rint(got.accuracy.cpu().numpy() * N).astype(np.int64), res.hits)
    assert np.array_equal(np.rint(got.mean_exit.cpu().numpy() * N).astype(np.int64), res.exit_sum)
    assert np.array_equal(got.cost_sum.cpu().numpy().view(np.uint64), res.cost_sum)
    for s in range(len(res.hits)):
        assert np.array_equal(_bits(res.thresholds[s, :E1 - 1]), _bits(got.table[np.arange(E1 - 1), res.digits[s, :E1 - 1]])), s
    for i, v in enumerate(got.front_vector):                          # a front entry of that search carries the chain's threshold bits
        assert np.array_equal(_bits(got.front_thresholds[i]), _bits(res.thresholds[int(v)])), i
    # every neighbour of one finished chain, scored by the search: none is better (there is no budget: all are admissible)
    s = int(np.argmax(res.rounds))
    nb = np.repeat(res.digits[s:s + 1], (E1 - 1) * P, axis=0)
    for e in range(E1 - 1):
        nb[e * P:(e + 1) * P, e] = np.arange(P)
    sc = pkg.sweep.threshold_search((conf, correct), num_per_exit=P, mixtures=nb, semantics="policy", cost=rag, want_all=True)
    h = np.rint(sc.accuracy.cpu().numpy() * N).astype(np.int64)
    c = sc.cost_sum.cpu().numpy()
    w = int(res.hit_value[s])
    J = [w * int(h[i]) - int(c[i]) for i in range(len(h))]
    assert max(J) == res.J[s] and len(set(J)) > 10
    # and with a budget: of the admissible ones none is better, although a better one exists outside it
    assert res.cost_sum[3] > res.start_cost_sum[3] and res.rounds[3] >= 3                     # chain 3 = (everybody leaves at once, 10^8) goes up
    budget = (int(res.start_cost_sum[3]) + int(res.cost_sum[3])) // 2
    capped = pkg.sweep.threshold_refine((conf, correct), num_per_exit=P, start=np.array([[0] * E1]), hit_value=10 ** 8, max_rounds=64, cost=rag,
                                        budget=budget)
    assert capped.status[0] == 0 and capped.rounds[0] >= 1 and capped.cost_sum[0] <= budget
    nb = np.repeat(capped.digits[:1], (E1 - 1) * P, axis=0)
    for e in range(E1 - 1):
        nb[e * P:(e + 1) * P, e] = np.arange(P)
    sc = pkg.sweep.threshold_search((conf, correct), num_per_exit=P, mixtures=nb, semantics="policy", cost=rag, want_all=True)
    h = np.rint(sc.accuracy.cpu().numpy() * N).astype(np.int64)
    c = sc.cost_sum.cpu().numpy()
    J = [10 ** 8 * int(h[i]) - int(c[i]) for i in range(len(h))]
    inside = [J[i] for i in range(len(J)) if int(c[i]) <= budget]
    assert max(inside) == capped.J[0] and max(J) > capped.J[0]


def _front_start(sr, i):
    return np.array([sr.digits(sr.front_vector[i]) + [0]])


def test_a_search_result_as_the_start(pkg):
    """The front of a sampled cost search, refined at the front's own trade-offs: no chain ends below its start, and some end above."""
    E1, N, P = 24, 500, 10
    conf, correct = _table(5, E1, N)
    sr = pkg.sweep.threshold_search((conf, correct), num_per_exit=P, mixtures=3000, seed=42, semantics="policy", cost=np.arange(E1))
    ws = pkg.sweep.front_hit_values(sr)[:4]
    F = len(sr.front_vector)
    assert F >= 3 and len(ws) >= 2
    res = pkg.sweep.threshold_refine((conf, correct), num_per_exit=P, start=sr, hit_value=ws, max_rounds=64, cost=np.arange(E1))
    assert len(res.hits) == F * len(ws)
    assert res.start_hits.tolist() == np.repeat(sr.front_hits, len(ws)).tolist()
    assert res.start_cost_sum.tolist() == np.repeat(sr.front_cost_sum, len(ws)).tolist()
    assert all(j >= j0 for j, j0 in zip(res.J, res.start_J)) and max(res.rounds) >= 3
    s = int(np.argmax(res.rounds))
    st, w = _front_start(sr, s // len(ws)), int(ws[s % len(ws)])     # the chain that moved most, alone and against the restatement
    alone = pkg.sweep.threshold_refine((conf, correct), num_per_exit=P, start=st, hit_value=w, max_rounds=64)
    _check(alone, [RR.refine(conf, correct, None, P, st[0].tolist(), w, max_rounds=64)], "front start")
    assert np.array_equal(alone.digits[0], res.digits[s]) and int(alone.hits[0]) == int(res.hits[s])
    other = pkg.sweep.threshold_search((conf[:, ::-1].copy(), correct), num_per_exit=P, mixtures=50, semantics="policy", cost=np.arange(E1))
    with pytest.raises(ValueError, match="bit for bit"):
        pkg.sweep.threshold_refine((conf * 0.5, correct), num_per_exit=P, start=other, hit_value=3)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_into_a_forward(pkg):
    """dump-all -> csf_table -> threshold_refine -> select -> forward(thresholds=): the forward's exits and correct documents are the chain's."""
    import torch
    cfg = pkg.ModelConfig.tiny(EE_config=dict(TINY_CASES["tiny_ramp"]))
    W = pkg.synth.make_weights(cfg, seed=7, head_gain=4.0)
    B = 16
    docs = pkg.synth.make_documents(cfg, B, seed=11, text_len=48, min_words=3)
    t = {k: torch.from_numpy(docs[k]).cuda() for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}
    m = pkg.LayoutLMv3EEForSequenceClassification(cfg, weights=W, max_docs=B, max_text_len=48)
    dump = m.engine.forward(**t, dump_all=True, want_all=True, whole_layers=True, xprobe=False)
    al = dump.all_logits.detach().cpu().numpy().astype(np.float64)     # (E1, B, K): the rows a whole-layers forward decides on, bit for bit
    E1 = al.shape[0]
    refs = al[-1].argmax(-1)
    refs[::5] = (refs[::5] + 1) % al.shape[-1]                       # the final exit is not always right
    table, correct = pkg.sweep.csf_table(al, refs, as_csf=True)
    cost = pkg.sweep.exit_costs(cfg, docs["attention_mask"], unit=1e3)
    w = int(cost[-1].max())                                           # a correct document is worth one full-depth pass
    res = pkg.sweep.threshold_refine((table, correct), num_per_exit=4, start=_starts(E1, 4), hit_value=[0, w // 4, w], cost=cost)
    assert max(res.rounds) >= 1 and len(res.front()) >= 2
    corr = correct.cpu().numpy().astype(np.int64)
    c64 = cost.astype(np.int64)
    for kw in (dict(min_accuracy=float(res.accuracy.max())), dict(max_mean_cost=float(res.mean_cost.min())),
               dict(max_mean_cost=float(np.median(res.mean_cost)))):
        i = res.select_index(**kw)
        thr = res.select(**kw)
        assert isinstance(thr, list) and len(thr) == E1 and all(type(x) is float for x in thr)
        out = m.early_exit(**t, thresholds=thr, whole_layers=True, xprobe=False)
        ex = out.exit_layer.detach().cpu().numpy().astype(np.int64)
        assert int(ex.sum()) == int(res.exit_sum[i]) and np.bincount(ex, minlength=E1).sum() == B, (kw, ex.tolist())
        assert int(corr[ex, np.arange(B)].sum()) == int(res.hits[i]), kw
        assert int((out.logits.detach().cpu().numpy().argmax(-1) == refs).sum()) == int(res.hits[i]), kw
        assert int(c64[ex, np.arange(B)].sum()) == int(res.cost_sum[i]), kw
    m.engine.close()
