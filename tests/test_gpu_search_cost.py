"""The cost-weighted threshold search on the GPU (ee_threshold_search_cost / sweep.threshold_search(cost=)): everything against the numpy
restatement (tests/search_cost_ref.py) on integers or bit patterns -- per-vector cost sums beyond 2^32, the hits-bucket front with its tie
rule -- through both main kernels (the E1 = 7 instantiation and the run-time form, with and without a pad word in the record); with unit
costs against the exit-index search that ships; then against the policy scan and end to end into a forward."""
import numpy as np
import pytest

from . import search_cost_ref as RC
from . import search_ref as R
from .conftest import TINY_CASES

pytestmark = pytest.mark.gpu
SEM = {"reference": R.REFERENCE, "policy": R.POLICY}


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _table(seed, E1, N):
    """tests/test_gpu_search.py's synthetic confidence table (later exits surer and more often right), without its copied entries."""
    rng = np.random.default_rng(seed)
    conf = rng.beta(2.0 + np.arange(E1)[:, None] * 1.5, 2.0, (E1, N))
    correct = (rng.random((E1, N)) < np.linspace(0.3, 0.9, E1)[:, None]).astype(np.uint8)
    return conf, correct


def _ragged(E1, N):
    """cost[e][n] = 2 e w_n + 3 (e + 1): a document's weight spans six orders of magnitude, sums pass 2^32."""
    w = np.random.default_rng(1234).integers(1, 2 ** 20, N)
    e = np.arange(E1)[:, None]
    return 2 * e * w[None, :] + 3 * (e + 1)


def _check(res, ref, N, tag):
    """One cost SearchResult (want_all) against the restatement's dict: table bits, per-vector integers, the whole front."""
    assert np.array_equal(_bits(res.table), _bits(ref["table"])), tag
    assert np.array_equal(_np(res.accuracy), ref["hits"] / float(N)), tag
    assert np.array_equal(_np(res.mean_exit), ref["exit_sum"] / float(N)), tag
    assert res.cost_sum.dtype.is_floating_point is False and _np(res.cost_sum).tolist() == ref["cost_sum"], tag
    assert len(res.front_vector) == len(ref["front_vector"]), (tag, len(res.front_vector), len(ref["front_vector"]))
    assert res.front_cost_sum.dtype == np.uint64 and res.front_cost_sum.tolist() == ref["front_cost_sum"], tag
    assert res.front_exit_sum.tolist() == ref["front_exit_sum"] and res.front_hits.tolist() == ref["front_hits"], tag
    assert res.front_vector.tolist() == ref["front_vector"], tag
    assert np.array_equal(_bits(res.front_thresholds), _bits(ref["front_thresholds"])), tag
    assert np.array_equal(res.front_accuracy, np.array(ref["front_hits"]) / float(N)), tag
    assert np.array_equal(res.front_mean_cost, np.array(ref["front_cost_sum"], dtype=np.uint64) / float(N)), tag
    assert np.array_equal(res.front_mean_exit, np.array(ref["front_exit_sum"]) / float(N)), tag
    assert (np.diff(res.front_cost_sum.astype(np.float64)) > 0).all() and (np.diff(res.front_hits) > 0).all(), tag
    for i, v in enumerate(res.front_vector[:8]):
        assert res.digits(v) == ref["digits"][int(v)].tolist(), (tag, i)


# ---- the 4096-vector grid through the E1 = 7 instantiation ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid_case():
    """E1 = 7, P = 4: 4096 vectors; N = 4100 crosses the 1024-document LDS chunk (half the plain search's) four times."""
    conf, correct = _table(77, 7, 4100)
    return dict(conf=conf, correct=correct, ragged=_ragged(7, 4100), results={})


def _ragged_grid(pkg, case, semantics):
    if semantics not in case["results"]:
        ref = RC.search_cost(case["conf"], case["correct"], case["ragged"], 4, R.GRID, SEM[semantics])
        res = pkg.sweep.threshold_search((case["conf"], case["correct"]), num_per_exit=4, mixtures="grid", semantics=semantics, want_all=True,
                                         cost=case["ragged"])
        case["results"][semantics] = (res, ref)
    return case["results"][semantics]


@pytest.mark.parametrize("semantics", ["reference", "policy"])
def test_unit_cost_equals_the_exit_index_search(pkg, grid_case, semantics):
    conf, correct = grid_case["conf"], grid_case["correct"]
    E1, N = conf.shape
    kw = dict(num_per_exit=4, mixtures="grid", semantics=semantics, want_all=True)
    plain = pkg.sweep.threshold_search((conf, correct), **kw)
    assert plain.front_cost_sum is None and plain.cost_sum is None and len(plain.front_vector) >= 8
    unit = pkg.sweep.threshold_search((conf, correct), cost=np.arange(E1), **kw)
    assert unit.num_vectors == 4096 and unit.num_samples == N
    assert unit.front_cost_sum.tolist() == plain.front_exit_sum.tolist() == unit.front_exit_sum.tolist()
    assert np.array_equal(unit.front_hits, plain.front_hits) and np.array_equal(unit.front_vector, plain.front_vector)
    assert np.array_equal(_bits(unit.front_thresholds), _bits(plain.front_thresholds)) and np.array_equal(_bits(unit.table), _bits(plain.table))
    assert np.array_equal(_np(unit.cost_sum), np.rint(_np(plain.mean_exit) * N).astype(np.int64))
    assert np.array_equal(_np(unit.accuracy), _np(plain.accuracy)) and np.array_equal(_np(unit.mean_exit), _np(plain.mean_exit))
    wide = pkg.sweep.threshold_search((conf, correct), cost=np.ascontiguousarray(np.broadcast_to(np.arange(E1)[:, None], (E1, N))), **kw)
    for f in ("table", "front_thresholds", "front_vector", "front_hits", "front_exit_sum", "front_cost_sum", "front_mean_cost"):
        assert np.array_equal(getattr(unit, f), getattr(wide, f)), f
    assert np.array_equal(_np(unit.cost_sum), _np(wide.cost_sum))


@pytest.mark.parametrize("semantics", ["reference", "policy"])
def test_ragged_costs_sums_beyond_32_bits(pkg, grid_case, semantics):
    res, ref = _ragged_grid(pkg, grid_case, semantics)
    # what the case is there for, on the restatement alone
    assert len(ref["front_vector"]) >= 8 and max(ref["cost_sum"]) > 2 ** 32
    plain = R.pareto_front(ref["hits"], ref["exit_sum"], 4100 * 6 + 1)
    assert len(set(ref["front_vector"]) - set(plain[2].tolist())) >= 1      # the cost front is not the exit-index front
    _check(res, ref, 4100, semantics)


@pytest.mark.parametrize("semantics", ["reference", "policy"])
def test_non_monotone_full_range_costs(pkg, grid_case, semantics):
    cost = np.random.default_rng(99).integers(0, 2 ** 32, (7, 4100))
    ref = RC.search_cost(grid_case["conf"], grid_case["correct"], cost, 4, R.GRID, SEM[semantics])
    assert len(ref["front_vector"]) >= 4 and cost.max() >= 2 ** 31
    res = pkg.sweep.threshold_search((grid_case["conf"], grid_case["correct"]), num_per_exit=4, mixtures="grid", semantics=semantics, want_all=True,
                                     cost=cost)
    _check(res, ref, 4100, semantics)


# ---- the run-time kernel: a record without a pad word, and 23 exits ---------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", ["reference", "policy"])
def test_no_pad_word(pkg, semantics):
    """E1 = 8: E1P = E1, the record has no spare word.  3^7 = 2187 vectors (no multiple of 256), N = 700."""
    conf, correct = _table(9, 8, 700)
    cost = _ragged(8, 700)
    ref = RC.search_cost(conf, correct, cost, 3, R.GRID, SEM[semantics])
    res = pkg.sweep.threshold_search((conf, correct), num_per_exit=3, mixtures="grid", semantics=semantics, want_all=True, cost=cost)
    assert res.num_vectors == 2187
    _check(res, ref, 700, semantics)


def test_runtime_path_sampled(pkg):
    """E1 = 23, V = 3001 sampled, N = 1000: crosses the 341-document chunk twice."""
    E1, N, P, V = 23, 1000, 10, 3001
    conf, correct = _table(9, E1, N)
    cost = _ragged(E1, N)
    ref = RC.search_cost(conf, correct, cost, P, R.SAMPLED, R.POLICY, V=V, seed=42)
    res = pkg.sweep.threshold_search((conf, correct), num_per_exit=P, mixtures=V, seed=42, want_all=True, cost=cost)
    _check(res, ref, N, "sampled")
    lean = pkg.sweep.threshold_search((conf, correct), num_per_exit=P, mixtures=V, seed=42, cost=cost)
    assert lean.cost_sum is None and lean.accuracy is None            # the optional outputs left out (NULL): the sums go to the workspace
    assert lean.front_cost_sum.tolist() == ref["front_cost_sum"] and lean.front_vector.tolist() == ref["front_vector"]


def test_smallest_shape(pkg):
    conf, correct = np.array([[0.75], [0.25]]), np.array([[1], [0]], dtype=np.uint8)
    cost = np.array([[5], [7]])
    for name, sem in SEM.items():
        ref = RC.search_cost(conf, correct, cost, 2, R.SAMPLED, sem, V=1, seed=1)
        res = pkg.sweep.threshold_search((conf, correct), num_per_exit=2, mixtures=1, seed=1, semantics=name, want_all=True, cost=cost)
        _check(res, ref, 1, name)
        assert len(res.front_vector) == 1


def test_tie_rule_names_the_lower_index(pkg):
    """Every vector planted twice (rows v and v + 20 carry the same digits): equal (cost_sum, hits), and the front must name the first."""
    conf, correct = _table(21, 3, 300)
    rows = np.random.default_rng(3).integers(0, 6, (20, 3))
    mix = np.concatenate([rows, rows])
    cost = _ragged(3, 300)
    for name, sem in SEM.items():
        ref = RC.search_cost(conf, correct, cost, 6, R.MIXTURES, sem, V=40, mixtures=mix)
        a = pkg.sweep.threshold_search((conf, correct), num_per_exit=6, mixtures=mix, semantics=name, want_all=True, cost=cost)
        _check(a, ref, 300, name)
        assert len(a.front_vector) >= 2 and (a.front_vector < 20).all()
        assert np.array_equal(_np(a.cost_sum)[:20], _np(a.cost_sum)[20:])
        b = pkg.sweep.threshold_search((conf, correct), num_per_exit=6, mixtures=mix, semantics=name, want_all=True, cost=cost)
        for f in ("table", "front_thresholds", "front_vector", "front_hits", "front_exit_sum", "front_cost_sum"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        assert np.array_equal(_np(a.cost_sum), _np(b.cost_sum)) and np.array_equal(_np(a.accuracy), _np(b.accuracy))


# ---- against what ships ------------------------------------------------------------------------------------------------------------------------
def test_front_rows_through_the_policy_scan(pkg, grid_case):
    """POLICY: every reported row of the ragged case, given to ee_criterion_scan as the thresholds of a policy, reproduces its (cost_sum, hits).
    The scan wants logits: two labels whose margin criterion tanh(d / 2) is the table's value lowered by 1e-9 of itself.  A document whose
    confidence IS a threshold (each exit's lowest and highest) then stays at or below it, as under the search's strict compare, and no other
    compare changes: every confidence above a threshold is above it by more than 1e-7 of it (asserted on the table)."""
    import torch
    res, _ = _ragged_grid(pkg, grid_case, "policy")
    conf, correct, cost = grid_case["conf"], grid_case["correct"], grid_case["ragged"]
    E1, N = conf.shape
    for e in range(E1 - 1):
        gap = (conf[e][None, :] - res.table[e][:, None]) / res.table[e][:, None]
        assert gap[gap > 0].min() > 1e-7, e
    d = 2.0 * np.arctanh(conf * (1.0 - 1e-9))
    logits = torch.from_numpy(np.stack([d, np.zeros_like(d)], axis=-1)).cuda()                  # (E1, N, 2): one upload for all the scans
    assert len(res.front_vector) >= 8
    for i, row in enumerate(res.front_thresholds):
        exits = _np(pkg.criterion_scan_device(logits, row, "margin")[0]).astype(np.int64)
        assert int(cost[exits, np.arange(N)].sum()) == int(res.front_cost_sum[i]), i
        assert int(correct[exits, np.arange(N)].sum()) == int(res.front_hits[i]), i
        assert int(exits.sum()) == int(res.front_exit_sum[i]), i


def test_end_to_end_into_a_forward(pkg):
    """dump-all -> exit_costs -> threshold_search(cost=) -> select -> early_exit(thresholds=) delivers the selected entry's cost sum and hits."""
    import torch
    cfg = pkg.ModelConfig.tiny(EE_config=dict(TINY_CASES["tiny_ramp"]))
    W = pkg.synth.make_weights(cfg, seed=7, head_gain=4.0)
    B = 16
    docs = pkg.synth.make_documents(cfg, B, seed=11, text_len=48, min_words=3)
    t = {k: torch.from_numpy(docs[k]).cuda() for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}
    m = pkg.LayoutLMv3EEForSequenceClassification(cfg, weights=W, max_docs=B, max_text_len=48)
    dump = m.engine.forward(**t, dump_all=True, want_all=True, whole_layers=True, xprobe=False)
    al = _np(dump.all_logits).astype(np.float64)                     # (E1, B, K): the rows a whole-layers forward decides on, bit for bit
    E1 = al.shape[0]
    refs = al[-1].argmax(-1)
    refs[::5] = (refs[::5] + 1) % al.shape[-1]                       # the final exit is not always right
    cost = pkg.sweep.exit_costs(cfg, docs["attention_mask"], unit=1e3)
    assert cost.shape == (E1, B) and len(np.unique(cost[-1])) > 1    # ragged: the documents differ in length
    res = pkg.sweep.threshold_search(al, refs, num_per_exit=4, mixtures="grid", semantics="policy", cost=cost)
    assert res.num_vectors == 4 ** (E1 - 1) and len(res.front_vector) >= 2
    correct = (al.argmax(-1) == refs[None, :])
    c64 = cost.astype(np.int64)
    for kw in (dict(min_accuracy=float(res.front_accuracy[-1])), dict(min_accuracy=float(res.front_accuracy[len(res.front_accuracy) // 2])),
               dict(max_mean_cost=float(res.front_mean_cost[0])), dict(max_mean_cost=float(res.front_mean_cost[len(res.front_mean_cost) // 2]))):
        i = res.select_index(**kw)
        thr = res.select(**kw)
        assert isinstance(thr, list) and len(thr) == E1 and all(type(x) is float for x in thr)
        out = m.early_exit(**t, thresholds=thr, whole_layers=True, xprobe=False)
        ex = _np(out.exit_layer).astype(np.int64)
        assert int(c64[ex, np.arange(B)].sum()) == int(res.front_cost_sum[i]), (kw, ex.tolist())
        assert int(correct[ex, np.arange(B)].sum()) == int(res.front_hits[i]), kw
        assert int((_np(out.logits).argmax(-1) == refs).sum()) == int(res.front_hits[i]), kw
    m.engine.close()
