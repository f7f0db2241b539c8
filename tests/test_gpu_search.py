"""The threshold search on the GPU (ee_threshold_search / sweep.threshold_search): everything against the numpy restatement
(tests/search_ref.py) on integers or bit patterns -- the percentile table against np.percentile, the per-vector sums, the front with its tie
rule -- through both main kernels (the E1 = 7 instantiation and the run-time form), all three digit sources and both exit rules; then against
what already ships (threshold_sweep, ee_criterion_scan) and end to end into a forward."""
import numpy as np
import pytest

from . import search_ref as R
from .conftest import TINY_CASES, load_golden, sweep_ref_inputs

pytestmark = pytest.mark.gpu
SEM = {"reference": R.REFERENCE, "policy": R.POLICY}


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _check(res, ref, N, tag, all_vectors=True):
    """One SearchResult against the restatement's dict: table bits, per-vector integers, the whole front."""
    assert np.array_equal(_bits(res.table), _bits(ref["table"])), tag
    if all_vectors:
        assert np.array_equal(_np(res.accuracy), ref["hits"] / float(N)), tag
        assert np.array_equal(_np(res.mean_exit), ref["exit_sum"] / float(N)), tag
    assert len(res.front_vector) == len(ref["front_vector"]), (tag, len(res.front_vector), len(ref["front_vector"]))
    assert np.array_equal(res.front_exit_sum, ref["front_exit_sum"]) and np.array_equal(res.front_hits, ref["front_hits"]), tag
    assert np.array_equal(res.front_vector.astype(np.int64), ref["front_vector"]), tag
    assert np.array_equal(_bits(res.front_thresholds), _bits(ref["front_thresholds"])), tag
    assert np.array_equal(res.front_accuracy, ref["front_hits"] / float(N)) and np.array_equal(res.front_mean_exit, ref["front_exit_sum"] / float(N)), tag
    for i, v in enumerate(res.front_vector[:8]):
        assert res.digits(v) == ref["digits"][int(v)].tolist(), (tag, i)


def _table(seed, E1, N, dup=0.0):
    """A synthetic confidence table in (0, 1) -- later exits surer and more often right -- with a share of the entries copied from other documents."""
    rng = np.random.default_rng(seed)
    conf = rng.beta(2.0 + np.arange(E1)[:, None] * 1.5, 2.0, (E1, N))
    if dup > 0:
        n_dup = int(N * dup)
        for e in range(E1):
            dst = rng.choice(N, n_dup, replace=False)
            conf[e, dst] = conf[e, rng.integers(0, N, n_dup)]
    correct = (rng.random((E1, N)) < np.linspace(0.3, 0.9, E1)[:, None]).astype(np.uint8)
    return conf, correct


# ---- golden: the reference's own mixtures ---------------------------------------------------------------------------------------------------
def test_golden_mixtures_reference_semantics(pkg):
    g = load_golden("sweep_ref")
    V = int(g["n_generated"])
    conf, correct, thr = g["conf"], g["correct"], g["thresholds"][:V]
    E1, N = conf.shape
    table = R.percentile_table(conf, 10)
    dg = np.zeros((V, E1), dtype=np.int64)
    for e in range(E1 - 1):
        dg[:, e] = (_bits(thr[:, e])[:, None] == _bits(table[e])[None, :]).argmax(1)
    ref = R.search(conf, correct, 10, R.MIXTURES, R.REFERENCE, V=V, mixtures=dg)
    assert len(ref["front_vector"]) == 35
    res = pkg.sweep.threshold_search((conf, correct), num_per_exit=10, mixtures=dg, semantics="reference", want_all=True)
    want = np.stack([np.percentile(conf[e], np.linspace(0, 100, 10)) for e in range(E1 - 1)])
    assert np.array_equal(_bits(res.table[:E1 - 1]), _bits(want)) and (res.table[E1 - 1] == 0).all()
    assert np.array_equal(_np(res.accuracy), g["accuracy"][:V]) and np.array_equal(_np(res.mean_exit), g["mean_exit"][:V])
    _check(res, ref, N, "golden")
    assert np.array_equal(_bits(res.front_thresholds), _bits(thr[res.front_vector.astype(np.int64)]))     # rows of the reference's own draw


# ---- the whole grid through the E1 = 7 instantiation; the cross-check with what ships ------------------------------------------------------------
@pytest.fixture(scope="module")
def grid_case():
    """E1 = 7, P = 4: 4096 vectors; N = 4100 crosses the 2048-document LDS chunk twice.  Logits, so that the scans can be run on them."""
    logits, refs = sweep_ref_inputs(seed=77, E1=7, N=4100, K=16)
    return dict(logits=logits, refs=refs, tables={}, results={})


def _grid(pkg, case, criterion, semantics):
    key = (criterion, semantics)
    if key not in case["results"]:
        if criterion not in case["tables"]:
            t, c = pkg.sweep.csf_table(case["logits"], case["refs"], criterion=criterion, as_csf=True)
            case["tables"][criterion] = (_np(t), _np(c))
        conf, correct = case["tables"][criterion]
        ref = R.search(conf, correct, 4, R.GRID, SEM[semantics])
        res = pkg.sweep.threshold_search(case["logits"], case["refs"], criterion=criterion, num_per_exit=4, mixtures="grid", semantics=semantics,
                                         want_all=True)
        case["results"][key] = (res, ref)
    return case["results"][key]


@pytest.mark.parametrize("semantics", ["reference", "policy"])
def test_grid_exact(pkg, grid_case, semantics):
    res, ref = _grid(pkg, grid_case, "max_confidence", semantics)
    assert res.num_vectors == 4096 and res.num_samples == 4100
    _check(res, ref, 4100, semantics)
    assert len(res.front_vector) >= 8
    if semantics == "policy":
        other = _grid(pkg, grid_case, "max_confidence", "reference")[1]
        assert int(((other["hits"] != ref["hits"]) | (other["exit_sum"] != ref["exit_sum"])).sum()) > 0


def test_grid_front_rows_through_threshold_sweep(pkg, grid_case):
    """REFERENCE: every reported row, given back to sweep.threshold_sweep as thresholds, reproduces its (exit_sum, hits)."""
    res, _ = _grid(pkg, grid_case, "max_confidence", "reference")
    conf, correct = grid_case["tables"]["max_confidence"]
    for hist in (False, True):                                       # the ranked kernel needs 8 V >= N: pad with copies; the direct one with a histogram
        rows = np.tile(res.front_thresholds, (1 + 4100 // (8 * len(res.front_thresholds)) + 1, 1)) if not hist else res.front_thresholds
        acc, mex, _ = pkg.sweep.threshold_sweep(conf, correct, rows, want_hist=hist)
        F = len(res.front_thresholds)
        assert np.array_equal(np.rint(_np(acc)[:F] * 4100).astype(np.int64), res.front_hits.astype(np.int64))
        assert np.array_equal(np.rint(_np(mex)[:F] * 4100).astype(np.int64), res.front_exit_sum.astype(np.int64))
        assert np.array_equal(_np(acc)[:F], res.front_accuracy) and np.array_equal(_np(mex)[:F], res.front_mean_exit)


@pytest.mark.parametrize("criterion", ["max_confidence", "entropy"])
def test_grid_front_rows_through_the_policy_scan(pkg, grid_case, criterion):
    """POLICY: every reported row, given to ee_criterion_scan as the thresholds of a policy, reproduces its (exit_sum, hits).  The entropy runs
    through the negated table and comes back as real entropy thresholds."""
    res, ref = _grid(pkg, grid_case, criterion, "policy")
    if criterion == "entropy":
        _check(res, dict(ref, table=-ref["table"], front_thresholds=-ref["front_thresholds"]), 4100, "entropy")
    import torch
    correct = grid_case["tables"][criterion][1]
    assert len(res.front_vector) >= 8
    logits = torch.from_numpy(grid_case["logits"]).cuda()            # one upload for all the scans
    for i, row in enumerate(res.front_thresholds):
        exits = _np(pkg.criterion_scan_device(logits, row, criterion)[0]).astype(np.int64)
        assert int(exits.sum()) == int(res.front_exit_sum[i]), (criterion, i)
        assert int(correct[exits, np.arange(4100)].sum()) == int(res.front_hits[i]), (criterion, i)


# ---- ties ----------------------------------------------------------------------------------------------------------------------------------
def test_ties_every_threshold_is_a_table_value(pkg):
    """E1 = 4, P = 5, N = 257: (N - 1) j / 4 is an integer, so every threshold IS a confidence, and a third of the confidences are shared by
    several documents: '>=' and '>' part company exactly here."""
    conf, correct = _table(5, 4, 257, dup=1.0 / 3.0)
    lo, hi, t = R.percentile_indexes(257, 5)
    assert all(x == 0.0 or l == h for l, h, x in zip(lo, hi, t))
    out = {}
    for name, sem in SEM.items():
        ref = R.search(conf, correct, 5, R.GRID, sem)
        assert np.isin(ref["table"][:3], conf).all()
        res = pkg.sweep.threshold_search((conf, correct), num_per_exit=5, mixtures="grid", semantics=name, want_all=True)
        assert res.num_vectors == 125
        _check(res, ref, 257, name)
        out[name] = ref
    assert int(((out["reference"]["hits"] != out["policy"]["hits"]) | (out["reference"]["exit_sum"] != out["policy"]["exit_sum"])).sum()) > 0


# ---- the run-time kernel, sampled vectors --------------------------------------------------------------------------------------------------------
def test_runtime_path_sampled(pkg):
    """E1 = 23 (config 3's exits: the grid is refused, the sample is not), V = 3001 (no multiple of 256), N = 1000 (crosses the 682-document chunk)."""
    E1, N, P, V = 23, 1000, 10, 3001
    conf, correct = _table(9, E1, N)
    with pytest.raises(ValueError, match="sample it"):
        pkg.sweep.threshold_search((conf, correct), num_per_exit=P, mixtures="grid")
    ref = R.search(conf, correct, P, R.SAMPLED, R.POLICY, V=V, seed=42)
    a = pkg.sweep.threshold_search((conf, correct), num_per_exit=P, mixtures=V, seed=42, want_all=True)
    _check(a, ref, N, "sampled")
    b = pkg.sweep.threshold_search((conf, correct), num_per_exit=P, mixtures=V, seed=42, want_all=True)
    for f in ("table", "front_thresholds", "front_vector", "front_hits", "front_exit_sum"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert np.array_equal(_np(a.accuracy), _np(b.accuracy)) and np.array_equal(_np(a.mean_exit), _np(b.mean_exit))
    ref2 = R.search(conf, correct, P, R.SAMPLED, R.REFERENCE, V=V, seed=43)
    c = pkg.sweep.threshold_search((conf, correct), num_per_exit=P, mixtures=V, seed=43, semantics="reference", want_all=True)
    _check(c, ref2, N, "sampled, seed 43")
    assert not np.array_equal(ref2["digits"], ref["digits"])
    d = pkg.sweep.threshold_search((conf, correct), num_per_exit=P, mixtures=V, seed=43)
    assert d.accuracy is None and d.mean_exit is None                 # the optional outputs left out (NULL)
    assert not (len(d.front_vector) == len(a.front_vector) and np.array_equal(d.front_vector, a.front_vector))     # another seed, another front


def test_smallest_shape(pkg):
    conf, correct = np.array([[0.75], [0.25]]), np.array([[1], [0]], dtype=np.uint8)
    for name, sem in SEM.items():
        ref = R.search(conf, correct, 2, R.SAMPLED, sem, V=1, seed=1)
        res = pkg.sweep.threshold_search((conf, correct), num_per_exit=2, mixtures=1, seed=1, semantics=name, want_all=True)
        _check(res, ref, 1, name)
        assert len(res.front_vector) == 1


def test_tie_rule_names_the_lower_index(pkg):
    """Every vector planted twice (rows v and v + 20 carry the same digits): equal (exit_sum, hits), and the front must name the first."""
    conf, correct = _table(21, 3, 300)
    rng = np.random.default_rng(3)
    rows = rng.integers(0, 6, (20, 3))
    mix = np.concatenate([rows, rows])
    for name, sem in SEM.items():
        ref = R.search(conf, correct, 6, R.MIXTURES, sem, V=40, mixtures=mix)
        res = pkg.sweep.threshold_search((conf, correct), num_per_exit=6, mixtures=mix, semantics=name, want_all=True)
        _check(res, ref, 300, name)
        assert len(res.front_vector) >= 2 and (res.front_vector < 20).all()
        assert np.array_equal(_np(res.accuracy)[:20], _np(res.accuracy)[20:])


# ---- end to end: dumped logits -> search -> select -> the thresholds of a forward ---------------------------------------------------------------
def test_end_to_end_into_a_forward(pkg):
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
    res = pkg.sweep.threshold_search(al, refs, num_per_exit=4, mixtures="grid", semantics="policy")
    assert res.num_vectors == 4 ** (E1 - 1) and len(res.front_vector) >= 2
    correct = (al.argmax(-1) == refs[None, :])
    for kw in (dict(min_accuracy=float(res.front_accuracy[-1])), dict(min_accuracy=float(res.front_accuracy[len(res.front_accuracy) // 2])),
               dict(max_mean_exit=float(res.front_mean_exit[0]))):
        i = res.select_index(**kw)
        thr = res.select(**kw)
        assert isinstance(thr, list) and len(thr) == E1 and all(type(x) is float for x in thr)
        out = m.early_exit(**t, thresholds=thr, whole_layers=True, xprobe=False)
        ex = _np(out.exit_layer).astype(np.int64)
        assert int(ex.sum()) == int(res.front_exit_sum[i]), (kw, ex.tolist())
        assert int(correct[ex, np.arange(B)].sum()) == int(res.front_hits[i]), kw
        assert int((_np(out.logits).argmax(-1) == refs).sum()) == int(res.front_hits[i]), kw
    m.engine.close()
