"""The evaluation report on the GPU (ee_exit_metrics / metrics.exit_report) against the numpy restatement (tests/metrics_ref.py), and on the minted
fixture also against the values the reference's own functions gave.  Integers (confusion, exit histogram, accuracy = hits / N, f1_micro) must be
exact; float metrics within 1e-10 relative with a 1e-300 absolute floor: they are float64 sums of at most N = 2500 non-negative terms, so summation
order accounts for N 2^-53 <= 6e-13, and the device's exp / log differ from the host's by a few ulp.  Measured on an MI355X: see the
``report_measured`` lines of each test (the largest relative difference of any case was below 1e-14)."""
import numpy as np
import pytest

from . import metrics_ref as MR
from .conftest import TINY_CASES, load_golden, report_measured

pytestmark = pytest.mark.gpu
FLOATS = ("brier_loss", "nll", "f1_macro", "ece", "aurc", "average_confidence")
RTOL, FLOOR = 1e-10, 1e-300


def _logits(seed, E1, N, K):
    """Seeded dumped logits (E1,N,K) and labels (N,): later exits are sharper and more often right."""
    rng = np.random.default_rng(seed)
    refs = rng.integers(0, K, N).astype(np.int64)
    L = rng.standard_normal((E1, N, K)) * np.linspace(1.0, 2.5, E1)[:, None, None]
    L[:, np.arange(N), refs] += np.linspace(0.8, 3.0, E1)[:, None]
    return L, refs


def _assert_no_near_ties(conf, what):
    """Two confidences of a row are exactly equal or clearly apart, so that the device and the restatement cannot group them differently."""
    for r, row in enumerate(np.atleast_2d(conf)):
        s = np.sort(row)
        gap = np.diff(s)
        assert ((gap == 0) | (gap > 1e-9 * s[1:])).all(), (what, r, float(gap[gap > 0].min()))


def _rows_conf(L, refs, temperatures=None, exits=None):
    """(R,N) confidences of every row the report scores, on the host."""
    E1, N, _ = L.shape
    T = None if temperatures is None else np.asarray(temperatures, dtype=np.float64)
    rows = [MR.row_quantities(L[e], refs, None if T is None else T[e])["conf"] for e in range(E1)]
    if exits is not None:
        rows.append(MR.row_quantities(L[exits, np.arange(N)], refs, None if T is None else T[exits])["conf"])
    return np.stack(rows)


def _compare(rep, ref, tag, table=False):
    """One ExitReport against the restatement's dict; returns the largest relative difference of a float metric."""
    worst = 0.0
    for name in ("accuracy", "f1_micro"):
        assert np.array_equal(getattr(rep, name), ref[name]), (tag, name, getattr(rep, name), ref[name])
    for name in FLOATS:
        got, want = getattr(rep, name), ref[name]
        assert got.shape == want.shape, (tag, name)
        if table and name in ("brier_loss", "nll", "f1_macro"):
            assert np.isnan(got).all(), (tag, name, got)
            continue
        diff = np.abs(got - want)
        print(tag, name, "max |diff|", diff.max(), "got", got.tolist())
        assert (diff <= RTOL * np.abs(want) + FLOOR).all(), (tag, name, got.tolist(), want.tolist())
        nz = want != 0
        if nz.any():
            worst = max(worst, float((diff[nz] / np.abs(want[nz])).max()))
    if ref["exit_hist"] is None:
        assert rep.exit_hist is None and rep.policy is None
    else:
        assert rep.exit_hist.dtype == np.int64 and np.array_equal(rep.exit_hist, ref["exit_hist"]), (tag, rep.exit_hist)
        assert rep.policy == len(rep.accuracy) - 1
    if rep.confusion is not None:
        assert rep.confusion.dtype == np.int64 and np.array_equal(rep.confusion, ref["confusion"]), tag
    return worst


# ---- the minted fixture -----------------------------------------------------------------------------------------------------------------------
def test_fixture_every_exit_and_the_operating_point(pkg):
    g = load_golden("exit_metrics_ref")
    L, refs, exits = g["logits"].astype(np.float64), g["references"], g["exits"]
    _assert_no_near_ties(_rows_conf(L, refs, exits=exits), "fixture")
    rep = pkg.exit_report(L, refs, exits=exits, want_confusion=True)
    worst = _compare(rep, MR.report(L, refs, exits=exits), "fixture")
    for j, name in enumerate(g["names"].tolist()):                  # the reference's own values: accuracy, brier_loss, nll, f1_micro, f1_macro, aurc
        want = np.concatenate([g["per_exit"][:, j], g["point"][j:j + 1]])
        got = getattr(rep, name)
        if name in ("accuracy", "f1_micro"):
            assert np.array_equal(got, want), (name, got, want)
        else:
            rel = np.abs(got - want) / np.abs(want)
            worst = max(worst, float(rel.max()))
            assert (rel <= RTOL).all(), (name, got.tolist(), want.tolist())
    ece = pkg.calibration.expected_calibration_error
    want = np.array([ece(refs, L[e]) for e in range(3)] + [ece(refs, L[exits, np.arange(L.shape[1])])])
    assert (np.abs(rep.ece - want) <= RTOL * want + FLOOR).all(), (rep.ece.tolist(), want.tolist())
    d = rep.as_reference_dict()
    assert d["exit_2 _aurc"] == rep.aurc[2] and d["nll"] == rep.nll[3]
    report_measured("test_fixture_every_exit_and_the_operating_point", "largest relative difference", worst)


# ---- shapes: chunk edges of the 1024-wide walks, N = 1 and n_bins = 1, K below / at / above 16, one exit and seven ------------------------------
_FLAGS = [(True, True), (True, False), (False, True), (False, False), (True, True), (True, False)]      # (exits, temperatures): all four at every N
SHAPES = [(N, K, E1) + _FLAGS[i] for N in (1, 2, 63, 1024, 1025, 2500) for i, (K, E1) in enumerate((K, E1) for K in (2, 16, 17) for E1 in (1, 7))]


@pytest.mark.parametrize("N,K,E1,with_exits,with_T", SHAPES)
def test_shapes_against_the_restatement(pkg, N, K, E1, with_exits, with_T):
    L, refs = _logits(1000 + N + K + E1, E1, N, K)
    rng = np.random.default_rng(N * 31 + K)
    exits = rng.integers(0, E1, N).astype(np.int32) if with_exits else None
    T = np.linspace(0.6, 1.9, E1) if with_T else None
    _assert_no_near_ties(_rows_conf(L, refs, T, exits), "shapes")
    rep = pkg.exit_report(L, refs, temperatures=T, exits=exits, want_confusion=True)
    assert rep.num_samples == N and rep.num_exits == E1 and rep.confusion.shape == (E1 + int(with_exits), K, K)
    worst = _compare(rep, MR.report(L, refs, temperatures=T, exits=exits), f"N{N} K{K} E{E1}")
    report_measured(f"test_shapes_against_the_restatement[{N}-{K}-{E1}-{with_exits}-{with_T}]", "largest relative difference", worst)


def test_explicit_bin_counts_and_a_two_dimensional_input(pkg):
    L, refs = _logits(77, 3, 300, 5)
    _assert_no_near_ties(_rows_conf(L, refs), "bins")
    for bins in (1, 15, 299, 1024):
        _compare(pkg.exit_report(L, refs, n_bins=bins), MR.report(L, refs, n_bins=bins), f"bins {bins}")
    one = pkg.exit_report(L[1], refs)                               # (N,K): one exit
    assert one.num_exits == 1 and one.policy is None
    _compare(one, MR.report(L[1:2], refs), "2-d")


# ---- ties ---------------------------------------------------------------------------------------------------------------------------------------
def test_ties_through_the_table_form(pkg):
    """Confidences rounded to two decimals at N = 2500: hundreds of ties and duplicate ECE edges.  AURC and ECE follow the document order."""
    rng = np.random.default_rng(5)
    E1, N = 3, 2500
    conf = np.round(rng.beta(2.0 + np.arange(E1)[:, None] * 1.5, 2.0, (E1, N)), 2)
    correct = (rng.random((E1, N)) < conf).astype(np.uint8)
    exits = rng.integers(0, E1, N).astype(np.int32)
    assert all(len(np.unique(conf[e])) <= 101 for e in range(E1))
    _assert_no_near_ties(conf, "rounded")
    rep = pkg.exit_report((conf, correct), exits=exits)
    assert rep.confusion is None
    _compare(rep, MR.report((conf, correct), exits=exits), "ties", table=True)
    # the same documents in reverse order: another order inside every tie, another AURC -- in the restatement and on the device alike
    rev = pkg.exit_report((conf[:, ::-1].copy(), correct[:, ::-1].copy()))
    ref_rev = MR.report((conf[:, ::-1], correct[:, ::-1]))
    _compare(rev, ref_rev, "ties reversed", table=True)
    assert (ref_rev["aurc"] != MR.report((conf, correct))["aurc"]).all() and (rev.aurc != rep.aurc[:E1]).all()
    assert np.array_equal(rev.accuracy, rep.accuracy[:E1])


def test_duplicated_rows_with_different_labels(pkg):
    """Whole rows of logits duplicated, the copies labelled differently: equal confidences whose correctness differs."""
    L, refs = _logits(9, 3, 600, 16)
    src = np.arange(0, 300, 2)
    L[:, 300:300 + len(src)] = L[:, src]
    refs[300:300 + len(src)] = (refs[src] + np.arange(len(src)) % 3) % 16
    exits = (np.arange(600) % 3).astype(np.int32)
    exits[300:300 + len(src)] = exits[src]                           # so that the operating-point row has the duplicates too
    conf = _rows_conf(L, refs, exits=exits)
    _assert_no_near_ties(conf, "duplicates")
    assert all((np.diff(np.sort(row)) == 0).sum() >= len(src) for row in conf)
    _compare(pkg.exit_report(L, refs, exits=exits, want_confusion=True), MR.report(L, refs, exits=exits), "duplicates")


# ---- corners ------------------------------------------------------------------------------------------------------------------------------------
def test_all_correct_all_wrong_and_an_absent_class(pkg):
    L, _ = _logits(21, 2, 500, 8)
    L[:, :, 7] -= 50.0                                               # class 7 is never predicted
    pred = L.argmax(-1)
    assert (pred[0] != pred[1]).any()
    right = pkg.exit_report(L[0], pred[0], want_confusion=True)
    assert right.accuracy[0] == 1.0 and right.aurc[0] == 0.0 and right.f1_micro[0] == 1.0
    classes = len(np.unique(pred[0]))
    assert classes == 7 and abs(right.f1_macro[0] - 1.0) <= 1e-15    # seven classes of F1 = 1 averaged over seven, not over K = 8
    _compare(right, MR.report(L[:1], pred[0]), "all correct")
    wrong_refs = (pred[0] + 1) % 7                                   # never the prediction, never class 7
    wrong = pkg.exit_report(L[0], wrong_refs)
    assert wrong.accuracy[0] == 0.0 and wrong.f1_macro[0] == 0.0
    # every risk is 1 and the weights of the N - 1 steps of the curve sum to (N - 1) / N: that, not 1, is the reference's AURC of an all-wrong row
    assert abs(wrong.aurc[0] - 499.0 / 500.0) <= RTOL
    _compare(wrong, MR.report(L[:1], wrong_refs), "all wrong")
    mixed = pkg.exit_report(L, pred[1], want_confusion=True)         # exit 1 all right, exit 0 partly
    ref = MR.report(L, pred[1])
    _compare(mixed, ref, "absent class")
    cm = mixed.confusion[0]
    assert cm[7].sum() == 0 and cm[:, 7].sum() == 0
    present = [c for c in range(8) if cm[c].sum() + cm[:, c].sum() > 0]
    assert len(present) == 7
    by_hand = np.mean([2.0 * cm[c, c] / (cm[c].sum() + cm[:, c].sum()) for c in present])
    assert abs(mixed.f1_macro[0] - by_hand) <= 1e-12 and abs(mixed.f1_macro[0] - by_hand * 7 / 8) > 1e-3


# ---- determinism, refusals ------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_on_the_default_and_on_a_side_stream(pkg):
    import torch
    L, refs = _logits(33, 7, 2500, 16)
    exits = np.random.default_rng(34).integers(0, 7, 2500).astype(np.int32)
    dev = [torch.from_numpy(x).cuda() for x in (L, refs, exits)]

    def bits(rep):
        cols = [getattr(rep, n) for n in pkg.metrics.FIELDS]
        return np.stack(cols).view(np.int64).tobytes() + rep.confusion.tobytes() + rep.exit_hist.tobytes()

    first = bits(pkg.exit_report(dev[0], dev[1], exits=dev[2], want_confusion=True))
    assert bits(pkg.exit_report(dev[0], dev[1], exits=dev[2], want_confusion=True)) == first
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = [bits(pkg.exit_report(dev[0], dev[1], exits=dev[2], want_confusion=True)) for _ in range(2)]
    torch.cuda.current_stream().wait_stream(side)
    assert again[0] == first and again[1] == first


def test_refusals_before_anything_is_enqueued(pkg):
    import torch
    L, refs = _logits(1, 3, 50, 4)
    bad_exits = np.zeros(50, dtype=np.int32)
    bad_exits[7] = 3                                                 # E1
    bad_refs = refs.copy()
    bad_refs[11] = 4                                                 # K
    for move in (lambda x: x, lambda x: torch.from_numpy(x).cuda()):
        with pytest.raises(ValueError, match="exits"):
            pkg.exit_report(move(L), move(refs), exits=move(bad_exits))
        with pytest.raises(ValueError, match="label"):
            pkg.exit_report(move(L), move(bad_refs))
    with pytest.raises(ValueError, match="finite and positive"):
        pkg.exit_report(L, refs, temperatures=[1.0, 0.0, 2.0])
    assert pkg.exit_report(L, refs).accuracy.shape == (3,)          # and the same inputs, mended, go through


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_from_a_dump_all_forward(pkg):
    """dump-all forward -> criterion_scan_device -> exit_report(exits=) equals the restatement; exit_hist is the bincount of the exits."""
    import torch
    cfg = pkg.ModelConfig.tiny(EE_config=dict(TINY_CASES["tiny_ramp"]))
    W = pkg.synth.make_weights(cfg, seed=7, head_gain=4.0)
    B = 16
    docs = pkg.synth.make_documents(cfg, B, seed=11, text_len=48, min_words=3)
    t = {k: torch.from_numpy(docs[k]).cuda() for k in ("input_ids", "attention_mask", "bbox", "pixel_values")}
    m = pkg.LayoutLMv3EEForSequenceClassification(cfg, weights=W, max_docs=B, max_text_len=48)
    dump = m.engine.forward(**t, dump_all=True, want_all=True, whole_layers=True, xprobe=False)
    logits = dump.all_logits.to(torch.float64)                       # (E1, B, K), stays on the device
    al = logits.cpu().numpy()
    E1 = al.shape[0]
    refs = al[-1].argmax(-1)
    refs[::5] = (refs[::5] + 1) % al.shape[-1]                       # the final exit is not always right
    conf = _rows_conf(al, refs)
    thr = np.median(conf, axis=1)                                    # about half of the documents that reach an exit leave there
    exits_dev = pkg.criterion_scan_device(logits, thr, "max_confidence")[0]
    exits = exits_dev.cpu().numpy().astype(np.int64)
    assert len(np.unique(exits)) >= 2
    _assert_no_near_ties(_rows_conf(al, refs, exits=exits), "end to end")
    rep = pkg.exit_report(logits, refs, exits=exits_dev, want_confusion=True)
    _compare(rep, MR.report(al, refs, exits=exits), "end to end")
    assert np.array_equal(rep.exit_hist, np.bincount(exits, minlength=E1))
    eff = rep.efficiency(cost=np.arange(1, E1 + 1))
    assert abs(sum(eff["exit_distribution"].values()) - 1.0) <= 1e-12 and 0.0 <= eff["GFLOPs reduction"] < 1.0
    m.engine.close()
