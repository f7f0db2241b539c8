"""CPU-side proof that tests/test_gpu_gemm_f32_routes.py can see a fault (as tests/test_host_gemm_routes.py is for the split GEMM's routes).

On the operands of the GPU tests (tests/gemm_f32_routes_ref.py draws them on the CPU), the float64 reference of every faulted variant below differs
from the true reference by at least ten times the tolerance the GPU test applies there: max(2 max(err32, err_seq), 1e-6), err32 = the error of
torch's f32 GEMM on the CPU on the same operands, err_seq = that of the k-sequential f32 loop.  A fault that writes a row it must not, or leaves one
unwritten, shows in the `written` mask: the GPU tests see it through the sentinel of their buffers, at any size."""
import numpy as np
import pytest

from . import gemm_f32_routes_ref as G


def _moved(bad, true):
    """max|bad - true| over the rows both references write."""
    (cb, wb), (ct, wt) = bad, true
    both = wb & wt
    return float(np.abs(cb[both] - ct[both]).max()) if both.any() else 0.0


@pytest.mark.parametrize("N", G.RESID_NS)
@pytest.mark.parametrize("combo", G.RESID_COMBOS)
@pytest.mark.parametrize("kind", G.MAP_KINDS)
def test_residual_map_faults_move_the_reference(N, combo, kind):
    A, W, b, R = G.small_operands(N, G.RESID_K, 21)
    tol = G.tolerance(*G.yardsticks(A, W, b, G.EPI_RESID, resid=R))
    for M in G.RESID_MS:
        rs, rr = G.resid_case_maps(combo, kind, M, G.ROWS, seed=N + M)
        kw = dict(row_src=rs, resid=R, resid_row_src=rr)
        true = G.ref64(A, W, b, G.EPI_RESID, M, **kw)
        assert true[1].all() and not np.isnan(true[0]).any()
        out_row = np.arange(M)
        true_rr = out_row if rr is None else rr
        for mut, wrong_rr in (("resid_by_a_map", out_row if rs is None else rs), ("resid_by_out_row", out_row)):
            moved = _moved(G.ref64(A, W, b, G.EPI_RESID, M, mut=mut, **kw), true)
            if np.array_equal(wrong_rr, true_rr):               # A mapped, residual dense: reading it at the output row is right
                assert mut == "resid_by_out_row" and combo == "a_mapped_resid_dense" or M == 1, (mut, combo, M)
                assert moved == 0.0
            else:
                assert moved >= 10 * tol, (mut, combo, kind, M, moved, tol)
        if rs is not None and rr is not None:                   # the maps differ in every entry: every row of the output sees either fault
            bad = G.ref64(A, W, b, G.EPI_RESID, M, mut="resid_by_a_map", **kw)[0]
            assert (np.abs(bad - true[0]).max(1) >= 10 * tol).all()


@pytest.mark.parametrize("epi", G.QSCALE_EPIS, ids=[G.EPI_NAMES[e] for e in G.QSCALE_EPIS])
@pytest.mark.parametrize("cols", G.QSCALE_COLS)
def test_scale_faults_move_the_reference(epi, cols):
    N, K, M, scale = G.QSCALE_N, G.QSCALE_K, G.QSCALE_M, G.QSCALE
    A, W, b, _ = G.small_operands(N, K, 22)
    kw = dict(scale_cols=cols, scale=scale)
    tol = G.tolerance(*G.yardsticks(A, W, b, epi, **kw))
    true = G.ref64(A, W, b, epi, M, **kw)
    if cols < N:                                                 # the tile behind the border scaled too
        bad = G.ref64(A, W, b, epi, M, mut="scale_one_tile_more", **kw)
        assert _moved(bad, true) >= 10 * tol
        assert np.array_equal(bad[0][:, :cols], true[0][:, :cols]) and np.array_equal(bad[0][:, cols + G.BN:], true[0][:, cols + G.BN:])
    if cols > 0:                                                 # the tile in front of the border left alone
        bad = G.ref64(A, W, b, epi, M, mut="scale_one_tile_less", **kw)
        assert _moved(bad, true) >= 10 * tol
        if epi == G.EPI_GELU:                                    # the scale behind the function instead of in front of it
            assert _moved(G.ref64(A, W, b, epi, M, mut="scale_behind_epilogue", **kw), true) >= 10 * tol
        else:                                                    # the bias epilogue has no function to be on the wrong side of
            assert _moved(G.ref64(A, W, b, epi, M, mut="scale_behind_epilogue", **kw), true) == 0.0


@pytest.mark.parametrize("epi", G.EPIS, ids=[G.EPI_NAMES[e] for e in G.EPIS])
def test_lambda_faults_move_the_reference(epi):
    N, K, M = G.LAMBDA_N, G.LAMBDA_K, G.LAMBDA_M
    A, W, b, R = G.small_operands(N, K, 23)
    lam = G.lambda_vector(N, 23)
    kw = dict(col_scale=lam, resid=R if epi == G.EPI_RESID else None)
    tol = G.tolerance(*G.yardsticks(A, W, b, epi, **kw))
    true = G.ref64(A, W, b, epi, M, **kw)
    assert _moved(G.ref64(A, W, b, epi, M, resid=kw["resid"]), true) >= 10 * tol      # lambda ignored
    if epi == G.EPI_RESID:
        assert _moved(G.ref64(A, W, b, epi, M, mut="lambda_on_residual", **kw), true) >= 10 * tol
    moved = _moved(G.ref64(A, W, b, epi, M, mut="lambda_in_front_of_epilogue", **kw), true)
    if epi in (G.EPI_GELU, G.EPI_TANH):
        assert moved >= 10 * tol
    else:                                                        # the identity commutes with a factor (up to float64 rounding)
        assert moved <= 1e-12


@pytest.mark.parametrize("M,max_m", [c for c in G.M_ON_DEVICE if c[0] > 0])
def test_a_written_clamped_row_shows_in_the_guard(M, max_m):
    """Rows past M are staged as copies of row M - 1; a kernel that stored one would write a finite row where the GPU test wants the sentinel."""
    A, W, b, R = G.small_operands(G.M_ON_DEVICE_N, G.M_ON_DEVICE_K, 24)
    for epi in G.EPIS:
        kw = dict(resid=R if epi == G.EPI_RESID else None, rows_out=max_m + 64)
        (ct, wt), (cb, wb) = G.ref64(A, W, b, epi, M, **kw), G.ref64(A, W, b, epi, M, mut="clamped_row_written", **kw)
        assert wt[:M].all() and not wt[M:].any() and np.isnan(ct[M:]).all()
        assert wb[M] and not wt[M] and not np.isnan(cb[M]).any() and np.array_equal(cb[:M], ct[:M])


def test_an_empty_stage_writes_nothing():
    A, W, b, _ = G.small_operands(G.M_ON_DEVICE_N, G.M_ON_DEVICE_K, 24)
    for M, max_m in G.M_ON_DEVICE:
        C, written = G.ref64(A, W, b, G.EPI_BIAS, M, rows_out=max_m + 64)
        assert int(written.sum()) == M and np.isnan(C[M:]).all()


@pytest.mark.parametrize("M", G.GROUP_MS)
def test_a_dropped_second_group_moves_the_reference(M):
    """Queue 0 owns m-groups 0, 8, 16: a kernel that never took gl >= 1 would leave m-panels 64 .. unwritten.  The GPU test finds NaN (the
    sentinel) there; a zero-filled buffer would be wrong by more than ten tolerances as well."""
    panels = -(-M // G.BM)
    groups = -(-panels // G.GM)
    assert groups > G.QUEUES and (groups - 1) // G.QUEUES == (1 if M == G.GROUP_MS[0] else 2) and panels % G.GM == 1      # a partial last group
    A, W, b, _ = G.operands(M, G.GROUP_N, G.GROUP_K, seed=25)
    tol = G.tolerance(*G.yardsticks(A, W, b, G.EPI_BIAS))
    (ct, wt), (cb, wb) = G.ref64(A, W, b, G.EPI_BIAS, M), G.ref64(A, W, b, G.EPI_BIAS, M, mut="second_group_dropped")
    first = G.QUEUES * G.GM * G.BM
    assert wt.all() and wb[:first].all() and not wb[first:].any() and np.isnan(cb[first:]).all()
    assert np.abs(ct[first:]).max(1).min() >= 10 * tol


def test_batch_mates_layouts_put_the_probe_rows_where_they_say():
    lay = G.mates_layouts(G.ROWS)
    probe = np.arange(G.ROWS - 8, G.ROWS)
    for name, (m, at) in lay.items():
        assert np.array_equal(m[at:at + 8], probe) and len(m) == at + 8 and m.max() < G.ROWS and not np.isin(m[:at], probe).any(), name
    assert len(lay["tail_of_257"][0]) == 257 and 257 % G.BM == 1
    M = len(lay["group_8_of_8193"][0])
    assert M == G.GROUP_MS[0] and (M - 1) // G.BM // G.GM == G.QUEUES      # its last row lies in group 8, the second group of queue 0
