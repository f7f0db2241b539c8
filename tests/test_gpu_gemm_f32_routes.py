"""The f32 GEMM (csrc/gemm_f32.hip) alone, launched as a forward launches it, through ee_debug_gemm_f32: M read from device memory under a grid
sized by max_rows, a residual row map of its own, scale_cols / scale, col_scale, and more than one m-group per XCD queue -- against float64 and
against the launches whose bits they must share.  ee_debug_gemm (tests/test_gpu_kernels.py) can set none of these.

Acceptance rule (test_f32_gemm_against_float64): max|got - ref64| <= max(2 * max(err32, err_seq), 1e-6).  err32 = the error of torch's f32 GEMM,
err_seq = that of the k-sequential one-accumulator f32 loop, both with the case's epilogue over every row of operand tensors of at least 296 rows,
never on the kernel under test (tests/gemm_f32_routes_ref.py yardsticks: the expressions tests/test_host_gemm_f32_routes.py proves the faults
against).  Every err goes through report_measured with its two yardsticks before the assertions.

Every launch runs twice into two buffers filled with a NaN pattern, GUARD rows longer than the launch is sized for: the two must hold the same
bits, and rows >= M the pattern.  Every case runs both staging kernels (0 = LDS-DMA, what the path runs; 1 = register-staged).  Bit identity
claimed and checked: M from the device == M from the host; work queues == static grid stride; row maps == pre-gathered dense copies; columns
outside [0, scale_cols) == the unscaled launch, inside (bias epilogue) == 0.125 x its bits; a lambda of ones == no lambda (residual epilogue); a row
alone == the row among batch mates, in any tile and any group.  The two staging kernels are not claimed to be bit-equal to each other."""
import ctypes as C
import functools

import numpy as np
import pytest

from . import gemm_f32_routes_ref as G
from .conftest import report_measured
from .test_gpu_kernels import GUARD, SENTINEL, _stream, _torch

pytestmark = pytest.mark.gpu

STAGINGS = (0, 1)
STAGING_NAMES = {0: "dma", 1: "reg"}


def _dev(a):
    return None if a is None else _torch().from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=4)
def _small(N, K, seed):
    """(host operands, device operands) of a ROWS-row case."""
    host = G.small_operands(N, K, seed)
    return host, tuple(_dev(x) for x in host)


def _launch(pkg, A, W, out, M, *, bias=None, resid=None, epi=G.EPI_BIAS, staging=0, use_queue=1, rs=None, rrs=None, scale_cols=0, scale=1.0, col_scale=None,
            max_m=0, m_on_device=0, wgs_per_cu=0):
    """One ee_debug_gemm_f32 call on device tensors; `out` is the caller's (guard rows and all)."""
    a = pkg.capi.DebugGemmF32Args()
    N, K = W.shape
    for k, v in dict(A=A, W=W, bias=bias, resid=resid, Cout=out, row_src=rs, resid_row_src=rrs, col_scale=col_scale).items():
        setattr(a, k, None if v is None else v.data_ptr())
    for k, v in dict(M=M, N=N, K=K, epi=epi, staging=staging, use_queue=use_queue, rows_A=A.shape[0], rows_resid=0 if resid is None else resid.shape[0],
                     scale_cols=scale_cols, scale=scale, max_m=max_m, m_on_device=m_on_device, wgs_per_cu=wgs_per_cu).items():
        setattr(a, k, v)
    pkg.capi.check(pkg.capi.load().ee_debug_gemm_f32(C.byref(a), _stream()), None, "ee_debug_gemm_f32")
    _torch().cuda.synchronize()


def _run(pkg, A, W, M, what, **kw):
    """Two launches into two guarded buffers: the same bits in both, the sentinel in every row >= M.  The M rows as int32 words."""
    torch = _torch()
    sized = max(M, kw.get("max_m", 0) if kw.get("m_on_device") else 0)
    outs = []
    for _ in range(2):
        out = torch.full((sized + GUARD, W.shape[0]), SENTINEL, dtype=torch.int32, device="cuda")
        _launch(pkg, A, W, out, M, **kw)
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), f"{what}: two launches differ"
    assert torch.equal(outs[0][M:], torch.full_like(outs[0][M:], SENTINEL)), f"{what}: a write at or past row M = {M}"
    return outs[0][:M]


def _values(words):
    return words.view(_torch().float32).double().cpu().numpy()


def _accept(tag, got_words, ref, yard):
    """report, then the rule; ref: float64 rows on the host."""
    got = _values(got_words)
    assert got.shape == ref.shape and not np.isnan(got).any(), f"{tag}: rows the launch left unwritten"
    err = float(np.abs(got - ref).max()) if got.size else 0.0
    report_measured(f"gemm_f32_routes[{tag}]", f"max|err| (err32 torch {yard[0]:.3e}, k-sequential {yard[1]:.3e})", err)
    return err <= G.tolerance(*yard)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. M from device memory, the grid sized by max_m
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _m_on_device_ref(epi):
    """float64 rows of every operand row and the yardsticks of one epilogue (shared by the seven cases)."""
    A, W, b, R = G.small_operands(G.M_ON_DEVICE_N, G.M_ON_DEVICE_K, 24)
    resid = R if epi == G.EPI_RESID else None
    return G.ref64(A, W, b, epi, G.ROWS, resid=resid)[0], G.yardsticks(A, W, b, epi, resid=resid)


@pytest.mark.parametrize("M,max_m", G.M_ON_DEVICE, ids=[f"M{m}-max{x}" for m, x in G.M_ON_DEVICE])
def test_m_from_device_memory_under_a_larger_grid(pkg, M, max_m):
    """As every layer GEMM behind an exit: g.m_ptr = &counts[cur].n_rows, the launch sized by max_rows.  Rows [M, max_m + GUARD) keep their bytes
    (M = 0: the whole buffer); rows [0, M) have the bits of the launch that takes M from the host with a grid sized by M."""
    torch = _torch()
    _, (A, W, b, R) = _small(G.M_ON_DEVICE_N, G.M_ON_DEVICE_K, 24)
    ok = True
    for epi in G.EPIS:
        ref, yard = _m_on_device_ref(epi)
        for staging in STAGINGS:
            tag = f"m_on_device M={M} max_m={max_m} {G.EPI_NAMES[epi]} {STAGING_NAMES[staging]}"
            kw = dict(bias=b, resid=R if epi == G.EPI_RESID else None, epi=epi, staging=staging)
            base = _run(pkg, A, W, M, tag + " host M static grid", use_queue=0, **kw)
            ok &= _accept(tag, base, ref[:M], yard)
            for use_queue in (1, 0):
                got = _run(pkg, A, W, M, f"{tag} queue={use_queue}", use_queue=use_queue, max_m=max_m, m_on_device=1, **kw)
                assert torch.equal(got, base), f"{tag} queue={use_queue}: M from the device changed the bits of rows [0, M)"
            assert torch.equal(_run(pkg, A, W, M, tag + " host M queue", use_queue=1, **kw), base), f"{tag}: the work queues changed the bits"
    assert ok, "outside max(2 max(err32, err_seq), 1e-6), see the measured values"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. a residual row map of its own
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _resid_yard(N):
    A, W, b, R = G.small_operands(N, G.RESID_K, 21)
    return G.yardsticks(A, W, b, G.EPI_RESID, resid=R)


@pytest.mark.parametrize("N", G.RESID_NS)
@pytest.mark.parametrize("combo", G.RESID_COMBOS)
@pytest.mark.parametrize("kind", G.MAP_KINDS)
def test_residual_rows_come_through_their_own_map(pkg, N, combo, kind):
    """a_dense_resid_mapped: the attention-output launch behind a compaction (context dense, residual through x_rows); both_mapped: two maps that
    differ in every entry; a_mapped_resid_dense: the reverse.  Against float64, and bit-equal to the dense launch on pre-gathered copies."""
    torch = _torch()
    (Ah, Wh, bh, Rh), (A, W, b, R) = _small(N, G.RESID_K, 21)
    yard = _resid_yard(N)
    ok = True
    for M in G.RESID_MS:
        rs, rr = G.resid_case_maps(combo, kind, M, G.ROWS, seed=N + M)
        ref = G.ref64(Ah, Wh, bh, G.EPI_RESID, M, row_src=rs, resid=Rh, resid_row_src=rr)[0]
        d_rs, d_rr = _dev(rs), _dev(rr)
        A_g = A if rs is None else A[d_rs.long()].contiguous()
        R_g = R if rr is None else R[d_rr.long()].contiguous()
        for staging in STAGINGS:
            tag = f"resid_map N={N} {combo} {kind} M={M} {STAGING_NAMES[staging]}"
            got = _run(pkg, A, W, M, tag, bias=b, resid=R, epi=G.EPI_RESID, staging=staging, rs=d_rs, rrs=d_rr)
            ok &= _accept(tag, got, ref, yard)
            dense = _run(pkg, A_g, W, M, tag + " pre-gathered", bias=b, resid=R_g, epi=G.EPI_RESID, staging=staging)
            assert torch.equal(got, dense), f"{tag}: the mapped launch differs from the dense launch on gathered copies"
    assert ok, "outside max(2 max(err32, err_seq), 1e-6), see the measured values"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. scale_cols / scale
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", G.QSCALE_EPIS, ids=[G.EPI_NAMES[e] for e in G.QSCALE_EPIS])
def test_scale_cols_scales_whole_leading_tiles_only(pkg, epi):
    """The fused Q | K | V GEMM: columns [0, scale_cols) times 0.125 behind the bias, in front of the epilogue function."""
    torch = _torch()
    N, K, M, scale = G.QSCALE_N, G.QSCALE_K, G.QSCALE_M, G.QSCALE
    (Ah, Wh, bh, _), (A, W, b, _) = _small(N, K, 22)
    ok = True
    for staging in STAGINGS:
        plain = None
        for cols in G.QSCALE_COLS:
            tag = f"scale_cols={cols} {G.EPI_NAMES[epi]} {STAGING_NAMES[staging]}"
            got = _run(pkg, A, W, M, tag, bias=b, epi=epi, staging=staging, scale_cols=cols, scale=scale)
            ok &= _accept(tag, got, G.ref64(Ah, Wh, bh, epi, M, scale_cols=cols, scale=scale)[0], G.yardsticks(Ah, Wh, bh, epi, scale_cols=cols, scale=scale))
            if cols == 0:
                plain = got
                assert torch.equal(got, _run(pkg, A, W, M, tag + " scale 1", bias=b, epi=epi, staging=staging)), f"{tag}: a scale without columns changed bits"
                continue
            assert torch.equal(got[:, cols:], plain[:, cols:]), f"{tag}: a column at or past scale_cols differs from the unscaled launch"
            if epi == G.EPI_BIAS:                                # 0.125 is a power of two: the scaled value is the unscaled one with another exponent
                want = plain[:, :cols].view(torch.float32) * scale
                assert torch.equal(got[:, :cols].view(torch.float32), want), f"{tag}: a scaled column is not 0.125 x the unscaled bits"
            else:
                assert not torch.equal(got[:, :cols], plain[:, :cols])
    assert ok, "outside max(2 max(err32, err_seq), 1e-6), see the measured values"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. col_scale
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", G.EPIS, ids=[G.EPI_NAMES[e] for e in G.EPIS])
def test_col_scale_sits_behind_the_epilogue_and_in_front_of_the_residual(pkg, epi):
    """BEiT's lambda: epi(acc + bias) lambda (+ resid)."""
    torch = _torch()
    N, K, M = G.LAMBDA_N, G.LAMBDA_K, G.LAMBDA_M
    (Ah, Wh, bh, Rh), (A, W, b, R) = _small(N, K, 23)
    lam = G.lambda_vector(N, 23)
    d_lam, ones = _dev(lam), torch.ones(N, dtype=torch.float32, device="cuda")
    resid_h, resid = (Rh, R) if epi == G.EPI_RESID else (None, None)
    ref = G.ref64(Ah, Wh, bh, epi, M, resid=resid_h, col_scale=lam)[0]
    yard = G.yardsticks(Ah, Wh, bh, epi, resid=resid_h, col_scale=lam)
    ok = True
    for staging in STAGINGS:
        tag = f"col_scale {G.EPI_NAMES[epi]} {STAGING_NAMES[staging]}"
        kw = dict(bias=b, resid=resid, epi=epi, staging=staging)
        ok &= _accept(tag, _run(pkg, A, W, M, tag, col_scale=d_lam, **kw), ref, yard)
        if epi == G.EPI_RESID:
            assert torch.equal(_run(pkg, A, W, M, tag + " ones", col_scale=ones, **kw), _run(pkg, A, W, M, tag + " none", **kw)), \
                f"{tag}: a lambda of ones changed the bits"
    assert ok, "outside max(2 max(err32, err_seq), 1e-6), see the measured values"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. more than one m-group per XCD queue
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", G.GROUP_MS)
def test_queues_walk_every_group_they_own(pkg, M):
    """65 / 129 m-panels: queue 0 owns groups 0, 8 (, 16), the last of one panel with seven padding slots per n-tile.  Every row against float64;
    the bits of the static grid stride; once more with M on the device under a grid sized for M + 127."""
    torch = _torch()
    Ah, Wh, bh, _ = G.operands(M, G.GROUP_N, G.GROUP_K, seed=25)
    A, W, b = _dev(Ah), _dev(Wh), _dev(bh)
    ref, yard = G.ref64(Ah, Wh, bh, G.EPI_BIAS, M)[0], G.yardsticks(Ah, Wh, bh, G.EPI_BIAS)
    ok = True
    for staging in STAGINGS:
        tag = f"queue_groups M={M} {STAGING_NAMES[staging]}"
        got = _run(pkg, A, W, M, tag, bias=b, staging=staging, use_queue=1)
        ok &= _accept(tag, got, ref, yard)
        assert torch.equal(got, _run(pkg, A, W, M, tag + " static", bias=b, staging=staging, use_queue=0)), f"{tag}: queues and static grid differ"
        assert torch.equal(got, _run(pkg, A, W, M, tag + " M on device", bias=b, staging=staging, use_queue=1, max_m=M + 127, m_on_device=1)), \
            f"{tag}: M from the device changed the bits"
    assert ok, "outside max(2 max(err32, err_seq), 1e-6), see the measured values"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. a row does not depend on its batch mates
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", G.EPIS, ids=[G.EPI_NAMES[e] for e in G.EPIS])
def test_f32_gemm_rows_do_not_depend_on_batch_mates(pkg, epi):
    """What test_bench_size_early_exit_properties[fp32] rests on: the same eight A rows alone (M = 8), across the ragged tail of a 257-row
    launch and across the border of groups 7 and 8 of an 8193-row launch (gemm_f32_routes_ref.mates_layouts) have the same bits."""
    torch = _torch()
    (Ah, Wh, bh, Rh), (A, W, b, R) = _small(G.MATES_N, G.MATES_K, 26)
    resid_h, resid = (Rh, R) if epi == G.EPI_RESID else (None, None)
    yard = G.yardsticks(Ah, Wh, bh, epi, resid=resid_h)
    ok = True
    for staging in STAGINGS:
        got = {}
        for lay, (rs, at) in G.mates_layouts(G.ROWS).items():
            rr = ((rs.astype(np.int64) + 3) % G.ROWS).astype(np.int32) if epi == G.EPI_RESID else None      # a function of the A row: the probes keep theirs
            tag = f"batch_mates {lay} {G.EPI_NAMES[epi]} {STAGING_NAMES[staging]}"
            rows = _run(pkg, A, W, len(rs), tag, bias=b, resid=resid, epi=epi, staging=staging, rs=_dev(rs), rrs=_dev(rr))
            ok &= _accept(tag, rows, G.ref64(Ah, Wh, bh, epi, len(rs), row_src=rs, resid=resid_h, resid_row_src=rr)[0], yard)
            got[lay] = rows[at:at + 8].clone()
        for lay in ("tail_of_257", "group_8_of_8193"):
            d = int((got[lay] != got["alone"]).any(1).sum())
            report_measured(f"gemm_f32_routes[batch_mates {G.EPI_NAMES[epi]} {STAGING_NAMES[staging]}]", f"{lay}: rows of 8 whose bits differ from the rows alone", float(d))
        assert torch.equal(got["alone"], got["tail_of_257"]) and torch.equal(got["alone"], got["group_8_of_8193"]), (G.EPI_NAMES[epi], STAGING_NAMES[staging])
    assert ok, "outside max(2 max(err32, err_seq), 1e-6), see the measured values"
