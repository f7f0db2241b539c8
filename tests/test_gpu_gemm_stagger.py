"""The 16-wave k-loop of the 256 x 256 split GEMM (csrc/gemm_split_kernel.h, "STAGGERED K-LOOP": waves 8-15 issue a stage's last MFMA block
behind the NEXT stage's barrier) at every loop length and row edge at which a held-back block can be lost, doubled, read from an overwritten
slot or dropped at the tile hand-over.

Every (epilogue, output) pair the path launches on the 256 x 256 configuration: bias -> f32, bias -> split, GELU -> split (the
gemm_split_ffn_up.hip unit), tanh -> f32, residual -> f32 with an f32 residual (ee_debug_gemm_split) and with a split residual
(ee_debug_gemm_split_resid, route 2).

K: 32 (one stage: the whole deferral is the block behind the loop), 64 (the ring), 96 (odd stage count, the last slot flips), 768 (production).
M = 256 (t - 1) + rem, t = the smallest tile count the router sends to the 256 x 256 configuration, rem in 1, 127, 128, 129, 255: the late
half of the last tile (rows 128-255 of a tile belong to waves 8-15) all dead, at the edge, with one live row, nearly full.  One case per
epilogue with more tiles than workgroups at K = 64: a hand-over with a held-back block pending on every tile.

Checked for every case:
  * bit for bit against the 128 x 128 configuration (four waves, one per SIMD, no stagger; same MFMA form, k order and term order): EVERY
    row of the first tile and of the last two tiles, recomputed through row_src in one launch small enough to route there (the split
    residual: every row of the launch, through route 1 of its hook);
  * against float64: max|got - ref| <= max(2 * err32, 1e-6), err32 = the error of a plain f32 GEMM (torch, TF32 off) on the same operands,
    taken over every row of the operand tensors (tests/test_gpu_gemm_resid.py says why);
  * three launches give the bits of one; the guard rows behind row M keep their bits (inside the launch helpers).
The operands of an (epilogue, K) pair and their float64 reference are made once, at the largest M; a smaller M uses their first rows.
"""
import pytest

from .conftest import report_measured
from .test_gpu_gemm_resid import ROUTE_128, ROUTE_256, _case, _resid_gemm, _split_planes_value
from .test_gpu_kernels import (EPI_BIAS, EPI_GELU, EPI_RESID, EPI_TANH, SCALE_CTX, SCALE_H1, SCALE_QKV, SCALE_X, _cus, _first_c_tiles, _operands,
                               _ref_and_err32, _split_cfg, _split_gemm, _split_values, _torch, _w_scale)

pytestmark = pytest.mark.gpu

# (name, N, epilogue, split output, A scale, output scale): the launches of the path on the 256 x 256 configuration through ee_debug_gemm_split
EPILOGUES = [
    ("bias", 2304, EPI_BIAS, 0, SCALE_X, 1.0),
    ("bias_split_out", 2304, EPI_BIAS, 1, SCALE_X, SCALE_QKV),
    ("gelu_split_out", 3072, EPI_GELU, 1, SCALE_X, SCALE_H1),
    ("tanh", 768, EPI_TANH, 0, SCALE_X, 1.0),
    ("resid_f32", 768, EPI_RESID, 0, SCALE_CTX, 1.0),
]
KS = [32, 64, 96, 768]
REMS = [1, 127, 128, 129, 255]
N_RESID = 768


def _edge_rows(M):
    """Every row of the first 256-row tile and of the last two."""
    tiles = (M + 255) // 256
    return sorted(set(range(0, min(256, M))) | set(range(256 * max(tiles - 2, 0), M)))


def _check_split(pkg, tag, spec, A, W, b, R, ref, err32, M, want_more_tiles_than_cus=False):
    torch = _torch()
    name, N, epi, out_split, a_scale, out_scale = spec
    cus = _cus()
    assert _split_cfg(M, N, cus) == "C", (M, N, cus)
    if want_more_tiles_than_cus:
        assert ((M + 255) // 256) * (N // 256) > cus
    ws = _w_scale(W)
    rows3 = _split_gemm(pkg, A, W, b, R, M, epi, out_split, a_scale, ws, out_scale, iters=3)
    rows1 = _split_gemm(pkg, A, W, b, R, M, epi, out_split, a_scale, ws, out_scale, iters=1)
    pick = _edge_rows(M)
    rs = torch.tensor(pick, dtype=torch.int32, device="cuda")
    assert _split_cfg(len(pick), N, cus) == "P", (len(pick), N, cus)
    sub = _split_gemm(pkg, A, W, b, R, len(pick), epi, out_split, a_scale, ws, out_scale, rs=rs)
    diff = int((sub != rows1[rs.long()]).any(1).sum())
    report_measured(f"gemm_stagger[{tag}]", f"rows of {len(pick)} whose bits differ from the 128 x 128 configuration's", float(diff))
    got = _split_values(rows1, N, out_split, out_scale)
    assert not got.isnan().any()
    err = float((got - ref[:M]).abs().max())
    report_measured(f"gemm_stagger[{tag}]", f"max|err| (err32 {err32:.3e})", err)
    assert torch.equal(rows3, rows1), f"{tag}: three launches differ from one"
    assert diff == 0, f"{tag}: {diff} rows differ from the 128 x 128 configuration"
    assert err <= max(2.0 * err32, 1e-6), (tag, err, err32)


def _split_operands(spec, K, rows):
    name, N, epi, _, _, _ = spec
    A, W, b, R, _ = _operands(rows, N, K, epi, seed=31 * K + N + epi, gather=False)
    ref, err32 = _ref_and_err32(A, W, b, R, None, epi)
    return A, W, b, R, ref, err32


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("spec", EPILOGUES, ids=[s[0] for s in EPILOGUES])
def test_staggered_k_loop_equals_the_four_wave_configuration_and_float64(pkg, spec, K):
    """Module docstring: every k-loop length x every row edge of the last tile, per epilogue."""
    N = spec[1]
    base = 256 * (_first_c_tiles(N, _cus()) - 1)
    A, W, b, R, ref, err32 = _split_operands(spec, K, base + max(REMS))
    for rem in REMS:
        _check_split(pkg, f"{spec[0]},K={K},M={base + rem}", spec, A, W, b, R, ref, err32, base + rem)


@pytest.mark.parametrize("spec", EPILOGUES, ids=[s[0] for s in EPILOGUES])
def test_staggered_k_loop_across_the_tile_hand_over(pkg, spec):
    """More tiles than workgroups at K = 64 (the loop is exactly the ring), a ragged last tile with one live row in its late half: every
    workgroup hands over to a next tile with the last stage's block still held back."""
    N, K = spec[1], 64
    M = 256 * (_cus() // (N // 256) + 1) + 129
    A, W, b, R, ref, err32 = _split_operands(spec, K, M)
    _check_split(pkg, f"{spec[0]},handover,M={M}", spec, A, W, b, R, ref, err32, M, want_more_tiles_than_cus=True)


def _resid_operands(K, rows):
    torch = _torch()
    A, W, b, R, rs, rrs = _case(rows, N_RESID, K, seed=17 * K + 3, maps="different")
    Rq = _split_planes_value(R, SCALE_X)
    ref = A[rs.long()].double() @ W.double().t() + b.double() + Rq[rrs.long()].double()
    err32 = float(((A @ W.t() + b + Rq).double() - (A.double() @ W.double().t() + b.double() + Rq.double())).abs().max())
    return A, W, b, R, rs, rrs, ref, err32


def _check_resid(pkg, tag, A, W, b, R, rs, rrs, ref, err32, M):
    """The split residual (row maps of its own for both operands): route 2 = the 256 x 256 configuration whatever the row count."""
    torch = _torch()
    ws = _w_scale(W)
    args = (A, W, b, R, M, SCALE_CTX, ws, SCALE_X, rs[:M].contiguous(), rrs[:M].contiguous())
    c3 = _resid_gemm(pkg, *args, ROUTE_256, iters=3)
    c1 = _resid_gemm(pkg, *args, ROUTE_256, iters=1)
    p1 = _resid_gemm(pkg, *args, ROUTE_128)
    diff = int((c1 != p1).any(1).sum())
    report_measured(f"gemm_stagger[{tag}]", f"rows of {M} whose bits differ from the 128 x 128 configuration's", float(diff))
    got = c1.view(torch.float32).double()
    assert not got.isnan().any()
    err = float((got - ref[:M]).abs().max())
    report_measured(f"gemm_stagger[{tag}]", f"max|err| (err32 {err32:.3e})", err)
    assert torch.equal(c3, c1), f"{tag}: three launches differ from one"
    assert diff == 0, f"{tag}: {diff} rows differ from the 128 x 128 configuration"
    assert err <= max(2.0 * err32, 1e-6), (tag, err, err32)


@pytest.mark.parametrize("K", KS)
def test_staggered_k_loop_with_the_split_residual(pkg, K):
    """The residual epilogue as the layers launch it (split-plane residual staged through LDS: its piece 0 is issued in the LAST k-stage, behind
    the late waves' held-back block), every k-loop length x every row edge."""
    base = 256 * (_first_c_tiles(N_RESID, _cus()) - 1)
    A, W, b, R, rs, rrs, ref, err32 = _resid_operands(K, base + max(REMS))
    for rem in REMS:
        _check_resid(pkg, f"resid_split,K={K},M={base + rem}", A, W, b, R, rs, rrs, ref, err32, base + rem)


def test_staggered_k_loop_with_the_split_residual_across_the_tile_hand_over(pkg):
    K = 64
    M = 256 * (_cus() // (N_RESID // 256) + 1) + 129
    assert ((M + 255) // 256) * (N_RESID // 256) > _cus()
    A, W, b, R, rs, rrs, ref, err32 = _resid_operands(K, M)
    _check_resid(pkg, f"resid_split,handover,M={M}", A, W, b, R, rs, rrs, ref, err32, M)
