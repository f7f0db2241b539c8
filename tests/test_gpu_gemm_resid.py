"""The residual epilogue of the split GEMM as the layers launch it -- split-plane residual, a row map of its own -- through
ee_debug_gemm_split_resid, at every edge of the 256 x 256 configuration's staged residual read (csrc/gemm_split_kernel.h, "RESIDUAL THROUGH
LDS").

Every case is checked twice:
  * against float64 at the tolerance of test_gpu_kernels.py::test_split_gemm_at_the_routed_config_against_float64:
    max|got - ref| <= max(2 * err32, 1e-6), err32 = the error of a plain f32 GEMM (torch, TF32 off) on the same operands.  The residual of
    both is the value the split planes hold (hi + lo of the clamped, scaled input: csrc/mmee_common.h "Split-f16 operand rows"), which is
    what a layer's residual is: a LayerNorm output that exists only as split planes.  err32 is a maximum over samples, and a launch of one
    row has only N of them: over 768 samples of these operands it comes out anywhere between 5e-7 and 2e-6 (measured), around a kernel
    error of 1.0 - 1.1e-6 that is the SAME in both routes.  So the operand tensors handed to the hook always have at least 296 rows (the
    launch uses M of them) and err32 is taken over all of them: the same operands, enough samples for the yardstick to be one.
    The A operand of the edge cases has the magnitude of what the attention-output GEMM reads with the scale it is given here (context rows
    are convex combinations of V rows: 0.25 x N(0, 1) under kSplitScaleCtx = 64), not N(0, 1): with N(0, 1) rows the error of BOTH routes at
    K = 768 is 1.3 - 2.1e-6, that of torch's f32 GEMM 0.9 - 1.0e-6 at N = 256 but 2.6 - 3.5e-6 at N = 768 (it picks another kernel), and one
    of 108 sub-cases missed the bound by yardstick alone (M = 300, N = 256, K = 768, no map: 2.09e-6 against 2 x 0.99e-6, bits equal to the
    direct route's).  The large case keeps N(0, 1) rows under the FFN's scale.
  * bit for bit against route 1, the forced 128 x 128 configuration: it reads the residual straight into registers and has the same MFMA
    form, k order and term order, so any differing bit is a bug of the staging.

The row counts of the edge cases are a tile or two; the router sends such launches to the 128 x 128 configuration on any device with more
than a dozen CUs, so the side under test is route 2 (the 256 x 256 configuration whatever the row count).  Route 0 (the router's choice) is
compared as well, and the one large case checks that the router itself picks the staged configuration there.
"""
import pytest

from .conftest import report_measured
from .test_gpu_kernels import SCALE_CTX, SCALE_H1, SCALE_X, _check_guard, _cus, _guarded, _ptr, _split_cfg, _stream, _torch, _w_scale

pytestmark = pytest.mark.gpu

ROUTE_DEFAULT, ROUTE_128, ROUTE_256 = 0, 1, 2
SPLIT_CLAMP = 60000.0            # csrc/mmee_common.h kSplitClamp
MAPS = ("none", "same", "different")


def _resid_gemm(pkg, A, W, b, R, M, a_scale, w_scale, resid_scale, rs, rrs, route, iters=1):
    """One ee_debug_gemm_split_resid call; the M output rows as int32 words (f32 bits) after checking the guard rows."""
    torch = _torch()
    N, K = W.shape
    out = _guarded(M, N)
    lib = pkg.capi.load()
    pkg.capi.check(lib.ee_debug_gemm_split_resid(_ptr(A), _ptr(W), _ptr(b), _ptr(R), _ptr(out), M, N, K, a_scale, w_scale, resid_scale, _ptr(rs),
                                                 A.shape[0], _ptr(rrs), R.shape[0], route, iters, None, _stream()), None,
                   "ee_debug_gemm_split_resid")
    torch.cuda.synchronize()
    _check_guard(out, M, f"ee_debug_gemm_split_resid route {route}")
    return out[:M]


def _split_planes_value(R, scale):
    """What the split planes of an f32 tensor hold, as f32 (hi + lo carries at most 22 bits: exact)."""
    torch = _torch()
    x = (R * scale).clamp(-SPLIT_CLAMP, SPLIT_CLAMP)
    hi = x.half()
    lo = (x - hi.float()).half()
    return (hi.float() + lo.float()) / scale


def _case(M, N, K, seed, maps, a_gain=0.25, r_gain=1.0, r_offset=0.0):
    torch = _torch()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    extra = max(M, 256) + 40 - M      # rows beyond M: what the row maps pick from, and samples for err32 (module docstring)
    A = torch.randn(M + extra, K, generator=gen, device="cuda") * a_gain
    W = torch.randn(N, K, generator=gen, device="cuda") * 0.02
    b = torch.randn(N, generator=gen, device="cuda")
    R = torch.randn(M + extra, N, generator=gen, device="cuda") * r_gain
    if r_offset:      # magnitudes around r_offset, either sign
        R = (R + r_offset) * torch.sign(torch.randn(M + extra, N, generator=gen, device="cuda"))
    rs = rrs = None
    if maps != "none":      # non-decreasing with repeats, as the row map behind a compaction is
        rs = torch.sort(torch.randint(0, M + extra, (M,), generator=gen, device="cuda")).values.to(torch.int32)
        rrs = rs
    if maps == "different":      # the residual's rows in no order at all
        rrs = torch.randint(0, M + extra, (M,), generator=gen, device="cuda").to(torch.int32)
    return A, W, b, R, rs, rrs


def _check(pkg, name, M, N, K, a_scale, A, W, b, R, rs, rrs, want_default=None):
    torch = _torch()
    ws = _w_scale(W)
    staged = _resid_gemm(pkg, A, W, b, R, M, a_scale, ws, SCALE_X, rs, rrs, ROUTE_256)
    direct = _resid_gemm(pkg, A, W, b, R, M, a_scale, ws, SCALE_X, rs, rrs, ROUTE_128)
    routed = _resid_gemm(pkg, A, W, b, R, M, a_scale, ws, SCALE_X, rs, rrs, ROUTE_DEFAULT)
    if want_default is not None:
        assert _split_cfg(M, N, _cus()) == want_default
    diff = int((staged != direct).any(1).sum())
    report_measured(f"gemm_resid[{name}]", "rows whose bits differ between the 256 x 256 and the 128 x 128 route", float(diff))
    Ag = A[rs.long()] if rs is not None else A[:M]
    Rq = _split_planes_value(R, SCALE_X)
    Rg = Rq[rrs.long()] if rrs is not None else Rq[:M]
    ref = Ag.double() @ W.double().t() + b.double() + Rg.double()
    err32 = float(((A @ W.t() + b + Rq).double() - (A.double() @ W.double().t() + b.double() + Rq.double())).abs().max())      # over every row of the operands
    got = staged.view(torch.float32).double()
    assert not got.isnan().any()
    err = float((got - ref).abs().max())
    report_measured(f"gemm_resid[{name}]", f"max|err| (err32 {err32:.3e})", err)
    assert diff == 0, f"{name}: {diff} rows differ between the staged and the direct residual read"
    assert torch.equal(routed, direct), f"{name}: the routed launch differs"
    assert err <= max(2.0 * err32, 1e-6), (name, err, err32)


@pytest.mark.parametrize("K", [32, 64, 768])
@pytest.mark.parametrize("N", [256, 768])
@pytest.mark.parametrize("M", [1, 63, 255, 256, 257, 300])
def test_staged_residual_equals_the_direct_read_and_float64(pkg, M, N, K):
    """Rows past M, a last tile with one live row (257), a wave whose rows are all dead (1, 63, 300), full tiles (256); one N-tile and three;
    a one-stage k-loop with no earlier stage to hide the first piece under (K = 32), the ring depth (64), a long loop (768); no row map, one
    map for both operands (non-decreasing with repeats), a residual map of its own in no order."""
    for i, maps in enumerate(MAPS):
        A, W, b, R, rs, rrs = _case(M, N, K, seed=1000 * i + M + N + K, maps=maps)
        _check(pkg, f"M={M},N={N},K={K},map={maps}", M, N, K, SCALE_CTX, A, W, b, R, rs, rrs)


def test_staged_residual_with_more_tiles_than_workgroups(pkg):
    """M = 256 (CUs / 3 + 2), N = 768, K = 64: more tiles than workgroups, so every workgroup hands over to a next tile with residual pieces
    in flight, and the k-loop is exactly the ring; the router picks the 256 x 256 configuration by itself."""
    cus = _cus()
    M, N, K = 256 * (cus // 3 + 2), 768, 64
    A, W, b, R, rs, rrs = _case(M, N, K, seed=77, maps="different", a_gain=1.0)
    _check(pkg, f"handover,M={M}", M, N, K, SCALE_H1, A, W, b, R, rs, rrs, want_default="C")


def test_staged_residual_near_the_plane_clamp(pkg):
    """Residual values on both sides of the 60 000 clamp of the split planes (|16 x| from 59 200 to 60 800): the planes hold the clamped
    value, and the staged read must hand on exactly what the direct read does."""
    M, N, K = 300, 768, 64
    A, W, b, R, rs, rrs = _case(M, N, K, seed=5, maps="same", r_gain=25.0, r_offset=SPLIT_CLAMP / SCALE_X)
    assert float(R.abs().max()) * SCALE_X > SPLIT_CLAMP > float(R.abs().min()) * SCALE_X
    _check(pkg, "clamp", M, N, K, SCALE_CTX, A, W, b, R, rs, rrs)
