"""The routes of launch_gemm_split (csrc/gemm_split.hip) that no other file launches alone -- split-K, the CLS probe, one term -- and the two
epilogue operands no other hook can set, through ee_debug_gemm_routes, against float64 and against the launches whose bits they must share.

Which case reaches which instantiation (CfgP = 128 x 128 tiles, 4 waves, three-deep ring, static tiles; CfgC = 256 x 256, 16 waves, staggered
k-loop, work queues; TAG 1 = the probe's kernel name, the only one that honours k_splits):
  gemm_split_kernel<CfgP, BIAS, f32, TAG 1>, k_splits = S     test_split_k_* (every case of gemm_routes_ref.SPLIT_K_CASES; through the probe's lines of the router
                                                              and through MMEE_FLAG_LOW_LATENCY's), batch independence, composed
  the same, k_splits = 1                                      the K-slice launches those are compared with (small-batch rule); probe bias -> f32
  <CfgP, GELU, split, TAG 1>, <CfgP, RESID, f32, TAG 1>,      test_probe_route_*: probe = 1 (M on the device, row_src = document offsets) against
  <CfgP, TANH, f32, TAG 1>                                    probe = 0 (the small-batch rule picks the same instantiation: the probe's own lines
                                                              of the router are what is under test) and float64
  <CfgP, BIAS, split, TAG 1>                                  probe = 1 with the pair outside the probe's list (falls through to the small-batch rule)
  <CfgC, GELU, split, TERMS 1>, <CfgC, BIAS, split, TERMS 1>, test_one_term_*: gemm_routes_ref.ONE_TERM, K = 32 (one stage: a late wave's whole block runs
  <CfgC, RESID, f32, role 2 / 3, TERMS 1>                     behind the loop), 64 (the ring), 96, 768 (3072), last tile's late half dead / edge / one row
  <CfgC, TANH, f32>, <CfgC, BIAS, f32> (three terms)          terms = 1 with a pair that has no one-term kernel
  <CfgP, BIAS, split, TAG 1> / <CfgC, BIAS, split>            scale_cols / scale at M = 129 / at the first M the router sends to CfgC
  <CfgP, RESID, f32, TAG 1> / <CfgC, RESID, f32> (staged)     col_scale through routes 1 / 2 of the residual epilogue

Acceptance rule (tests/test_gpu_kernels.py, tests/test_gpu_gemm_resid.py): max|got - ref64| <= max(2 * err32, 1e-6), err32 = the error of torch's f32
GEMM (TF32 off) on the same operands over every row of operand tensors of at least 296 rows.  Every err, err32 and count of differing rows goes
through report_measured before the assertions.  The operands are drawn on the CPU by tests/gemm_routes_ref.py, where tests/test_host_gemm_routes.py
shows that they see each fault of a route at ten times these tolerances.

A split-K output is one buffer of S + 1 parts, (max_m + 64) N floats apart, filled with a NaN pattern: rows >= M of every part and the whole
extra part must keep their bits.  Bit identity claimed and checked: part p == the one-part launch on the contiguous K slice p (same MFMA form,
same k order, zero accumulator, element-wise split_rows); three launches == one; a row's parts do not depend on its batch mates; probe = 1 ==
probe = 0; terms = 1 == terms = 3 where no one-term kernel exists.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from . import gemm_routes_ref as G
from . import rows_ref as R
from .conftest import report_measured
from .hook_util import _encode_split
from .test_gpu_gemm_resid import _case, _split_planes_value
from .test_gpu_kernels import (EPI_BIAS, EPI_GELU, EPI_RESID, EPI_TANH, GUARD, SCALE_CTX, SCALE_H1, SCALE_QKV, SCALE_X, SENTINEL, _check_guard, _cus,
                               _decode_split, _first_c_tiles, _guarded, _operands, _ptr, _split_cfg, _stream, _torch, _w_scale)

pytestmark = pytest.mark.gpu


def _dev(a):
    torch = _torch()
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _routes(pkg, A, W, out, M, a_scale, w_scale, *, bias=None, resid=None, epi=EPI_BIAS, out_split=0, out_scale=1.0, resid_scale=0.0, rs=None, rrs=None,
            route=0, role_tag=0, probe=0, terms=3, k_splits=1, split_stride=0, scale_cols=0, scale=1.0, col_scale=None, max_m=0, m_on_device=0, iters=1):
    """One ee_debug_gemm_routes call on device tensors; `out` is the caller's (guard rows and all)."""
    a = pkg.capi.DebugGemmRoutesArgs()
    N, K = W.shape
    for k, v in dict(A=A, W=W, bias=bias, resid=resid, Cout=out, row_src=rs, resid_row_src=rrs, col_scale=col_scale).items():
        setattr(a, k, None if v is None else v.data_ptr())
    for k, v in dict(M=M, N=N, K=K, epi=epi, out_split=out_split, a_scale=a_scale, w_scale=w_scale, out_scale=out_scale, resid_scale=resid_scale,
                     rows_A=A.shape[0], rows_resid=0 if resid is None else resid.shape[0], route=route, role_tag=role_tag, probe=probe, terms=terms,
                     k_splits=k_splits, split_stride=split_stride, scale_cols=scale_cols, scale=scale, max_m=max_m, m_on_device=m_on_device,
                     iters=iters).items():
        setattr(a, k, v)
    pkg.capi.check(pkg.capi.load().ee_debug_gemm_routes(C.byref(a), None, _stream()), None, "ee_debug_gemm_routes")
    _torch().cuda.synchronize()


def _one_part(pkg, A, W, M, a_scale, w_scale, **kw):
    """A launch that writes one f32 / split output of M rows; the rows as int32 words after checking the guard rows."""
    out = _guarded(M, W.shape[0])
    _routes(pkg, A, W, out, M, a_scale, w_scale, **kw)
    _check_guard(out, M, "ee_debug_gemm_routes")
    return out[:M]


def _f64(words):
    return words.view(_torch().float32).double()


def _maxerr(got, ref):
    return float((got - ref).abs().max())


def _accept(tag, what, err, err32):
    report_measured(f"gemm_routes[{tag}]", f"{what}: max|err| (err32 {err32:.3e})", err)
    return err <= max(2.0 * err32, 1e-6)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. split-K
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _split_k_operands(N, K, kind, rows):
    """Device operands A, W, b of a split-K case (made once per shape and row count)."""
    A, W, b, _ = (_dev(x) for x in G.operands(rows, N, K, kind, seed=N + K))
    return A, W, b


def _slice_refs(A, W, S):
    """Per part: (float64 product of the K slice over every row of A, err32 of the slice)."""
    K = A.shape[1]
    refs = []
    for p in range(S):
        ks = G.k_slice(K, S, p)
        a, w = A[:, ks].contiguous(), W[:, ks].contiguous()
        ref = a.double() @ w.double().t()
        refs.append((a, w, ref, _maxerr((a @ w.t()).double(), ref)))
    return refs


def _split_k_launch(pkg, A, W, M, max_m, S, a_scale, ws, rs, on_device, iters=1, probe=0):
    """The (S + 1)-part buffer of a split-K launch after the guard checks, as [S + 1, max_m + 64, N] int32 words."""
    torch = _torch()
    N = W.shape[0]
    stride = (max_m + GUARD) * N
    buf = torch.full((S + 1, max_m + GUARD, N), SENTINEL, dtype=torch.int32, device="cuda")
    _routes(pkg, A, W, buf, M, a_scale, ws, k_splits=S, split_stride=stride, rs=rs, max_m=max_m if on_device else 0, m_on_device=int(on_device),
            iters=iters, probe=probe)
    assert torch.equal(buf[:S, M:], torch.full_like(buf[:S, M:], SENTINEL)), "a write at or past row M of a part"
    assert torch.equal(buf[S], torch.full_like(buf[S], SENTINEL)), "a write past the last part"
    return buf


def _check_split_k(pkg, tag, N, K, S, kind, M, gather, on_device, max_m=None, rows=None, probe=0):
    torch = _torch()
    rows = rows or max(M, 256) + 44
    assert rows >= G.MIN_ROWS
    A, W, b = _split_k_operands(N, K, kind, rows)
    _, a_scale = G.KIND[kind]
    ws = _w_scale(W)
    max_m = (max_m or M) if on_device else M
    rs = _dev(G.row_map(M, rows, seed=N + K + S)) if gather else None
    pick = rs.long() if gather else slice(0, M)
    buf = _split_k_launch(pkg, A, W, M, max_m, S, a_scale, ws, rs, on_device, probe=probe)
    buf3 = _split_k_launch(pkg, A, W, M, max_m, S, a_scale, ws, rs, on_device, iters=3, probe=probe)
    ok = True
    bit_diff = 0
    for p, (a, w, ref, err32) in enumerate(_slice_refs(A, W, S)):
        alone = _one_part(pkg, a, w, M, a_scale, ws, rs=rs)       # the small-batch rule: the same instantiation with k_splits = 1
        d = int((alone != buf[p, :M]).any(1).sum())
        report_measured(f"gemm_routes[{tag}]", f"part {p}: rows of {M} whose bits differ from the one-part launch of the K slice", float(d))
        bit_diff += d
        got = _f64(buf[p, :M])
        assert not got.isnan().any(), (tag, p)
        ok &= _accept(tag, f"part {p}", _maxerr(got, ref[pick]), err32)
    done = buf[0, :M].view(torch.float32).clone()
    for p in range(1, S):                                         # ln_rows<PRE>: the parts in order, in f32, then the bias
        done += buf[p, :M].view(torch.float32)
    done += b
    full = A.double() @ W.double().t() + b.double()
    ok &= _accept(tag, "completed", _maxerr(done.double(), full[pick]), _maxerr((A @ W.t() + b).double(), full))
    assert torch.equal(buf3, buf), f"{tag}: three launches differ from one"
    assert bit_diff == 0, f"{tag}: {bit_diff} part rows differ from the one-part launch of their K slice"
    assert ok, f"{tag}: outside max(2 err32, 1e-6), see the measured values"


# per (N, K, S): (M, row map, M on the device with max_m = 300, probe).  Every triple has M = 129 and another variant, every variant two triples or
# more.  probe = 1: the X-space probe's launches take the probe's lines of the router (the others those of MMEE_FLAG_LOW_LATENCY) to the same kernel.
SPLIT_K_ROWS = {
    (256, 128, 4): [(129, False, False, 0), (1, True, True, 1)],
    (256, 256, 4): [(129, True, True, 1), (127, False, False, 0)],
    (256, 192, 2): [(129, False, False, 0), (128, True, False, 0)],
    (256, 256, 2): [(129, False, True, 0), (300, False, False, 0)],
    (768, 768, 8): [(129, True, True, 0), (1, False, False, 0)],
    (768, 3072, 4): [(129, False, True, 1), (127, True, False, 1)],
    (768, 3072, 8): [(129, True, False, 0), (300, False, False, 0)],
    (1024, 4096, 8): [(129, False, False, 0), (128, False, False, 0)],
}


@pytest.mark.parametrize("case", G.SPLIT_K_CASES, ids=[f"N{c[0]}-K{c[1]}-S{c[2]}" for c in G.SPLIT_K_CASES])
def test_split_k_parts_equal_the_k_slice_launches_and_float64(pkg, case):
    """Module docstring.  M on the device with max_m = 300 and M = 129: the launch has three M-tiles, the third all dead; it must write nothing."""
    N, K, S, kind = case
    assert (K // 32) % S == 0
    for M, gather, on_device, probe in SPLIT_K_ROWS[(N, K, S)]:
        _check_split_k(pkg, f"split_k N={N} K={K} S={S} M={M} map={int(gather)} dev={int(on_device)} probe={probe}", N, K, S, kind, M, gather, on_device,
                       max_m=300, probe=probe)


def test_split_k_second_tile_of_a_workgroup(pkg):
    """The CfgP grid is one workgroup per CU at most: with CUs < tiles x S <= 2 CUs some workgroups run a second (tile, part) in turn, re-deriving
    ks_pop, kt0 and c_shift and re-priming the ring behind the epilogue -- one 709-row document at the base shape on 256 CUs.  M (and so the tile
    count) is read from the device."""
    cus = _cus()
    for N, K, S, kind in ((768, 768, 8, "ctx"), (256, 256, 2, "ctx")):
        per_m_tile = (N // 128) * S
        t = cus // per_m_tile + 1                                # the smallest number of M-tiles with tiles x S > CUs
        if t * per_m_tile <= 2 * cus:
            break
    else:
        pytest.fail(f"no row count with CUs < tiles x S <= 2 CUs on {cus} CUs")
    M = 128 * (t - 1) + 1
    tiles = -(-M // 128) * (N // 128)
    assert cus < tiles * S <= 2 * cus and (-(-(M - 1) // 128)) * (N // 128) * S <= cus, (M, tiles, S, cus)
    _check_split_k(pkg, f"split_k second tile N={N} K={K} S={S} M={M} tiles x S={tiles * S} CUs={cus}", N, K, S, kind, M, True, True, max_m=M + 60,
                   rows=M + 44)


@pytest.mark.parametrize("N,K,S,kind", [(768, 768, 8, "ctx"), (256, 128, 4, "h1")])
def test_split_k_parts_do_not_depend_on_batch_mates(pkg, N, K, S, kind):
    """the same eight A rows alone, at positions 45..52 of a tile, and in the second tile of a launch."""
    torch = _torch()
    rows = 340
    A, W, b = _split_k_operands(N, K, kind, rows)
    _, a_scale = G.KIND[kind]
    ws = _w_scale(W)
    probe = list(range(rows - 8, rows))                          # the last rows of A: row_src is non-decreasing
    layouts = {"alone": probe, "at_45": list(range(45)) + probe + [rows - 1] * 3, "second_tile": list(range(128 + 13)) + probe}
    got = {}
    for lay, src in layouts.items():
        at = src.index(probe[0])
        rs = torch.tensor(src, dtype=torch.int32, device="cuda")
        got[lay] = _split_k_launch(pkg, A, W, len(src), len(src), S, a_scale, ws, rs, False)[:S, at:at + 8].clone()
    for lay in ("at_45", "second_tile"):
        d = int((got[lay] != got["alone"]).any(-1).sum())
        report_measured(f"gemm_routes[split_k batch mates N={N} K={K} S={S}]", f"{lay}: (part, row) pairs of {8 * S} whose bits differ", float(d))
    assert torch.equal(got["alone"], got["at_45"]) and torch.equal(got["alone"], got["second_tile"])


@pytest.mark.parametrize("N,K,S,kind", [(768, 768, 8, "ctx"), (768, 3072, 8, "h1")])
def test_split_k_parts_completed_by_ln_rows(pkg, N, K, S, kind):
    """As layer_rest does it under MMEE_FLAG_LOW_LATENCY: the parts to ln_rows<PRE> (S parts, the bias, a gathered split-plane residual), against
    float64 LN(A W^T + b + resid) under the per-row rule of tests/rows_ref.py (yardstick: the same in torch float32 on the CPU)."""
    torch = _torch()
    M, rows = 129, 300
    An, Wn, bn, _ = G.operands(rows, N, K, kind, seed=N + K)
    A, W, b = _split_k_operands(N, K, kind, rows)
    assert np.array_equal(A.cpu().numpy(), An)
    _, a_scale = G.KIND[kind]
    rng = np.random.default_rng([N, K, S])
    resid = R.on_grid(0.2 * rng.standard_normal((M + 9, N)))    # values a plane of scale 16 holds exactly
    rr = rng.integers(0, M + 9, M).astype(np.int32)
    g, beta = (1 + .1 * rng.standard_normal(N)).astype(np.float32), (.05 * rng.standard_normal(N)).astype(np.float32)
    buf = _split_k_launch(pkg, A, W, M, M, S, a_scale, _w_scale(W), None, False)
    dst = torch.full((M + 4, N), SENTINEL, dtype=torch.int32, device="cuda")
    t = [_dev(np.array([M], np.int32)), _dev(g), _dev(beta), _dev(_encode_split(resid, R.SPLIT_SCALE)), _dev(rr)]
    err = C.c_int32(-1)
    pkg.capi.check(pkg.capi.load().ee_debug_ln_rows(_ptr(buf), _ptr(dst), None, _ptr(t[0]), M + 2, N, _ptr(t[1]), _ptr(t[2]), R.EPS, None, 0.0, S,
                                                    (M + GUARD) * N, _ptr(b), _ptr(t[3]), _ptr(t[4]), 1.0 / R.SPLIT_SCALE, C.byref(err), _stream()),
                   None, "ee_debug_ln_rows")
    torch.cuda.synchronize()
    assert err.value == 0
    assert torch.equal(dst[M:], torch.full_like(dst[M:], SENTINEL))
    got = dst[:M].view(torch.float32).double().cpu().numpy()
    x64 = G.product64(An[:M], Wn) + bn.astype(np.float64) + resid[rr].astype(np.float64)
    ref = R.layer_norm(x64, g, beta, R.EPS)
    x32 = torch.from_numpy(An[:M]) @ torch.from_numpy(Wn).t() + torch.from_numpy(bn) + torch.from_numpy(resid[rr])
    y32 = R._torch_ln(x32, g, beta, R.EPS).numpy()
    e, e32 = R.per_row_max(got - ref), R.per_row_max(y32.astype(np.float64) - ref)
    tol = R.tolerance(e32)
    worst = int(np.argmax(e / tol))
    report_measured(f"gemm_routes[split_k + ln_rows N={N} K={K} S={S}]", f"max|err| over {M} rows (worst row {worst}: err32 {e32[worst]:.3e}, err / tol "
                    f"{e[worst] / tol[worst]:.2f})", float(e.max()))
    assert not np.isnan(got).any()
    assert (e <= tol).all(), [(int(r), float(e[r]), float(e32[r])) for r in np.nonzero(~(e <= tol))[0]][:8]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the probe route
# ---------------------------------------------------------------------------------------------------------------------------------------
# the four (epilogue, output) pairs of the probe's list in launch_gemm_split: (name, N, K, epilogue, split output, A scale, output scale)
PROBE_PAIRS = [
    ("gelu_split_out", 3072, 768, EPI_GELU, 1, SCALE_X, SCALE_H1),
    ("resid", 768, 768, EPI_RESID, 0, SCALE_CTX, 1.0),
    ("bias", 768, 768, EPI_BIAS, 0, SCALE_X, 1.0),
    ("tanh", 768, 768, EPI_TANH, 0, SCALE_X, 1.0),
]
PROBE_DOCS, PROBE_MAX_DOCS = 37, 64


def _probe_case(N, K, epi, seed):
    """37 documents of a batch sized for 64: A rows at document offsets, a residual (split planes) at rows of its own."""
    torch = _torch()
    gen = torch.Generator(device="cpu").manual_seed(seed)
    doc_off = torch.cumsum(torch.randint(1, 17, (PROBE_DOCS,), generator=gen), 0) - 1
    A, W, b, R_, _, _ = _case(int(doc_off[-1]) + 1, N, K, seed=seed, maps="none", a_gain=0.25 if epi == EPI_RESID else 1.0)
    assert A.shape[0] >= G.MIN_ROWS and int(doc_off[-1]) < A.shape[0]
    rs = doc_off.to(torch.int32).cuda()
    rrs = torch.randint(0, R_.shape[0], (PROBE_DOCS,), generator=gen).to(torch.int32).cuda() if epi == EPI_RESID else None
    return A, W, b, (R_ if epi == EPI_RESID else None), rs, rrs


def _epilogue64(x, epi):
    torch = _torch()
    return torch.nn.functional.gelu(x) if epi == EPI_GELU else torch.tanh(x) if epi == EPI_TANH else x


def _values(rows, N, out_split, out_scale):
    return _decode_split(rows, N, out_scale) if out_split else _f64(rows)


@pytest.mark.parametrize("pair", PROBE_PAIRS, ids=[p[0] for p in PROBE_PAIRS])
def test_probe_route_equals_the_small_batch_route_and_float64(pkg, pair):
    """probe = 1 as layer_probe launches it: M (37) on the device in a launch sized for 64, row_src = the documents' offsets, the residual at rows
    of its own from split planes.  terms = 1 changes nothing: a probe keeps three terms."""
    torch = _torch()
    name, N, K, epi, out_split, a_scale, out_scale = pair
    A, W, b, R_, rs, rrs = _probe_case(N, K, epi, seed=N + K + epi)
    ws = _w_scale(W)
    M = PROBE_DOCS
    kw = dict(bias=b, resid=R_, epi=epi, out_split=out_split, out_scale=out_scale, resid_scale=SCALE_X if R_ is not None else 0.0, rs=rs, rrs=rrs,
              role_tag=2 if epi == EPI_RESID else 0)
    probe = _one_part(pkg, A, W, M, a_scale, ws, probe=1, max_m=PROBE_MAX_DOCS, m_on_device=1, **kw)
    probe3 = _one_part(pkg, A, W, M, a_scale, ws, probe=1, max_m=PROBE_MAX_DOCS, m_on_device=1, iters=3, **kw)
    probe_t1 = _one_part(pkg, A, W, M, a_scale, ws, probe=1, terms=1, max_m=PROBE_MAX_DOCS, m_on_device=1, **kw)
    assert _split_cfg(M, N, _cus()) == "P"
    small = _one_part(pkg, A, W, M, a_scale, ws, probe=0, **kw)
    for what, other in (("probe = 0", small), ("three launches", probe3), ("terms = 1", probe_t1)):
        report_measured(f"gemm_routes[probe {name}]", f"rows of {M} whose bits differ from {what}", float((other != probe).any(1).sum()))
    got = _values(probe, N, out_split, out_scale)
    x64, x32 = A.double() @ W.double().t() + b.double(), A @ W.t() + b
    if R_ is not None:
        Rq = _split_planes_value(R_, SCALE_X)
        ref = x64[rs.long()] + Rq[rrs.long()].double()
        err32 = _maxerr((x32 + Rq).double(), x64 + Rq.double())
    else:
        ref = _epilogue64(x64, epi)[rs.long()]
        err32 = _maxerr(_epilogue64(x32, epi).double(), _epilogue64(x64, epi))
    assert not got.isnan().any()
    ok = _accept(f"probe {name}", "against float64", _maxerr(got, ref), err32)
    assert torch.equal(probe, small), f"{name}: probe = 1 differs from the small-batch route"
    assert torch.equal(probe, probe3), f"{name}: three launches differ from one"
    assert torch.equal(probe, probe_t1), f"{name}: terms = 1 changed a probe's bits"
    assert ok


def test_probe_route_with_a_pair_outside_its_list(pkg):
    """probe = 1 with (bias, split output): not a shape the probe launches, so the launch falls through to the router's other rules and must
    give the default route's bits."""
    torch = _torch()
    N, K = 768, 768
    A, W, b, _, rs, _ = _probe_case(N, K, EPI_BIAS, seed=5)
    ws = _w_scale(W)
    kw = dict(bias=b, epi=EPI_BIAS, out_split=1, out_scale=SCALE_QKV, rs=rs)
    probe = _one_part(pkg, A, W, PROBE_DOCS, SCALE_X, ws, probe=1, max_m=PROBE_MAX_DOCS, m_on_device=1, **kw)
    plain = _one_part(pkg, A, W, PROBE_DOCS, SCALE_X, ws, probe=0, **kw)
    report_measured("gemm_routes[probe bias_split_out]", "rows whose bits differ from probe = 0", float((probe != plain).any(1).sum()))
    x64 = A.double() @ W.double().t() + b.double()
    ok = _accept("probe bias_split_out", "against float64", _maxerr(_decode_split(probe, N, SCALE_QKV), x64[rs.long()]), _maxerr((A @ W.t() + b).double(), x64))
    assert torch.equal(probe, plain)
    assert ok


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. one term
# ---------------------------------------------------------------------------------------------------------------------------------------
def _hi(x, scale):
    """fp16(clamp(scale x)) / scale as f32: the hi plane, which is all a one-term kernel reads."""
    return (x * scale).clamp(-G.SPLIT_CLAMP, G.SPLIT_CLAMP).half().float() / scale


ONE_TERM_CASES = [(spec, K) for spec in G.ONE_TERM for K in spec[7]]


@pytest.mark.parametrize("spec,K", ONE_TERM_CASES, ids=[f"{s[0]}-K{K}" for s, K in ONE_TERM_CASES])
def test_one_term_kernels_against_the_float64_product_of_the_hi_planes(pkg, spec, K):
    """MMEE_FLAG_ONE_TERM's kernels run the staggered 16-wave k-loop with a block of 4 MFMAs instead of 12.  M = 256 (t - 1) + rem, t = the
    smallest tile count the router sends three-term launches to the 256 x 256 configuration (one-term launches always go there): rem = 1, 128,
    129 = the late half of the last tile dead, at its edge, with one live row.  Reference: the float64 product of the hi planes alone; err32 on
    those rounded operands.  Operands and references are made once, at the largest M."""
    torch = _torch()
    name, N, epi, out_split, kind, out_scale, role_tag, _ = spec
    base = 256 * (_first_c_tiles(N, _cus()) - 1)
    rows = base + max(G.ONE_TERM_REMS)
    _, a_scale = G.KIND[kind]
    A, W, b, R_ = (_dev(x) for x in G.operands(rows, N, K, kind, seed=K + epi + role_tag, resid=epi == EPI_RESID))
    ws = _w_scale(W)
    Ah, Wh = _hi(A, a_scale), _hi(W, ws)
    x64, x32 = Ah.double() @ Wh.double().t() + b.double(), Ah @ Wh.t() + b
    if epi == EPI_RESID:
        Rq = _split_planes_value(R_, SCALE_X)
        ref, f32 = x64 + Rq.double(), x32 + Rq
    else:
        ref, f32 = _epilogue64(x64, epi), _epilogue64(x32, epi)
    err32 = _maxerr(f32.double(), ref)
    del x64, x32, f32
    kw = dict(bias=b, resid=R_, epi=epi, out_split=out_split, out_scale=out_scale, resid_scale=SCALE_X if R_ is not None else 0.0, role_tag=role_tag, terms=1)
    ok = True
    for rem in G.ONE_TERM_REMS:
        M = base + rem
        tag = f"one_term {name} K={K} M={M}"
        one = _one_part(pkg, A, W, M, a_scale, ws, **kw)
        one3 = _one_part(pkg, A, W, M, a_scale, ws, iters=3, **kw)
        got = _values(one, N, out_split, out_scale)
        assert not got.isnan().any(), tag
        ok &= _accept(tag, "against the hi planes' float64 product", _maxerr(got, ref[:M]), err32)
        assert torch.equal(one3, one), f"{tag}: three launches differ from one"
    assert ok


@pytest.mark.parametrize("epi", [EPI_TANH, EPI_BIAS], ids=["tanh", "bias_f32"])
def test_one_term_without_a_one_term_kernel_runs_three_terms(pkg, epi):
    """launch_gemm_split: "anything else runs the three terms" -- tanh and bias -> f32 have no one-term instantiation."""
    torch = _torch()
    M, N, K = 129, 768, 768
    A, W, b, _, _ = _operands(M + 200, N, K, epi, seed=3 + epi, gather=False)
    ws = _w_scale(W)
    one = _one_part(pkg, A, W, M, SCALE_X, ws, bias=b, epi=epi, terms=1)
    three = _one_part(pkg, A, W, M, SCALE_X, ws, bias=b, epi=epi, terms=3)
    report_measured(f"gemm_routes[terms=1 {'tanh' if epi == EPI_TANH else 'bias_f32'}]", "rows whose bits differ from terms = 3", float((one != three).any(1).sum()))
    x64 = _epilogue64(A.double() @ W.double().t() + b.double(), epi)
    ok = _accept(f"terms=1 epi {epi}", "against the three-term float64 product", _maxerr(_f64(one), x64[:M]), _maxerr(_epilogue64(A @ W.t() + b, epi).double(), x64))
    assert torch.equal(one, three)
    assert ok


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the epilogue operands
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["P", "C"])
def test_scale_cols_scales_the_first_columns_only(pkg, cfg):
    """Q / sqrt(d) over columns [0, N / 3) of a bias -> split launch (the fused Q | K | V GEMM): columns N / 3 - 1 and N / 3 sit on the two sides."""
    N, K, scale = G.QSCALE_N, G.QSCALE_K, G.QSCALE
    cols = N // 3
    cus = _cus()
    M = 129 if cfg == "P" else 256 * (_first_c_tiles(N, cus) - 1) + 1
    assert _split_cfg(M, N, cus) == cfg
    rows = max(M, 256) + 44
    A, W, b, _ = (_dev(x) for x in G.operands(rows, N, K, "x", seed=9))
    got = _decode_split(_one_part(pkg, A, W, M, SCALE_X, _w_scale(W), bias=b, out_split=1, out_scale=SCALE_QKV, scale_cols=cols, scale=scale), N, SCALE_QKV)
    x64, x32 = A.double() @ W.double().t() + b.double(), A @ W.t() + b
    unscaled = x64.clone()
    x64[:, :cols] *= scale
    x32[:, :cols] *= scale
    err32 = _maxerr(x32.double(), x64)
    tag = f"scale_cols cfg={cfg} M={M}"
    ok = _accept(tag, "against float64", _maxerr(got, x64[:M]), err32)
    tol = max(2.0 * err32, 1e-6)
    for c, scaled in ((cols - 1, True), (cols, False)):
        right, wrong = (x64, unscaled * scale) if not scaled else (x64, unscaled)
        e_right, e_wrong = _maxerr(got[:, c], right[:M, c]), _maxerr(got[:, c], wrong[:M, c])
        report_measured(f"gemm_routes[{tag}]", f"column {c}: max|err| against the {'scaled' if scaled else 'unscaled'} reference (against the other one "
                        f"{e_wrong:.3e})", e_right)
        assert e_right <= tol < 10 * tol <= e_wrong, (c, e_right, e_wrong, tol)
    assert ok


@pytest.mark.parametrize("route", [1, 2], ids=["route1_cfgp", "route2_cfgc_staged"])
def test_col_scale_applies_in_front_of_the_residual(pkg, route):
    """BEiT's per-column factor on a residual launch (split residual, a row map of its own): (acc + bias) lambda + resid."""
    torch = _torch()
    M, N, K = 129, G.LAMBDA_N, G.LAMBDA_K
    rows = 300
    A, W, b, R_ = (_dev(x) for x in G.operands(rows, N, K, "ctx", seed=13, resid=True))
    rng = np.random.default_rng(13)
    lam = _dev((1.0 + 0.5 * rng.standard_normal(N)).astype(np.float32))
    rrs = _dev(rng.integers(0, rows, M).astype(np.int32))
    out = _one_part(pkg, A, W, M, SCALE_CTX, _w_scale(W), bias=b, resid=R_, epi=EPI_RESID, resid_scale=SCALE_X, rrs=rrs, route=route, role_tag=2,
                    col_scale=lam)
    Rq = _split_planes_value(R_, SCALE_X)
    x64 = (A.double() @ W.double().t() + b.double()) * lam.double()
    err32 = _maxerr(((A @ W.t() + b) * lam + Rq).double(), x64 + Rq.double())
    ref = x64[:M] + Rq[rrs.long()].double()
    assert _accept(f"col_scale route={route}", "against float64", _maxerr(_f64(out), ref), err32)
