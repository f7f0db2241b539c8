"""Kernel-level parity: the layer GEMMs alone against float64 at the tile configurations the release router picks, the CfgP <=> CfgC
bit-identity the small-batch rule relies on, the f32 GEMM's two staging kernels, and label counts other than 16 end to end.

Acceptance rule of a GEMM against its float64 reference (as test_gpu_parity.py::test_split_gemm_kernel_against_float64):
max|got - ref| <= max(2 * err32, 1e-6), err32 = the error of a plain f32 GEMM (torch, TF32 off) on the same operands.
"""
import ctypes as C
import zlib

import numpy as np
import pytest

from .conftest import H256_KW, report_measured

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4
EPI_BIAS, EPI_GELU, EPI_RESID, EPI_TANH = 0, 1, 2, 3
EPI_NAMES = {EPI_BIAS: "bias", EPI_GELU: "gelu", EPI_RESID: "resid", EPI_TANH: "tanh"}
# activation scales of the split planes (csrc/mmee_common.h kSplitScaleX / Ctx / H1 / QKV)
SCALE_X, SCALE_CTX, SCALE_H1, SCALE_QKV = 16.0, 64.0, 16.0, 16.0
GUARD = 64                       # rows past M in every output buffer; they must keep SENTINEL's bits
SENTINEL = 0x7FA5A5A5            # a NaN bit pattern no kernel writes


def _torch():
    import torch
    assert torch.backends.cuda.matmul.allow_tf32 is False, "err32 must be a true f32 GEMM"
    return torch


def _cus():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def _split_cfg(M, N, cus):
    """The release router's choice for a layer GEMM (csrc/gemm_split.hip:64): the 128 x 128 CfgP kernel when the default 256 x 256
    tiles would leave more than half of the CUs without one, else CfgC."""
    return "P" if ((M + 255) // 256) * (N // 256) * 2 <= cus else "C"


def _first_c_tiles(N, cus):
    """Smallest number of 256-row M-tiles that routes an N-wide GEMM to CfgC."""
    return cus // (2 * (N // 256)) + 1


def _w_scale(W):
    """ee_finalize's weight scale (build_split under ee_finalize in csrc/capi.hip): the power of two that puts max|w| in [2^12, 2^13), capped at 2^8."""
    mx = float(W.abs().max())
    e = 8 if mx == 0.0 else min(8, 13 - int(np.frexp(mx)[1]))
    return float(2.0 ** e)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def _guarded(M, N):
    torch = _torch()
    return torch.full((M + GUARD, N), SENTINEL, dtype=torch.int32, device="cuda")


def _check_guard(out, M, what):
    torch = _torch()
    assert torch.equal(out[M:], torch.full_like(out[M:], SENTINEL)), f"{what}: a write past row M"


def _decode_split(rows_i32, N, scale):
    torch = _torch()
    h = rows_i32.view(torch.float16).view(rows_i32.shape[0], N // 16, 2, 16)       # 64-byte groups [hi 16 | lo 16]
    return (h[:, :, 0].double() + h[:, :, 1].double()).reshape(rows_i32.shape[0], N) / scale


def _epilogue(x, epi, R):
    torch = _torch()
    if epi == EPI_GELU:
        return torch.nn.functional.gelu(x)
    if epi == EPI_TANH:
        return torch.tanh(x)
    if epi == EPI_RESID:
        return x + R
    return x


def _ref_and_err32(A, W, b, R, rs, epi):
    """float64 reference and the plain f32 GEMM's max error on the same (gathered) operands."""
    torch = _torch()
    Ag = A[rs.long()] if rs is not None else A
    Rg = None if R is None else (R[rs.long()] if rs is not None else R)
    ref = _epilogue(Ag.double() @ W.double().t() + b.double(), epi, None if Rg is None else Rg.double())
    f32 = _epilogue(Ag @ W.t() + b, epi, Rg)
    return ref, float((f32.double() - ref).abs().max())


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. split GEMM at every configuration the release router picks
# ---------------------------------------------------------------------------------------------------------------------------------------
def _split_gemm(pkg, A, W, b, R, M, epi, out_split, a_scale, w_scale, out_scale, rs=None, iters=1):
    """One ee_debug_gemm_split call; returns the M output rows as int32 words (f32 bits, or split-f16 pairs) after checking the guard rows."""
    torch = _torch()
    N, K = W.shape
    out = _guarded(M, N)
    lib = pkg.capi.load()
    pkg.capi.check(lib.ee_debug_gemm_split(_ptr(A), _ptr(W), _ptr(b), _ptr(R), _ptr(out), M, N, K, epi, out_split, a_scale, w_scale,
                                           out_scale, _ptr(rs), A.shape[0], iters, None, _stream()), None, "ee_debug_gemm_split")
    torch.cuda.synchronize()
    _check_guard(out, M, "ee_debug_gemm_split")
    return out[:M]


def _split_values(rows, N, out_split, out_scale):
    torch = _torch()
    return _decode_split(rows, N, out_scale) if out_split else rows.view(torch.float32).double()


def _operands(M, N, K, epi, seed, gather, ln_like=False, w_outliers=False):
    torch = _torch()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rows_A = M + max(40, M // 16) if gather else M
    A = torch.randn(rows_A, K, generator=gen, device="cuda")
    if ln_like:
        # LayerNorm-like rows: most values O(1), a few outlier channels near +-100, and a sprinkle of values below 1e-3, whose lo plane
        # (value * scale - hi) falls into the f16 subnormal range
        ch = torch.randperm(K, generator=gen, device="cuda")[:6]
        A[:, ch] = 100.0 * torch.sign(A[:, ch]) + A[:, ch]
        tiny = torch.rand(rows_A, K, generator=gen, device="cuda") < 0.05
        A = torch.where(tiny, A * 1e-4, A)
    W = torch.randn(N, K, generator=gen, device="cuda") * 0.02
    if w_outliers:                # max|w| ~ 40: ee_finalize's scale is 2^7, below the 2^8 cap
        idx = torch.randperm(N * K, generator=gen, device="cuda")[:16]
        W.view(-1)[idx] = 40.0 * torch.sign(W.view(-1)[idx])
    b = torch.randn(N, generator=gen, device="cuda")
    R = torch.randn(rows_A, N, generator=gen, device="cuda") if epi == EPI_RESID else None
    rs = None
    if gather:
        rs = torch.sort(torch.randperm(rows_A, generator=gen, device="cuda")[:M]).values.to(torch.int32)
    return A, W, b, R, rs


# (name, N, K, epi, out_split, a_scale, out_scale, gather, M = 256 * (t - 1) + rem with t = _first_c_tiles, cfg wanted, extras)
SPLIT_CASES = [
    ("qkv", 2304, 768, EPI_BIAS, 0, SCALE_X, 1.0, False, 1, "C", {}),
    ("qkv_split_out", 2304, 768, EPI_BIAS, 1, SCALE_X, SCALE_QKV, False, 255, "C", {}),
    ("qkv_layernorm_rows", 2304, 768, EPI_BIAS, 1, SCALE_X, SCALE_QKV, False, 129, "C", dict(ln_like=True)),
    ("qkv_weight_scale_below_cap", 2304, 768, EPI_BIAS, 0, SCALE_X, 1.0, False, 200, "C", dict(w_outliers=True)),
    ("attn_out", 768, 768, EPI_RESID, 0, SCALE_CTX, 1.0, False, 255, "C", {}),
    ("attn_out_gathered", 768, 768, EPI_RESID, 0, SCALE_CTX, 1.0, True, 1, "C", {}),
    ("attn_out_last_p", 768, 768, EPI_RESID, 0, SCALE_CTX, 1.0, False, 0, "P", {}),       # M = 256 (t - 1): the last M before CfgC
    ("ffn_up", 3072, 768, EPI_GELU, 1, SCALE_X, SCALE_H1, False, 1, "C", {}),
    ("ffn_up_ragged", 3072, 768, EPI_GELU, 1, SCALE_X, SCALE_H1, False, 255, "C", {}),
    ("ffn_down", 768, 3072, EPI_RESID, 0, SCALE_H1, 1.0, False, 255, "C", {}),
    ("head_dense", 768, 768, EPI_TANH, 0, SCALE_X, 1.0, False, 1, "C", {}),
]


@pytest.mark.parametrize("case", SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_split_gemm_at_the_routed_config_against_float64(pkg, case):
    """The layer GEMMs at production's N / K / epilogue / scales, at M just past the P/C threshold with a ragged last tile (CfgC, the
    16x16x32 default; FFN-up = the gemm_split_ffn_up.hip unit; N <= 768 = the tile_order 1 queue walk), against float64; guard rows
    untouched; three launches (queue counter reset between them) give the bits of one."""
    name, N, K, epi, out_split, a_scale, out_scale, gather, rem, want, extra = case
    cus = _cus()
    M = 256 * (_first_c_tiles(N, cus) - 1) + rem
    assert _split_cfg(M, N, cus) == want, (M, N, cus)
    if want == "C":
        assert _split_cfg(M - rem, N, cus) == "P"          # the smallest tile count past the threshold
    A, W, b, R, rs = _operands(M, N, K, epi, seed=zlib.crc32(name.encode()) & 0xFFFF, gather=gather, **extra)
    ws = _w_scale(W)
    if extra.get("w_outliers"):
        assert ws == 128.0
    rows3 = _split_gemm(pkg, A, W, b, R, M, epi, out_split, a_scale, ws, out_scale, rs, iters=3)
    rows1 = _split_gemm(pkg, A, W, b, R, M, epi, out_split, a_scale, ws, out_scale, rs, iters=1)
    assert _torch().equal(rows3, rows1), "three launches differ from one"
    got = _split_values(rows1, N, out_split, out_scale)
    assert not got.isnan().any()
    ref, err32 = _ref_and_err32(A, W, b, R, rs, epi)
    err = float((got - ref).abs().max())
    report_measured(f"split_gemm[{name},M={M},cfg={want}]", f"max|err| (err32 {err32:.3e})", err)
    assert err <= max(2.0 * err32, 1e-6), (name, M, err, err32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. CfgP <=> CfgC bit identity and batch invariance
# ---------------------------------------------------------------------------------------------------------------------------------------
# every (epilogue, output) pair the small-batch rule routes to CfgP (csrc/gemm_split.hip:64-72), at the N of the GEMM that uses it
P_ROUTES = [
    ("bias", 2304, 768, EPI_BIAS, 0, SCALE_X, 1.0),
    ("bias_split_out", 2304, 768, EPI_BIAS, 1, SCALE_X, SCALE_QKV),
    ("gelu_split_out", 3072, 768, EPI_GELU, 1, SCALE_X, SCALE_H1),          # CfgC side = the gemm_split_ffn_up.hip unit
    ("resid", 768, 768, EPI_RESID, 0, SCALE_CTX, 1.0),
    ("tanh", 768, 768, EPI_TANH, 0, SCALE_X, 1.0),
]


@pytest.mark.parametrize("route", P_ROUTES, ids=[r[0] for r in P_ROUTES])
def test_cfgp_rows_equal_cfgc_rows_bit_for_bit(pkg, route):
    """gemm_split_kernel.h (CfgP) and DESIGN.md "Small launches take small tiles": CfgP's MFMA form, k order and term order are CfgC's,
    so a row recomputed in a small launch (CfgP) has the bits it had in a large one (CfgC)."""
    torch = _torch()
    name, N, K, epi, out_split, a_scale, out_scale = route
    cus = _cus()
    M = 256 * (_first_c_tiles(N, cus) - 1) + 77
    assert _split_cfg(M, N, cus) == "C"
    A, W, b, R, _ = _operands(M, N, K, epi, seed=7 + N + epi, gather=False)
    ws = _w_scale(W)
    full = _split_gemm(pkg, A, W, b, R, M, epi, out_split, a_scale, ws, out_scale)
    gen = torch.Generator(device="cpu").manual_seed(N + epi)
    pick = {0, 1, 255, 256, M - 1} | set(torch.randint(0, M, (11,), generator=gen).tolist())
    rows = torch.tensor(sorted(pick), dtype=torch.int32, device="cuda")
    assert _split_cfg(len(pick), N, cus) == "P"
    sub = _split_gemm(pkg, A, W, b, R, len(pick), epi, out_split, a_scale, ws, out_scale, rs=rows)
    same = bool(torch.equal(sub, full[rows.long()]))
    report_measured(f"cfgp_vs_cfgc[{name}]", "rows with differing bits", float((sub != full[rows.long()]).any(1).sum()))
    assert same, f"{name}: CfgP rows differ from CfgC rows"


@pytest.mark.parametrize("route", P_ROUTES, ids=[r[0] for r in P_ROUTES])
def test_split_gemm_rows_do_not_depend_on_batch_mates(pkg, route):
    """a document's bits do not depend on its batch mates or the batch size.  The same eight A rows are computed
    alone, at an odd offset inside a 128-row CfgP tile, and at an odd offset inside a 256-row CfgC tile of a large launch."""
    torch = _torch()
    name, N, K, epi, out_split, a_scale, out_scale = route
    cus = _cus()
    t = _first_c_tiles(N, cus)
    nA = 256 * t + 64
    A, W, b, R, _ = _operands(nA, N, K, epi, seed=11 + N + epi, gather=False)
    ws = _w_scale(W)
    probe = list(range(nA - 8, nA))                                 # the eight rows under test: the last ones of A (row_src is non-decreasing)
    layouts = {
        "alone": probe,                                              # positions 0..7
        "in_p_tile": list(range(0, 45)) + probe + [nA - 1] * 3,      # positions 45..52 of a CfgP tile
        "in_c_tile": list(range(0, 256 * (t - 1) + 141)) + probe,    # positions 141..148 of the last (ragged) CfgC tile
    }
    got = {}
    for lay, src in layouts.items():
        rs = torch.tensor(src, dtype=torch.int32, device="cuda")
        at = src.index(probe[0])
        assert (_split_cfg(len(src), N, cus) == "C") == (lay == "in_c_tile")
        got[lay] = _split_gemm(pkg, A, W, b, R, len(src), epi, out_split, a_scale, ws, out_scale, rs=rs)[at:at + 8]
    assert torch.equal(got["alone"], got["in_p_tile"]), name
    assert torch.equal(got["alone"], got["in_c_tile"]), name


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. the f32 GEMM (gemm_f32.hip): LDS-DMA kernel (epi | 256, what the path runs) and the register-staged one
# ---------------------------------------------------------------------------------------------------------------------------------------
def _f32_gemm(pkg, A, W, b, R, M, epi, wgs_per_cu, rs=None):
    torch = _torch()
    N, K = W.shape
    out = _guarded(M, N)
    lib = pkg.capi.load()
    pkg.capi.check(lib.ee_debug_gemm(_ptr(A), _ptr(W), _ptr(b), _ptr(R), _ptr(out), M, N, K, epi, wgs_per_cu, _ptr(rs), None, _stream()),
                   None, "ee_debug_gemm")
    torch.cuda.synchronize()
    _check_guard(out, M, "ee_debug_gemm")
    return out[:M]


def _f32_cases():
    """A covering set of the cross product: every (staging kernel, M) pair seven or eight times, the other axes drawn (no repeats)."""
    rng = np.random.default_rng(2024)
    Ms = [1, 127, 129, 4097]
    out = []
    while len(out) < 60:
        i = len(out)
        dma, M = i % 2, Ms[(i // 2) % 4]
        N, K = int(rng.choice([128, 768, 3072])), int(rng.choice([32, 768, 3072]))
        if M == 4097 and N == 3072 and K == 3072:
            K = 768                      # keep the largest operands to one size class (the suite's run time)
        c = (bool(dma), M, N, K, int(rng.integers(0, 4)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), int(rng.integers(0, 2)))
        if c not in out:
            out.append(c)
    for axis, values in enumerate([(False, True), Ms, (128, 768, 3072), (32, 768, 3072), (0, 1, 2, 3), (False, True), (False, True), (0, 1)]):
        assert {c[axis] for c in out} == set(values), axis
    return out


def _err32_k_sequential(A, W, b, R, rs, epi, ref):
    """max error of the textbook f32 GEMM: one f32 accumulator per output, k = 0, 1, ..., K - 1 in order, bias and epilogue after."""
    torch = _torch()
    At = (A[rs.long()] if rs is not None else A).t().contiguous()
    Wt = W.t().contiguous()
    acc = torch.zeros(At.shape[1], Wt.shape[1], dtype=torch.float32, device="cuda")
    for k in range(At.shape[0]):
        acc.addcmul_(At[k][:, None], Wt[k][None, :])
    Rg = None if R is None else (R[rs.long()] if rs is not None else R)
    return float((_epilogue(acc + b, epi, Rg).double() - ref).abs().max())


F32_CASES = _f32_cases()


def _f32_id(c):
    dma, M, N, K, epi, gather, static, wgs = c
    return f"{'dma' if dma else 'reg'}-M{M}-N{N}-K{K}-{EPI_NAMES[epi]}{'-rows' if gather else ''}{'-static' if static else ''}-w{wgs}"


@pytest.mark.parametrize("case", F32_CASES, ids=[_f32_id(c) for c in F32_CASES])
def test_f32_gemm_against_float64(pkg, case):
    torch = _torch()
    dma, M, N, K, epi, gather, static, wgs = case
    A, W, b, R, rs = _operands(M, N, K, epi, seed=M * 7 + N * 3 + K + epi, gather=gather)
    flags = epi | (256 if dma else 0) | (16 if static else 0)
    o1 = _f32_gemm(pkg, A, W, b, R, M, flags, wgs, rs)
    o2 = _f32_gemm(pkg, A, W, b, R, M, flags, wgs, rs)
    assert torch.equal(o1, o2), "two launches differ"
    got = o1.view(torch.float32).double()
    assert not got.isnan().any()
    ref, err32 = _ref_and_err32(A, W, b, R, rs, epi)
    err = float((got - ref).abs().max())
    # The yardstick is the larger of torch's f32 GEMM error and the k-sequential f32 loop's.  torch alone is not a fixed yardstick here:
    # at M <= 129 with K >= 768 its GEMM sums more accurately than any one-accumulator chain, and this kernel (one f32 MFMA accumulator
    # per output, k in order) measured up to 3.4x torch's error there (e.g. M 129, N 768, K 3072, GELU: 1.08e-05 against 3.17e-06)
    # while matching torch at M = 4097 (ratios 0.94-1.06) -- the kernel's error does not change with M, torch's algorithm does.
    # Against the k-sequential loop the kernel measured 0.89-1.38x over these cases; both numbers are reported.
    err_seq = _err32_k_sequential(A, W, b, R, rs, epi, ref)
    report_measured(f"f32_gemm[{_f32_id(case)}]", f"max|err| (err32 torch {err32:.3e}, k-sequential {err_seq:.3e})", err)
    assert err <= max(2.0 * max(err32, err_seq), 1e-6), (err, err32, err_seq)


@pytest.mark.parametrize("M,N,K,epi", [(129, 768, 768, EPI_BIAS), (4097, 3072, 768, EPI_GELU), (127, 768, 3072, EPI_RESID),
                                       (1, 128, 32, EPI_TANH)])
def test_f32_gemm_staging_kernels_agree(pkg, M, N, K, epi):
    """The two staging kernels are not claimed to be bit-equal (their k-loops differ): within the float64 rule of each other."""
    torch = _torch()
    A, W, b, R, rs = _operands(M, N, K, epi, seed=M + N + K + epi, gather=True)
    d = _f32_gemm(pkg, A, W, b, R, M, epi | 256, 0, rs).view(torch.float32).double()
    r = _f32_gemm(pkg, A, W, b, R, M, epi, 0, rs).view(torch.float32).double()
    _, err32 = _ref_and_err32(A, W, b, R, rs, epi)
    diff = float((d - r).abs().max())
    report_measured(f"f32_gemm_dma_vs_reg[M={M},N={N},K={K},{EPI_NAMES[epi]}]", f"max|dma - reg| (err32 {err32:.3e}, bit-equal {bool(diff == 0)})",
                    diff)
    assert diff <= max(2.0 * err32, 1e-6), (diff, err32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. label counts other than 16, against the live oracle
# ---------------------------------------------------------------------------------------------------------------------------------------
K_CASES = [(shape, K, strategy) for shape in ("tiny", "h256") for K in (2, 10, 64) for strategy in ("ramp", "gate")]


def _k_config(pkg, shape, K, strategy, criterion="max_confidence"):
    ee = dict(exits=["text_avg", "text_visual_concat", 1, 2, 3], encoder_layer_strategy=strategy, inference_strategy=criterion)
    kw = dict(H256_KW) if shape == "h256" else dict(num_hidden_layers=3)
    return pkg.ModelConfig.tiny(EE_config=ee, num_labels=K, **kw), ee


def _conf_thr(oracle, store):
    """A threshold in the widest gap of the middle half of all max-softmax confidences."""
    conf = oracle.softmax64(store).max(-1)
    s = np.sort(conf.ravel())
    k = int(np.argmax(np.diff(s)[len(s) // 4: 3 * len(s) // 4])) + len(s) // 4
    thr = 0.5 * (s[k] + s[k + 1])
    assert np.abs(conf - thr).min() > 1e-5
    return thr


@pytest.mark.parametrize("shape,K,strategy", K_CASES)
def test_label_count_vs_oracle(pkg, oracle, shape, K, strategy):
    """head_out / exit_decide / compaction at K != 16 (K = 2 with the gate: policy and gate logits of one width): dump-all rows and head
    logits against oracle.forward_all, then early exit at a threshold in a gap, dense and ragged rows, every schedule."""
    cfg, ee = _k_config(pkg, shape, K, strategy)
    W = pkg.synth.make_weights(cfg, seed=40 + K, head_gain=6.0)
    docs = pkg.synth.make_documents(cfg, 7, seed=50 + K, text_len=40, min_words=2)
    ref = oracle.forward_all(cfg, W, docs, ee["exits"], strategy=strategy)
    assert ref["logits_store"].shape[-1] == K
    precision = "split" if shape == "h256" else "fp32"
    eng = pkg.EarlyExitEngine(cfg, max_docs=8, max_text_len=40, precision=precision, xprobe=False)
    assert eng.precision == precision
    eng.load_weights(W)
    args = (docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"])
    for dense in (False, True):
        out = eng.forward(*args, dump_all=True, dense_rows=dense, want_all=True, want_head=True, validate=True)
        al, hl = out.all_logits.cpu().numpy(), out.head_logits.cpu().numpy()
        assert al.shape == ref["logits_store"].shape and hl.shape == ref["exit_logits"].shape
        report_measured(f"labels[{shape},K={K},{strategy},dense={int(dense)}]", "max|dlogit|", float(np.abs(al - ref["logits_store"]).max()))
        np.testing.assert_allclose(al, ref["logits_store"], rtol=0, atol=LOGIT_TOL)
        np.testing.assert_allclose(hl, ref["exit_logits"], rtol=0, atol=LOGIT_TOL)
    thr = _conf_thr(oracle, ref["logits_store"])
    ex, pred, _ = oracle.policy_scan(ref["logits_store"], thr)
    for dense in (False, True):
        for kw in (dict(), dict(whole_layers=True), dict(probe_always=True)):
            o = eng.forward(*args, thresholds=thr, dense_rows=dense, **kw)
            assert np.array_equal(o.exit_layer.cpu().numpy(), ex), (dense, kw)
            np.testing.assert_allclose(o.logits.cpu().numpy(), pred, rtol=0, atol=LOGIT_TOL)
    eng.close()


def test_label_count_entropy_vs_oracle(pkg, oracle):
    """The entropy criterion at K = 10 (split kernels, H = 256): head criteria against the oracle, and early exit with the criterion's own
    sign (entropy BELOW the threshold, EE/models/EE_modules.py:137-144) at thresholds in the widest gap of each exit's entropies."""
    K = 10
    cfg, ee = _k_config(pkg, "h256", K, "ramp", criterion="entropy")
    W = pkg.synth.make_weights(cfg, seed=61, head_gain=6.0)
    docs = pkg.synth.make_documents(cfg, 7, seed=62, text_len=40, min_words=2)
    ref = oracle.forward_all(cfg, W, docs, ee["exits"], strategy="ramp", criterion="entropy")
    eng = pkg.EarlyExitEngine(cfg, max_docs=8, max_text_len=40, precision="split", xprobe=False)
    eng.load_weights(W)
    args = (docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"])
    out = eng.forward(*args, dump_all=True, want_all=True, want_head=True, validate=True)
    np.testing.assert_allclose(out.all_logits.cpu().numpy(), ref["logits_store"], rtol=0, atol=LOGIT_TOL)
    np.testing.assert_allclose(out.head_logits.cpu().numpy(), ref["exit_logits"], rtol=0, atol=LOGIT_TOL)
    np.testing.assert_allclose(out.head_crit.cpu().numpy(), ref["exit_crit"], rtol=0, atol=2e-5 * max(1.0, float(np.abs(ref["exit_crit"]).max())))
    x = ref["logits_store"].astype(np.float64)
    ent = np.log(np.exp(x).sum(-1)) - (x * np.exp(x)).sum(-1) / np.exp(x).sum(-1)          # EE/models/EE_modules.py:149-154
    E1 = ent.shape[0]
    margin = 1e-4 * max(1.0, float(np.abs(ent).max()))
    thr = np.zeros(E1)
    for e in range(E1):
        srt = np.sort(ent[e])
        k = int(np.argmax(np.diff(srt)))
        thr[e] = 0.5 * (srt[k] + srt[k + 1]) if srt[k + 1] - srt[k] > 4 * margin else -1.0
    assert np.abs(ent - thr[:, None]).min() > margin
    hit = ent < thr[:, None]
    hit[-1] = True
    ex = hit.argmax(0).astype(np.int32)
    assert len(np.unique(ex)) >= 2
    for dense in (False, True):
        o = eng.forward(*args, thresholds=thr, dense_rows=dense)
        assert np.array_equal(o.exit_layer.cpu().numpy(), ex)
        np.testing.assert_allclose(o.logits.cpu().numpy(), x[ex, np.arange(x.shape[1])], rtol=0, atol=LOGIT_TOL)
    eng.close()


def test_label_count_per_exit_temperatures_vs_oracle(pkg, oracle):
    """Per-exit temperatures and thresholds at K = 10 (split kernels): exits, predictions and confidences against the oracle's policy."""
    K = 10
    cfg, ee = _k_config(pkg, "h256", K, "gate")
    W = pkg.synth.make_weights(cfg, seed=71, head_gain=6.0)
    docs = pkg.synth.make_documents(cfg, 7, seed=72, text_len=40, min_words=2)
    ref = oracle.forward_all(cfg, W, docs, ee["exits"], strategy="gate")
    E1 = ref["logits_store"].shape[0]
    temps = np.random.default_rng(3).uniform(0.5, 3.0, E1)
    store = oracle.temperature_scale(ref["logits_store"], temps)
    conf = oracle.softmax64(store).max(-1)
    thr = np.zeros(E1)
    for e in range(E1):
        s = np.sort(conf[e])
        k = int(np.argmax(np.diff(s)))
        thr[e] = 0.5 * (s[k] + s[k + 1])
    assert np.abs(conf - thr[:, None]).min() > 1e-4
    ex, pred, cf = oracle.policy_scan(store, thr)
    eng = pkg.EarlyExitEngine(cfg, max_docs=8, max_text_len=40, precision="split", xprobe=False)
    eng.load_weights(W)
    for dense in (False, True):
        o = eng.forward(docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"], thresholds=thr, temperatures=temps,
                        dense_rows=dense)
        assert np.array_equal(o.exit_layer.cpu().numpy(), ex)
        np.testing.assert_allclose(o.logits.cpu().numpy(), pred, rtol=0, atol=LOGIT_TOL)
        np.testing.assert_allclose(o.confidence.cpu().numpy(), cf, rtol=0, atol=1e-4)
    eng.close()


@pytest.mark.parametrize("K", [2, 10, 64])
def test_result_rows_at_label_counts(pkg, K):
    """ee_pack_results / ee_unpack_results at K != 16: the host form of dist.pack_results, word for word."""
    torch = _torch()
    lib = pkg.capi.load()
    n = 777
    lg = torch.randn(n, K, device="cuda")
    lg[3, K - 1] = float("nan")
    lg[4, 0] = 1e-42
    ex = (torch.arange(n, device="cuda", dtype=torch.int32) % 7) - 1
    cf = torch.rand(n, device="cuda")
    ref = pkg.dist.pack_results(lg, ex, cf)
    rows = torch.full((n + 4, K + 2), SENTINEL, dtype=torch.int32, device="cuda")
    st = _stream()
    pkg.capi.check(lib.ee_pack_results(_ptr(lg), _ptr(ex), _ptr(cf), n, K, _ptr(rows), st), None, "ee_pack_results")
    torch.cuda.synchronize()
    assert torch.equal(rows[:n], ref)
    assert torch.equal(rows[n:], torch.full_like(rows[n:], SENTINEL))
    lg2, ex2, cf2 = torch.empty_like(lg), torch.empty_like(ex), torch.empty_like(cf)
    pkg.capi.check(lib.ee_unpack_results(_ptr(rows), n, K, _ptr(lg2), _ptr(ex2), _ptr(cf2), st), None, "ee_unpack_results")
    torch.cuda.synchronize()
    assert torch.equal(lg2.view(torch.int32), lg.view(torch.int32)) and torch.equal(ex2, ex) and torch.equal(cf2, cf)


@pytest.mark.parametrize("K", [2, 10, 64])
def test_policy_scan_device_at_label_counts(pkg, oracle, K):
    """ee_policy_scan on a random (E+1, N, K) store against oracle.policy_scan: exits equal, predictions and confidences to float64 rounding."""
    rng = np.random.default_rng(100 + K)
    E1, N = 6, 3001
    store = rng.standard_normal((E1, N, K)) * np.linspace(1.0, 4.0, E1)[:, None, None]
    conf = oracle.softmax64(store).max(-1)
    thr = np.zeros(E1)
    for e in range(E1):                                          # per exit, the widest gap around the 60 % quantile of its confidences
        c = np.sort(conf[e])
        j = int(0.6 * N) - 8 + int(np.argmax(np.diff(c[int(0.6 * N) - 9: int(0.6 * N) + 8])))
        thr[e] = 0.5 * (c[j] + c[j + 1])
    assert np.abs(conf - thr[:, None]).min() > 1e-12
    ex, pred, cf = oracle.policy_scan(store, thr)
    gex, gpred, gcf, counts = pkg.policy.policy_scan_device(store, thr, want_conf=True)
    assert np.array_equal(gex.cpu().numpy(), ex)
    assert len(np.unique(ex)) >= 3
    np.testing.assert_array_equal(gpred.cpu().numpy(), pred)
    np.testing.assert_allclose(gcf.cpu().numpy(), cf, rtol=1e-12, atol=0)
    assert counts.cpu().numpy().tolist() == np.bincount(ex, minlength=E1).tolist()
