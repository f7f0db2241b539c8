"""Inputs and float64 references of tests/test_gpu_gemm_routes.py, on the CPU: the operands are drawn here (numpy, so that a machine without a GPU
has the same ones), the GPU tests copy them to the device, and tests/test_host_gemm_routes.py shows on them that each of the faults a route of
launch_gemm_split can have moves the float64 reference by at least ten times the tolerance the GPU test applies.

Acceptance rule (tests/test_gpu_kernels.py, tests/test_gpu_gemm_resid.py): max|got - ref64| <= max(2 * err32, 1e-6), err32 = the error of torch's
f32 GEMM on the same operands, over every row of operand tensors of at least 296 rows."""
import numpy as np

F32, F64 = np.float32, np.float64
EPI_BIAS, EPI_GELU, EPI_RESID, EPI_TANH = 0, 1, 2, 3
SCALE_X, SCALE_CTX, SCALE_H1, SCALE_QKV = 16.0, 64.0, 16.0, 16.0      # csrc/mmee_common.h kSplitScaleX / Ctx / H1 / QKV
SPLIT_CLAMP = 60000.0                                                  # kSplitClamp
MIN_ROWS = 296                                                         # rows of every operand tensor err32 is taken over

# The split-K cases: (N, K, S, kind).  kind "ctx": the attention-output GEMM's A operand (context rows, 0.25 x N(0, 1) under kSplitScaleCtx),
# "h1": the FFN-down GEMM's (N(0, 1) under kSplitScaleH1); tests/test_gpu_gemm_resid.py's docstring says why the two differ.
#   stages per part: 1, 2 (X-space probe at a small intermediate size: shorter than CfgP's three-deep ring), 3 (the minimum of
#   ee_low_latency_k_splits; the base attention output), 4, 24, 12, 16
SPLIT_K_CASES = [
    (256, 128, 4, "h1"), (256, 256, 4, "h1"), (256, 192, 2, "ctx"), (256, 256, 2, "ctx"),
    (768, 768, 8, "ctx"), (768, 3072, 4, "h1"), (768, 3072, 8, "h1"), (1024, 4096, 8, "h1"),
]
KIND = {"ctx": (0.25, SCALE_CTX), "h1": (1.0, SCALE_H1), "x": (1.0, SCALE_X)}      # kind -> (gain of A, plane scale of A)

# The one-term kernels: (name, N, epilogue, split output, kind of A, output scale, role_tag, Ks)
ONE_TERM = [
    ("gelu_split_out", 3072, EPI_GELU, 1, "x", SCALE_H1, 0, (32, 64, 96, 768)),
    ("bias_split_out", 2304, EPI_BIAS, 1, "x", SCALE_QKV, 0, (32, 64, 96, 768)),
    ("resid_role2", 768, EPI_RESID, 0, "ctx", 1.0, 2, (32, 64, 96, 768)),
    ("resid_role3", 768, EPI_RESID, 0, "h1", 1.0, 3, (32, 64, 96, 768, 3072)),
]
ONE_TERM_REMS = (1, 128, 129)

# the epilogue operands: Q / sqrt(d) over the first third of a fused Q | K | V GEMM, BEiT's per-column factor on a residual GEMM
QSCALE_N, QSCALE_K, QSCALE = 768, 256, 0.125
LAMBDA_N, LAMBDA_K = 768, 768


def operands(rows, N, K, kind, seed, resid=False):
    """A [rows, K], W [N, K], b [N] (and R [rows, N]) float32.  One stream per tensor: W and b do not depend on `rows`, and the first rows of A
    are the same for every `rows`."""
    gain, _ = KIND[kind]
    draw = lambda tag, shape: np.random.default_rng([seed, N, K, tag]).standard_normal(shape, dtype=F32)
    A = draw(0, (rows, K)) * F32(gain)
    W = draw(1, (N, K)) * F32(0.02)
    b = draw(2, (N,))
    R = draw(3, (rows, N)) if resid else None
    return A, W, b, R


def row_map(M, rows, seed):
    """Non-decreasing with repeats, as the row map behind a compaction is."""
    return np.sort(np.random.default_rng([seed, M, rows, 7]).integers(0, rows, M)).astype(np.int32)


def w_scale(W):
    """ee_finalize's weight scale: the power of two that puts max|w| in [2^12, 2^13), capped at 2^8 (tests/test_gpu_kernels.py _w_scale)."""
    mx = float(np.abs(W).max())
    return float(2.0 ** (8 if mx == 0.0 else min(8, 13 - int(np.frexp(mx)[1]))))


def hi_plane(x, scale):
    """The hi plane of a split row as a value: fp16(clamp(scale * x)) / scale, float32 (exact)."""
    xs = np.clip(np.asarray(x, F32) * F32(scale), -SPLIT_CLAMP, SPLIT_CLAMP)
    return (xs.astype(np.float16).astype(F32) / F32(scale)).astype(F32)


def planes_value(x, scale):
    """hi + lo of a split row as a value, float32 (22 bits: exact)."""
    xs = np.clip(np.asarray(x, F32) * F32(scale), -SPLIT_CLAMP, SPLIT_CLAMP)
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(F32)).astype(np.float16)
    return ((hi.astype(F32) + lo.astype(F32)) / F32(scale)).astype(F32)


def k_slice(K, S, p):
    return slice(p * (K // S), (p + 1) * (K // S))


def product64(A, W, ks=slice(None)):
    return np.asarray(A, F64)[:, ks] @ np.asarray(W, F64)[:, ks].T


def tolerance(err32):
    return max(2.0 * float(err32), 1e-6)


def err32_of(f32_result, ref64):
    return float(np.abs(np.asarray(f32_result, F64) - ref64).max())


def gemm32(A, W, ks=slice(None)):
    """torch's float32 GEMM on the CPU: the yardstick of the host tests."""
    import torch
    a, w = torch.from_numpy(np.ascontiguousarray(A[:, ks])), torch.from_numpy(np.ascontiguousarray(W[:, ks]))
    return (a @ w.t()).numpy()


# ---------------------------------------------------------------------------------------------------------------------------------------
# references, with the faults the tests must be able to see (mut)
# ---------------------------------------------------------------------------------------------------------------------------------------
def split_k_parts_ref(A, W, b, S, mut=""):
    """float64 [S, rows, N]: part p = A[:, slice p] W[:, slice p]^T; no bias (the LayerNorm kernel behind the GEMM adds it)."""
    K = A.shape[1]
    parts = []
    for p in range(S):
        ks = k_slice(K, S, p)
        if mut == "neighbour_slice" and p == 1:
            ks = k_slice(K, S, (p + 1) % S)                     # a wrong kt0
        if mut == "drop_last_stage" and p == S - 1:
            ks = slice(ks.start, ks.stop - 32)                  # nk rounded down
        parts.append(product64(A, W, ks))
        if mut == "bias_on_every_part":
            parts[-1] = parts[-1] + np.asarray(b, F64)
    if mut == "parts_exchanged":                                # a wrong c_shift / ks_pop
        parts[0], parts[1] = parts[1], parts[0]
    return np.stack(parts)


def completed_ref(parts64, b, mut=""):
    """What ln_rows<PRE> completes: the parts, then the bias."""
    return parts64.sum(0) + np.asarray(b, F64)


def q_scale_ref(A, W, b, scale_cols, scale, mut=""):
    """(A W^T + b) with columns [0, scale_cols) multiplied by scale."""
    y = product64(A, W) + np.asarray(b, F64)
    n = scale_cols + 1 if mut == "scale_one_column_more" else scale_cols
    y[:, :n] *= scale
    return y


def col_scale_ref(A, W, b, lam, Rq, mut=""):
    """(A W^T + b) lam + R: the factor in front of the residual."""
    y = (product64(A, W) + np.asarray(b, F64)) * np.asarray(lam, F64)
    return y + np.asarray(Rq, F64) * (np.asarray(lam, F64) if mut == "lambda_on_residual" else 1.0)


def one_term_operands(A, W, a_scale, ws):
    return hi_plane(A, a_scale), hi_plane(W, ws)


def three_term_operands(A, W, a_scale, ws):
    return planes_value(A, a_scale), planes_value(W, ws)
