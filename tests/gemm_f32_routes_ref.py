"""Inputs and float64 references of tests/test_gpu_gemm_f32_routes.py, on the CPU (the pattern of tests/gemm_routes_ref.py): the operands are drawn
here (numpy, so that a machine without a GPU has the same ones), the GPU tests copy them to the device, and tests/test_host_gemm_f32_routes.py
shows on them that each fault the f32 GEMM (csrc/gemm_f32.hip) can have in an operand only a forward sets moves the float64 reference by at least
ten times the tolerance the GPU test applies.

The operation, as gemm_store_tile writes it:
    C[r] = epi((A[row_src[r]] W^T + b) * (column < scale_cols ? scale : 1)) * col_scale (+ resid[resid_row_src[r]])      for r < M, nothing else

Acceptance rule (tests/test_gpu_kernels.py test_f32_gemm_against_float64): max|got - ref64| <= max(2 * max(err32, err_seq), 1e-6); err32 = the
error of torch's f32 GEMM with the same epilogue, err_seq = that of the k-sequential one-accumulator f32 loop, both over EVERY row of operand
tensors of at least MIN_ROWS rows (A row i with residual row i: a yardstick is a property of the operands' distribution, not of a row map) and
never on the kernel under test."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
EPI_BIAS, EPI_GELU, EPI_RESID, EPI_TANH = 0, 1, 2, 3
EPIS = (EPI_BIAS, EPI_GELU, EPI_RESID, EPI_TANH)
EPI_NAMES = {EPI_BIAS: "bias", EPI_GELU: "gelu", EPI_RESID: "resid", EPI_TANH: "tanh"}
MIN_ROWS = 296                 # rows of every operand tensor the yardsticks are taken over
ROWS = 300                     # the operand tensors of every case but the queue-group ones
BM, BN, BK = 128, 128, 32      # the tile of gemm_f32.hip
GM, QUEUES = 8, 8              # m-panels per group, XCD-local queues: queue q owns groups q, q + 8, ...

# M on the device: (M, max_m).  An empty stage in a one-tile and a three-tile launch; one row under two tiles; the last row of a tile missing with
# max_m on the edge; a full tile under five; one row into the second tile; a ragged third tile under nine (more than one group)
M_ON_DEVICE = [(0, 1), (0, 300), (1, 129), (127, 128), (128, 513), (129, 130), (257, 1100)]
M_ON_DEVICE_N, M_ON_DEVICE_K = 256, 64
# a residual map of its own
RESID_NS, RESID_K, RESID_MS = (128, 256), 64, (1, 129, 257)
RESID_COMBOS = ("a_dense_resid_mapped", "both_mapped", "a_mapped_resid_dense")
MAP_KINDS = ("sorted", "shuffled")
# Q / sqrt(d) over the leading columns of a fused Q | K | V GEMM
QSCALE_N, QSCALE_K, QSCALE_M, QSCALE = 384, 64, 129, 0.125
QSCALE_COLS = (0, 128, 256, 384)
QSCALE_EPIS = (EPI_BIAS, EPI_GELU)
# BEiT's lambda
LAMBDA_N, LAMBDA_K, LAMBDA_M = 256, 64, 129
# more than one m-group per queue: 65 and 129 m-panels = 9 and 17 groups, queue 0 owns 2 and 3 of them, the last one of one panel
GROUP_MS, GROUP_N, GROUP_K = (8193, 16385), 256, 32
# batch mates
MATES_N, MATES_K = 256, 64


def operands(rows, N, K, seed, resid=False):
    """A [rows, K], W [N, K], b [N] (and R [rows, N]) float32.  One stream per tensor: W and b do not depend on `rows`, and the first rows of A
    and R are the same for every `rows`."""
    draw = lambda tag, shape: np.random.default_rng([seed, N, K, tag]).standard_normal(shape, dtype=F32)
    A = draw(0, (rows, K))
    W = draw(1, (N, K)) * F32(0.02)
    b = draw(2, (N,))
    R = draw(3, (rows, N)) if resid else None
    return A, W, b, R


def lambda_vector(N, seed):
    """BEiT's layer scale as the issue draws it: 1 + 0.5 N(0, 1)."""
    return (1.0 + 0.5 * np.random.default_rng([seed, N, 11]).standard_normal(N)).astype(F32)


def row_map(M, rows, seed, kind="sorted"):
    """"sorted": non-decreasing with repeats, as the row map behind a compaction is; "shuffled": the same entries in a drawn order, as the heads'
    gather of CLS rows may be."""
    rng = np.random.default_rng([seed, M, rows, 7])
    m = np.sort(rng.integers(0, rows, M)).astype(np.int32)
    return m if kind == "sorted" else rng.permutation(m).astype(np.int32)


def differing_map(base, rows, seed):
    """A map into `rows` rows that differs from `base` in every entry."""
    base = np.asarray(base, np.int64)
    step = np.random.default_rng([seed, len(base), rows, 13]).integers(1, rows, len(base))
    out = ((base + step) % rows).astype(np.int32)
    assert (out != base).all()
    return out


def resid_case_maps(combo, kind, M, rows, seed):
    """(row_src, resid_row_src) of a residual-map case; None = dense.  The residual's map differs in every entry from A's (from the output row
    where A is dense)."""
    rs = None if combo == "a_dense_resid_mapped" else row_map(M, rows, seed, kind)
    if combo == "a_mapped_resid_dense":
        if M > 1:
            assert (rs != np.arange(M)).any()
        return rs, None
    return rs, differing_map(np.arange(M) if rs is None else rs, rows, seed)


def mates_layouts(rows):
    """The row maps of the batch-mates case: the last eight rows of A alone, at positions 249 .. 256 of a 257-row launch (the end of its second
    tile and the one row of its ragged third), and at positions 8185 .. 8192 of an 8193-row launch (the end of m-panel 63 and the one row of
    m-panel 64 = group 8, the second group of queue 0: M = 8193 has no other row there).  name -> (map, position of the first probe row)."""
    probe = np.arange(rows - 8, rows)
    fill = lambda n: np.arange(n) % (rows - 8)
    return {"alone": (probe.astype(np.int32), 0),
            "tail_of_257": (np.concatenate([fill(249), probe]).astype(np.int32), 249),
            "group_8_of_8193": (np.concatenate([fill(8185), probe]).astype(np.int32), 8185)}


def tolerance(err32, err_seq):
    return max(2.0 * max(float(err32), float(err_seq)), 1e-6)


def _erf64(x):
    import torch
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=F64))).numpy()


def epilogue(x, epi):
    """GELU (erf form) / tanh in the precision of x; the identity for the bias and residual epilogues."""
    if epi == EPI_GELU:
        if x.dtype == F64:
            return x * 0.5 * (1.0 + _erf64(x * 0.70710678118654752440))
        import torch
        return torch.nn.functional.gelu(torch.from_numpy(np.ascontiguousarray(x))).numpy()
    return np.tanh(x) if epi == EPI_TANH else x


# ---------------------------------------------------------------------------------------------------------------------------------------
# the float64 reference, with the faults the GPU tests must be able to see (mut)
# ---------------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("resid_by_a_map", "resid_by_out_row", "scale_one_tile_more", "scale_one_tile_less", "scale_behind_epilogue", "lambda_on_residual",
             "lambda_in_front_of_epilogue", "clamped_row_written", "second_group_dropped")


def ref64(A, W, b, epi, M, *, row_src=None, resid=None, resid_row_src=None, scale_cols=0, scale=1.0, col_scale=None, rows_out=None, mut=""):
    """(C [rows_out, N] float64, written [rows_out] bool): what a launch leaves in an output buffer of rows_out >= M rows.  Rows the kernel does
    not write are NaN in C, as the sentinel of the GPU tests' buffers is."""
    assert mut == "" or mut in MUTATIONS, mut
    N = W.shape[0]
    rows_out = M if rows_out is None else rows_out
    C = np.full((rows_out, N), np.nan, F64)
    written = np.zeros(rows_out, bool)
    if M == 0:
        return C, written
    out_row = np.arange(M)
    rs = out_row if row_src is None else np.asarray(row_src[:M], np.int64)
    x = np.asarray(A, F64)[rs] @ np.asarray(W, F64).T + (0.0 if b is None else np.asarray(b, F64))
    cols = scale_cols + (BN if mut == "scale_one_tile_more" else -BN if mut == "scale_one_tile_less" else 0)
    sc = np.where(np.arange(N) < min(max(cols, 0), N), F64(scale), 1.0)
    lam = np.ones(N, F64) if col_scale is None else np.asarray(col_scale, F64)
    if mut == "scale_behind_epilogue":
        y = epilogue(x, epi) * sc * lam
    elif mut == "lambda_in_front_of_epilogue":
        y = epilogue(x * sc * lam, epi)
    else:
        y = epilogue(x * sc, epi) * lam
    if epi == EPI_RESID:
        rr = out_row if resid_row_src is None else np.asarray(resid_row_src[:M], np.int64)
        if mut == "resid_by_a_map":
            rr = rs
        if mut == "resid_by_out_row":
            rr = out_row
        y = y + np.asarray(resid, F64)[rr] * (lam if mut == "lambda_on_residual" else 1.0)
    C[:M] = y
    written[:M] = True
    if mut == "clamped_row_written":                            # the staging clamp r = min(r, M - 1) reaching the store
        assert rows_out > M
        C[M] = C[M - 1]
        written[M] = True
    if mut == "second_group_dropped":                           # gl >= 1 never taken: queue 0 stops behind its first group
        first = QUEUES * GM * BM                                # m-panel 64 = the first row of group 8
        C[first:] = np.nan
        written[first:] = False
    return C, written


# ---------------------------------------------------------------------------------------------------------------------------------------
# the yardsticks on the CPU (tests/test_host_gemm_f32_routes.py; the GPU tests take theirs on the device by the same expressions)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _finish32(acc, b, epi, resid, scale_cols, scale, col_scale):
    """bias, scale, epilogue function, lambda and the dense residual behind an f32 product, every step in f32 in the kernel's order."""
    N = acc.shape[1]
    x = (acc + b).astype(F32)
    if scale_cols:
        x = (x * np.where(np.arange(N) < scale_cols, F32(scale), F32(1.0)).astype(F32)).astype(F32)
    y = np.asarray(epilogue(x, epi), F32)
    if col_scale is not None:
        y = (y * np.asarray(col_scale, F32)).astype(F32)
    if epi == EPI_RESID:
        y = (y + resid).astype(F32)
    return y


def yardsticks(A, W, b, epi, *, resid=None, scale_cols=0, scale=1.0, col_scale=None):
    """(err32, err_seq) over every row of A (with residual row i for A row i): torch's f32 GEMM and the k-sequential one-accumulator loop."""
    import torch
    assert A.shape[0] >= MIN_ROWS
    ref, _ = ref64(A, W, b, epi, A.shape[0], resid=resid, scale_cols=scale_cols, scale=scale, col_scale=col_scale)
    kw = dict(scale_cols=scale_cols, scale=scale, col_scale=col_scale)
    g32 = (torch.from_numpy(A) @ torch.from_numpy(W).t()).numpy()
    seq = np.zeros((A.shape[0], W.shape[0]), F32)
    for k in range(A.shape[1]):
        seq += A[:, k, None] * W[None, :, k]
    err = lambda acc: float(np.abs(_finish32(acc, b, epi, resid, **kw).astype(F64) - ref).max())
    return err(g32), err(seq)


@functools.lru_cache(maxsize=None)
def small_operands(N, K, seed):
    """The ROWS-row operand set of a small case, drawn once: (A, W, b, R)."""
    return operands(ROWS, N, K, seed, resid=True)
