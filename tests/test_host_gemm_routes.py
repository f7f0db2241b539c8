"""CPU-side proof that tests/test_gpu_gemm_routes.py can see a fault (as tests/test_host_rows_ref.py is for the row kernels), and the agreement of
the split-K rule with the hook's divisibility refusal.

On the operands of the GPU tests (tests/gemm_routes_ref.py draws them on the CPU), the float64 reference of every faulted variant below differs
from the true reference by at least ten times the tolerance the GPU test applies there: max(2 err32, 1e-6), err32 = the error of torch's f32 GEMM
on the CPU on the same operands."""
import itertools

import numpy as np
import pytest

from . import gemm_routes_ref as G

ROWS = 300                       # at least G.MIN_ROWS rows, as the GPU tests' operand tensors


def _maxdiff(a, b):
    return float(np.abs(a - b).max())


@pytest.mark.parametrize("case", G.SPLIT_K_CASES, ids=[f"N{c[0]}-K{c[1]}-S{c[2]}" for c in G.SPLIT_K_CASES])
def test_split_k_faults_move_the_reference(case):
    N, K, S, kind = case
    assert ROWS >= G.MIN_ROWS
    A, W, b, _ = G.operands(ROWS, N, K, kind, seed=N + K)
    true = G.split_k_parts_ref(A, W, b, S)
    tol_part = [G.tolerance(G.err32_of(G.gemm32(A, W, G.k_slice(K, S, p)), true[p])) for p in range(S)]
    full = G.completed_ref(true, b)
    tol_full = G.tolerance(G.err32_of(G.gemm32(A, W) + b, full))
    assert _maxdiff(full, G.product64(A, W) + b.astype(np.float64)) <= 1e-12      # the parts are the product
    # a part summed over the neighbouring K slice: the part and the completed row are wrong
    bad = G.split_k_parts_ref(A, W, b, S, "neighbour_slice")
    assert _maxdiff(bad[1], true[1]) >= 10 * tol_part[1]
    assert _maxdiff(G.completed_ref(bad, b), full) >= 10 * tol_full
    # two parts exchanged: every per-part check fails, the sum cannot
    bad = G.split_k_parts_ref(A, W, b, S, "parts_exchanged")
    assert _maxdiff(bad[0], true[0]) >= 10 * tol_part[0] and _maxdiff(bad[1], true[1]) >= 10 * tol_part[1]
    assert _maxdiff(G.completed_ref(bad, b), full) <= tol_full
    # a part missing its last stage
    if K // 32 // S > 1:
        bad = G.split_k_parts_ref(A, W, b, S, "drop_last_stage")
        assert _maxdiff(bad[S - 1], true[S - 1]) >= 10 * tol_part[S - 1]
        assert _maxdiff(G.completed_ref(bad, b), full) >= 10 * tol_full
    else:                                                        # a one-stage part: the whole part is gone
        assert _maxdiff(np.zeros_like(true[S - 1]), true[S - 1]) >= 10 * tol_part[S - 1]
    # the bias added to every part
    bad = G.split_k_parts_ref(A, W, b, S, "bias_on_every_part")
    assert min(_maxdiff(bad[p], true[p]) / tol_part[p] for p in range(S)) >= 10
    assert _maxdiff(G.completed_ref(bad, b), full) >= 10 * tol_full


def test_epilogue_operand_faults_move_the_reference():
    N, K, scale, cols = G.QSCALE_N, G.QSCALE_K, G.QSCALE, G.QSCALE_N // 3
    A, W, b, _ = G.operands(ROWS, N, K, "x", seed=9)
    true = G.q_scale_ref(A, W, b, cols, scale)
    f32 = G.gemm32(A, W) + b
    f32[:, :cols] *= np.float32(scale)
    tol = G.tolerance(G.err32_of(f32, true))
    bad = G.q_scale_ref(A, W, b, cols, scale, "scale_one_column_more")
    assert _maxdiff(bad[:, cols], true[:, cols]) >= 10 * tol and _maxdiff(bad[:, :cols], true[:, :cols]) == 0.0

    N, K = G.LAMBDA_N, G.LAMBDA_K
    A, W, b, R = G.operands(ROWS, N, K, "ctx", seed=13, resid=True)
    lam = (1.0 + 0.5 * np.random.default_rng(13).standard_normal(N)).astype(np.float32)
    Rq = G.planes_value(R, G.SCALE_X)
    true = G.col_scale_ref(A, W, b, lam, Rq)
    tol = G.tolerance(G.err32_of((G.gemm32(A, W) + b) * lam + Rq, true))
    assert _maxdiff(G.col_scale_ref(A, W, b, lam, Rq, "lambda_on_residual"), true) >= 10 * tol


ONE_TERM_CASES = [(spec, K) for spec in G.ONE_TERM for K in spec[7]]


@pytest.mark.parametrize("spec,K", ONE_TERM_CASES, ids=[f"{s[0]}-K{K}" for s, K in ONE_TERM_CASES])
def test_term_count_faults_move_the_reference(spec, K):
    """The lo planes included in a one-term product, and omitted from a three-term one: the two references are further apart than ten times
    either tolerance (the epilogues are 1-Lipschitz or the identity; the difference is taken in front of them, the yardstick too)."""
    name, N, epi, _, kind, _, role_tag, _ = spec
    _, a_scale = G.KIND[kind]
    A, W, b, _ = G.operands(ROWS, N, K, kind, seed=K + epi + role_tag)
    ws = G.w_scale(W)
    Ah, Wh = G.one_term_operands(A, W, a_scale, ws)
    one, three = G.product64(Ah, Wh) + b.astype(np.float64), G.product64(A, W) + b.astype(np.float64)
    tol_one = G.tolerance(G.err32_of(G.gemm32(Ah, Wh) + b, one))
    tol_three = G.tolerance(G.err32_of(G.gemm32(A, W) + b, three))
    assert _maxdiff(one, three) >= 10 * max(tol_one, tol_three), (name, K, _maxdiff(one, three), tol_one, tol_three)
    Ap, Wp = G.three_term_operands(A, W, a_scale, ws)           # what the three terms read: within the tolerance of the f32 operands
    assert _maxdiff(G.product64(Ap, Wp) + b.astype(np.float64), three) <= tol_three


def test_low_latency_rule_divides_the_k_stages(pkg):
    """ee_low_latency_k_splits never returns an S that ee_debug_gemm_routes refuses ((K / 32) % S != 0: the kernel's nk = K / 32 / S would drop
    the tail): every N, K among the multiples of 128 up to 1024 / 4096, a few row and CU counts."""
    rule = pkg.capi.load().ee_low_latency_k_splits
    for N, K, rows, cus in itertools.product(range(128, 1025, 128), range(128, 4097, 128), (1, 129, 709, 5672), (64, 256, 304)):
        S = int(rule(rows, N, K, cus))
        assert S in (1, 2, 4, 8) and (K // 32) % S == 0, (rows, N, K, cus, S)
        assert S == 1 or K // 32 // S >= 3, (rows, N, K, cus, S)
