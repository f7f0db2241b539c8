// f32-grade GEMM on the f16 matrix cores by operand splitting: C[M,N] = A[M,K] * W[N,K]^T (+ fused epilogue).
//
// Same role as gemm_f32.hip for the four big Linear layers of an encoder layer (QKV HF:243-258, attention output
// HF:299-303, FFN up + GELU HF:485-497, FFN down HF:508-512) in precision mode MMEE_PRECISION_F32_SPLIT.
//
// Why: v_mfma_f32_32x32x2_f32 peaks at 157 TFLOP/s; v_mfma_f32_32x32x16_f16 at 2.5 PFLOP/s.  Every f32 operand is kept
// as two f16 planes hi + lo (22 significant bits, mmee_common.h "Split-f16 operand rows") and the product is formed as
//     a*w  ~=  a_lo*w_hi + a_hi*w_lo + a_hi*w_hi          (a_lo*w_lo ~ 2^-22 relative is dropped)
// with three f16 MFMAs accumulating in f32: 3/16 of the matrix-pipe time of the f32 MFMA for the same MACs.  Measured
// against an f64 reference (tools/split_accuracy.hip, K = 768 / 3072, N(0,1) x N(0,0.02) operands): rms relative error
// 3.2e-7 / 6.1e-7 for this scheme against 5.0e-7 / 9.9e-7 for the f32 MFMA chain — the 16-long dot product inside the
// f16 MFMA is summed with fewer roundings than eight chained 2-long f32 MFMAs, so the split result is the MORE accurate
// of the two.  Both meet the 1e-4 logit tolerance with the same margin; exit indices stay bit-exact on the fixtures.
//
// Design (gfx950):
//   * 128 x 256 output tile per 512-thread workgroup (8 waves as 2 x 4, each a 64x64 sub-tile = 2x2 MFMA tiles),
//     two workgroups per CU (4 waves per SIMD, <= 128 VGPRs): one workgroup's epilogue (GELU is ~35 VALU instructions
//     per element) runs under the other's MFMA stream, and at 4 waves per SIMD the LDS-DMA issue cost of one wave
//     (~25-35 cycles per 1 KiB piece, tools/mfma_peak.hip) is covered by the other three.
//   * K stage = 16 (one MFMA k-step): a row contributes 32 B of hi and 32 B of lo = one 64-byte LDS row
//     [hi k0-7 | hi k8-15 | lo k0-7 | lo k8-15], which is also one contiguous 64-byte group of the split row in memory; stage = (128 + 256) rows x 64 B = 24 KiB, 3-deep ring (72 KiB).
//   * global -> LDS by global_load_lds_dwordx4 with an SGPR base and a 32-bit per-lane offset (the cheapest form to
//     issue): a piece is 16 rows x 64 B, 3 pieces per wave per stage; LDS rows are unpadded (the DMA writes linearly),
//     bank conflicts of the ds_read_b128 fragment reads are removed by XOR-ing the 16-byte chunk index with (row>>2)&3
//     on both the DMA source side and the read side.
//   * ring protocol per stage kt:  s_waitcnt vmcnt(3) (my pieces of stage kt landed, stage kt+1 may still fly) |
//     s_barrier (everyone's landed; everyone left stage kt-1) | issue stage kt+2 into the buffer stage kt-1 used |
//     8 ds_read_b128 + 12 MFMA on stage kt.
//   * persistent workgroups pulling tiles from the XCD-local queues of gemm_f32.hip; M read from device memory.
//   * epilogue through LDS as in gemm_f32.hip (whole-row 16-byte stores); the FFN-up epilogue writes its output as
//     split rows directly (the only consumer is the FFN-down GEMM), so H1 never exists in f32.
#include <cstdlib>
#include "mmee_common.h"

#include "gemm_split_kernel.h"

namespace mmee {

bool gemm_split_supports(int N, int K) { return N > 0 && K > 0 && N % 256 == 0 && K % 32 == 0; }

// the FFN-up instantiation lives in gemm_split_ffn_up.hip (a unit that can take its own scheduling strategy: gemm_split_kernel.h)
void launch_split_ffn_up(const GemmArgs& a, int max_m, int num_cus, hipStream_t s);

void launch_gemm_split(const GemmArgs& a_in, int epi, int max_m, int num_cus, hipStream_t s) {
    GemmArgs a = a_in;
    // queue order: with N <= 768 (attention output, FFN down: three N-tiles) the whole W operand stays in an XCD's L2, so the A panel is
    // what consecutive tickets should share (N fastest): FFN down 402 -> 414 TFLOP/s, attention output unchanged (tools/gemm_split_shapes.py);
    // wider GEMMs keep eight M-tiles per W tile back to back (QKV, FFN up: unchanged to -0.6 % with N fastest)
    a.tile_order = a.N <= 768 ? 1 : 0;
    // (ahead of the diagnostic library's forced configurations: only these instantiations honour k_splits -- ADVICE r03)
    if (a.probe) a.terms = 3;      // probes and exit heads keep three terms whatever the caller's mode (a probe shape outside the CfgP list fell through with terms == 1)
    // split-K parts are assigned statically (the queue walk of the kernel knows tiles, not parts): the forward's probes pass no queue head, and
    // one that a caller passes is not used
    if (a.probe && a.k_splits > 1) a.tile_counter = nullptr;
    if (a.probe) {      // CLS probe: 128 x 128 tiles under their own kernel name; same MFMA form, k order and term order as CfgC => the same bits
        if (a.out_split && epi == EPI_GELU) { launch_split_one<CfgP, EPI_GELU, true, false, 1>(a, max_m, num_cus, s); return; }
        if (!a.out_split && epi == EPI_RESID) { launch_split_one<CfgP, EPI_RESID, false, false, 1>(a, max_m, num_cus, s); return; }
        if (!a.out_split && epi == EPI_BIAS) { launch_split_one<CfgP, EPI_BIAS, false, false, 1>(a, max_m, num_cus, s); return; }      // Q of the CLS rows (xprobe.hip)
        if (!a.out_split && epi == EPI_TANH) { launch_split_one<CfgP, EPI_TANH, false, false, 1>(a, max_m, num_cus, s); return; }      // dense + tanh of an exit head
        // not a shape the probe launches: the default configuration below computes the same bits
    }
    // MMEE_FLAG_LOW_LATENCY: a layer's attention-output / FFN-down GEMM as S-way split-K (capi_forward.hip layer_rest; S from
    // ee_low_latency_k_splits).  The instantiation of the probe's split-K launch, static tile assignment: part p of a tile is alpha * acc over its
    // K / S, no bias (the caller passes none); the LayerNorm kernel behind it adds the parts in order, the bias and the residual.
    if (a.k_splits > 1 && !a.out_split && epi == EPI_BIAS && a.terms != 1) {
        a.tile_counter = nullptr;
        launch_split_one<CfgP, EPI_BIAS, false, false, 1>(a, max_m, num_cus, s);
        return;
    }
    a.k_splits = 1;      // every kernel below writes ONE part
    // ee_debug_gemm_split_resid's forced routes (residual epilogue, f32 output, three terms): the two configurations that compute the same bits,
    // one reading the residual straight into registers, one through LDS
    if (a.route == 1 && !a.out_split && epi == EPI_RESID) {
        a.tile_counter = nullptr;
        launch_split_one<CfgP, EPI_RESID, false, false, 1>(a, max_m, num_cus, s);
        return;
    }
    // Round 6, small batches (the reference evaluates at eval_batch_size = 1, EE/configs.py:36; bench.py `small_batch`): a forward of one document is
    // 709 rows -- 27 of the default 256 x 256 tiles in the Q|K|V projection, 9 in the attention-output GEMM, on 256 CUs.  When the default tiles
    // would leave more than half of the chip without one, a layer GEMM takes the CLS-probe launches' 128 x 128 / 4-wave configuration (four
    // times the tiles, static assignment): same MFMA form, k order and term order => the same bits, so nothing observable changes but the time.
    if (a.terms != 1 && a.route != 2 && (long)((max_m + 255) / 256) * (a.N / 256) * 2 <= (long)num_cus) {
        a.tile_counter = nullptr;
        if (a.out_split && epi == EPI_GELU) { launch_split_one<CfgP, EPI_GELU, true, false, 1>(a, max_m, num_cus, s); return; }
        if (a.out_split && epi == EPI_BIAS) { launch_split_one<CfgP, EPI_BIAS, true, false, 1>(a, max_m, num_cus, s); return; }
        if (!a.out_split && epi == EPI_RESID) { launch_split_one<CfgP, EPI_RESID, false, false, 1>(a, max_m, num_cus, s); return; }
        if (!a.out_split && epi == EPI_BIAS) { launch_split_one<CfgP, EPI_BIAS, false, false, 1>(a, max_m, num_cus, s); return; }
        if (!a.out_split && epi == EPI_TANH) { launch_split_one<CfgP, EPI_TANH, false, false, 1>(a, max_m, num_cus, s); return; }
        a.tile_counter = a_in.tile_counter;
    }
#ifdef MMEE_DIAG
    static const int order_env = diag_env_int("MMEE_GEMM_ORDER", -1);      // A/B of the queue order: 0 / 1 for every GEMM, 2 = N fastest where N <= 768
    if (order_env == 0 || order_env == 1) a.tile_order = order_env;
    else if (order_env == 2) a.tile_order = a.N <= 768 ? 1 : 0;
    else if (order_env == 3 || order_env == 4) a.tile_order = a.N >= 2304 ? order_env - 1 : a.tile_order;      // round 6: W-stationary (3) / A-panel (4) order for the wide GEMMs
    static const int forced = diag_env_int("MMEE_SPLIT_CFG", 0);      // 1 = CfgA, 2 = CfgB, 0 / 3 = CfgC
    const bool use_a = forced == 1;
    if (a.dbg_noload && (forced == 0 || forced == 3)) {      // timing diagnostics of the default configuration (tools/gemm_split_shapes.py)
        if (a.out_split && epi == EPI_GELU) launch_split_one<CfgC, EPI_GELU, true, true>(a, max_m, num_cus, s);
        else if (a.out_split) launch_split_one<CfgC, EPI_BIAS, true, true>(a, max_m, num_cus, s);
        else launch_split_one<CfgC, EPI_RESID, false, true>(a, max_m, num_cus, s);
        return;
    }
    if (a.dbg_noload) {      // timing diagnostics: only the two shapes the probes use
        if (a.out_split) launch_split_one<CfgA, EPI_GELU, true, true>(a, max_m, num_cus, s);
        else if (use_a) launch_split_one<CfgA, EPI_RESID, false, true>(a, max_m, num_cus, s);
        else launch_split_one<CfgB, EPI_RESID, false, true>(a, max_m, num_cus, s);
        return;
    }
    if (forced == 1 || forced == 2) {
        if (a.out_split) {
            if (epi == EPI_GELU && use_a) launch_split_one<CfgA, EPI_GELU, true>(a, max_m, num_cus, s);
            else if (epi == EPI_GELU) launch_split_one<CfgB, EPI_GELU, true>(a, max_m, num_cus, s);
            else if (use_a) launch_split_one<CfgA, EPI_BIAS, true>(a, max_m, num_cus, s);
            else launch_split_one<CfgB, EPI_BIAS, true>(a, max_m, num_cus, s);
            return;
        }
        if (use_a) {
            switch (epi) {
                case EPI_BIAS: launch_split_one<CfgA, EPI_BIAS, false>(a, max_m, num_cus, s); break;
                case EPI_GELU: launch_split_one<CfgA, EPI_GELU, false>(a, max_m, num_cus, s); break;
                case EPI_RESID: launch_split_one<CfgA, EPI_RESID, false>(a, max_m, num_cus, s); break;
                default: launch_split_one<CfgA, EPI_TANH, false>(a, max_m, num_cus, s); break;
            }
            return;
        }
        switch (epi) {
            case EPI_BIAS: launch_split_one<CfgB, EPI_BIAS, false>(a, max_m, num_cus, s); break;
            case EPI_GELU: launch_split_one<CfgB, EPI_GELU, false>(a, max_m, num_cus, s); break;
            case EPI_RESID: launch_split_one<CfgB, EPI_RESID, false>(a, max_m, num_cus, s); break;
            default: launch_split_one<CfgB, EPI_TANH, false>(a, max_m, num_cus, s); break;
        }
        return;
    }
#endif
    if (a.terms == 1) {      // MMEE_FLAG_ONE_TERM: the four layer GEMMs on one f16 term (a reported low-precision mode; anything else runs the three terms)
        if (a.out_split && epi == EPI_GELU) { launch_split_one<CfgC, EPI_GELU, true, false, 0, 1>(a, max_m, num_cus, s); return; }
        if (a.out_split && epi == EPI_BIAS) { launch_split_one<CfgC, EPI_BIAS, true, false, 0, 1>(a, max_m, num_cus, s); return; }
        if (!a.out_split && epi == EPI_RESID) {
            if (a.role_tag == 3) launch_split_one<CfgC, EPI_RESID, false, false, 3, 1>(a, max_m, num_cus, s);
            else launch_split_one<CfgC, EPI_RESID, false, false, 2, 1>(a, max_m, num_cus, s);
            return;
        }
    }
    if (a.out_split) {
        if (epi == EPI_GELU) launch_split_ffn_up(a, max_m, num_cus, s);      // CfgC, GELU, split output, three terms: gemm_split_ffn_up.hip
        else launch_split_one<CfgC, EPI_BIAS, true>(a, max_m, num_cus, s);
        return;
    }
    switch (epi) {
        case EPI_BIAS: launch_split_one<CfgC, EPI_BIAS, false>(a, max_m, num_cus, s); break;
        case EPI_GELU: launch_split_one<CfgC, EPI_GELU, false>(a, max_m, num_cus, s); break;
        case EPI_RESID:
            if (a.role_tag == 2) launch_split_one<CfgC, EPI_RESID, false, false, 2>(a, max_m, num_cus, s);
            else if (a.role_tag == 3) launch_split_one<CfgC, EPI_RESID, false, false, 3>(a, max_m, num_cus, s);
            else launch_split_one<CfgC, EPI_RESID, false>(a, max_m, num_cus, s);
            break;
        default: launch_split_one<CfgC, EPI_TANH, false>(a, max_m, num_cus, s); break;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// f32 rows -> split rows, and the |max| reduction that picks a weight tensor's scale
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void split_rows_kernel(const float* __restrict__ src, char* __restrict__ dst, const int* __restrict__ n_rows_ptr,
                                                         int n_rows_static, int K, float scale, int* __restrict__ err_flag) {
    const int n_rows = n_rows_ptr ? *n_rows_ptr : n_rows_static;
    const int k4 = K / 4;
    const size_t total = (size_t)n_rows * k4;
    float amax = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t r = i / k4;
        const int c = (int)(i - r * k4) * 4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + r * K + c);
        store_split4(dst + r * (size_t)K * 4, c, v, scale, amax);
    }
    split_flag_overflow(amax, err_flag);
}

void launch_split_rows(const float* src, void* dst, const int* n_rows_ptr, int n_rows_static, int max_rows, int K, float scale, int num_cus,
                       hipStream_t s, int* err_flag) {
    size_t total = (size_t)max_rows * (K / 4);
    size_t blocks = (total + 255) / 256;
    int grid = (int)(blocks < (size_t)num_cus * 16 ? blocks : (size_t)num_cus * 16);
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(split_rows_kernel, dim3(grid), dim3(256), 0, s, src, reinterpret_cast<char*>(dst), n_rows_ptr, n_rows_static, K, scale, err_flag);
}

// pixel_values [B][C][R][R] -> split rows [B * G * G][C * P * P] (one row per patch, k = (c, py, px) as Conv2d's weight flattens,
// HF:75-81): the A operand of the patch projection on the split kernel.  P % 4 == 0: four consecutive k are four consecutive pixels.
__global__ __launch_bounds__(256) void patch_split_kernel(const float* __restrict__ pix, char* __restrict__ dst, int n_patches, int C, int R,
                                                          int P, int G, float scale, int* __restrict__ err_flag) {
    const int K = C * P * P, k4 = K / 4;
    const size_t total = (size_t)n_patches * k4;
    float amax = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t r = i / k4;
        const int k = (int)(i - r * k4) * 4;
        const int b = (int)(r / (size_t)(G * G)), pr = (int)(r - (size_t)b * (G * G));
        const int gy = pr / G, gx = pr - gy * G;
        const int c = k / (P * P), rem = k - c * P * P;
        const int py = rem / P, px = rem - py * P;
        const f32x4 v = *reinterpret_cast<const f32x4*>(pix + (((size_t)b * C + c) * R + (size_t)(gy * P + py)) * R + gx * P + px);
        store_split4_quad(dst + r * (size_t)K * 4, k, v, scale, amax, threadIdx.x & 63);      // K % 16 == 0: a quad of lanes = one 64-byte group
    }
    split_flag_overflow(amax, err_flag);
}

void launch_patch_split(const float* pix, void* dst, int n_docs, int C, int R, int P, float scale, int num_cus, hipStream_t s, int* err_flag) {
    const int G = R / P;
    const size_t total = (size_t)n_docs * G * G * (C * P * P / 4);
    size_t blocks = (total + 255) / 256;
    int grid = (int)(blocks < (size_t)num_cus * 16 ? blocks : (size_t)num_cus * 16);
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(patch_split_kernel, dim3(grid), dim3(256), 0, s, pix, reinterpret_cast<char*>(dst), n_docs * G * G, C, R, P, G, scale, err_flag);
}

// The maximum is taken over the bit patterns with the sign cleared: non-negative floats order as uints, inf lies above every finite value
// and a NaN above inf, so *out is the exact max |src[i]| of a finite tensor and inf / a NaN as soon as one element is (fmaxf dropped a NaN:
// split_weight_rows then let a NaN weight through and split_rows_kernel clamped it to -60000).
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ src, size_t n, float* __restrict__ out) {
    unsigned m = 0u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = max(m, __float_as_uint(src[i]) & 0x7fffffffu);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned*>(out), m);
}

void launch_absmax(const float* src, size_t n, float* out_dev, hipStream_t s) {
    (void)hipMemsetAsync(out_dev, 0, sizeof(float), s);
    size_t blocks = (n + 255) / 256;
    int grid = (int)(blocks < 1024 ? blocks : 1024);
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(absmax_kernel, dim3(grid), dim3(256), 0, s, src, n, out_dev);
}

}  // namespace mmee
