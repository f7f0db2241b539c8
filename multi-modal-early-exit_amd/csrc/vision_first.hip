// Phase 1 of a vision-first call (include/mmee.h, ee_forward_vision): the input of the vision_avg exit from the patch projection alone.
//
//   vision_pool    : the visual rows up to layoutlmv3.norm (prepend cls_token, + pos_embed, LayerNorm eps 1e-6; EE/models/LayoutLMv3.py:358-373)
//                    and their column sums per (document, 32-row chunk).  It is embed_visual_kernel (prep_embed.hip) without what only the
//                    encoder needs: no model-level LayerNorm, no concat sums, no row stored, no packed layout read.  The workgroup <-> (document,
//                    chunk) assignment, the wave <-> row assignment and the order of every addition are that kernel's, and the row functions
//                    (wave_layernorm, block_write_partial: mmee_common.h) are shared, so after pool_finish the pooled row has the bits of
//                    ee_embedding_inputs' out_vision on the same pixels (tests/test_gpu_vision_first.py).
//   copy_survivors : the documents that stay behind exit 0 (the next stage's doc_orig, ascending, and its count) to the caller's arrays;
//                    entries from the count on are not written.
// HBM-bound: one wave per row, 16-byte vector loads; per document (Pv - 1) H floats read, ceil(Pv / 32) H floats written.
#include "mmee_common.h"
#include "mmee_kernels.h"

namespace mmee {

template <int NV, bool FULL = false>
__global__ __launch_bounds__(256) void vision_pool_kernel(VisionPoolArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int H = a.H, Pv = a.Pv;
    const int nch = (Pv + 31) / 32;
    const int b = blockIdx.x / nch, ch = blockIdx.x - b * nch;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f32x4 acc_v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc_v[i] = f32x4{0, 0, 0, 0};
    for (int t = 0; t < 8; ++t) {
        const int v = ch * 32 + wave * 8 + t;
        if (v >= Pv) break;
        f32x4 x[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = 4 * lane + 256 * i;
            if (FULL || c < H) {
                f32x4 e = (v == 0) ? *reinterpret_cast<const f32x4*>(a.cls_token + c)
                                   : *reinterpret_cast<const f32x4*>(a.vis_raw + ((size_t)b * (Pv - 1) + (v - 1)) * H + c);
                x[i] = e + *reinterpret_cast<const f32x4*>(a.pos_embed + (size_t)v * H + c);
            } else {
                x[i] = f32x4{0, 0, 0, 0};
            }
        }
        wave_layernorm<NV, FULL>(x, H, lane, a.ln_g, a.ln_b, a.eps);      // layoutlmv3.norm, eps 1e-6
#pragma unroll
        for (int i = 0; i < NV; ++i) acc_v[i] += x[i];
    }
    block_write_partial<NV>(lds, a.vis_part + ((size_t)b * nch + ch) * H, acc_v, H, lane, wave);
}

void launch_vision_pool(const VisionPoolArgs& a, hipStream_t s) {
    const int nv = (a.H + 255) / 256;
    const bool full = a.H == 256 * nv;
    const int grid = a.B * ((a.Pv + 31) / 32);
    const size_t lds = 4 * (size_t)a.H * sizeof(float);
    switch (nv) {      // the NV / FULL routes of launch_embed_visual's chunked form
        case 1: hipLaunchKernelGGL(vision_pool_kernel<1>, dim3(grid), dim3(256), lds, s, a); break;
        case 2: hipLaunchKernelGGL(vision_pool_kernel<2>, dim3(grid), dim3(256), lds, s, a); break;
        case 3: if (full) hipLaunchKernelGGL((vision_pool_kernel<3, true>), dim3(grid), dim3(256), lds, s, a);
                else hipLaunchKernelGGL(vision_pool_kernel<3>, dim3(grid), dim3(256), lds, s, a);
                break;
        default: if (full) hipLaunchKernelGGL((vision_pool_kernel<4, true>), dim3(grid), dim3(256), lds, s, a);
                 else hipLaunchKernelGGL(vision_pool_kernel<4>, dim3(grid), dim3(256), lds, s, a);
                 break;
    }
}

__global__ __launch_bounds__(256) void copy_survivors_kernel(const StageCounts* __restrict__ n_counts, const int* __restrict__ n_doc_orig, int cap,
                                                             int* __restrict__ survivors, int* __restrict__ count) {
    int n = n_counts->n_docs;
    n = n < 0 ? 0 : (n > cap ? cap : n);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) survivors[i] = n_doc_orig[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) *count = n;
}

void launch_copy_survivors(const StageCounts* n_counts, const int* n_doc_orig, int cap, int* survivors, int* count, hipStream_t s) {
    int grid = (cap + 255) / 256;
    if (grid > 64) grid = 64;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(copy_survivors_kernel, dim3(grid), dim3(256), 0, s, n_counts, n_doc_orig, cap, survivors, count);
}

}  // namespace mmee
