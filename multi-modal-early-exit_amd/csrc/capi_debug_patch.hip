// ee_debug_patch_project: the patch projection alone, on caller-provided device buffers; no handle.  The entry point makes the call
// patch_projection() of capi_forward.hip makes (launch_patch_projection: the f32 GEMM with the im2col A operand, or launch_patch_split and the
// split GEMM behind it) and, for the split form, builds the weight's split rows as ee_finalize does (split_weight_rows).  No kernel is defined
// here; what ee_create's geometry rule or the kernels' own predicates refuse is refused, not launched.  It synchronises and hands the kernels'
// error word to a host int32.  tests/test_gpu_pixel.py drives it against tests/pixel_ref.py.
#include "capi_debug.h"

using namespace mmee;
using namespace mmee::capi;

extern "C" {

int ee_debug_patch_project(const ee_debug_patch_project_args* a, void* stream) {
    const char* who = "ee_debug_patch_project";
    if (!a) return fail(nullptr, "%s: args must not be NULL", who);
    if (!a->pixel_values || !a->weight || !a->bias || !a->out || !a->err_flag_out || a->B < 1)
        return fail(nullptr, "%s: pixel_values, weight, bias, out and err_flag_out must not be NULL, B >= 1", who);
    const int B = a->B, C = a->C, R = a->R, P = a->P, H = a->H;
    if (!patch_geometry_ok(C, R, P))
        return fail(nullptr, "%s: unsupported patch geometry (R %% P == 0, P %% 4 == 0, R %% 4 == 0, C P P %% 32 == 0), got C %d, R %d, P %d", who, C, R, P);
    const int NP = (R / P) * (R / P), K = C * P * P;
    if ((long long)B * NP > (1ll << 24) || (long long)B * C * R * R > (1ll << 30))
        return fail(nullptr, "%s: B (R / P)^2 = %lld rows above 2^24, or B C R R above 2^30", who, (long long)B * NP);
    if (int rc = check_hidden(who, H)) return rc;
    if (a->form < 0 || a->form > 2)
        return fail(nullptr, "%s: form %d is none of 0 (f32, LDS-DMA kernel), 1 (f32, register-staged kernel), 2 (split)", who, a->form);
    if (a->form == 2 && !gemm_split_supports(H, K))
        return fail(nullptr, "%s: form 2 needs a shape gemm_split_supports takes (H %% 256 == 0, C P P %% 32 == 0), got H %d, C P P %d", who, H, K);
    if (a->form != 2 && a->a_split_out) return fail(nullptr, "%s: a_split_out is written by form 2 only", who);
    if (!have_device(who)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int cus = device_cus(who);
    if (!cus) return 1;

    Scratch sc;
    int *err_flag = nullptr, *queue = nullptr;
    if (!sc.get(&err_flag, 1) || !sc.get(&queue, 128)) return fail(nullptr, kScratchFailed, who);      // 8 XCD-local counters x 16 ints, zeroed
    PatchProjection p{};
    p.pix = a->pixel_values; p.B = B; p.C = C; p.R = R; p.P = P; p.H = H;
    p.w = a->weight; p.bias = a->bias; p.out = a->out;
    p.use_dma = a->form == 1 ? 2 : 1;
    p.tile_counter = queue; p.err_flag = err_flag;
    if (a->form == 2) {
        float *w_s = nullptr, *absmax = nullptr, *rows = reinterpret_cast<float*>(a->a_split_out);
        if (!sc.get(&w_s, (size_t)H * K) || !sc.get(&absmax, 1) || (!rows && !sc.get(&rows, (size_t)B * NP * K))) return fail(nullptr, kScratchFailed, who);
        if (int rc = split_weight_rows(nullptr, who, a->weight, H, K, w_s, absmax, cus, s, &p.w_inv)) return rc;
        p.w_split = w_s; p.split_rows = rows;
    }
    launch_patch_projection(p, cus, s, nullptr);
    return finish(who, s, err_flag, a->err_flag_out);
}

}  // extern "C"
