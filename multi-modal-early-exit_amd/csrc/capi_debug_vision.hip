// ee_debug_vision_pool: the phase-1 kernel of a vision-first call (vision_first.hip) alone, on caller-provided device buffers; no handle.  It makes
// the two launches ee_forward_vision makes behind the patch projection (launch_vision_pool, launch_pool_finish) and synchronises.  No kernel is
// defined here; what the launchers cannot take is refused, not launched.  tests/test_gpu_vision_first.py drives it against float64.
#include "capi_debug.h"

using namespace mmee;
using namespace mmee::capi;

extern "C" {

int ee_debug_vision_pool(const float* vis_raw, const float* cls_token, const float* pos_embed, const float* ln_g, const float* ln_b, float eps,
                         int32_t B, int32_t Pv, int32_t H, float* vis_part, float* pooled, void* stream) {
    const char* who = "ee_debug_vision_pool";
    if (!vis_raw || !cls_token || !pos_embed || !ln_g || !ln_b || !vis_part || !pooled)
        return fail(nullptr, "%s: vis_raw, cls_token, pos_embed, ln_g, ln_b, vis_part and pooled must not be NULL", who);
    // the row kernels hold a row as ceil(H / 256) x 4 floats per lane: whole 16-byte column groups, at most 1024 columns
    if (H < 4 || H > 1024 || H % 4 != 0) return fail(nullptr, "%s: hidden size %d is not a multiple of 4 in [4, 1024]", who, H);
    if (B < 1 || Pv < 2 || (long long)B * Pv > (1ll << 24))
        return fail(nullptr, "%s: bad shape (B >= 1, Pv >= 2: cls and at least one patch, B Pv <= 2^24), got B %d, Pv %d", who, B, Pv);
    if (!(eps > 0.f)) return fail(nullptr, "%s: eps must be positive", who);
    if (!have_device(who)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    VisionPoolArgs va{};
    va.vis_raw = vis_raw; va.cls_token = cls_token; va.pos_embed = pos_embed; va.ln_g = ln_g; va.ln_b = ln_b; va.eps = eps;
    va.B = B; va.Pv = Pv; va.H = H; va.vis_part = vis_part;
    launch_vision_pool(va, s);
    launch_pool_finish(vis_part, (Pv + 31) / 32, H, (float)Pv, pooled, B, s);
    return finish(who, s, nullptr, nullptr);
}

}  // extern "C"
