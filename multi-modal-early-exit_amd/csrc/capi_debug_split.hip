// ee_debug_split_rows, ee_debug_split_weight: the split-f16 encoders alone, on caller-provided device buffers; no handle.
// ee_debug_split_rows makes one launch_split_rows call (split_rows_kernel: the clamp form, store_split4) with an error word of its own;
// ee_debug_split_weight makes the split_weight_rows call build_split makes under ee_finalize (launch_absmax, split_weight_exponent,
// launch_split_rows) and hands its refusal on unchanged.  No kernel is defined here.  tests/test_gpu_split.py drives them against
// tests/split_ref.py, bit for bit.
#include <cmath>

#include "capi_debug.h"

using namespace mmee;
using namespace mmee::capi;

extern "C" {

int ee_debug_split_rows(const float* src, int32_t rows, int32_t K, float scale, void* dst_words, int32_t* err_flag_out, void* stream) {
    const char* who = "ee_debug_split_rows";
    if (!src || !dst_words || !err_flag_out) return fail(nullptr, "%s: src, dst_words and err_flag_out must not be NULL", who);
    if (rows < 0 || K < 16 || K % 16 != 0 || (long long)rows * K > (1ll << 30))
        return fail(nullptr, "%s: bad shape (rows >= 0, K a positive multiple of 16, rows K <= 2^30), got rows %d, K %d", who, rows, K);
    if (!(scale > 0.f) || !std::isfinite(scale)) return fail(nullptr, "%s: scale must be positive and finite", who);
    if (!have_device(who)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int cus = device_cus(who);
    if (!cus) return 1;
    Scratch sc;
    int* err_flag = nullptr;
    if (!sc.get(&err_flag, 1)) return fail(nullptr, kScratchFailed, who);      // zeroed
    launch_split_rows(src, dst_words, nullptr, rows, rows, K, scale, cus, s, err_flag);
    return finish(who, s, err_flag, err_flag_out);
}

int ee_debug_split_weight(const float* w, int32_t N, int32_t K, void* dst_words, float* inv_out, void* stream) {
    const char* who = "ee_debug_split_weight";
    if (!w || !dst_words || !inv_out) return fail(nullptr, "%s: w, dst_words and inv_out must not be NULL", who);
    if (N < 1 || K < 16 || K % 16 != 0 || (long long)N * K > (1ll << 30))
        return fail(nullptr, "%s: bad shape (N >= 1, K a positive multiple of 16, N K <= 2^30), got N %d, K %d", who, N, K);
    if (!have_device(who)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int cus = device_cus(who);
    if (!cus) return 1;
    Scratch sc;
    float* absmax = nullptr;
    if (!sc.get(&absmax, 1)) return fail(nullptr, kScratchFailed, who);
    float inv = 0.f;
    if (int rc = split_weight_rows(nullptr, who, w, N, K, reinterpret_cast<float*>(dst_words), absmax, cus, s, &inv)) return rc;
    *inv_out = inv;
    return finish(who, s, nullptr, nullptr);
}

}  // extern "C"
