// What the ee_debug_* hooks that run one kernel of the path on caller-provided device buffers share (capi_debug_attention.hip,
// capi_debug_rows.hip, capi_debug_xprobe.hip, capi_debug_exit.hip, capi_debug_patch.hip, capi_debug_split.hip, capi_debug_vision.hip; the GEMM hooks of capi_tools.hip take the device query and to_host).  Host code with internal linkage:
// the library exports none of it.  What every hook words alike is worded here; the refusals of a document table keep each hook's own words.
#pragma once
#include "capi_internal.h"

namespace mmee {
namespace capi {

// Row metadata from the caller's integers by the expression of row_meta_kernel (make_row_meta), for the hooks that take rows as
// pos / x0 / y1 / masked (capi_debug_attention.hip holds the kernel)
void launch_debug_row_meta(const int* pos, const int* x0, const int* y1, const int* masked, int rows, int coord_hi, RowMeta* meta, hipStream_t s);

namespace {

// the refusals every hook words alike
constexpr const char* kScratchFailed = "%s: hipMalloc of the scratch failed";
constexpr const char* kUploadFailed = "%s: host-to-device copy failed";

// the hidden sizes ee_create takes: the multiples of 128 up to 1024 (the row kernels hold a row as ceil(H / 256) x 4 floats per lane, the f32
// GEMM writes 128 columns per tile)
int check_hidden(const char* who, int H) {
    if (H < 128 || H > 1024 || H % 128 != 0) return fail(nullptr, "%s: hidden size %d is not a multiple of 128 in [128, 1024]", who, H);
    return 0;
}

// the device's CU count; 0 (and the error message of `who` set) when its properties cannot be read
int device_cus(const char* who) {
    hipDeviceProp_t prop;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) { fail(nullptr, "%s: no device", who); return 0; }
    return prop.multiProcessorCount;
}

template <typename T>
bool to_host(std::vector<T>& dst, const T* dev, size_t n) {
    dst.resize(n);
    return n == 0 || hipMemcpy(dst.data(), dev, sizeof(T) * n, hipMemcpyDeviceToHost) == hipSuccess;
}

// scratch that the forward takes from a workspace nobody zeroes between launches: a non-zero byte pattern (negative as an int, a NaN as a float)
template <typename T>
bool get_dirty(Scratch& sc, T** out, size_t count, hipStream_t s) {
    return sc.get(out, count) && hipMemsetAsync(*out, 0xA5, count * sizeof(T), s) == hipSuccess;
}

// A document-offsets array of the caller's on the host, and what the launches are sized by.  The rules (off[0] == 0, every length >= 1) are
// the same for every table; the hooks word the refusals, each in the order of its other per-document checks.
struct DocTable {
    std::vector<int> off;               // [n + 1]
    int max_len = 0, rows = 0;          // the longest document; off[n]
    unsigned long long sum_sq = 0;      // sum of the squared lengths (StageCounts)
    int len(int d) const { return off[d + 1] - off[d]; }
    bool read(const int* dev_off, int n_docs) {      // false: the copy failed
        if (!to_host(off, dev_off, (size_t)n_docs + 1)) return false;
        for (int d = 0; d < n_docs; ++d) {
            max_len = std::max(max_len, len(d));
            sum_sq += (unsigned long long)len(d) * len(d);
        }
        rows = off[n_docs];
        return true;
    }
};

// pos / x0 / y1 of every row inside [0, max_pos] / [0, max_coord], on host copies: 0, or the refusal
int check_row_ints(const char* who, const int* pos, const int* x0, const int* y1, int rows, int max_pos, int max_coord) {
    std::vector<int> hp, hx, hy;
    if (!to_host(hp, pos, (size_t)rows) || !to_host(hx, x0, (size_t)rows) || !to_host(hy, y1, (size_t)rows))
        return fail(nullptr, "%s: copy of the row integers failed", who);
    for (int i = 0; i < rows; ++i) {
        if (hp[i] < 0 || hp[i] > max_pos) return fail(nullptr, "%s: pos[%d] = %d outside [0, max_pos = %d]", who, i, hp[i], max_pos);
        if (hx[i] < 0 || hx[i] > max_coord || hy[i] < 0 || hy[i] > max_coord)
            return fail(nullptr, "%s: x0 / y1 of row %d = %d / %d outside [0, max_coord = %d]", who, i, hx[i], hy[i], max_coord);
    }
    return 0;
}

// The operands of the relative-position bias that the hooks build as ee_finalize does: the delta ranges and the two bucket LUTs on the device,
// each padded by 4 bytes.  l1 / l2 are what the asynchronous uploads read: the struct outlives them (the hooks synchronise before they return).
struct BiasLuts {
    int c1, n1, c2, n2;
    unsigned char *lut1 = nullptr, *lut2 = nullptr;
    std::vector<unsigned char> l1, l2;
    BiasLuts(int max_pos, int max_coord) : c1(max_pos), n1(2 * max_pos + 1), c2(max_coord), n2(2 * max_coord + 1), l1(n1), l2(n2) {}
};
// what launch_pair_index holds in LDS: 0, or the refusal
int check_pair_index_staging(const char* who, const BiasLuts& b, int max_len) {
    if ((size_t)max_len * sizeof(RowMeta) + (size_t)b.n1 + b.n2 + 32 > 64 * 1024)
        return fail(nullptr, "%s: the pair-index kernel stages max_len rows and both LUTs in 64 KB of LDS (max_len %d, max_pos %d, max_coord %d)", who, max_len,
                    b.c1, b.c2);
    return 0;
}
int upload_bias_luts(const char* who, BiasLuts& b, Scratch& sc, int bins1, int max_rel_pos, int bins2, int max_rel_2d_pos, hipStream_t s) {
    if (!sc.get(&b.lut1, (size_t)b.n1 + 4) || !sc.get(&b.lut2, (size_t)b.n2 + 4)) return fail(nullptr, kScratchFailed, who);
    bucket_lut_host(bins1, max_rel_pos, b.c1, b.l1.data());
    bucket_lut_host(bins2, max_rel_2d_pos, b.c2, b.l2.data());
    if (hipMemcpyAsync(b.lut1, b.l1.data(), b.n1, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(b.lut2, b.l2.data(), b.n2, hipMemcpyHostToDevice, s) != hipSuccess)
        return fail(nullptr, kUploadFailed, who);
    return 0;
}

// the tail of a hook: synchronise, the kernels' error word to the host (err_flag null: the kernels have none), the launch status
int finish(const char* who, hipStream_t s, const int* err_flag, int32_t* err_flag_out) {
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(nullptr, "%s: launch failed: %s", who, hipGetErrorString(e));
    if (err_flag && hipMemcpy(err_flag_out, err_flag, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail(nullptr, "%s: copy of err_flag failed", who);
    return launch_status(nullptr, who);
}

}  // namespace
}  // namespace capi
}  // namespace mmee
