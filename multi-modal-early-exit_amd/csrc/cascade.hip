// Model cascades (the definition is in include/mmee.h): the three launches of a stage boundary.  A stage is a whole forward of one handle, which
// this file never touches; what happens between two stages is
//   cascade_select_kernel   which documents of the stage are deferred: those that left at the stage's final exit and whose delivered row
//                           does not pass the stage's final threshold.  Their original slots, in order, and their number (a device word).
//   cascade_gather_kernel   the next stage's inputs: rows of the caller's arrays at those slots, up to 8 arrays in one launch.  The one
//                           bandwidth-sized step (a pixel row of the real models is 602 112 bytes).
//   cascade_merge_kernel    the next stage's results into the cascade's outputs at those slots, with the global exit index and the stage.
// The criterion is csf_row_f64 (mmee_kernels.h), the function csf_table_kernel calls, on (double) of the delivered float32 row: a criterion
// table of the concatenated dump-all arrays holds the same bits, which is what lets the dumped-array tools choose the deferral threshold.
#include "ranked_common.h"

namespace mmee {

// One workgroup of 1024 threads walks the stage's documents in chunks of 1024 (the shape of exit_decide_body): thread <-> document, then
// ballot -> popcount prefix -> cross-wave prefix in LDS (block1024_count) -> running carry = the document's place among the deferred.
__global__ __launch_bounds__(1024) void cascade_select_kernel(CascadeSelectArgs a) {
    __shared__ int s_slots[16];
    __shared__ int s_carry;
    const int tid = threadIdx.x;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < a.n; base += 1024) {
        const int i = base + tid;
        bool defer = false;
        if (i < a.n) {
            int am;
            const double c = csf_row_f64(a.criterion, a.logits + (size_t)i * a.K, a.K, am);
            if (a.crit) a.crit[i] = c;
            defer = a.exit_layer[i] == a.final_exit && !crit_fires(a.criterion, c, a.thr);      // strict: a NaN row never fires and is deferred
        }
        const BlockScan<int> place = block1024_count(defer, s_slots);
        const int carry = s_carry;
        if (defer) a.next_orig[carry + place.exclusive] = a.orig ? a.orig[i] : i;
        __syncthreads();                                             // every thread has read the carry and the slots
        if (tid == 0) s_carry = carry + place.total;
        __syncthreads();
    }
    if (tid == 0) *a.count = s_carry;
}

void launch_cascade_select(const CascadeSelectArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(cascade_select_kernel, dim3(1), dim3(1024), 0, s, a);
}

// dst[j] <- src[slots[j]] for j < count, one array.  blockIdx.y strides over the documents, blockIdx.x and the thread over the row's chunks
// of sizeof(V) bytes; kGatherLoads independent loads are issued before the first store, so a thread keeps that many requests in flight.
constexpr int kGatherThreads = 256, kGatherLoads = 4;

template <typename V>
__device__ __forceinline__ void gather_rows(const char* __restrict__ src, char* __restrict__ dst, size_t row_bytes, const int* __restrict__ slots,
                                            int count) {
    const size_t chunks = row_bytes / sizeof(V);
    const size_t step = (size_t)gridDim.x * kGatherThreads;
    for (int j = blockIdx.y; j < count; j += gridDim.y) {
        const V* from = reinterpret_cast<const V*>(src + (size_t)slots[j] * row_bytes);
        V* to = reinterpret_cast<V*>(dst + (size_t)j * row_bytes);
        size_t c = (size_t)blockIdx.x * kGatherThreads + threadIdx.x;
        for (; c + (kGatherLoads - 1) * step < chunks; c += kGatherLoads * step) {
            V v[kGatherLoads];
#pragma unroll
            for (int u = 0; u < kGatherLoads; ++u) v[u] = from[c + u * step];
#pragma unroll
            for (int u = 0; u < kGatherLoads; ++u) to[c + u * step] = v[u];
        }
        for (; c < chunks; c += step) to[c] = from[c];
    }
}

// grid (chunk blocks of the longest row, min(cap, 65535)): the grid is sized by the static bound, the count is read from the device word
__global__ __launch_bounds__(kGatherThreads) void cascade_gather_kernel(CascadeGatherArgs a) {
    const int count = *a.count;
    if ((int)blockIdx.y >= count) return;                            // workgroups past the count touch nothing
    for (int r = 0; r < a.n_arrays; ++r) {
        const char* src = a.src[r];
        char* dst = a.dst[r];
        const size_t rb = a.row_bytes[r];
        const size_t align = (size_t)reinterpret_cast<uintptr_t>(src) | (size_t)reinterpret_cast<uintptr_t>(dst) | rb;
        if (align % 16 == 0) gather_rows<uint4>(src, dst, rb, a.slots, count);
        else if (align % 8 == 0) gather_rows<uint2>(src, dst, rb, a.slots, count);
        else gather_rows<unsigned>(src, dst, rb, a.slots, count);
    }
}

void launch_cascade_gather(const CascadeGatherArgs& a, int cap, hipStream_t s) {
    size_t longest = 0;
    for (int r = 0; r < a.n_arrays; ++r) longest = a.row_bytes[r] > longest ? a.row_bytes[r] : longest;
    const int gx = grid_1d((long long)((longest + 15) / 16), kGatherThreads * kGatherLoads, 64);
    hipLaunchKernelGGL(cascade_gather_kernel, dim3(gx, cap < 65535 ? cap : 65535), dim3(kGatherThreads), 0, s, a);
}

// one thread per (document j, label k) of a later stage's n documents; the thread of label 0 also writes the document's three scalars
__global__ __launch_bounds__(256) void cascade_merge_kernel(CascadeMergeArgs a) {
    const size_t total = (size_t)a.n * a.K;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const int j = (int)(t / a.K), k = (int)(t - (size_t)j * a.K);
        const int slot = a.slots[j];
        a.out_logits[(size_t)slot * a.K + k] = a.logits[t];
        if (k == 0) {
            a.out_exit[slot] = a.exit_layer[j] + a.exit_offset;
            a.out_conf[slot] = a.conf[j];
            a.out_stage[slot] = a.stage;
        }
    }
}

void launch_cascade_merge(const CascadeMergeArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(cascade_merge_kernel, dim3(grid_1d((long long)a.n * a.K, 256, 4096)), dim3(256), 0, s, a);
}

}  // namespace mmee
