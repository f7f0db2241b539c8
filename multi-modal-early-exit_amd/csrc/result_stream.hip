// The result stream (MMEE_FLAG_STREAM_RESULTS, include/mmee.h): behind every exit's decide launch, one launch that packs the documents which
// LEFT at that exit into a dense segment of host-visible memory, so that the host can act on them while deeper layers still run on the rest.
// The decide kernels are not touched (they sit at their register limit): the leavers are recovered from what the decide
// launch left behind -- the old stage's document list, the new stage's, and the out_* rows.
#include "mmee_kernels.h"

namespace mmee {

__device__ __forceinline__ int imin(int x, int y) { return x < y ? x : y; }

// One workgroup of 1024 threads walks the documents of the stage that reached the exit in chunks of 1024 (the shape of exit_decide_body).
//   thread <-> document: both lists ascend by original slot and the new one is a subsequence of the old, so document i of the old list left
//   iff its slot is absent from the first min(i + 1, n_new) entries of the new list: a lower-bound search, at most 11 loads at 1024 documents.
//   leavers: wave ballot -> popcount prefix -> cross-wave prefix in LDS -> running carry = dense rank in ascending slot order.
// The chunk's leaver slots are staged in LDS; then the whole workgroup writes the chunk's rows word by word, consecutive lanes storing
// consecutive words of the segment (K + 3 words per row: contiguous runs on the bus, not one 4 (K + 3)-byte scatter per thread).  Ordinary
// vector stores: the host reads nothing before the event recorded behind this launch has completed.
__global__ __launch_bounds__(1024) void emit_leavers_kernel(EmitArgs a) {
    __shared__ int s_cnt[16];
    __shared__ int s_slot[1024];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = a.K + 3;
    const int n = imin(a.counts->n_docs, a.cap);
    const int n_new = a.n_doc_orig ? imin(a.n_counts->n_docs, a.cap) : 0;
    const int before = a.exit_index > 0 ? a.done[0] : 0;
    __syncthreads();                                         // every thread has read the running count before thread 0 rewrites it
    int carry = 0;                                           // leavers of the chunks so far: the same value in every thread
    for (int base = 0; base < n; base += 1024) {
        const int i = base + tid;
        bool left = false;
        int orig = 0;
        if (i < n) {
            orig = a.doc_orig[i];
            int lo = 0, hi = imin(n_new, i + 1);
            const int end = hi;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (a.n_doc_orig[mid] < orig) lo = mid + 1;
                else hi = mid;
            }
            left = !(lo < end && a.n_doc_orig[lo] == orig);
        }
        const unsigned long long ballot = __ballot(left);
        const int below = __popcll(ballot & ((1ull << lane) - 1ull));
        if (lane == 0) s_cnt[wave] = __popcll(ballot);
        __syncthreads();
        int wbefore = 0, total = 0;
        for (int w = 0; w < 16; ++w) {
            if (w < wave) wbefore += s_cnt[w];
            total += s_cnt[w];
        }
        if (left) s_slot[wbefore + below] = orig;
        __syncthreads();
        const int first = before + carry;
        for (int w = tid; w < total * W; w += 1024) {
            const int r = w / W, c = w - r * W;
            const int slot = s_slot[r];
            const int v = c < a.K ? __float_as_int(a.out_logits[(size_t)slot * a.K + c]) : c == a.K ? a.out_exit[slot]
                          : c == a.K + 1 ? __float_as_int(a.out_conf[slot]) : slot;
            if (first + r < a.cap) a.rows[(size_t)first * W + w] = v;
        }
        carry += total;
        __syncthreads();                                     // s_cnt and s_slot are rewritten by the next chunk
    }
    if (tid == 0) {
        a.done[0] = before + carry;
        a.cum[a.exit_index] = before + carry;
    }
}

void launch_emit_leavers(const EmitArgs& a, hipStream_t s) { hipLaunchKernelGGL(emit_leavers_kernel, dim3(1), dim3(1024), 0, s, a); }

}  // namespace mmee
