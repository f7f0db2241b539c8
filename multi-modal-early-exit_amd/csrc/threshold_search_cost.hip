// The cost-weighted threshold search (ee_threshold_search_cost, include/mmee.h): ee_threshold_search's candidates and exit rules, but a vector is
// charged cost_sum(v) = sum_n cost[exit(v, n)][n] -- what the caller says a document costs when it leaves at an exit (FLOPs of the packed path:
// sweep.exit_costs) -- and the front is the one of (cost_sum down, hits up).  The ranking pass, the percentile table and the digits are the
// search's own (SweepRanks, launch_search_table, ranked_common.h).
//   search_cost_pack_kernel   cost (E1, N) -> (N, E1P): the rank records' layout, so that a chunk of documents is one contiguous copy.
//   search_cost_main_kernel   ranked_walk (ranked_common.h) over chunks of HALF as many documents: rank records and cost rows of the same
//                             documents side by side in LDS, the cost rows copied by the walk's staging hook.  The selected record carries its
//                             exit in r & 63, so the document's cost is ONE per-lane LDS read of s_cost[i * E1P + (r & 63)] (at most E1
//                             consecutive words across the wave: distinct banks or the same address) and a 64-bit add; no second select per
//                             exit.  Per vector: (hits, exit_sum) and cost_sum to the workspace (cost_sum to the caller's array when given)
//                             and one 64-bit atomicMin(best_cost[hits], cost_sum).
//   search_cost_pick_kernel   over the vectors: cost_sum[v] == best_cost[hits[v]] -> atomicMin(best_vec[hits[v]], v): the lowest index among the
//                             cheapest of a hits bucket, without 64 + 32 bits in one word.
//   search_cost_front_kernel  one workgroup over the N + 1 hits buckets from the most hits down: a bucket is on the front iff its cost is below
//                             that of every non-empty bucket with MORE hits (prefix min with a running carry), compacted by its dense place
//                             among the kept (block1024_scan, block1024_count); counted in a first pass, placed from the end in a second:
//                             ascending in cost.
// Buckets are by hits and not by cost because hits <= N is the small integer of the pair: cost sums reach 2^56.
#include "ranked_common.h"

namespace mmee {

constexpr unsigned long long kNoCost = ~0ull;           // an empty hits bucket: cost sums stay below 2^56

__global__ __launch_bounds__(256) void search_cost_pack_kernel(const unsigned* __restrict__ cost, int E1, int E1P, int N, unsigned* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)N * E1P) return;
    const int n = (int)(i / E1P), e = (int)(i - (long long)n * E1P);
    out[i] = e < E1 ? cost[(size_t)e * N + n] : 0u;                  // the pad words are never read: a record's exit is < E1
}

template <int E1C>      // E1C > 0: compile-time exit count (unrolled, rank words in registers); 0: run-time E1 (rank words in the thread's private array)
__global__ __launch_bounds__(256, 2) void search_cost_main_kernel(const unsigned* __restrict__ rec, const unsigned* __restrict__ cost_t,
                                                                  const unsigned* __restrict__ trank, SearchVectors sv, int E1, int E1P, int N, int P,
                                                                  int policy, double* __restrict__ acc, double* __restrict__ mean_exit,
                                                                  uint2* __restrict__ hits_exits, unsigned long long* __restrict__ cost_sum,
                                                                  unsigned long long* __restrict__ best_cost) {
    extern __shared__ unsigned s_mem[];                              // CHUNK documents x E1P rank words | CHUNK x E1P cost words | trank (E1 x P words)
    unsigned* s_rec = s_mem;
    unsigned* s_cost = s_mem + kSearchChunkWords / 2;
    unsigned* s_trank = s_mem + kSearchChunkWords;
    const int chunk = (kSearchChunkWords / 2) / E1P;
    for (int i = threadIdx.x; i < E1 * P; i += 256) s_trank[i] = trank[i];
    __syncthreads();
    const unsigned long long v = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned vv = v < sv.V ? (unsigned)v : sv.V - 1u;
    const int n_e = E1C > 0 ? E1C : E1;
    unsigned tq[E1C > 0 ? E1C : 64];
    if constexpr (E1C > 0) {
        unsigned dg[E1C];
        search_digits(sv, vv, E1, P, E1C - 1, [&](int e, unsigned d) { dg[e] = d; });
#pragma unroll
        for (int e = 0; e < E1C - 1; ++e) tq[e] = s_trank[e * P + dg[e]];
    } else {
        search_digits(sv, vv, E1, P, E1 - 1, [&](int e, unsigned d) { tq[e] = s_trank[e * P + d]; });
    }
    tq[n_e - 1] = policy ? 0u : s_trank[(n_e - 1) * P];              // POLICY: the final exit takes whoever is left; REFERENCE: the rank of 0.0
    unsigned n_correct = 0, sum_exit = 0;
    unsigned long long sum_cost = 0;
    const auto stage_cost = [&](int n0, int i) {                     // the chunk's cost rows, in the same loop as its rank records
        reinterpret_cast<uint4*>(s_cost)[i] = reinterpret_cast<const uint4*>(cost_t + (size_t)n0 * E1P)[i];
    };
    ranked_walk<E1C>(rec, s_rec, E1, E1P, N, chunk, [&](int e) { return tq[e]; }, stage_cost, [&](int i, unsigned r) {
        const unsigned ex = r & 63u;
        n_correct += (r >> 6) & 1u;
        sum_exit += ex;
        sum_cost += s_cost[i * E1P + ex];                            // the gather: one LDS read per lane, the exit is already in the record
    });
    if (v < sv.V) {
        if (acc) acc[v] = (double)n_correct / (double)N;
        if (mean_exit) mean_exit[v] = (double)sum_exit / (double)N;
        hits_exits[v] = make_uint2(n_correct, sum_exit);
        cost_sum[v] = sum_cost;
        atomicMin(&best_cost[n_correct], sum_cost);
    }
}

__global__ __launch_bounds__(256) void search_cost_pick_kernel(const uint2* __restrict__ hits_exits, const unsigned long long* __restrict__ cost_sum,
                                                               unsigned V, const unsigned long long* __restrict__ best_cost,
                                                               unsigned* __restrict__ best_vec) {
    for (unsigned long long v = (unsigned long long)blockIdx.x * 256 + threadIdx.x; v < V; v += (unsigned long long)gridDim.x * 256) {
        const unsigned h = hits_exits[v].x;
        if (cost_sum[v] == best_cost[h]) atomicMin(&best_vec[h], (unsigned)v);
    }
}

// One workgroup of 1024 threads walks the hits buckets in chunks of 1024 from the MOST hits down: position j is bucket n_buckets - 1 - j.
//   on the front  <=>  cost < the cost of every bucket with more hits: the exclusive prefix min of the chunk and a running carry (an empty
//                      bucket holds all-ones and is below nothing);
//   dense place   the exclusive count of the kept and a running carry give the entry's rank from the END; the first pass only counts, the
//                 second writes entry count - 1 - rank: ascending in cost and in hits.
// Each kept thread writes its entry and gathers its threshold row from `table` by the vector's digits.
__global__ __launch_bounds__(1024) void search_cost_front_kernel(const unsigned long long* __restrict__ best_cost, const unsigned* __restrict__ best_vec,
                                                                 const uint2* __restrict__ hits_exits, int n_buckets, SearchVectors sv, int E1, int P,
                                                                 const double* __restrict__ table, int* __restrict__ front_count,
                                                                 unsigned long long* __restrict__ front_cost_sum, int* __restrict__ front_exit_sum,
                                                                 int* __restrict__ front_hits, unsigned* __restrict__ front_vector,
                                                                 double* __restrict__ front_thr) {
    __shared__ unsigned long long s_min[16];
    __shared__ int s_cnt[16];
    const auto umin = [](unsigned long long a, unsigned long long b) { return a < b ? a : b; };
    const int tid = threadIdx.x;
    int n_kept = 0;
    for (int pass = 0; pass < 2; ++pass) {
        unsigned long long carry_min = kNoCost;                      // over the chunks so far: the same values in every thread
        int carry_cnt = 0;
        for (int base = 0; base < n_buckets; base += 1024) {
            const int j = base + tid, h = n_buckets - 1 - j;
            const unsigned long long c = j < n_buckets ? best_cost[h] : kNoCost;
            const BlockScan<unsigned long long> above = block1024_scan(c, kNoCost, umin, s_min);
            const bool keep = c < umin(carry_min, above.exclusive);  // an empty bucket (all-ones) never is
            const BlockScan<int> kept = block1024_count(keep, s_cnt);
            if (pass == 1 && keep) {
                const int pos = n_kept - 1 - (carry_cnt + kept.exclusive);        // 0 <= pos < n_kept <= n_buckets = the outputs' N + 1 entries
                const unsigned v = best_vec[h];
                front_cost_sum[pos] = c;
                front_exit_sum[pos] = (int)hits_exits[v].y;
                front_hits[pos] = h;
                front_vector[pos] = v;
                double* row = front_thr + (size_t)pos * E1;
                search_digits(sv, v, E1, P, E1 - 1, [&](int e, unsigned d) { row[e] = table[e * P + d]; });
                row[E1 - 1] = table[(E1 - 1) * P];
            }
            carry_min = umin(carry_min, above.total);
            carry_cnt += kept.total;
            __syncthreads();                                         // s_min and s_cnt are rewritten by the next chunk
        }
        n_kept = carry_cnt;
    }
    if (tid == 0) front_count[0] = n_kept;
}

// false: the workspace allocation failed and nothing was launched
bool launch_threshold_search_cost(const SearchCostArgs& ca, const SearchPercentiles& pc, hipStream_t s) {
    const SearchArgs& a = ca.base;
    const int E1P = (a.E1 + 3) & ~3, n_buckets = a.N + 1, policy = a.semantics == SEARCH_POLICY ? 1 : 0;
    const SweepRanks r(a.conf, a.correct, a.E1, E1P, a.N, nullptr, 0, policy, s);
    if (!r.ok) return false;
    // one workspace: best_cost | per-vector cost sums (when the caller keeps none) | (hits, exit_sum) per vector | transposed costs | best_vec | trank
    const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_best = 0, o_sum = o_best + up((size_t)n_buckets * 8), o_hx = o_sum + (ca.cost_sum ? 0 : up((size_t)a.V * 8)),
                 o_cost = o_hx + up((size_t)a.V * 8), o_vec = o_cost + up((size_t)a.N * E1P * 4), o_trank = o_vec + up((size_t)n_buckets * 4),
                 bytes = o_trank + up((size_t)a.E1 * a.P * 4);
    char* ws = nullptr;
    if (hipMallocAsync((void**)&ws, bytes, s) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    unsigned long long* best_cost = reinterpret_cast<unsigned long long*>(ws + o_best);
    unsigned long long* sums = ca.cost_sum ? ca.cost_sum : reinterpret_cast<unsigned long long*>(ws + o_sum);
    uint2* hx = reinterpret_cast<uint2*>(ws + o_hx);
    unsigned* cost_t = reinterpret_cast<unsigned*>(ws + o_cost);
    unsigned* best_vec = reinterpret_cast<unsigned*>(ws + o_vec);
    unsigned* trank = reinterpret_cast<unsigned*>(ws + o_trank);
    (void)hipMemsetAsync(best_cost, 0xFF, (size_t)n_buckets * 8, s);
    (void)hipMemsetAsync(best_vec, 0xFF, (size_t)n_buckets * 4, s);
    hipLaunchKernelGGL(search_cost_pack_kernel, dim3((unsigned)(((long long)a.N * E1P + 255) / 256)), dim3(256), 0, s, ca.cost, a.E1, E1P, a.N, cost_t);
    launch_search_table(r.sorted, a.E1, a.N, a.P, pc, policy, a.table, trank, s);
    const SearchVectors sv{a.source, a.V, a.seed, a.mixtures};
    const unsigned grid = (unsigned)(((unsigned long long)a.V + 255) / 256);
    const size_t lds = (size_t)kSearchChunkWords * 4 + (size_t)a.E1 * a.P * 4;
    (void)ensure_dynamic_lds<&search_cost_main_kernel<7>>("search_cost_main_kernel", 80 * 1024);
    (void)ensure_dynamic_lds<&search_cost_main_kernel<0>>("search_cost_main_kernel", 80 * 1024);
    if (a.E1 == 7)
        hipLaunchKernelGGL((search_cost_main_kernel<7>), dim3(grid), dim3(256), lds, s, r.rec, cost_t, trank, sv, a.E1, E1P, a.N, a.P, policy, a.acc,
                           a.mean_exit, hx, sums, best_cost);
    else
        hipLaunchKernelGGL((search_cost_main_kernel<0>), dim3(grid), dim3(256), lds, s, r.rec, cost_t, trank, sv, a.E1, E1P, a.N, a.P, policy, a.acc,
                           a.mean_exit, hx, sums, best_cost);
    hipLaunchKernelGGL(search_cost_pick_kernel, dim3(grid_1d((long long)a.V, 256, 65536)), dim3(256), 0, s, hx, sums, a.V, best_cost, best_vec);
    hipLaunchKernelGGL(search_cost_front_kernel, dim3(1), dim3(1024), 0, s, best_cost, best_vec, hx, n_buckets, sv, a.E1, a.P, a.table, a.front_count,
                       ca.front_cost_sum, a.front_exit_sum, a.front_hits, a.front_vector, a.front_thresholds);
    (void)hipFreeAsync(ws, s);
    return true;
}

}  // namespace mmee
