// Entry points of libmmee_hip.so that never see a handle: bucket LUT, shader-clock stamps, policy / patience / threshold sweeps, temperature
// fit, the evaluation report (ee_exit_metrics), result packing, the three launches of a cascade's stage boundary (ee_cascade_select / _gather /
// _merge), the device-side input feed, and the GEMM micro-benchmark hooks (ee_debug_gemm,
// ee_debug_gemm_split, ee_debug_gemm_split_resid, ee_debug_gemm_routes, ee_debug_gemm_f32, ee_debug_attn_stamps).  The L-BFGS fits are in capi_fit.hip, the hooks that run one kernel of the path alone for its
// float64 test in capi_debug_*.hip.
#include <math.h>
#include <string.h>

#include <vector>

#include "capi_debug.h"

using namespace mmee;
using namespace mmee::capi;

namespace {

// A small host vector on the device for the length of one entry point: hipMallocAsync + hipMemcpyAsync here, hipFreeAsync (in stream order) on
// every way out of the scope.  err: null, or what failed.
template <typename T>
struct TempUpload {
    T* dev = nullptr;
    hipStream_t s;
    const char* err = nullptr;
    TempUpload(const T* host, size_t n, hipStream_t stream) : s(stream) {
        if (hipMallocAsync((void**)&dev, sizeof(T) * n, s) != hipSuccess) { dev = nullptr; err = "hipMallocAsync failed"; }
        else if (hipMemcpyAsync(dev, host, sizeof(T) * n, hipMemcpyHostToDevice, s) != hipSuccess) err = "host-to-device copy failed";
    }
    TempUpload(const TempUpload&) = delete;
    ~TempUpload() { if (dev) (void)hipFreeAsync(dev, s); }
};

// The common tail of the threshold scans: device check, the thresholds (n_up doubles: ee_rule_scan packs its patience behind them) to the
// device, counts zeroed, one launch.  what: the upload's name in the error message.
int run_threshold_scan(const char* who, const char* what, ScanArgs a, const double* thr_host, size_t n_up, int event, int rule, void* stream) {
    if (!have_device(who)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const TempUpload<double> up(thr_host, n_up, s);
    if (up.err) return fail(nullptr, "%s: %s %s", who, what, up.err);
    if (a.counts && hipMemsetAsync(a.counts, 0, sizeof(int) * a.E1, s) != hipSuccess) return fail(nullptr, "%s: memset failed", who);
    a.thr = up.dev;
    if (n_up > (size_t)a.E1) a.pat = reinterpret_cast<const int*>(up.dev + a.E1);
    if (a.N > 0) launch_exit_scan(a, event, rule, s);
    return launch_status(nullptr, who);
}

// the parameters ee_threshold_search and ee_threshold_search_cost share
SearchArgs search_args(const double* conf, const uint8_t* correct, int32_t E1, int32_t N, int32_t P, int32_t source, int64_t V, uint64_t seed,
                       const uint8_t* mixtures, int32_t semantics, double* table, double* acc, double* mean_exit, int32_t* front_count,
                       int32_t* front_exit_sum, int32_t* front_hits, uint32_t* front_vector, double* front_thresholds) {
    SearchArgs a{};
    a.conf = conf; a.correct = correct; a.E1 = E1; a.N = N; a.P = P; a.source = source; a.semantics = semantics; a.V = (unsigned)V; a.seed = seed;
    a.mixtures = mixtures; a.table = table; a.acc = acc; a.mean_exit = mean_exit; a.front_count = front_count; a.front_exit_sum = front_exit_sum;
    a.front_hits = front_hits; a.front_vector = front_vector; a.front_thresholds = front_thresholds;
    return a;
}

}  // namespace

extern "C" {

int ee_bucket_lut(int32_t num_buckets, int32_t max_distance, int32_t max_delta, uint8_t* out_host) {
    if (!out_host || num_buckets < 4 || num_buckets > 256 || max_delta < 0) return 1;
    bucket_lut_host(num_buckets, max_distance, max_delta, out_host);
    return 0;
}

// The split-K rule of MMEE_FLAG_LOW_LATENCY (include/mmee.h): the largest S of {8, 4, 2} that divides the K / 32 k-stages of the 128 x 128 tile
// configuration, leaves every part at least 3 stages (its stage ring is three deep: a shorter part would never fill it) and keeps
// tiles x S <= MMEE_LL_TILES_PER_CU x num_cus; else 1.  The tiles are those of the static row count, so S is a function of the call.
// MMEE_LL_TILES_PER_CU: 2 (two workgroups of the launch per CU) against 1, measured at B = 1, 2, 4 with tools/low_latency_ab.py on two builds
// of this file (profiles/low_latency_ab.txt).  The parts buffer of ee_create is sized for 2.
#ifndef MMEE_LL_TILES_PER_CU
#define MMEE_LL_TILES_PER_CU 2
#endif
static_assert(MMEE_LL_TILES_PER_CU == 1 || MMEE_LL_TILES_PER_CU == 2, "the parts buffer holds 2 x num_cus tiles");
int32_t ee_low_latency_k_splits(int32_t max_rows, int32_t N, int32_t K, int32_t num_cus) {
    if (max_rows < 1 || N < 128 || N % 128 != 0 || K < 32 || K % 32 != 0 || num_cus < 1) return 1;
    const long stages = K / 32, tiles = (((long)max_rows + 127) / 128) * (N / 128);
    for (int S = 8; S >= 2; S /= 2)
        if (stages % S == 0 && stages / S >= 3 && tiles * S <= (long)MMEE_LL_TILES_PER_CU * num_cus) return S;
    return 1;
}

// Shader-clock stamps (bench.py: docs_per_sec_per_ghz).  s_memtime counts shader clocks, s_memrealtime a constant 100 MHz.  The shader-clock
// counters of different CUs are NOT aligned with each other (measured, round 5: pairing a stamp taken on one CU with a later stamp taken on
// another CU of the same XCD gave 1.5 ... 3.3 "GHz" over a few milliseconds), so a stamp records one (s_memtime, s_memrealtime) pair PER CU --
// slot = XCC_ID x 256 + HW_ID bits 15:8 (CU, shader array, shader engine) -- and two stamps are compared slot by slot: the offsets cancel.
// 2048 one-wave workgroups, eight per CU on average, so practically every CU is reached by both stamps; the reader skips empty slots.
__global__ void clock_stamp_kernel(unsigned long long* __restrict__ out) {
    if (threadIdx.x != 0) return;
    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 7u;      // HW_REG_XCC_ID
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);            // HW_REG_HW_ID: CU_ID 11:8, SH_ID 12, SE_ID 15:13
    const unsigned slot = xcc * 256u + ((hw >> 8) & 255u);
    const unsigned long long t = __builtin_amdgcn_s_memtime(), r = __builtin_amdgcn_s_memrealtime();
    // several workgroups may land on one CU: the pair is written as one 16-byte store, so whichever wins leaves a consistent pair
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    *reinterpret_cast<u64x2*>(out + 2 * slot) = u64x2{t, r};
}

int ee_clock_stamp(uint64_t* out_dev, void* stream) {
    if (!out_dev) return fail(nullptr, "ee_clock_stamp: null argument");
    if (!have_device("ee_clock_stamp")) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(out_dev, 0, MMEE_CLOCK_STAMP_WORDS * sizeof(uint64_t), s) != hipSuccess) return fail(nullptr, "ee_clock_stamp: memset failed");
    hipLaunchKernelGGL(clock_stamp_kernel, dim3(2048), dim3(64), 0, s, reinterpret_cast<unsigned long long*>(out_dev));
    return launch_status(nullptr, "ee_clock_stamp");
}

int ee_policy_scan(const double* logits, int32_t E1, int32_t N, int32_t K, const double* thresholds, int32_t* exits,
                   double* predictions, double* confidence, int32_t* counts, void* stream) {
    if (!thresholds || E1 < 1 || E1 > 256 || N < 0 || K < 1 || (N > 0 && (!logits || !exits)))
        return fail(nullptr, "ee_policy_scan: bad argument");
    ScanArgs a{};
    a.logits = logits; a.sign = 1.0; a.E1 = E1; a.N = N; a.K = K;
    a.exits = exits; a.pred = predictions; a.conf = confidence; a.counts = counts;
    return run_threshold_scan("ee_policy_scan", "threshold", a, thresholds, E1, SCAN_MSP, RULE_PLAIN, stream);
}

int ee_criterion_scan(const double* logits, int32_t E1, int32_t N, int32_t K, int32_t criterion, const double* thresholds, int32_t* exits,
                      double* predictions, double* confidence, int32_t* counts, void* stream) {
    if (!thresholds || E1 < 1 || E1 > 256 || N < 0 || K < 1 || (N > 0 && (!logits || !exits)))
        return fail(nullptr, "ee_criterion_scan: bad argument (1 <= E1 <= 256, N >= 0, K >= 1, logits / thresholds / exits not NULL)");
    if (criterion != MMEE_CRIT_MAX_CONFIDENCE && criterion != MMEE_CRIT_ENTROPY && criterion != MMEE_CRIT_MARGIN)
        return fail(nullptr, "ee_criterion_scan: criterion %d is not a threshold criterion (MMEE_CRIT_MAX_CONFIDENCE, _ENTROPY, _MARGIN; "
                             "patience: ee_patience_scan)", criterion);
    ScanArgs a{};
    a.logits = logits; a.sign = crit_sign(criterion); a.E1 = E1; a.N = N; a.K = K;
    a.exits = exits; a.pred = predictions; a.conf = confidence; a.counts = counts;
    const int event = criterion == MMEE_CRIT_ENTROPY ? SCAN_ENTROPY : criterion == MMEE_CRIT_MARGIN ? SCAN_MARGIN : SCAN_MSP;
    return run_threshold_scan("ee_criterion_scan", "threshold", a, thresholds, E1, event, RULE_PLAIN, stream);
}

int ee_patience_scan(const double* logits, int32_t E1, int32_t N, int32_t K, int32_t patience, int32_t* exits, double* predictions,
                     double* confidence, int32_t* counts, void* stream) {
    if (patience < 1 || E1 < 1 || N < 0 || K < 1 || (N > 0 && (!logits || !exits))) return fail(nullptr, "ee_patience_scan: bad argument");
    if (!have_device("ee_patience_scan")) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (counts && hipMemsetAsync(counts, 0, sizeof(int) * E1, s) != hipSuccess) return fail(nullptr, "ee_patience_scan: memset failed");
    ScanArgs a{};
    a.logits = logits; a.pat_all = patience; a.E1 = E1; a.N = N; a.K = K;
    a.exits = exits; a.pred = predictions; a.conf = confidence; a.counts = counts;
    if (N > 0) launch_exit_scan(a, SCAN_NONE, RULE_AGREE, s);
    return launch_status(nullptr, "ee_patience_scan");
}

int ee_lte_scan(const double* scores, const double* logits, int32_t E1, int32_t N, int32_t K, const double* thresholds, int32_t* exits,
                double* predictions, int32_t* counts, void* stream) {
    if (!thresholds || E1 < 1 || E1 > 256 || N < 0 || K < 1 || (N > 0 && (!scores || !exits)) || (predictions && !logits))
        return fail(nullptr, "ee_lte_scan: bad argument");
    ScanArgs a{};
    a.logits = logits; a.crit = scores; a.sign = -1.0; a.E1 = E1; a.N = N; a.K = K;      // score < threshold
    a.exits = exits; a.pred = predictions; a.counts = counts;
    return run_threshold_scan("ee_lte_scan", "threshold", a, thresholds, E1, SCAN_TABLE, RULE_PLAIN, stream);
}

int ee_gate_scan(const double* scores, const double* logits, int32_t E1, int32_t N, int32_t K, const double* thresholds, int32_t* exits,
                 double* predictions, double* confidence, int32_t* counts, void* stream) {
    if (!thresholds || E1 < 1 || E1 > 256 || N < 0 || K < 1 || (N > 0 && (!scores || !exits)) || (predictions && !logits))
        return fail(nullptr, "ee_gate_scan: bad argument (1 <= E1 <= 256, N >= 0, K >= 1, scores / thresholds / exits not NULL, predictions need the logits)");
    ScanArgs a{};
    a.logits = logits; a.crit = scores; a.sign = 1.0; a.E1 = E1; a.N = N; a.K = K;       // score > threshold
    a.exits = exits; a.pred = predictions; a.conf = confidence; a.counts = counts;
    return run_threshold_scan("ee_gate_scan", "threshold", a, thresholds, E1, SCAN_TABLE, RULE_PLAIN, stream);
}

int ee_rule_scan(const double* criterion, double sign, const double* logits, int32_t E1, int32_t N, int32_t K, const double* thresholds,
                 const int32_t* patience, int32_t rule, int32_t* exits, double* predictions, double* confidence, int32_t* counts, void* stream) {
    if (!thresholds || !patience || E1 < 1 || E1 > 256 || N < 0 || K < 1 || (N > 0 && (!criterion || !exits)) || (sign != 1.0 && sign != -1.0))
        return fail(nullptr, "ee_rule_scan: bad argument (1 <= E1 <= 256, sign is +1 or -1)");
    if (rule != MMEE_RULE_STREAK && rule != MMEE_RULE_EITHER) return fail(nullptr, "ee_rule_scan: rule %d is neither MMEE_RULE_STREAK nor MMEE_RULE_EITHER", rule);
    if (!logits && (rule == MMEE_RULE_EITHER || predictions)) return fail(nullptr, "ee_rule_scan: MMEE_RULE_EITHER and predictions need the logits");
    for (int e = 0; e < E1; ++e)
        if (patience[e] < 1) return fail(nullptr, "ee_rule_scan: patience[%d]=%d, every patience must be >= 1", e, patience[e]);
    std::vector<double> packed(E1 + (E1 + 1) / 2);                   // thresholds [E1] doubles, then the patience [E1] ints: one upload
    memcpy(packed.data(), thresholds, sizeof(double) * E1);
    memcpy(packed.data() + E1, patience, sizeof(int) * E1);
    ScanArgs a{};
    a.logits = logits; a.crit = criterion; a.sign = sign;
    a.E1 = E1; a.N = N; a.K = K; a.exits = exits; a.pred = predictions; a.conf = confidence; a.counts = counts;
    return run_threshold_scan("ee_rule_scan", "threshold / patience", a, packed.data(), packed.size(), SCAN_TABLE, rule, stream);
}

int ee_quota_scan(const double* table, double sign, int32_t E1, int32_t N, const int32_t* quotas, int32_t mode, const double* thresholds, int32_t G,
                  int32_t* exits, double* cuts, int32_t* workspace, void* stream) {
    const char* who = "ee_quota_scan";
    if (E1 < 1 || E1 > 256 || N < 0 || N >= (1 << 28) || G < 1 || (sign != 1.0 && sign != -1.0))
        return fail(nullptr, "%s: bad argument (1 <= E1 <= 256, 0 <= N < 2^28, G >= 1, sign is +1 or -1)", who);
    if ((E1 > 1 && !quotas) || (N > 0 && (!table || !exits || !workspace))) return fail(nullptr, "%s: table, quotas, exits and workspace must not be NULL", who);
    if (mode != MMEE_QUOTA_EXACT && mode != MMEE_QUOTA_AT_LEAST)
        return fail(nullptr, "%s: unknown mode %d (MMEE_QUOTA_EXACT = %d, MMEE_QUOTA_AT_LEAST = %d)", who, mode, MMEE_QUOTA_EXACT, MMEE_QUOTA_AT_LEAST);
    if (mode == MMEE_QUOTA_AT_LEAST && !thresholds) return fail(nullptr, "%s: MMEE_QUOTA_AT_LEAST needs the thresholds", who);
    for (int e = 0; e + 1 < E1; ++e)
        if (quotas[e] < 0) return fail(nullptr, "%s: quotas[%d]=%d, a quota is a number of documents (>= 0)", who, e, quotas[e]);
    if (!have_device(who)) return 1;
    if (N == 0) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (G > N) G = N;
    const int groups = (N + G - 1) / G;
    // exits = -1 (still active) and cuts = NaN (no such document): both are the all-ones byte pattern
    if (hipMemsetAsync(exits, 0xFF, sizeof(int32_t) * (size_t)N, s) != hipSuccess ||
        (cuts && E1 > 1 && hipMemsetAsync(cuts, 0xFF, sizeof(double) * 2 * (size_t)groups * (E1 - 1), s) != hipSuccess))
        return fail(nullptr, "%s: memset failed", who);
    QuotaScanArgs a{};
    a.table = table; a.sign = sign; a.mode = mode; a.E1 = E1; a.N = N; a.G = G;
    a.exits = exits; a.cuts = cuts; a.rank = workspace;
    if (E1 == 1) {                                          // the last exit takes everybody: nothing to rank
        launch_quota_scan(a, s);
        return launch_status(nullptr, who);
    }
    // one upload (the caller's arrays, as the threshold scans do): the thresholds [E1] doubles when they are read, then the quotas [E1 - 1] ints
    const bool at_least = mode == MMEE_QUOTA_AT_LEAST;
    std::vector<double> packed((at_least ? E1 : 0) + E1 / 2 + 1);
    if (at_least) memcpy(packed.data(), thresholds, sizeof(double) * E1);
    memcpy(packed.data() + (at_least ? E1 : 0), quotas, sizeof(int32_t) * (E1 - 1));
    const TempUpload<double> up(packed.data(), packed.size(), s);
    if (up.err) return fail(nullptr, "%s: threshold / quota %s", who, up.err);
    a.thr = at_least ? up.dev : nullptr;
    a.quotas = reinterpret_cast<const int*>(up.dev + (at_least ? E1 : 0));
    launch_quota_scan(a, s);
    return launch_status(nullptr, who);
}

int ee_rolling_control(const double* table, double sign, const uint8_t* bad, int32_t E1, int32_t N, const double* path, int32_t V, uint64_t cut,
                       uint32_t seed, double alpha, double gamma, double p0, int32_t G, int32_t* exits, int64_t* log, double* p_out, void* stream) {
    const char* who = "ee_rolling_control";
    if (!table || !bad || !path || !exits || !log) return fail(nullptr, "%s: NULL argument (table, bad, path, exits and log are required; p_out may be NULL)", who);
    if (E1 < 2 || E1 > kCtlMaxE1) return fail(nullptr, "%s: E1 = %d, need 2 <= E1 <= %d", who, E1, kCtlMaxE1);
    if (N < 1 || N >= (1 << 28)) return fail(nullptr, "%s: N = %d, need 1 <= N < 2^28", who, N);
    if (G < 1) return fail(nullptr, "%s: G = %d, a group holds at least one document", who, G);
    if (V < 2 || V > (1 << 20)) return fail(nullptr, "%s: V = %d vectors, a path needs 2 <= V <= 2^20", who, V);
    if (sign != 1.0 && sign != -1.0) return fail(nullptr, "%s: sign is +1 or -1", who);
    if (cut < 1 || cut > (1ull << 32)) return fail(nullptr, "%s: cut %llu outside [1, 2^32]", who, (unsigned long long)cut);
    if (!(alpha > 0.0 && alpha < 1.0)) return fail(nullptr, "%s: alpha = %g, the risk level must lie in (0, 1)", who, alpha);
    if (!(gamma > 0.0) || !std::isfinite(gamma)) return fail(nullptr, "%s: gamma = %g, the step must be positive and finite", who, gamma);
    if (!(p0 >= 0.0 && p0 <= (double)(V - 1))) return fail(nullptr, "%s: p0 = %g outside [0, V - 1 = %d]", who, p0, V - 1);
    if (!have_device(who)) return 1;
    RollingControlArgs a{};
    a.table = table; a.bad = bad; a.path = path; a.E1 = E1; a.N = N; a.V = V; a.G = G > N ? N : G;
    a.sign = sign; a.alpha = alpha; a.gamma = gamma; a.p0 = p0; a.cut = cut; a.seed = seed;
    a.exits = exits; a.log = reinterpret_cast<long long*>(log); a.p_out = p_out;
    launch_rolling_control(a, reinterpret_cast<hipStream_t>(stream));
    return launch_status(nullptr, who);
}

int ee_cascade_select(const float* logits, const int32_t* exit_layer, const int32_t* orig, int32_t n, int32_t K, int32_t final_exit,
                      int32_t criterion, double threshold, int32_t* next_orig, int32_t* count_dev, double* crit_out, void* stream) {
    if (n < 0 || K < 1 || final_exit < 0 || !count_dev || (n > 0 && (!logits || !exit_layer || !next_orig)))
        return fail(nullptr, "ee_cascade_select: bad argument (n >= 0, K >= 1, final_exit >= 0, count_dev not NULL, logits / exit_layer / "
                             "next_orig not NULL when n > 0)");
    if (criterion != MMEE_CRIT_MAX_CONFIDENCE && criterion != MMEE_CRIT_ENTROPY && criterion != MMEE_CRIT_MARGIN)
        return fail(nullptr, "ee_cascade_select: criterion %d is not a threshold criterion (MMEE_CRIT_MAX_CONFIDENCE, _ENTROPY, _MARGIN)", criterion);
    if (!have_device("ee_cascade_select")) return 1;
    CascadeSelectArgs a{};
    a.logits = logits; a.exit_layer = exit_layer; a.orig = orig; a.n = n; a.K = K; a.final_exit = final_exit; a.criterion = criterion;
    a.thr = threshold; a.next_orig = next_orig; a.count = count_dev; a.crit = crit_out;
    launch_cascade_select(a, reinterpret_cast<hipStream_t>(stream));     // n == 0 too: the count is written
    return launch_status(nullptr, "ee_cascade_select");
}

int ee_cascade_gather(const ee_cascade_desc* descs, int32_t n_arrays, const int32_t* slots, const int32_t* count_dev, int32_t cap, void* stream) {
    if (n_arrays < 0 || n_arrays > kCascadeMaxArrays)
        return fail(nullptr, "ee_cascade_gather: %d arrays (one launch takes 0 .. %d descriptors)", n_arrays, kCascadeMaxArrays);
    if (cap < 0 || (n_arrays > 0 && !descs) || (n_arrays > 0 && cap > 0 && (!slots || !count_dev)))
        return fail(nullptr, "ee_cascade_gather: bad argument (cap >= 0, descs / slots / count_dev not NULL when there is something to copy)");
    CascadeGatherArgs a{};
    a.n_arrays = n_arrays; a.slots = slots; a.count = count_dev;
    for (int r = 0; r < n_arrays; ++r) {
        const ee_cascade_desc& d = descs[r];
        if (!d.src || !d.dst) return fail(nullptr, "ee_cascade_gather: descriptor %d has a NULL src / dst", r);
        if (d.row_bytes < 4 || d.row_bytes % 4 != 0)
            return fail(nullptr, "ee_cascade_gather: descriptor %d: row_bytes %lld is not a positive multiple of 4", r, (long long)d.row_bytes);
        if (reinterpret_cast<uintptr_t>(d.src) % 4 != 0 || reinterpret_cast<uintptr_t>(d.dst) % 4 != 0)
            return fail(nullptr, "ee_cascade_gather: descriptor %d: src / dst is not 4-byte aligned", r);
        a.src[r] = static_cast<const char*>(d.src); a.dst[r] = static_cast<char*>(d.dst); a.row_bytes[r] = (size_t)d.row_bytes;
    }
    if (!have_device("ee_cascade_gather")) return 1;
    if (n_arrays > 0 && cap > 0) launch_cascade_gather(a, cap, reinterpret_cast<hipStream_t>(stream));
    return launch_status(nullptr, "ee_cascade_gather");
}

int ee_cascade_merge(const float* logits, const int32_t* exit_layer, const float* confidence, const int32_t* slots, int32_t n, int32_t K,
                     int32_t exit_offset, int32_t stage, float* out_logits, int32_t* out_exit, float* out_confidence, int32_t* out_stage,
                     void* stream) {
    if (n < 0 || K < 1 || exit_offset < 0 || stage < 0 ||
        (n > 0 && (!logits || !exit_layer || !confidence || !slots || !out_logits || !out_exit || !out_confidence || !out_stage)))
        return fail(nullptr, "ee_cascade_merge: bad argument (n >= 0, K >= 1, exit_offset, stage >= 0, no NULL pointer when n > 0)");
    if (!have_device("ee_cascade_merge")) return 1;
    CascadeMergeArgs a{};
    a.logits = logits; a.exit_layer = exit_layer; a.conf = confidence; a.slots = slots; a.n = n; a.K = K; a.exit_offset = exit_offset;
    a.stage = stage; a.out_logits = out_logits; a.out_exit = out_exit; a.out_conf = out_confidence; a.out_stage = out_stage;
    if (n > 0) launch_cascade_merge(a, reinterpret_cast<hipStream_t>(stream));
    return launch_status(nullptr, "ee_cascade_merge");
}

int ee_rule_sweep(const double* conf, const double* logits, const int64_t* references, int32_t E1, int32_t N, int32_t K, const double* thr, int32_t V,
                  const int32_t* patiences, int32_t P, int32_t rule, double* acc, double* mean_exit, int32_t* exit_hist, void* stream) {
    if (!conf || !logits || !references || !thr || !patiences || !acc || !mean_exit || E1 < 1 || E1 > 64 || N < 1 || N >= (1 << 24) || K < 1 || V < 0 ||
        P < 1 || P > 128)
        return fail(nullptr, "ee_rule_sweep: bad argument (E1 <= 64, 1 <= N < 2^24, 1 <= P <= 128)");
    if (rule != MMEE_RULE_STREAK && rule != MMEE_RULE_EITHER) return fail(nullptr, "ee_rule_sweep: rule %d is neither MMEE_RULE_STREAK nor MMEE_RULE_EITHER", rule);
    for (int j = 0; j < P; ++j)
        if (patiences[j] < 1) return fail(nullptr, "ee_rule_sweep: patiences[%d]=%d, every patience must be >= 1", j, patiences[j]);
    if (!have_device("ee_rule_sweep")) return 1;
    if (V == 0) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const TempUpload<int> pats(patiences, P, s);
    if (pats.err) return fail(nullptr, "ee_rule_sweep: patience %s", pats.err);
    if (!launch_rule_sweep(conf, logits, reinterpret_cast<const long long*>(references), E1, N, K, thr, V, patiences, pats.dev, P, rule, acc, mean_exit,
                           exit_hist, s))
        return fail(nullptr, "ee_rule_sweep: hipMallocAsync failed");
    return launch_status(nullptr, "ee_rule_sweep");
}

int ee_patience_sweep(const double* logits, const int64_t* references, int32_t E1, int32_t N, int32_t K, const int32_t* patiences, int32_t V,
                      double* acc, double* mean_exit, int32_t* exit_hist, void* stream) {
    if (!logits || !references || !patiences || !acc || !mean_exit || E1 < 1 || E1 > 128 || N < 1 || K < 1 || V < 0)
        return fail(nullptr, "ee_patience_sweep: bad argument (E1 <= 128, N >= 1)");
    if (!have_device("ee_patience_sweep")) return 1;
    if (V > 0 && !launch_patience_sweep(logits, reinterpret_cast<const long long*>(references), E1, N, K, patiences, V, acc, mean_exit, exit_hist,
                                        reinterpret_cast<hipStream_t>(stream)))
        return fail(nullptr, "ee_patience_sweep: hipMallocAsync failed");
    return launch_status(nullptr, "ee_patience_sweep");
}

int ee_pack_results(const float* logits, const int32_t* exit_layer, const float* confidence, int32_t n, int32_t K, int32_t* rows, void* stream) {
    if (n < 0 || K < 1 || (n > 0 && (!logits || !exit_layer || !confidence || !rows))) return fail(nullptr, "ee_pack_results: bad argument");
    if (!have_device("ee_pack_results")) return 1;
    if (n > 0) launch_pack_results(logits, exit_layer, confidence, n, K, rows, reinterpret_cast<hipStream_t>(stream));
    return launch_status(nullptr, "ee_pack_results");
}

int ee_unpack_results(const int32_t* rows, int32_t n, int32_t K, float* logits, int32_t* exit_layer, float* confidence, void* stream) {
    if (n < 0 || K < 1 || (n > 0 && !rows)) return fail(nullptr, "ee_unpack_results: bad argument");
    if (!have_device("ee_unpack_results")) return 1;
    if (n > 0) launch_unpack_results(rows, n, K, logits, exit_layer, confidence, reinterpret_cast<hipStream_t>(stream));
    return launch_status(nullptr, "ee_unpack_results");
}

int ee_threshold_sweep(const double* conf, const uint8_t* correct, int32_t E1, int32_t N, const double* thr, int32_t V, double* acc,
                       double* mean_exit, int32_t* exit_hist, void* stream) {
    if (!conf || !correct || !thr || !acc || !mean_exit || E1 < 1 || E1 > 64 || N < 1 || V < 0)
        return fail(nullptr, "ee_threshold_sweep: bad argument");
    if (!have_device("ee_threshold_sweep")) return 1;
    if (V > 0) launch_threshold_sweep(conf, correct, E1, N, thr, V, acc, mean_exit, exit_hist, reinterpret_cast<hipStream_t>(stream));
    return launch_status(nullptr, "ee_threshold_sweep");
}

// The refusals ee_threshold_search and ee_threshold_search_cost share, in this order, before any device call; GRID sets *V.  0: accepted.
static int search_refuse(const char* who, int32_t E1, int32_t N, int32_t P, int32_t source, int64_t* V, const uint8_t* mixtures, int32_t semantics) {
    if (E1 < 2 || E1 > 64) return fail(nullptr, "%s: E1 = %d, need 2 <= E1 <= 64", who, E1);
    if (N < 1 || N >= (1 << 24)) return fail(nullptr, "%s: N = %d, need 1 <= N < 2^24 (a rank takes 24 bits of a record)", who, N);
    if (P < 2 || P > 64) return fail(nullptr, "%s: P = %d thresholds per exit, need 2 <= P <= 64", who, P);
    if (semantics != MMEE_SEARCH_REFERENCE && semantics != MMEE_SEARCH_POLICY)
        return fail(nullptr, "%s: semantics %d is neither MMEE_SEARCH_REFERENCE nor MMEE_SEARCH_POLICY", who, semantics);
    if (source == MMEE_SEARCH_GRID) {
        unsigned long long grid = 1;
        for (int e = 0; e < E1 - 1 && grid < (1ull << 32); ++e) grid *= (unsigned long long)P;
        if (grid >= (1ull << 32))
            return fail(nullptr, "%s: the grid of P = %d thresholds at %d exits has P^(E1-1) >= 2^32 vectors; sample it (MMEE_SEARCH_SAMPLED with V < 2^32)", who, P, E1 - 1);
        *V = (int64_t)grid;
    } else if (source == MMEE_SEARCH_SAMPLED || source == MMEE_SEARCH_MIXTURES) {
        if (*V < 1 || *V >= (1ll << 32)) return fail(nullptr, "%s: V = %lld vectors, need 1 <= V < 2^32", who, (long long)*V);
        if (source == MMEE_SEARCH_MIXTURES && !mixtures) return fail(nullptr, "%s: MMEE_SEARCH_MIXTURES without mixtures (NULL)", who);
    } else {
        return fail(nullptr, "%s: source %d is none of MMEE_SEARCH_GRID, _SAMPLED, _MIXTURES", who, source);
    }
    return 0;
}

// the percentiles' (lower index, upper index, weight): numpy's linspace, true_divide, (n - 1) * q, floor, in double
static SearchPercentiles search_percentiles(int N, int P) {
    SearchPercentiles pc{};
    const double step = 100.0 / (double)(P - 1);
    for (int j = 0; j < P; ++j) {
        const double perc = j == P - 1 ? 100.0 : (double)j * step;
        const double x = (double)(N - 1) * (perc / 100.0);
        if (x >= (double)(N - 1)) {
            pc.lo[j] = pc.hi[j] = N - 1;                            // numpy: previous = next = -1, gamma = x - (-1); the neighbours are equal
            pc.t[j] = x + 1.0;
        } else {
            const double f = floor(x);
            pc.lo[j] = (int)f;
            pc.hi[j] = (int)f + 1;
            pc.t[j] = x - f;
        }
    }
    return pc;
}

int ee_threshold_search(const double* conf, const uint8_t* correct, int32_t E1, int32_t N, int32_t P, int32_t source, int64_t V, uint64_t seed,
                        const uint8_t* mixtures, int32_t semantics, double* table, double* acc, double* mean_exit, int32_t* front_count,
                        int32_t* front_exit_sum, int32_t* front_hits, uint32_t* front_vector, double* front_thresholds, void* stream) {
    const char* who = "ee_threshold_search";
    if (!conf || !correct || !table || !front_count || !front_exit_sum || !front_hits || !front_vector || !front_thresholds)
        return fail(nullptr, "%s: NULL argument (conf, correct, table and the five front outputs are required; acc and mean_exit may be NULL)", who);
    if (search_refuse(who, E1, N, P, source, &V, mixtures, semantics)) return 1;
    const long long n_buckets = (long long)N * (E1 - 1) + 1;
    if (n_buckets > (1ll << 26))
        return fail(nullptr, "%s: N (E1-1) + 1 = %lld exit-sum buckets, more than 2^26", who, n_buckets);
    if (!have_device(who)) return 1;
    const SearchPercentiles pc = search_percentiles(N, P);
    const SearchArgs a = search_args(conf, correct, E1, N, P, source, V, seed, mixtures, semantics, table, acc, mean_exit, front_count, front_exit_sum,
                                     front_hits, front_vector, front_thresholds);
    if (!launch_threshold_search(a, pc, reinterpret_cast<hipStream_t>(stream))) return fail(nullptr, "%s: hipMallocAsync of the workspace failed", who);
    return launch_status(nullptr, who);
}

int ee_threshold_search_cost(const double* conf, const uint8_t* correct, const uint32_t* cost, int32_t E1, int32_t N, int32_t P, int32_t source,
                             int64_t V, uint64_t seed, const uint8_t* mixtures, int32_t semantics, double* table, double* acc, double* mean_exit,
                             uint64_t* cost_sum, int32_t* front_count, uint64_t* front_cost_sum, int32_t* front_exit_sum, int32_t* front_hits,
                             uint32_t* front_vector, double* front_thresholds, void* stream) {
    const char* who = "ee_threshold_search_cost";
    if (!conf || !correct || !cost || !table || !front_count || !front_cost_sum || !front_exit_sum || !front_hits || !front_vector || !front_thresholds)
        return fail(nullptr, "%s: NULL argument (conf, correct, cost, table and the six front outputs are required; acc, mean_exit and cost_sum may be NULL)", who);
    if (search_refuse(who, E1, N, P, source, &V, mixtures, semantics)) return 1;
    if (!have_device(who)) return 1;
    const SearchPercentiles pc = search_percentiles(N, P);
    SearchCostArgs c{};
    c.base = search_args(conf, correct, E1, N, P, source, V, seed, mixtures, semantics, table, acc, mean_exit, front_count, front_exit_sum, front_hits,
                         front_vector, front_thresholds);
    c.cost = cost; c.cost_sum = reinterpret_cast<unsigned long long*>(cost_sum); c.front_cost_sum = reinterpret_cast<unsigned long long*>(front_cost_sum);
    if (!launch_threshold_search_cost(c, pc, reinterpret_cast<hipStream_t>(stream))) return fail(nullptr, "%s: hipMallocAsync of the workspace failed", who);
    return launch_status(nullptr, who);
}

int ee_threshold_refine(const double* conf, const uint8_t* correct, const uint32_t* cost, int32_t E1, int32_t N, int32_t P, int32_t S,
                        const uint8_t* start, const uint64_t* hit_value, const uint64_t* budget, int32_t max_rounds, uint8_t* digits,
                        double* thresholds, int32_t* hits, int32_t* exit_sum, uint64_t* cost_sum, int32_t* rounds, int32_t* status,
                        int32_t* start_hits, uint64_t* start_cost_sum, double* table, void* stream) {
    const char* who = "ee_threshold_refine";
    if (!conf || !correct || !start || !hit_value || !digits)
        return fail(nullptr, "%s: NULL argument (conf, correct, start, hit_value and digits are required; cost, budget and the other outputs may be NULL)", who);
    int64_t one = 1;                                                 // the searches' range checks of E1, N and P
    if (search_refuse(who, E1, N, P, MMEE_SEARCH_SAMPLED, &one, nullptr, MMEE_SEARCH_POLICY)) return 1;
    if (S < 1 || S > 4096) return fail(nullptr, "%s: S = %d chains, need 1 <= S <= 4096", who, S);
    if (max_rounds < 1 || max_rounds > 4096) return fail(nullptr, "%s: max_rounds = %d, need 1 <= max_rounds <= 4096", who, max_rounds);
    if (!have_device(who)) return 1;
    const SearchPercentiles pc = search_percentiles(N, P);
    RefineArgs a{};
    a.conf = conf; a.correct = correct; a.cost = cost; a.E1 = E1; a.N = N; a.P = P; a.S = S; a.max_rounds = max_rounds; a.start = start;
    a.hit_value = reinterpret_cast<const unsigned long long*>(hit_value); a.budget = reinterpret_cast<const unsigned long long*>(budget);
    a.digits = digits; a.thresholds = thresholds; a.hits = hits; a.exit_sum = exit_sum; a.cost_sum = reinterpret_cast<unsigned long long*>(cost_sum);
    a.rounds = rounds; a.status = status; a.start_hits = start_hits; a.start_cost_sum = reinterpret_cast<unsigned long long*>(start_cost_sum);
    a.table = table;
    if (!launch_threshold_refine(a, pc, reinterpret_cast<hipStream_t>(stream)))
        return fail(nullptr, "%s: hipMallocAsync of the workspace failed (%zu bytes for the rounds)", who, threshold_refine_workspace_bytes(E1, N, P, S));
    return launch_status(nullptr, who);
}

size_t ee_threshold_refine_workspace_bytes(int32_t E1, int32_t N, int32_t P, int32_t S) {
    if (E1 < 2 || E1 > 64 || N < 1 || N >= (1 << 24) || P < 2 || P > 64 || S < 1 || S > 4096) return 0;
    return threshold_refine_workspace_bytes(E1, N, P, S);
}

int ee_msp_table(const double* logits, const int64_t* references, int32_t E1, int32_t N, int32_t K, double* conf, uint8_t* correct,
                 void* stream) {
    if (!logits || !conf || E1 < 1 || N < 1 || K < 1) return fail(nullptr, "ee_msp_table: bad argument");
    if (!have_device("ee_msp_table")) return 1;
    launch_csf_table(logits, (const long long*)references, E1, N, K, MMEE_CRIT_MAX_CONFIDENCE, conf, correct, reinterpret_cast<hipStream_t>(stream));
    return launch_status(nullptr, "ee_msp_table");
}

int ee_csf_table(const double* logits, const int64_t* references, int32_t E1, int32_t N, int32_t K, int32_t criterion, double* table,
                 uint8_t* correct, void* stream) {
    if (!logits || !table || E1 < 1 || N < 1 || K < 1 || (correct && !references))
        return fail(nullptr, "ee_csf_table: bad argument (logits / table not NULL, E1, N, K >= 1, correct needs the references)");
    if (criterion != MMEE_CRIT_MAX_CONFIDENCE && criterion != MMEE_CRIT_ENTROPY && criterion != MMEE_CRIT_MARGIN)
        return fail(nullptr, "ee_csf_table: criterion %d has no table (MMEE_CRIT_MAX_CONFIDENCE, _ENTROPY, _MARGIN have; patience is no "
                             "function of one row)", criterion);
    if (!have_device("ee_csf_table")) return 1;
    launch_csf_table(logits, (const long long*)references, E1, N, K, criterion, table, correct, reinterpret_cast<hipStream_t>(stream));
    return launch_status(nullptr, "ee_csf_table");
}

int ee_gate_table(const float* head_logits, const double* final_logits, int32_t E, int32_t N, int32_t K, double* table, void* stream) {
    if (!final_logits || !table || E < 0 || N < 1 || K < 1 || (E > 0 && !head_logits))
        return fail(nullptr, "ee_gate_table: bad argument (final_logits / table not NULL, head_logits not NULL when E > 0, E >= 0, N, K >= 1)");
    if (!have_device("ee_gate_table")) return 1;
    launch_gate_table(head_logits, final_logits, E, N, K, table, reinterpret_cast<hipStream_t>(stream));
    return launch_status(nullptr, "ee_gate_table");
}

int ee_ensemble_logits(const double* logits, int32_t E1, int32_t N, int32_t K, const double* w, const double* b, double* out, void* stream) {
    if (!logits || !w || !out || E1 < 1 || N < 1 || K < 1)
        return fail(nullptr, "ee_ensemble_logits: bad argument (logits / w / out not NULL, E1, N, K >= 1)");
    if (!have_device("ee_ensemble_logits")) return 1;
    launch_ensemble_logits(logits, E1, N, K, w, b, out, reinterpret_cast<hipStream_t>(stream));
    return launch_status(nullptr, "ee_ensemble_logits");
}

static_assert(kMetricAccuracy == MMEE_METRIC_ACCURACY && kMetricBrier == MMEE_METRIC_BRIER && kMetricNll == MMEE_METRIC_NLL &&
              kMetricF1Micro == MMEE_METRIC_F1_MICRO && kMetricF1Macro == MMEE_METRIC_F1_MACRO && kMetricEce == MMEE_METRIC_ECE &&
              kMetricAurc == MMEE_METRIC_AURC && kMetricAvgConf == MMEE_METRIC_AVG_CONF && kMetricCount == MMEE_METRIC_COUNT,
              "the kernels' metric columns are the ABI's");
int ee_exit_metrics(const double* logits, const int64_t* references, const double* conf, const uint8_t* correct, const double* temperatures,
                    const int32_t* exits, int32_t E1, int32_t N, int32_t K, int32_t n_bins, double* out, int64_t* confusion, int64_t* exit_hist,
                    void* stream) {
    const char* who = "ee_exit_metrics";
    if (!out) return fail(nullptr, "%s: NULL argument (out is required)", who);
    if (logits && !references) return fail(nullptr, "%s: NULL argument (logits need the references)", who);
    if (!logits && (!conf || !correct)) return fail(nullptr, "%s: NULL argument (without logits the table form needs conf and correct)", who);
    if (!logits && confusion) return fail(nullptr, "%s: the table form has no predictions: confusion must be NULL", who);
    if (exit_hist && !exits) return fail(nullptr, "%s: exit_hist counts the values of exits, which is NULL", who);
    if (E1 < 1 || E1 > 256) return fail(nullptr, "%s: E1 = %d, need 1 <= E1 <= 256", who, E1);
    if (N < 1) return fail(nullptr, "%s: N = %d, need N >= 1", who, N);
    if (N > kMetricsMaxN) return fail(nullptr, "%s: N = %d, more than 2^20: the counting sort of a row is O(N^2)", who, N);
    if (logits && K < 1) return fail(nullptr, "%s: K = %d, need K >= 1", who, K);
    if (n_bins > kMetricsMaxBins) return fail(nullptr, "%s: n_bins = %d, more than %d", who, n_bins, kMetricsMaxBins);
    if (!have_device(who)) return 1;
    MetricsArgs a{};
    a.logits = logits; a.references = reinterpret_cast<const long long*>(references); a.conf = conf; a.correct = correct;
    a.temperatures = temperatures; a.exits = exits; a.E1 = E1; a.N = N; a.K = logits ? K : 1;
    a.n_bins = n_bins > 0 ? n_bins : (N - 1 < 1 ? 1 : N - 1 > 100 ? 100 : N - 1);
    a.out = out; a.confusion = reinterpret_cast<unsigned long long*>(confusion); a.exit_hist = reinterpret_cast<unsigned long long*>(exit_hist);
    if (!launch_exit_metrics(a, reinterpret_cast<hipStream_t>(stream))) return fail(nullptr, "%s: hipMallocAsync of the workspace failed", who);
    return launch_status(nullptr, who);
}

int ee_temperature_fit(const double* logits, const int64_t* labels, int32_t E1, int32_t N, int32_t K, int32_t max_iter,
                       double* temperature, double* nll, double* accuracy, double* avg_confidence, int32_t* iterations, void* stream) {
    if (!logits || !labels || !temperature || E1 < 1 || N < 1 || K < 2) return fail(nullptr, "ee_temperature_fit: bad argument");
    if (!have_device("ee_temperature_fit")) return 1;
    launch_temperature_fit(logits, (const long long*)labels, E1, N, K, max_iter > 0 ? max_iter : 100, temperature, nll, accuracy,
                           avg_confidence, iterations, reinterpret_cast<hipStream_t>(stream));
    return launch_status(nullptr, "ee_temperature_fit");
}

// ---- device-side input feed (N2) ----------------------------------------------------------------------------------------
int ee_preprocess_images(const uint8_t* images, const void* desc, int32_t B, int32_t R, int32_t max_h, void* workspace,
                         size_t workspace_bytes, float* pixel_values, uint8_t* resized_u8, void* stream) {
    constexpr int KMAX = 64;
    if (!images || !desc || !workspace || !pixel_values || B < 1 || R < 1 || max_h < 1) return fail(nullptr, "ee_preprocess_images: bad argument");
    // the one side the host can see: a taller page needs more than KMAX taps per output pixel (the widths are the caller's duty, include/mmee.h)
    if ((long long)max_h > (long long)((KMAX - 1) / 2) * R)
        return fail(nullptr, "ee_preprocess_images: max_h %d is above %d R = %lld (the tap tables hold %d taps per output pixel)", max_h, (KMAX - 1) / 2,
                    (long long)((KMAX - 1) / 2) * R, KMAX);
    if (!have_device("ee_preprocess_images")) return 1;
    // workspace layout: lut[256] f32 | bounds[B*2*R] int2 | kk[B*2*R*KMAX] int | tmp[B*max_h*R*3] u8
    const size_t o_lut = 0, o_b = 1024, o_k = o_b + sizeof(int2) * (size_t)B * 2 * R;
    const size_t o_t = (o_k + sizeof(int) * (size_t)B * 2 * R * KMAX + 255) & ~(size_t)255;
    const size_t need = o_t + (size_t)B * max_h * R * 3;
    if (workspace_bytes < need) return fail(nullptr, "ee_preprocess_images: workspace needs %zu bytes", need);
    char* ws = static_cast<char*>(workspace);
    float lut[256];
    for (int u = 0; u < 256; ++u) {              // HF rescale (float64 product -> float32) then normalize in float32
        const float v = (float)((double)u * (1.0 / 255.0));
        lut[u] = (v - 0.5f) / 0.5f;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemcpyAsync(ws + o_lut, lut, sizeof(lut), hipMemcpyHostToDevice, s) != hipSuccess) return fail(nullptr, "ee_preprocess_images: lut copy failed");
    launch_preprocess_images(images, static_cast<const ImageDesc*>(desc), B, R, KMAX, max_h, reinterpret_cast<int2*>(ws + o_b),
                             reinterpret_cast<int*>(ws + o_k), reinterpret_cast<unsigned char*>(ws + o_t),
                             reinterpret_cast<const float*>(ws + o_lut), pixel_values, resized_u8, s);
    return launch_status(nullptr, "ee_preprocess_images");
}

size_t ee_preprocess_workspace_bytes(int32_t B, int32_t R, int32_t max_h) {
    constexpr int KMAX = 64;
    const size_t o_b = 1024, o_k = o_b + sizeof(int2) * (size_t)B * 2 * R;
    const size_t o_t = (o_k + sizeof(int) * (size_t)B * 2 * R * KMAX + 255) & ~(size_t)255;
    return o_t + (size_t)B * max_h * R * 3;
}

int ee_collate_pad(const int64_t* ids, const int64_t* boxes, const int64_t* offsets, int32_t B, int32_t T, int64_t pad_id,
                   int64_t* out_ids, int64_t* out_mask, int64_t* out_bbox, void* stream) {
    if (!ids || !boxes || !offsets || !out_ids || !out_mask || !out_bbox || B < 1 || T < 1) return fail(nullptr, "ee_collate_pad: bad argument");
    if (!have_device("ee_collate_pad")) return 1;
    launch_collate_pad((const long long*)ids, (const long long*)boxes, (const long long*)offsets, B, T, pad_id,
                       (long long*)out_ids, (long long*)out_mask, (long long*)out_bbox, reinterpret_cast<hipStream_t>(stream));
    return launch_status(nullptr, "ee_collate_pad");
}

// ---- debug / micro-benchmark hooks: run ONE kernel of the path on caller-provided device buffers ------------------------
int ee_debug_gemm(const float* A, const float* W, const float* bias, const float* resid, float* Cout, int32_t M, int32_t N,
                  int32_t K, int32_t epi, int32_t wgs_per_cu, const int32_t* row_src, uint64_t* clk_probe, void* stream) {
    if (!A || !W || !Cout || M < 1 || N % 128 || K % 32 || epi < 0 || (epi & 15) > 3) return fail(nullptr, "ee_debug_gemm: bad argument");
    const int cus = device_cus("ee_debug_gemm");
    if (!cus) return 1;
    GemmArgs g{};
    g.A = A; g.lda = K; g.W = W; g.bias = bias; g.C = Cout; g.ldc = N; g.resid = resid; g.ldr = N; g.m_static = M; g.N = N; g.K = K;
    g.scale = 1.f;
    g.clk_probe = (unsigned long long*)clk_probe;
    static int* dbg_head = nullptr;
    if (!dbg_head && hipMalloc((void**)&dbg_head, 512) != hipSuccess) return fail(nullptr, "ee_debug_gemm: hipMalloc failed");
    if (hipMemsetAsync(dbg_head, 0, 512, reinterpret_cast<hipStream_t>(stream)) != hipSuccess) return fail(nullptr, "ee_debug_gemm: memset failed");
#ifndef MMEE_DIAG
    if (epi & (32 | 512 | 1024)) return fail(nullptr, "ee_debug_gemm: timing variants (wrong results) exist in the diagnostic library only (make diag)");
#endif
    g.tile_counter = (epi & 16) ? nullptr : dbg_head;    // epi | 16 = static grid stride (A/B switch)
    g.dbg_noload = ((epi & 32) ? 1 : 0) | ((epi & 512) ? 2 : 0) | ((epi & 1024) ? 4 : 0) | (((epi >> 12) & 255) << 8);   // epi bits 12..19: stagger (x 8128 cycles) for odd wave slots   // epi | 512 = no k-loop barrier (DMA variant; timing diagnostic, wrong results)
    g.prio_mode = (epi >> 6) & 3;                         // epi | 64 / 128: static priority variants
    g.use_dma = ((epi >> 8) & 1) ? 1 : 2;                 // epi | 256: LDS-DMA staging kernel, else the register-staged one                    // epi | 32 = no in-loop global loads (timing diagnostic)
    epi &= 15;
    g.row_src = row_src;
    g.resid_row_src = row_src;
    if (epi == EPI_RESID && !resid) return fail(nullptr, "ee_debug_gemm: residual epilogue without a residual");
    if (wgs_per_cu < 0) {   // diagnostic: stamped build, |wgs_per_cu| workgroups per CU, 8 uint64 per workgroup in clk_probe
        launch_gemm_f32_stamped(g, epi, -wgs_per_cu * cus, reinterpret_cast<hipStream_t>(stream));
    } else {
        set_gemm_wgs_per_cu(wgs_per_cu);
        launch_gemm_f32(g, epi, AMODE_ROWS, M, cus, reinterpret_cast<hipStream_t>(stream));
        set_gemm_wgs_per_cu(0);
    }
    return launch_status(nullptr, "ee_debug_gemm");
}

int ee_debug_attn_stamps(uint64_t* out8) {
    unsigned long long* d = mmee::attention_idx_stamps() ? mmee::attention_idx_stamps() : mmee::attention_pair_stamps();
    if (!out8 || !d) return fail(nullptr, "ee_debug_attn_stamps: no stamped launch has run (set MMEE_ATTN_STAMPS=1 before the first forward)");
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out8, d, 64, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(nullptr, "ee_debug_attn_stamps: copy failed");
    (void)hipMemset(d, 0, 64);
    return 0;
}

// a row map of the caller's, on a host copy: every entry inside [0, rows)
static int check_row_map(const char* who, const char* what, const int32_t* map, int M, int rows) {
    std::vector<int> h;
    if (!to_host(h, map, (size_t)M)) return fail(nullptr, "%s: copy of %s failed", who, what);
    for (int i = 0; i < M; ++i)
        if (h[i] < 0 || h[i] >= rows) return fail(nullptr, "%s: %s[%d] = %d outside [0, %d)", who, what, i, h[i], rows);
    return 0;
}

// What the three split-GEMM hooks share: the operands to split planes (resid_scale != 0: the f32 residual too), M to the device when the
// kernel is to read it there, `iters` launches (the first untimed), the time per launch.  dbg: the timing-diagnostic bits of ee_debug_gemm_split.
static int run_debug_gemm_split(const char* who, const ee_debug_gemm_routes_args& a, int dbg, float* ms_out, hipStream_t s) {
    const int N = a.N, K = a.K, M = a.M, rows_A = a.rows_A, rows_resid = a.rows_resid, iters = a.iters;
    const int max_m = a.m_on_device ? a.max_m : M;
    GemmArgs g{};
    g.lda = K; g.bias = a.bias; g.C = a.Cout; g.ldc = N; g.resid = a.resid; g.ldr = N; g.m_static = M; g.N = N; g.K = K;
    g.scale_cols = a.scale_cols; g.scale = a.scale; g.col_scale = a.col_scale;
    g.alpha = 1.0f / (a.a_scale * a.w_scale); g.out_split = a.out_split ? 1 : 0; g.out_scale = a.out_scale;
    g.row_src = a.row_src; g.resid_row_src = a.resid_row_src; g.route = a.route; g.role_tag = a.role_tag; g.probe = a.probe ? 1 : 0;
    g.terms = a.terms; g.k_splits = a.k_splits; g.split_stride = a.split_stride; g.dbg_noload = dbg;
    const int cus = device_cus(who);
    if (!cus) return 1;
    const bool split_resid = a.resid && a.resid_scale != 0.f;
    float *As = nullptr, *Ws = nullptr, *Rs = nullptr;
    int *heads = nullptr, *m_dev = nullptr, *err_flag = nullptr;      // err_flag: the launches' error word, for a caller that asks for it
    if (hipMalloc((void**)&As, (size_t)rows_A * K * 4) != hipSuccess || hipMalloc((void**)&Ws, (size_t)N * K * 4) != hipSuccess ||
        hipMalloc((void**)&heads, 512) != hipSuccess || (a.m_on_device && hipMalloc((void**)&m_dev, sizeof(int)) != hipSuccess) ||
        (split_resid && hipMalloc((void**)&Rs, (size_t)rows_resid * N * 4) != hipSuccess) ||
        (a.err_flag_out && (hipMalloc((void**)&err_flag, sizeof(int)) != hipSuccess || hipMemsetAsync(err_flag, 0, sizeof(int), s) != hipSuccess))) {
        (void)hipFree(As); (void)hipFree(Ws); (void)hipFree(heads); (void)hipFree(m_dev); (void)hipFree(Rs); (void)hipFree(err_flag);
        return fail(nullptr, "%s: hipMalloc failed", who);
    }
    g.err_flag = err_flag;
    mmee::launch_split_rows(a.A, As, nullptr, rows_A, rows_A, K, a.a_scale, cus, s, err_flag);
    mmee::launch_split_rows(a.W, Ws, nullptr, N, N, K, a.w_scale, cus, s, err_flag);
    // the probes of a forward take their tiles statically (capi_forward.hip layer_probe): no queue head
    g.A = As; g.W = Ws; g.tile_counter = a.probe ? nullptr : heads;
    if (split_resid) {
        mmee::launch_split_rows(a.resid, Rs, nullptr, rows_resid, rows_resid, N, a.resid_scale, cus, s, err_flag);
        g.resid = Rs; g.resid_split_inv = 1.0f / a.resid_scale;
    }
    if (m_dev) {      // (M lives until the synchronisation below)
        (void)hipMemcpyAsync(m_dev, &M, sizeof(int), hipMemcpyHostToDevice, s);
        g.m_ptr = m_dev;
    }
    // diagnostic builds (any dbg bit; bit 256 = "diagnostic build, nothing removed") report the shader clock they ran at:
    // ms_out[1] = GHz averaged over the workgroups of the last launch
    unsigned long long* clk = nullptr;
    const int n_clk = 2 * 2 * cus;
    if (dbg && ms_out) {
        if (hipMalloc((void**)&clk, n_clk * 8) == hipSuccess) (void)hipMemsetAsync(clk, 0, n_clk * 8, s);
        g.clk_probe = clk;
    }
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipMemsetAsync(heads, 0, 512, s);
    launch_gemm_split(g, a.epi, max_m, cus, s);          // first launch untimed (code object load)
    (void)hipEventRecord(e0, s);
    for (int i = 1; i < iters; ++i) {
        (void)hipMemsetAsync(heads, 0, 512, s);
        launch_gemm_split(g, a.epi, max_m, cus, s);
    }
    (void)hipEventRecord(e1, s);
    const hipError_t err = hipStreamSynchronize(s);
    float ms = 0.f;
    if (iters > 1) (void)hipEventElapsedTime(&ms, e0, e1);
    if (ms_out) *ms_out = iters > 1 ? ms / (float)(iters - 1) : 0.f;
    if (clk) {
        std::vector<unsigned long long> hc(n_clk);
        (void)hipMemcpy(hc.data(), clk, n_clk * 8, hipMemcpyDeviceToHost);
        double sum = 0;
        int n = 0;
        for (int i = 0; i + 1 < n_clk; i += 2)
            if (hc[i + 1]) { sum += (double)hc[i] / (double)hc[i + 1] * 0.1; ++n; }
        ms_out[1] = n ? (float)(sum / n) : 0.f;
        (void)hipFree(clk);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    const bool err_read = !err_flag || hipMemcpy(a.err_flag_out, err_flag, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(As); (void)hipFree(Ws); (void)hipFree(heads); (void)hipFree(m_dev); (void)hipFree(Rs); (void)hipFree(err_flag);
    if (err == hipSuccess && !err_read) return fail(nullptr, "%s: copy of err_flag failed", who);
    if (err != hipSuccess || hipGetLastError() != hipSuccess) return fail(nullptr, "%s: launch failed: %s", who, hipGetErrorString(err));
    return 0;
}

// the operands ee_debug_gemm_split and ee_debug_gemm_split_resid share, as the arguments of the hook they wrap: one part, three terms, no
// column factors, M from the host
static ee_debug_gemm_routes_args plain_split_args(const float* A, const float* W, const float* bias, const float* resid, float* Cout, int M, int N, int K,
                                                  int epi, float a_scale, float w_scale, const int32_t* row_src, int rows_A, int iters) {
    ee_debug_gemm_routes_args a{};
    a.A = A; a.W = W; a.bias = bias; a.resid = resid; a.Cout = Cout; a.M = M; a.N = N; a.K = K; a.epi = epi;
    a.a_scale = a_scale; a.w_scale = w_scale; a.row_src = row_src; a.rows_A = rows_A; a.terms = 3; a.k_splits = 1; a.scale = 1.f; a.iters = iters;
    return a;
}

int ee_debug_gemm_split(const float* A, const float* W, const float* bias, const float* resid, float* Cout, int32_t M, int32_t N,
                        int32_t K, int32_t epi, int32_t out_split, float a_scale, float w_scale, float out_scale,
                        const int32_t* row_src, int32_t rows_A, int32_t iters, float* ms_out, void* stream) {
    const int dbg = epi >> 4;            // diagnostic bits (timing only): 16 no in-loop DMA, 32 no barrier, 64 no DMA wait, 128 no epilogue
    epi &= 15;
#ifndef MMEE_DIAG
    if (dbg) return fail(nullptr, "ee_debug_gemm_split: timing variants (wrong results) exist in the diagnostic library only (make diag)");
#endif
    if (!A || !W || !Cout || M < 1 || rows_A < 1 || !mmee::gemm_split_supports(N, K) || epi < 0 || epi > 3 || iters < 1)
        return fail(nullptr, "ee_debug_gemm_split: bad argument (N %% 256, K %% 32)");
    if (epi == EPI_RESID && !resid) return fail(nullptr, "ee_debug_gemm_split: residual epilogue without a residual");
    ee_debug_gemm_routes_args a = plain_split_args(A, W, bias, resid, Cout, M, N, K, epi, a_scale, w_scale, row_src, rows_A, iters);
    a.out_split = out_split; a.out_scale = out_scale;
    a.resid_row_src = row_src; a.rows_resid = rows_A;      // an f32 residual, gathered as A is
    return run_debug_gemm_split("ee_debug_gemm_split", a, dbg, ms_out, reinterpret_cast<hipStream_t>(stream));
}

int ee_debug_gemm_split_resid(const float* A, const float* W, const float* bias, const float* resid, float* Cout, int32_t M, int32_t N,
                              int32_t K, float a_scale, float w_scale, float resid_scale, const int32_t* row_src, int32_t rows_A,
                              const int32_t* resid_row_src, int32_t rows_resid, int32_t route, int32_t iters, float* ms_out, void* stream) {
    const char* who = "ee_debug_gemm_split_resid";
    if (!A || !W || !resid || !Cout || M < 1 || rows_A < 1 || rows_resid < 1 || !mmee::gemm_split_supports(N, K) || iters < 1 || route < 0 ||
        route > 2 || !(a_scale > 0.f) || !(w_scale > 0.f) || resid_scale < 0.f)
        return fail(nullptr, "%s: bad argument (N %% 256, K %% 32, route 0 / 1 / 2)", who);
    if ((!row_src && M > rows_A) || (!resid_row_src && M > rows_resid)) return fail(nullptr, "%s: M rows without a row map need M rows of A / of the residual", who);
    if (row_src) { const int rc = check_row_map(who, "row_src", row_src, M, rows_A); if (rc) return rc; }
    if (resid_row_src) { const int rc = check_row_map(who, "resid_row_src", resid_row_src, M, rows_resid); if (rc) return rc; }
    ee_debug_gemm_routes_args a = plain_split_args(A, W, bias, resid, Cout, M, N, K, EPI_RESID, a_scale, w_scale, row_src, rows_A, iters);
    a.resid_scale = resid_scale; a.resid_row_src = resid_row_src; a.rows_resid = rows_resid; a.route = route;
    a.role_tag = K > N ? 3 : 2;          // the layer's kernel names: FFN down / attention output
    return run_debug_gemm_split(who, a, 0, ms_out, reinterpret_cast<hipStream_t>(stream));
}

int ee_debug_gemm_routes(const ee_debug_gemm_routes_args* args, float* ms_out, void* stream) {
    const char* who = "ee_debug_gemm_routes";
    if (!args) return fail(nullptr, "%s: args must not be NULL", who);
    const ee_debug_gemm_routes_args& a = *args;
    if (!a.A || !a.W || !a.Cout || a.M < 1 || a.rows_A < 1 || !mmee::gemm_split_supports(a.N, a.K) || a.epi < 0 || a.epi > 3 || a.iters < 1 ||
        !(a.a_scale > 0.f) || !(a.w_scale > 0.f) || (a.out_split && !(a.out_scale > 0.f)))
        return fail(nullptr, "%s: bad argument (A, W, Cout not NULL, M, rows_A, iters >= 1, N %% 256, K %% 32, epi 0 .. 3, scales positive)", who);
    if (a.epi == EPI_RESID && (!a.resid || a.rows_resid < 1 || a.resid_scale < 0.f || a.resid_scale != a.resid_scale))
        return fail(nullptr, "%s: the residual epilogue needs resid, rows_resid >= 1 and resid_scale >= 0", who);
    if (a.terms != 1 && a.terms != 3) return fail(nullptr, "%s: terms %d is neither 1 nor 3", who, a.terms);
    if (a.k_splits != 1 && a.k_splits != 2 && a.k_splits != 4 && a.k_splits != 8) return fail(nullptr, "%s: k_splits %d is none of 1, 2, 4, 8", who, a.k_splits);
    if ((a.K / 32) % a.k_splits != 0)
        return fail(nullptr, "%s: k_splits %d does not divide the %d k-stages of K = %d (the kernel would drop the last %d)", who, a.k_splits, a.K / 32, a.K,
                    (a.K / 32) % a.k_splits);
    if (a.k_splits > 1 && (a.epi != EPI_BIAS || a.out_split || a.terms == 1 || a.bias))
        return fail(nullptr, "%s: k_splits %d needs the bias epilogue, an f32 output, three terms and no bias pointer (anything else writes one part)", who,
                    a.k_splits);
    if (a.m_on_device && a.M > a.max_m) return fail(nullptr, "%s: M %d is above max_m %d", who, a.M, a.max_m);
    if (a.scale_cols < 0 || a.scale_cols > a.N || a.scale_cols % 64 != 0)
        return fail(nullptr, "%s: scale_cols %d is not a multiple of 64 in [0, N = %d]", who, a.scale_cols, a.N);
    if (a.route < 0 || a.route > 2 || (a.role_tag != 0 && a.role_tag != 2 && a.role_tag != 3))
        return fail(nullptr, "%s: route %d outside 0 / 1 / 2 or role_tag %d none of 0, 2, 3", who, a.route, a.role_tag);
    if (a.k_splits > 1 && a.split_stride < (size_t)(a.m_on_device ? a.max_m : a.M) * a.N)
        return fail(nullptr, "%s: split_stride %zu is below the %d x %d floats of a part", who, a.split_stride, a.m_on_device ? a.max_m : a.M, a.N);
    const bool resid = a.epi == EPI_RESID;
    if ((!a.row_src && a.M > a.rows_A) || (resid && !a.resid_row_src && a.M > a.rows_resid))
        return fail(nullptr, "%s: M rows without a row map need M rows of A / of the residual", who);
    if (a.row_src) { const int rc = check_row_map(who, "row_src", a.row_src, a.M, a.rows_A); if (rc) return rc; }
    if (resid && a.resid_row_src) { const int rc = check_row_map(who, "resid_row_src", a.resid_row_src, a.M, a.rows_resid); if (rc) return rc; }
    ee_debug_gemm_routes_args b = a;
    if (!resid) { b.resid = nullptr; b.resid_row_src = nullptr; }
    return run_debug_gemm_split(who, b, 0, ms_out, reinterpret_cast<hipStream_t>(stream));
}

// The f32 counterpart: one launch_gemm_f32 on the arguments of a forward (forward_gemm_args) plus the caller's.  lda = K, ldc = ldr = N: no
// launch of a forward uses other strides.
int ee_debug_gemm_f32(const ee_debug_gemm_f32_args* args, void* stream) {
    const char* who = "ee_debug_gemm_f32";
    if (!args) return fail(nullptr, "%s: args must not be NULL", who);
    const ee_debug_gemm_f32_args& a = *args;
    if (!a.A || !a.W || !a.Cout) return fail(nullptr, "%s: A, W and Cout must not be NULL", who);
    if (a.N < 1 || a.K < 1 || a.N % 128 != 0 || a.K % 32 != 0)
        return fail(nullptr, "%s: N %d is not a positive multiple of 128 or K %d not one of 32", who, a.N, a.K);
    if (a.M < 0) return fail(nullptr, "%s: M %d is negative", who, a.M);
    if (a.epi < 0 || a.epi > 3) return fail(nullptr, "%s: epi %d outside 0 .. 3 (bias, GELU, residual, tanh; this hook takes no flag bits)", who, a.epi);
    if (a.staging != 0 && a.staging != 1) return fail(nullptr, "%s: staging %d is neither 0 (LDS-DMA kernel) nor 1 (register-staged kernel)", who, a.staging);
    if (a.epi == EPI_RESID && !a.resid) return fail(nullptr, "%s: the residual epilogue needs resid", who);
    if (a.epi != EPI_RESID && a.resid) return fail(nullptr, "%s: resid is read by the residual epilogue (epi 2) alone, got epi %d", who, a.epi);
    if (a.scale_cols < 0 || a.scale_cols > a.N || a.scale_cols % 128 != 0)
        return fail(nullptr, "%s: scale_cols %d is not a multiple of 128 in [0, N = %d] (the kernel decides per 128-column tile side)", who, a.scale_cols, a.N);
    if (a.m_on_device && a.max_m < 1) return fail(nullptr, "%s: max_m %d is below 1", who, a.max_m);
    if (a.m_on_device && a.M > a.max_m) return fail(nullptr, "%s: M %d is above max_m %d", who, a.M, a.max_m);
    if (a.wgs_per_cu < 0) return fail(nullptr, "%s: wgs_per_cu %d is negative (0: the default)", who, a.wgs_per_cu);
    const bool resid = a.epi == EPI_RESID;
    if (!a.row_src && a.M > a.rows_A) return fail(nullptr, "%s: M %d rows without row_src need M rows of A, rows_A is %d", who, a.M, a.rows_A);
    if (resid && !a.resid_row_src && a.M > a.rows_resid)
        return fail(nullptr, "%s: M %d rows without resid_row_src need M rows of the residual, rows_resid is %d", who, a.M, a.rows_resid);
    const int cus = device_cus(who);
    if (!cus) return 1;
    if (a.row_src) { const int rc = check_row_map(who, "row_src", a.row_src, a.M, a.rows_A); if (rc) return rc; }
    if (resid && a.resid_row_src) { const int rc = check_row_map(who, "resid_row_src", a.resid_row_src, a.M, a.rows_resid); if (rc) return rc; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // 8 XCD-local queue heads x one 64-byte line, then the device word of M; reused by every call (the hook synchronises before it returns)
    static int* words = nullptr;
    if (!words && hipMalloc((void**)&words, 512 + 64) != hipSuccess) { words = nullptr; return fail(nullptr, "%s: hipMalloc failed", who); }
    if (hipMemsetAsync(words, 0, 512 + 64, s) != hipSuccess) return fail(nullptr, "%s: memset failed", who);
    GemmArgs g = forward_gemm_args(nullptr);
    g.A = a.A; g.lda = a.K; g.W = a.W; g.bias = a.bias; g.C = a.Cout; g.ldc = a.N; g.N = a.N; g.K = a.K; g.m_static = a.M;
    g.row_src = a.row_src;
    if (resid) { g.resid = a.resid; g.ldr = a.N; g.resid_row_src = a.resid_row_src; }
    g.scale_cols = a.scale_cols; g.scale = a.scale; g.col_scale = a.col_scale;
    g.use_dma = a.staging == 0 ? 1 : 2;
    g.tile_counter = a.use_queue ? words : nullptr;
    const int M = a.M;                   // (lives until the synchronisation below)
    if (a.m_on_device) {
        if (hipMemcpyAsync(words + 128, &M, sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) return fail(nullptr, kUploadFailed, who);
        g.m_ptr = words + 128;
    }
    set_gemm_wgs_per_cu(a.wgs_per_cu);
    launch_gemm_f32(g, a.epi, AMODE_ROWS, a.m_on_device ? a.max_m : M, cus, s);
    set_gemm_wgs_per_cu(0);
    return finish(who, s, nullptr, nullptr);
}

}  // extern "C"
