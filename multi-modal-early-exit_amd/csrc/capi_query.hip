// What reads the last forward of a handle back (ee_profile*, ee_stream_next, ee_last_stage_counts, ee_last_flops, ee_last_layer_plan, ee_suggest_probe_mask)
// and the one-line setters that arm the next one (ee_set_*).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "capi_internal.h"

using namespace mmee;
using namespace mmee::capi;

namespace {

// kernel roles reported by ee_profile_read; the HIP symbol each role launches is in the second column
const char* const kProfNames[] = {
    "prep|doc_prep_kernel+doc_scan_kernel+row_meta_kernel",
    "embed_text|embed_text_kernel",
    "gemm_patch|patch_split_kernel+gemm_split_kernel<.., 0, false> (f32: gemm_f32_kernel<0,1>)",
    "embed_visual|embed_visual_kernel+pool_finish_kernel",
    "gemm_qkv|gemm_f32_kernel<0,0>",
    "attention|attention_f32_kernel",
    "gemm_attn_out|gemm_f32_kernel<2,0>",
    "layernorm|ln_rows_kernel",
    "gemm_ffn_up|gemm_f32_kernel<1,0>",
    "gemm_ffn_down|gemm_f32_kernel<2,0>",
    "exit_head|gemm_f32_kernel<3,0>+head_out_kernel (use_lte: head_out_lte_kernel)",
    "exit_decide|exit_decide[_patience|_lte][_streak|_either][_audit]_kernel (by criterion / use_lte, exit rule, audited call)",
    "compact|compact_rows_kernel",
    "gather_cls|gather_cls_kernel",
    "cls_probe|attention_idx_kernel+gemm_split_kernel<.., 1>+ln_rows_kernel+gather_cls_kernel (CLS rows of an exit layer, before its decision)",
    // nested roles: each is timed INSIDE the role named in brackets (so a sum over roles must leave them out)
    "pair_index|pair_index_kernel [inside prep]",
    "patch_split|patch_split_kernel [inside gemm_patch]",
    "head_out|head_out_kernel / head_out_lte_kernel [inside exit_head]",
    // (not nested) MMEE_FLAG_STREAM_RESULTS: one launch behind every exit's decide launch
    "emit_leavers|emit_leavers_kernel",
    // (not nested) ee_set_ensemble: one launch between every exit's head and its decide launch
    "exit_ensemble|exit_ensemble_kernel",
    "exit_quota_rank|exit_quota_crit_kernel+exit_quota_rank_kernel",
    // (not nested) ee_set_controller: two launches behind the final exit's decide launch
    "controller|audit_tally_kernel+controller_step_kernel",
    // (not nested) ee_set_deadline: one launch in front of the call and one in front of every exit's decide launch
    "deadline|deadline_begin_kernel+deadline_check_kernel",
};
static_assert(sizeof(kProfNames) / sizeof(kProfNames[0]) == P_COUNT, "one name per profile role");
static_assert(kDeadlineNone == MMEE_DEADLINE_NONE && kDeadlineNone != MMEE_DEADLINE_OFF, "the values include/mmee.h documents");

// Synchronises the stream, then copies the first n StageCounts (of the last forward) to the host.
int read_stage_counts(ee_handle* h, void* stream, int n, std::vector<StageCounts>& sc) {
    HIP_OK(h, hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    sc.resize(n);
    HIP_OK(h, hipMemcpy(sc.data(), h->counts, sizeof(StageCounts) * n, hipMemcpyDeviceToHost));
    return 0;
}

// a device array of the controller's, replaced: the old one leaves the handle's allocations and is freed (the caller has synchronised)
template <typename T>
int ctl_realloc(ee_handle* h, T** p, size_t count) {
    if (*p) {
        auto it = std::find(h->allocs.begin(), h->allocs.end(), static_cast<void*>(*p));
        if (it != h->allocs.end()) h->allocs.erase(it);
        (void)hipFree(*p);
        *p = nullptr;
    }
    return count ? dev_alloc(h, p, count) : 0;
}

}  // namespace

extern "C" {

int ee_profile(ee_handle* h, int32_t enable) {
    if (!h) return 1;
    h->prof_on = enable != 0;
    h->prof_recs.clear();
    h->prof_used = 0;
    return 0;
}

int ee_profile_read(ee_handle* h, int32_t idx, char* name_out, int32_t name_cap, double* total_ms, int32_t* launches) {
    if (!h) return 1;
    if (idx < 0 || idx >= P_COUNT) return 2;
    (void)hipDeviceSynchronize();
    double ms = 0.0;
    int n = 0;
    for (auto& r : h->prof_recs)
        if (r.id == idx) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) { ms += t; ++n; }
        }
    if (name_out && name_cap > 0) {
        strncpy(name_out, kProfNames[idx], name_cap - 1);
        name_out[name_cap - 1] = 0;
    }
    if (total_ms) *total_ms = ms;
    if (launches) *launches = n;
    return 0;
}

int ee_last_stage_counts(ee_handle* h, int32_t* docs_out, int32_t* rows_out, int32_t cap, int32_t* n_stages_out, void* stream) {
    if (!h || !h->rec.last_stages) return fail(h, "ee_last_stage_counts: no forward has run");
    const ForwardRecord& r = h->rec;
    std::vector<StageCounts> sc;
    if (read_stage_counts(h, stream, r.last_stages, sc)) return 1;
    const int err = take_errors(h, true, true);       // every forward enqueued so far has finished: all of their flags are reported here
    if (n_stages_out) *n_stages_out = r.last_stages;
    for (int i = 0; i < r.last_stages && i < cap; ++i) {
        if (docs_out) docs_out[i] = sc[r.exit_stage[i]].n_docs;
        if (rows_out) rows_out[i] = sc[r.exit_stage[i]].n_rows;
    }
    return report_errors(h, err, "a forward since the last check");
}

int ee_last_k_splits(ee_handle* h, int32_t* attn_out, int32_t* ffn_down) {
    if (!h || !h->rec.last_stages) return fail(h, "ee_last_k_splits: no forward has run");
    if (attn_out) *attn_out = h->rec.ks_attn_out;
    if (ffn_down) *ffn_down = h->rec.ks_ffn_down;
    return 0;
}

int ee_stream_next(ee_handle* h, int32_t* exit_index, const int32_t** rows, int32_t* n_rows) {
    if (!h || !exit_index || !rows || !n_rows) return fail(h, "ee_stream_next: null argument");
    if (!h->stream_armed) return fail(h, "ee_stream_next: no forward with MMEE_FLAG_STREAM_RESULTS has run on this handle");
    const int E1 = (int)h->stream_ev.size(), W = h->cfg.num_labels + 3;
    *exit_index = -1; *rows = nullptr; *n_rows = 0;
    if (h->stream_next >= E1) return 0;           // every chunk of the last flagged forward has been delivered
    const int e = h->stream_next;
    HIP_OK(h, hipEventSynchronize(h->stream_ev[e]));
    const int32_t* cum = h->stream_host + (size_t)h->cfg.max_docs * W;
    const int lo = e ? cum[e - 1] : 0, hi = cum[e];
    if (lo < 0 || hi < lo || hi > h->cfg.max_docs)
        return fail(h, "ee_stream_next: exit %d reports documents [%d, %d) of at most %d: the forward did not run to this exit (see ee_last_stage_counts)", e,
                    lo, hi, h->cfg.max_docs);
    *exit_index = e; *rows = h->stream_host + (size_t)lo * W; *n_rows = hi - lo;
    h->stream_next = e + 1;
    return 0;
}

int ee_set_inputs_embeds(ee_handle* h, const float* embeds) {
    if (!h) return 1;
    if (embeds && h->cfg.arch == MMEE_ARCH_BEIT) return fail(h, "ee_set_inputs_embeds: an image-only model has no text embeddings");
    h->next_inputs_embeds = embeds;
    return 0;
}

int ee_set_hidden_states_out(ee_handle* h, float* out) {
    if (!h) return 1;
    h->next_hidden_out = out;
    return 0;
}

int ee_set_head_mask(ee_handle* h, const float* mask) {
    if (!h) return 1;
    h->next_head_mask = mask;
    return 0;
}

int ee_set_attentions_out(ee_handle* h, float* out) {
    if (!h) return 1;
    h->next_attn_out = out;
    return 0;
}

int ee_set_criterion(ee_handle* h, int32_t criterion) {
    if (!h) return 1;
    if (criterion != MMEE_CRIT_MAX_CONFIDENCE && criterion != MMEE_CRIT_ENTROPY && criterion != MMEE_CRIT_PATIENCE && criterion != MMEE_CRIT_MARGIN &&
        criterion != MMEE_CRIT_GATE)
        return fail(h, "ee_set_criterion: unknown criterion %d", criterion);
    if (criterion == MMEE_CRIT_GATE && h->cfg.strategy != MMEE_STRATEGY_GATE)
        return fail(h, "ee_set_criterion: unknown criterion %d on a MMEE_STRATEGY_RAMP handle: MMEE_CRIT_GATE scores the 2-way heads of MMEE_STRATEGY_GATE, "
                       "which this handle does not have", criterion);
    if (criterion == MMEE_CRIT_GATE && h->cfg.use_lte)
        return fail(h, "ee_set_criterion: MMEE_CRIT_GATE on a use_lte handle: learning-to-exit and the gate score are two exit decisions");
    if (criterion == MMEE_CRIT_PATIENCE && h->cfg.use_lte)
        return fail(h, "ee_set_criterion: MMEE_CRIT_PATIENCE on a use_lte handle: learning-to-exit and patience are two exit decisions");
    if (criterion == MMEE_CRIT_PATIENCE && h->rule != MMEE_RULE_PLAIN)
        return fail(h, "ee_set_criterion: MMEE_CRIT_PATIENCE under exit rule %d: PABEE has no threshold event for MMEE_RULE_STREAK / MMEE_RULE_EITHER "
                       "to build on (ee_set_exit_rule(h, MMEE_RULE_PLAIN) first)", h->rule);
    if (criterion == MMEE_CRIT_GATE && h->ens_on)
        return fail(h, "ee_set_criterion: MMEE_CRIT_GATE while an exit ensemble is set: the gate decision does not read the policy row the ensemble "
                       "replaces (not built); clear it first, ee_set_ensemble(h, NULL, NULL)");
    if (criterion == MMEE_CRIT_PATIENCE && h->quota_mode != MMEE_QUOTA_OFF)
        return fail(h, "ee_set_criterion: MMEE_CRIT_PATIENCE while quotas are set: PABEE's decision carries per-document state, no rank is defined for it "
                       "(ee_set_quotas(h, NULL, 0, 0) first)");
    if (criterion == MMEE_CRIT_PATIENCE && h->dl_on)
        return fail(h, "ee_set_criterion: MMEE_CRIT_PATIENCE while a deadline is set: a cut must fire at once, and PABEE's decision carries "
                       "per-document state and no threshold (ee_set_deadline(h, MMEE_DEADLINE_OFF, NULL) first)");
    if (h->ctl_on && criterion != h->cfg.criterion)
        return fail(h, "ee_set_criterion: a controller is set: its path is ordered for the direction of the criterion it was set under, and the "
                       "patience criterion has no threshold to steer (ee_set_controller(h, NULL, ...) first)");
    h->cfg.criterion = criterion;      // read by the decide kernel's arguments of every later ee_forward
    return 0;
}

int ee_set_quotas(ee_handle* h, const int32_t* quotas, int32_t n, int32_t mode) {
    if (!h) return 1;
    const ee_config& c = h->cfg;
    const int E = c.n_embedding_exits + c.n_encoder_exits;
    const int32_t want = quotas ? mode : MMEE_QUOTA_OFF;
    if (quotas) {
        if (mode != MMEE_QUOTA_EXACT && mode != MMEE_QUOTA_AT_LEAST)
            return fail(h, "ee_set_quotas: unknown mode %d (MMEE_QUOTA_EXACT = %d, MMEE_QUOTA_AT_LEAST = %d)", mode, MMEE_QUOTA_EXACT, MMEE_QUOTA_AT_LEAST);
        if (n != E) return fail(h, "ee_set_quotas: %d entries, the handle has E = %d exits below the final one (one quota per exit)", n, E);
        for (int e = 0; e < n; ++e)
            if (quotas[e] < 0) return fail(h, "ee_set_quotas: quotas[%d]=%d, a quota is a number of documents (>= 0)", e, quotas[e]);
        if (c.criterion == MMEE_CRIT_PATIENCE)
            return fail(h, "ee_set_quotas: a handle under MMEE_CRIT_PATIENCE: PABEE's decision carries per-document state, no rank is defined for it (not built)");
        if (h->rule != MMEE_RULE_PLAIN)
            return fail(h, "ee_set_quotas: a handle under MMEE_RULE_STREAK / MMEE_RULE_EITHER (rule %d): their decisions carry per-document state, no rank "
                           "is defined for them (not built; ee_set_exit_rule(h, MMEE_RULE_PLAIN) first)", h->rule);
        if (c.use_lte)
            return fail(h, "ee_set_quotas: a use_lte handle: the learning-to-exit decision reads another score, no rank is defined for it (not built)");
        if (h->dl_on)
            return fail(h, "ee_set_quotas: a deadline is set: a quota releases a fixed number of documents, a cut releases everybody "
                           "(not built; ee_set_deadline(h, MMEE_DEADLINE_OFF, NULL) first)");
        if (h->audit_cut)
            return fail(h, "ee_set_quotas: an audit is set: a rank would count the audited documents that stay as shadows, and n_{e+1} would no longer "
                           "be n_e - q_e (not built; ee_set_audit(h, 0, 0, 0) first)");
    }
    if (want != h->quota_mode)
        for (const auto& g : h->graphs)
            if (g.exec)
                return fail(h, "ee_set_quotas: the handle holds captured graphs and the call would switch the quota mode from %d to %d: a graph's launch "
                               "list is the one of its capture (ee_graph_destroy them first; new quota values under the same mode are fine)",
                            h->quota_mode, want);
    if (!quotas) {
        h->quota_mode = MMEE_QUOTA_OFF;
        h->quotas.clear();
        return 0;
    }
    if (!h->quota_crit) {
        double* qc = nullptr;
        int* qr = nullptr;
        if (dev_alloc(h, &qc, (size_t)c.max_docs) || dev_alloc(h, &qr, (size_t)c.max_docs)) return 1;
        h->quota_crit = qc; h->quota_rank = qr;
    }
    h->quotas.assign(quotas, quotas + n);      // eager forwards pass q_e by value; ee_graph_launch writes them to the graph's device vector
    h->quota_mode = mode;
    return 0;
}

int ee_has_quotas(const ee_handle* h) { return h ? h->quota_mode : 0; }

int ee_set_audit(ee_handle* h, uint64_t cut, uint32_t seed, int32_t slot_base) {
    if (!h) return 1;
    if (cut > (1ull << 32)) return fail(h, "ee_set_audit: cut %llu is above 2^32 (cut = floor(fraction 2^32 + 0.5), fraction in [0, 1])", (unsigned long long)cut);
    if (slot_base < 0) return fail(h, "ee_set_audit: slot_base %d is negative (it is the index of the call's first document in the caller's batch)", slot_base);
    if (cut && h->quota_mode != MMEE_QUOTA_OFF)
        return fail(h, "ee_set_audit: quotas are set: a rank would count the audited documents that stay as shadows, and n_{e+1} would no longer be "
                       "n_e - q_e (not built; ee_set_quotas(h, NULL, 0, 0) first)");
    if (cut && h->dl_on)
        return fail(h, "ee_set_audit: a deadline is set: the audit's shadows would run on past the cut "
                       "(not built; ee_set_deadline(h, MMEE_DEADLINE_OFF, NULL) first)");
    if (cut)                                       // (a capture is refused while an audit is set, so held graphs mean the audit is off)
        for (const auto& g : h->graphs)
            if (g.exec)
                return fail(h, "ee_set_audit: the handle holds captured graphs: a graph's launch list is the one of its capture, and audited calls "
                               "are eager (ee_graph_destroy them first)");
    if (!cut && h->ctl_on)
        return fail(h, "ee_set_audit: a controller is set: the audit is the sample its loss is counted on (ee_set_controller(h, NULL, ...) first)");
    if (cut && !h->audit_delivered) {
        int* d = nullptr;
        if (dev_alloc(h, &d, (size_t)h->cfg.max_docs)) return 1;
        h->audit_delivered = d;
    }
    h->audit_cut = cut; h->audit_seed = seed; h->audit_slot_base = slot_base;      // passed by value to the decide launches of every later ee_forward
    return 0;
}

int ee_has_audit(const ee_handle* h) { return h && h->audit_cut ? 1 : 0; }

int ee_set_controller(ee_handle* h, const double* path, int32_t V, double alpha, double gamma, double p0, uint32_t seed, int32_t log_cap) {
    if (!h) return 1;
    if (!path) { h->ctl_on = false; return 0; }                       // the arrays stay until the next controller or ee_destroy
    const ee_config& c = h->cfg;
    const int E1 = c.n_embedding_exits + c.n_encoder_exits + 1;
    for (const auto& g : h->graphs)
        if (g.exec)
            return fail(h, "ee_set_controller: the handle holds captured graphs: a graph's launch list is the one of its capture, and controlled calls "
                           "are eager (not built; ee_graph_destroy them first)");
    if (h->dl_on)
        return fail(h, "ee_set_controller: a deadline is set: the controller's audit shadows would run on past the cut "
                       "(not built; ee_set_deadline(h, MMEE_DEADLINE_OFF, NULL) first)");
    if (!h->audit_cut)
        return fail(h, "ee_set_controller: no audit is set: the controller's loss is counted on the audited sample (ee_set_audit with cut > 0 first)");
    if (c.criterion == MMEE_CRIT_PATIENCE)
        return fail(h, "ee_set_controller: a handle under MMEE_CRIT_PATIENCE: PABEE has no threshold for the controller to steer (not built)");
    if (h->rule != MMEE_RULE_PLAIN)
        return fail(h, "ee_set_controller: a handle under MMEE_RULE_STREAK / MMEE_RULE_EITHER (rule %d): the controller steers the thresholds of the "
                       "plain rule (not built; ee_set_exit_rule(h, MMEE_RULE_PLAIN) first)", h->rule);
    if (c.use_lte) return fail(h, "ee_set_controller: a use_lte handle: the learning-to-exit decision reads another score (not built)");
    // (quotas need no refusal of their own: a controller needs an audit, and ee_set_audit / ee_set_quotas refuse each other)
    if (E1 < 2 || E1 > kCtlMaxE1) return fail(h, "ee_set_controller: the handle has E1 = %d exits, need 2 <= E1 <= %d", E1, kCtlMaxE1);
    if (V < 2 || V > (1 << 20)) return fail(h, "ee_set_controller: V = %d vectors, a path needs 2 <= V <= 2^20", V);
    if (!(alpha > 0.0 && alpha < 1.0)) return fail(h, "ee_set_controller: alpha = %g, the risk level must lie in (0, 1)", alpha);
    if (!(gamma > 0.0) || !std::isfinite(gamma)) return fail(h, "ee_set_controller: gamma = %g, the step must be positive and finite", gamma);
    if (!(p0 >= 0.0 && p0 <= (double)(V - 1))) return fail(h, "ee_set_controller: p0 = %g outside [0, V - 1 = %d]", p0, V - 1);
    if (log_cap < 0 || log_cap > (1 << 24)) return fail(h, "ee_set_controller: log_cap = %d outside [0, 2^24]", log_cap);
    for (size_t i = 0; i < (size_t)V * E1; ++i)
        if (!std::isfinite(path[i]))
            return fail(h, "ee_set_controller: path[%zu][%zu] = %g is not finite", i / E1, i % E1, path[i]);
    HIP_OK(h, hipDeviceSynchronize());                                // an earlier forward may still read the arrays that are replaced
    const int W = controller_log_words(E1);
    if (ctl_realloc(h, &h->ctl_path, (size_t)V * E1) || ctl_realloc(h, &h->ctl_log, (size_t)log_cap * W)) { h->ctl_on = false; return 1; }
    if (!h->ctl_thr_dev &&
        (dev_alloc(h, &h->ctl_thr_dev, (size_t)E1) || dev_alloc(h, &h->ctl_state, (size_t)kCtlStateWords) ||
         dev_alloc(h, &h->ctl_tally, (size_t)controller_tally_words(E1)))) { h->ctl_on = false; return 1; }
    std::vector<double> thr(E1);
    controller_thresholds(path, V, E1, p0, crit_sign(c.criterion), thr.data());      // the first call's, by the function the step kernel runs
    long long state[kCtlStateWords] = {0, 0, 0, 0, 0};
    memcpy(&state[0], &p0, sizeof(double));
    HIP_OK(h, hipMemcpy(h->ctl_path, path, sizeof(double) * (size_t)V * E1, hipMemcpyHostToDevice));
    HIP_OK(h, hipMemcpy(h->ctl_thr_dev, thr.data(), sizeof(double) * E1, hipMemcpyHostToDevice));
    HIP_OK(h, hipMemcpy(h->ctl_state, state, sizeof(state), hipMemcpyHostToDevice));
    h->ctl_V = V; h->ctl_alpha = alpha; h->ctl_gamma = gamma; h->ctl_seed = seed; h->ctl_log_cap = log_cap; h->ctl_calls = 0;
    h->ctl_on = true;
    return 0;
}

int ee_has_controller(const ee_handle* h) { return h && h->ctl_on ? 1 : 0; }

int ee_controller_state(ee_handle* h, double* p, int64_t* calls, int64_t* steps, int64_t* sampled_sum, int64_t* disagree_sum, double* thr_out,
                        void* stream) {
    if (!h) return 1;
    if (!h->ctl_on) return fail(h, "ee_controller_state: no controller is set (ee_set_controller)");
    const int E1 = h->cfg.n_embedding_exits + h->cfg.n_encoder_exits + 1;
    HIP_OK(h, hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    long long state[kCtlStateWords];
    HIP_OK(h, hipMemcpy(state, h->ctl_state, sizeof(state), hipMemcpyDeviceToHost));
    if (thr_out) HIP_OK(h, hipMemcpy(thr_out, h->ctl_thr_dev, sizeof(double) * E1, hipMemcpyDeviceToHost));
    if (p) memcpy(p, &state[0], sizeof(double));
    if (calls) *calls = state[1];
    if (steps) *steps = state[2];
    if (sampled_sum) *sampled_sum = state[3];
    if (disagree_sum) *disagree_sum = state[4];
    return 0;
}

int ee_controller_log(ee_handle* h, int64_t* rows_out, int32_t cap, int32_t* n, void* stream) {
    if (!h || !n) return fail(h, "ee_controller_log: null argument");
    if (!h->ctl_on) return fail(h, "ee_controller_log: no controller is set (ee_set_controller)");
    if (cap < 0 || (cap > 0 && !rows_out)) return fail(h, "ee_controller_log: cap = %d rows without a buffer", cap);
    const int E1 = h->cfg.n_embedding_exits + h->cfg.n_encoder_exits + 1, W = controller_log_words(E1);
    HIP_OK(h, hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    long long calls = 0;
    HIP_OK(h, hipMemcpy(&calls, h->ctl_state + 1, sizeof(calls), hipMemcpyDeviceToHost));
    const long long held = std::min<long long>(calls, h->ctl_log_cap);
    const int take = (int)std::min<long long>(held, cap);
    *n = (int32_t)held;                                               // the rows the ring holds; the last `take` of them are copied, oldest first
    std::vector<long long> ring((size_t)held * W);                    // one copy of the rows the ring holds, put in order on the host
    if (held) HIP_OK(h, hipMemcpy(ring.data(), h->ctl_log, sizeof(long long) * ring.size(), hipMemcpyDeviceToHost));
    for (int j = 0; j < take; ++j) {
        const long long call = calls - take + j;
        memcpy(rows_out + (size_t)j * W, ring.data() + (size_t)(call % h->ctl_log_cap) * W, sizeof(long long) * W);
    }
    return 0;
}

// the deadline's device arrays and its pinned request word, at the first ee_set_deadline / ee_set_deadline_log of the handle
static int deadline_alloc(ee_handle* h, int E1) {
    if (h->dl_thr) return 0;
    int dev = 0, khz = 0;
    HIP_OK(h, hipGetDevice(&dev));
    HIP_OK(h, hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev));
    if (khz <= 0)
        return fail(h, "ee_set_deadline: the runtime reports a wall-clock rate of %d kHz: the device clock cannot be turned into ns", khz);
    uint64_t* word = nullptr;
    HIP_OK(h, hipHostMalloc((void**)&word, sizeof(uint64_t), hipHostMallocMapped));
    *word = 0;
    void* wdev = nullptr;
    if (hipHostGetDevicePointer(&wdev, word, 0) != hipSuccess) { (void)hipHostFree(word); return fail(h, "ee_set_deadline: hipHostGetDevicePointer failed"); }
    double* thr = nullptr;
    long long* st = nullptr;
    if (dev_alloc(h, &thr, (size_t)E1) || dev_alloc(h, &st, (size_t)kDlStateWords)) { (void)hipHostFree(word); return 1; }
    h->dl_khz = (uint32_t)khz; h->dl_word = word; h->dl_word_dev = reinterpret_cast<const unsigned long long*>(wdev);
    h->dl_thr = thr; h->dl_state = st;
    return 0;
}

// what keeps a handle from carrying a deadline (the definition's list): 0, or the refusal
static int deadline_refusal(ee_handle* h) {
    const ee_config& c = h->cfg;
    const int E1 = c.n_embedding_exits + c.n_encoder_exits + 1;
    if (E1 > kCtlMaxE1) return fail(h, "ee_set_deadline: the handle has E1 = %d exits, a deadline takes E1 <= %d", E1, kCtlMaxE1);
    if (c.criterion == MMEE_CRIT_PATIENCE)
        return fail(h, "ee_set_deadline: a handle under MMEE_CRIT_PATIENCE: a cut must fire at once, and PABEE's decision carries per-document state "
                       "and no threshold (not built)");
    if (h->rule != MMEE_RULE_PLAIN)
        return fail(h, "ee_set_deadline: a handle under MMEE_RULE_STREAK / MMEE_RULE_EITHER (rule %d): a cut must fire at once, and their decisions "
                       "carry per-document state (not built; ee_set_exit_rule(h, MMEE_RULE_PLAIN) first)", h->rule);
    if (c.use_lte) return fail(h, "ee_set_deadline: a use_lte handle: the learning-to-exit decision reads another score than the one a cut opens (not built)");
    if (h->quota_mode != MMEE_QUOTA_OFF)
        return fail(h, "ee_set_deadline: quotas are set: a quota releases a fixed number of documents, a cut releases everybody "
                       "(not built; ee_set_quotas(h, NULL, 0, 0) first)");
    if (h->ctl_on)                                                    // before the audit's refusal: a controller implies an audit
        return fail(h, "ee_set_deadline: a controller is set: its audit shadows would run on past the cut "
                       "(not built; ee_set_controller(h, NULL, ...) first)");
    if (h->audit_cut)
        return fail(h, "ee_set_deadline: an audit is set: its shadows would run on past the cut (not built; ee_set_audit(h, 0, 0, 0) first)");
    for (const auto& g : h->graphs)
        if (g.exec)
            return fail(h, "ee_set_deadline: the handle holds captured graphs: a graph's launch list is the one of its capture, and deadline calls "
                           "are eager (not built; ee_graph_destroy them first)");
    return 0;
}

int ee_set_deadline_log(ee_handle* h, int32_t log_cap) {
    if (!h) return 1;
    const int E1 = h->cfg.n_embedding_exits + h->cfg.n_encoder_exits + 1;
    if (log_cap < 0 || log_cap > (1 << 24)) return fail(h, "ee_set_deadline_log: log_cap = %d outside [0, 2^24]", log_cap);
    if (!h->dl_on && deadline_refusal(h)) return 1;                   // a handle that cannot carry a deadline gets no arrays either
    HIP_OK(h, hipDeviceSynchronize());                                // an earlier forward may still write the ring that is replaced
    if (deadline_alloc(h, E1)) return 1;
    if (log_cap != h->dl_log_cap || !h->dl_log) {
        h->dl_log_cap = 0;
        if (ctl_realloc(h, &h->dl_log, (size_t)log_cap * deadline_log_words(E1))) return 1;
        h->dl_log_cap = log_cap;
    }
    h->dl_log_first = __atomic_load_n(&h->dl_calls, __ATOMIC_RELAXED);
    return 0;
}

int ee_set_deadline(ee_handle* h, uint64_t budget_ns, const uint64_t* eta_ns) {
    if (!h) return 1;
    if (budget_ns == MMEE_DEADLINE_OFF) { h->dl_on = false; return 0; }      // the arrays and the log stay until ee_destroy
    const int E1 = h->cfg.n_embedding_exits + h->cfg.n_encoder_exits + 1;
    if (deadline_refusal(h)) return 1;
    if (!h->dl_thr && ee_set_deadline_log(h, MMEE_DEADLINE_LOG_DEFAULT)) return 1;
    // budget and eta are kernel ARGUMENTS of the launches of later calls: nothing in flight reads them, nothing to wait for
    h->dl_eta.assign((size_t)E1, 0);
    if (eta_ns) h->dl_eta.assign(eta_ns, eta_ns + E1);
    h->dl_budget = budget_ns;
    h->dl_on = true;
    return 0;
}

int ee_has_deadline(const ee_handle* h) { return h && h->dl_on ? 1 : 0; }

int ee_request_cut(ee_handle* h) {
    if (!h || !h->dl_word) return 1;                                  // no deadline was ever set: there is no call to cut (no message: any thread)
    // a monotone maximum: of two requesters the later call number stays, whichever of them stores last
    const uint64_t want = __atomic_load_n(&h->dl_calls, __ATOMIC_RELAXED);
    uint64_t cur = __atomic_load_n(h->dl_word, __ATOMIC_RELAXED);
    while (cur < want && !__atomic_compare_exchange_n(h->dl_word, &cur, want, false, __ATOMIC_RELEASE, __ATOMIC_RELAXED)) {}
    return 0;
}

int ee_deadline_log(ee_handle* h, int64_t* rows_out, int32_t cap, int32_t* n, void* stream) {
    if (!h || !n) return fail(h, "ee_deadline_log: null argument");
    if (!h->dl_thr) return fail(h, "ee_deadline_log: no deadline was set on this handle (ee_set_deadline)");
    if (cap < 0 || (cap > 0 && !rows_out)) return fail(h, "ee_deadline_log: cap = %d rows without a buffer", cap);
    const int E1 = h->cfg.n_embedding_exits + h->cfg.n_encoder_exits + 1, W = deadline_log_words(E1);
    HIP_OK(h, hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    const uint64_t calls = __atomic_load_n(&h->dl_calls, __ATOMIC_RELAXED);
    const long long held = std::min<long long>((long long)(calls - h->dl_log_first), h->dl_log_cap);
    const int take = (int)std::min<long long>(held, cap);
    *n = (int32_t)held;                                               // the rows the ring holds; the last `take` of them are copied, oldest first
    if (!take) return 0;
    std::vector<long long> ring((size_t)h->dl_log_cap * W);
    HIP_OK(h, hipMemcpy(ring.data(), h->dl_log, sizeof(long long) * ring.size(), hipMemcpyDeviceToHost));
    for (int j = 0; j < take; ++j) {
        const uint64_t call = calls - (uint64_t)take + (uint64_t)j + 1;          // 1-based: row (call - 1) % log_cap
        memcpy(rows_out + (size_t)j * W, ring.data() + (size_t)((call - 1) % (uint64_t)h->dl_log_cap) * W, sizeof(long long) * W);
    }
    return 0;
}

int ee_audit_selected(uint64_t cut, uint32_t seed, int32_t slot) { return audit_selected(cut, seed, slot) ? 1 : 0; }

int ee_set_ensemble(ee_handle* h, const double* w, const double* b) {
    if (!h) return 1;
    const ee_config& c = h->cfg;
    const int E1 = c.n_embedding_exits + c.n_encoder_exits + 1, K = c.num_labels;
    const bool on = w != nullptr;
    if (!on && b) return fail(h, "ee_set_ensemble: b without w (w == NULL clears the ensemble)");
    if (on) {
        for (int m = 0; m < E1; ++m)
            for (int j = 0; j < E1; ++j) {
                const double v = w[(size_t)m * E1 + j];
                if (!std::isfinite(v)) return fail(h, "ee_set_ensemble: w[%d][%d] is not finite", m, j);
                if (j > m && v != 0.0)
                    return fail(h, "ee_set_ensemble: w[%d][%d] = %g above the diagonal: exit %d has not run when exit %d decides (w is lower triangular)", m, j,
                                v, j, m);
            }
        for (int i = 0; b && i < E1 * K; ++i)
            if (!std::isfinite(b[i])) return fail(h, "ee_set_ensemble: b[%d][%d] is not finite", i / K, i % K);
        if (c.criterion == MMEE_CRIT_GATE)
            return fail(h, "ee_set_ensemble: a handle under MMEE_CRIT_GATE: the gate decision does not read the policy row the ensemble replaces, only "
                           "what leaves would change (not built)");
        if (c.use_lte)
            return fail(h, "ee_set_ensemble: a use_lte handle: the learning-to-exit decision does not read the policy row the ensemble replaces, only "
                           "what leaves would change (not built)");
    }
    if (on != h->ens_on)
        for (const auto& g : h->graphs)
            if (g.exec)
                return fail(h, "ee_set_ensemble: the handle holds captured graphs and the call would switch the ensemble %s: a graph's launch list is the "
                               "one of its capture (ee_graph_destroy them first)", on ? "on" : "off");
    if (!on) {
        h->ens_on = false;
        return 0;
    }
    HIP_OK(h, hipDeviceSynchronize());      // a forward in flight (or a replay) still reads the buffers
    if (!h->ens_state) {
        double *ew = nullptr, *eb = nullptr, *es = nullptr, *eo = nullptr;
        float* el = nullptr;
        if (dev_alloc(h, &ew, (size_t)E1 * E1) || dev_alloc(h, &eb, (size_t)E1 * K) || dev_alloc(h, &eo, (size_t)E1) ||
            dev_alloc(h, &el, (size_t)c.max_docs * K) || dev_alloc(h, &es, (size_t)E1 * c.max_docs * K))
            return 1;
        const std::vector<double> ones((size_t)E1, 1.0);
        HIP_OK(h, hipMemcpy(eo, ones.data(), sizeof(double) * E1, hipMemcpyHostToDevice));
        h->ens_w = ew; h->ens_b = eb; h->ens_ones = eo; h->ens_logits = el; h->ens_state = es;
    }
    const std::vector<double> zeros((size_t)E1 * K, 0.0);
    HIP_OK(h, hipMemcpy(h->ens_w, w, sizeof(double) * E1 * E1, hipMemcpyHostToDevice));
    HIP_OK(h, hipMemcpy(h->ens_b, b ? b : zeros.data(), sizeof(double) * E1 * K, hipMemcpyHostToDevice));
    h->ens_on = true;
    return 0;
}

int ee_has_ensemble(const ee_handle* h) { return h && h->ens_on ? 1 : 0; }

int ee_set_exit_rule(ee_handle* h, int32_t rule) {
    if (!h) return 1;
    if (rule != MMEE_RULE_PLAIN && rule != MMEE_RULE_STREAK && rule != MMEE_RULE_EITHER) return fail(h, "ee_set_exit_rule: unknown rule %d", rule);
    if (rule != MMEE_RULE_PLAIN && h->cfg.criterion == MMEE_CRIT_PATIENCE)
        return fail(h, "ee_set_exit_rule: rule %d under MMEE_CRIT_PATIENCE: PABEE has no threshold event for MMEE_RULE_STREAK / MMEE_RULE_EITHER to build on",
                    rule);
    if (rule != MMEE_RULE_PLAIN && h->quota_mode != MMEE_QUOTA_OFF)
        return fail(h, "ee_set_exit_rule: rule %d while quotas are set: MMEE_RULE_STREAK / MMEE_RULE_EITHER carry per-document state, no rank is defined "
                       "for them (ee_set_quotas(h, NULL, 0, 0) first)", rule);
    if (rule != MMEE_RULE_PLAIN && h->dl_on)
        return fail(h, "ee_set_exit_rule: rule %d while a deadline is set: a cut must fire at once, and MMEE_RULE_STREAK / MMEE_RULE_EITHER carry "
                       "per-document state (ee_set_deadline(h, MMEE_DEADLINE_OFF, NULL) first)", rule);
    if (rule != MMEE_RULE_PLAIN && h->ctl_on)
        return fail(h, "ee_set_exit_rule: rule %d while a controller is set: the controller steers the thresholds of the plain rule, and its replay "
                       "(ee_rolling_control) knows no other (ee_set_controller(h, NULL, ...) first)", rule);
    h->rule = rule;                    // picks the decide kernel of every later ee_forward / ee_graph_capture
    return 0;
}

int ee_set_patience(ee_handle* h, int32_t t) {
    if (!h) return 1;
    if (t < 1) return fail(h, "ee_set_patience: t=%d, the patience must be >= 1", t);
    h->patience = t;                   // eager forwards pass it by value; ee_graph_launch writes it to the graph's device vector
    h->patience_vec.clear();           // the broadcast replaces a per-exit vector
    return 0;
}

int ee_set_patience_vector(ee_handle* h, const int32_t* t, int32_t n) {
    if (!h) return 1;
    const int E1 = h->cfg.n_embedding_exits + h->cfg.n_encoder_exits + 1;
    if (!t || n != E1) return fail(h, "ee_set_patience_vector: %d entries, the handle has E + 1 = %d exits (one entry per exit, the final one ignored)", n, E1);
    for (int e = 0; e < n; ++e)
        if (t[e] < 1) return fail(h, "ee_set_patience_vector: t[%d]=%d, every patience must be >= 1", e, t[e]);
    h->patience_vec.assign(t, t + n);
    return 0;
}

int ee_set_probe_mask(ee_handle* h, int32_t enabled, uint64_t mask) {
    if (!h) return 1;
    h->mask_on = enabled != 0;
    h->probe_mask = mask;
    return 0;
}

// The cost model that used to pick the schedule inside ee_forward from "whichever earlier forward had finished" (rounds 2-4), as an explicit,
// deterministic query: which exit layers are worth probing first, judged from the stage populations of the LAST forward on this handle.  A
// probe pays when the rows it saves (attention, attention-out, FFN -- and under MMEE_FLAG_XPROBE the Q | K | V projection -- of the documents
// that leave) cost more than the probe itself (a pass over every K | V row, or every LayerNorm row in X space, for the CLS queries + three
// latency-bound GEMMs on one row per document).  Rates as measured on MI355X.
int ee_suggest_probe_mask(ee_handle* h, uint32_t flags, uint64_t* mask_out, void* stream) {
    if (!h || !mask_out) return fail(h, "ee_suggest_probe_mask: null argument");
    const ForwardRecord& r = h->rec;
    if (!r.last_stages) return fail(h, "ee_suggest_probe_mask: no forward has run");
    if (r.last_flags & MMEE_FLAG_NO_EXIT) return fail(h, "ee_suggest_probe_mask: the last forward was a dump (nobody left): run a thresholded forward first");
    std::vector<StageCounts> sc;
    if (read_stage_counts(h, stream, r.last_stages + 1, sc)) return 1;
    const ee_config& c = h->cfg;
    const bool beit = c.arch == MMEE_ARCH_BEIT;
    const double H = c.hidden_size, I = c.intermediate_size;
    const int L = c.num_hidden_layers;
    uint64_t mask = 0;
    bool xs = false;
    if (h->split && !beit && (flags & MMEE_FLAG_XPROBE) && h->Qc && h->pair_idx && c.rel_pos_bins <= 64 && c.rel_2d_pos_bins <= 64) {
        mmee::XProbeArgs chk{};
        chk.H = c.hidden_size; chk.heads = c.num_attention_heads; chk.bins1 = c.rel_pos_bins; chk.bins2 = c.rel_2d_pos_bins; chk.pair_idx = h->pair_idx;
        const int G = c.input_size / c.patch_size;
        xs = mmee::xprobe_supports(chk, r.last_T + G * G + 1);
    }
    for (int k = 0; k < c.n_encoder_exits && h->split; ++k) {
        const int l = c.encoder_exit_layers[k] - 1;
        if (l == L - 1) continue;                     // the last layer: always the probe alone (LayoutLMv3) / always whole (BEiT mean pooling)
        const int st = c.n_embedding_exits + k;      // stage whose documents reach this decision
        if (st + 1 > r.last_stages) break;
        const double rows = sc[st].n_rows, leave = (double)sc[st].n_rows - (double)sc[st + 1].n_rows;
        if (rows <= 0) { mask |= 1ull << l; continue; }
        const double len = (double)sc[st].sum_len_sq / rows;      // mean keys per query
        const double t_row = 2.0 * (H * H + 2.0 * H * I + (xs ? 3.0 * H * H : 0.0)) / 380e12 + 4.0 * len * H / 200e12;
        const double cost = ((2.0 * H + I) / 32.0) * 0.9e-6 + (xs ? 180e-6 + rows * 4.0 * H / 4.5e12 : 100e-6 + rows * 8.0 * H / 3.6e12);
        if (leave * t_row > 1.1 * cost) mask |= 1ull << l;
    }
    *mask_out = mask;
    return 0;
}

int ee_last_flops(ee_handle* h, double* gemm_flops, double* attn_flops, void* stream) {
    if (!h || !h->rec.last_stages) return fail(h, "ee_last_flops: no forward has run");
    const ForwardRecord& r = h->rec;
    std::vector<StageCounts> sc;
    if (read_stage_counts(h, stream, r.last_stages, sc)) return 1;
    const ee_config& c = h->cfg;
    const double H = c.hidden_size, I = c.intermediate_size;
    const int G = c.input_size / c.patch_size;
    double gf = 2.0 * r.last_B * G * G * (double)(c.num_channels * c.patch_size * c.patch_size) * H, af = 0.0;
    for (int l = 0; l < c.num_hidden_layers; ++l) {      // the CLS probes are not in here: ee_last_layer_plan reports them
        if (r.layer_qkv_stage[l] >= 0) gf += 2.0 * sc[r.layer_qkv_stage[l]].n_rows * 3.0 * H * H;
        if (r.layer_stage[l] >= 0) {
            const StageCounts& s = sc[r.layer_stage[l]];
            gf += 2.0 * s.n_rows * (H * H + 2.0 * H * I);
            af += 4.0 * (double)s.sum_len_sq * H;
        }
    }
    const int E = r.last_stages - 1;
    const double ko = c.strategy == MMEE_STRATEGY_RAMP ? c.num_labels : 2;
    for (int e = 0; e <= E; ++e) {
        const double n = sc[r.exit_stage[e]].n_docs;
        const bool fin = e == E;
        const double dense = (fin || c.exit_head_num_layers == 2) ? 2.0 * H * H : 0.0;
        const bool gate = !fin && c.strategy == MMEE_STRATEGY_GATE;
        if (!gate || r.last_gate_heads) gf += n * (dense + 2.0 * H * (fin ? c.num_labels : ko));
        if (gate) gf += n * (2.0 * H * H + 2.0 * H * c.num_labels);
    }
    if (gemm_flops) *gemm_flops = gf;
    if (attn_flops) *attn_flops = af;
    return 0;
}

int ee_last_layer_plan(ee_handle* h, int32_t* rows_qkv, int32_t* rows_main, int32_t* docs_probe, int32_t cap, double* probe_flops, void* stream) {
    if (!h || !h->rec.last_stages) return fail(h, "ee_last_layer_plan: no forward has run");
    const ForwardRecord& r = h->rec;
    std::vector<StageCounts> sc;
    if (read_stage_counts(h, stream, r.last_stages, sc)) return 1;
    const ee_config& c = h->cfg;
    const double H = c.hidden_size, I = c.intermediate_size;
    double pf = 0.0;
    for (int l = 0; l < c.num_hidden_layers; ++l) {
        const int q = r.layer_qkv_stage[l], m = r.layer_stage[l], p = r.layer_probe_stage[l];
        if (l < cap) {
            if (rows_qkv) rows_qkv[l] = q >= 0 ? sc[q].n_rows : 0;
            if (rows_main) rows_main[l] = m >= 0 ? sc[m].n_rows : 0;
            if (docs_probe) docs_probe[l] = p >= 0 ? sc[p].n_docs : 0;
        }
        // probe: 32 queries x every key of the document (QK^T and PV), then attention-out + FFN on one row per document
        if (p >= 0) {
            if (r.layer_xprobe[l])      // X space: q, u, v projections of one row per document + two passes of heads x H per row
                pf += 6.0 * sc[p].n_docs * H * H + 4.0 * (double)sc[p].n_rows * c.num_attention_heads * H + 2.0 * sc[p].n_docs * (H * H + 2.0 * H * I);
            else pf += 4.0 * 32.0 * sc[p].n_rows * H + 2.0 * sc[p].n_docs * (H * H + 2.0 * H * I);
        }
    }
    if (probe_flops) *probe_flops = pf;
    return 0;
}

}  // extern "C"
