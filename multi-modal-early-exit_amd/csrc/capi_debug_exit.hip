// ee_debug_head_out, ee_debug_exit_ensemble, ee_debug_exit_decide, ee_debug_exit_quota, ee_debug_exit_audit, ee_debug_rows_out: the exit stage of exit_stage.hip alone,
// and ee_debug_audit_tally, ee_debug_controller_step: the controller's two launches (controller.hip) alone, and ee_debug_deadline_check: the
// deadline's check launch (deadline.hip) with an injected clock, on caller-provided
// device buffers; no handle.  Each entry point makes the calls of the path's own launchers that capi_forward.hip makes (launch_head_out;
// launch_exit_ensemble; launch_decide -- under a quota launch_exit_quota_crit, launch_exit_quota_rank and launch_decide_quota -- and, behind it,
// launch_compact_rows as compact() does; launch_gather_cls / launch_rows_to_padded) and synchronises.  No kernel is defined or
// instantiated here; what the launchers cannot take is refused, not launched, and so is every row, document or offset outside the caller's
// buffers.  The stage arrays and the per-document state are the caller's, so a test chains exits: the n_* outputs of one call are the stage
// of the next.  tests/test_gpu_exit_stage.py drives them against tests/exit_stage_ref.py.
#include "capi_debug.h"

using namespace mmee;
using namespace mmee::capi;

namespace {

// a row map of the caller's on a host copy, every entry inside [0, rows): 0, or the refusal
int check_row_map(const char* who, const char* name, const int* map, int n, int rows) {
    std::vector<int> h;
    if (!to_host(h, map, (size_t)n)) return fail(nullptr, "%s: copy of %s failed", who, name);
    for (int i = 0; i < n; ++i)
        if (h[i] < 0 || h[i] >= rows) return fail(nullptr, "%s: %s[%d] = %d outside [0, %d rows)", who, name, i, h[i], rows);
    return 0;
}

// the document count of a launch from its device word: 0, or the refusal
int read_n_docs(const char* who, const int* n_docs, int max_docs, int* n) {
    if (hipMemcpy(n, n_docs, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail(nullptr, "%s: copy of n_docs failed", who);
    if (*n < 0 || *n > max_docs) return fail(nullptr, "%s: n_docs = %d outside [0, max_docs = %d] (the buffers are sized by max_docs)", who, *n, max_docs);
    return 0;
}

}  // namespace

extern "C" {

int ee_debug_head_out(const ee_debug_head_out_args* a, void* stream) {
    const char* who = "ee_debug_head_out";
    if (!a) return fail(nullptr, "%s: args must not be NULL", who);
    if (!a->in || !a->W || !a->b || !a->n_docs || !a->out) return fail(nullptr, "%s: in, W, b, n_docs and out must not be NULL", who);
    if (a->H < 4 || a->H > 1024 || a->H % 4 != 0) return fail(nullptr, "%s: hidden size %d is not a multiple of 4 in [4, 1024]", who, a->H);
    if (a->ld < a->H || a->ld % 4 != 0) return fail(nullptr, "%s: ld %d is below the hidden size %d or no multiple of 4", who, a->ld, a->H);
    if (a->Ko < 1) return fail(nullptr, "%s: Ko %d is below 1", who, a->Ko);
    if (a->in_rows < 1 || a->max_docs < 1 || a->max_docs > (1 << 20)) return fail(nullptr, "%s: bad counts (in_rows >= 1, 1 <= max_docs <= 2^20)", who);
    const bool lte = a->lte_out != nullptr;
    if (!lte && (a->lte_in || a->lte_gather || a->lte_w || a->lte_b)) return fail(nullptr, "%s: the LTE block is given without lte_out", who);
    if (lte) {
        if (!a->lte_in || !a->lte_w || !a->lte_b) return fail(nullptr, "%s: lte_out needs lte_in, lte_w and lte_b", who);
        if (a->lte_ld < a->H || a->lte_ld % 4 != 0) return fail(nullptr, "%s: lte_ld %d is below the hidden size %d or no multiple of 4", who, a->lte_ld, a->H);
        if (a->lte_rows < 1) return fail(nullptr, "%s: lte_rows %d is below 1", who, a->lte_rows);
        if (!(a->lte_split_inv >= 0.f)) return fail(nullptr, "%s: lte_split_inv must be 0 (f32 rows) or positive", who);
        if (a->lte_split_inv != 0.f && a->H % 16 != 0) return fail(nullptr, "%s: split rows need a hidden size that is a multiple of 16 (got %d)", who, a->H);
    }
    if (!have_device(who)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipStreamSynchronize(s) != hipSuccess) return fail(nullptr, "%s: the stream is in error", who);
    int n = 0;
    if (int rc = read_n_docs(who, a->n_docs, a->max_docs, &n)) return rc;
    if (a->gather) {
        if (int rc = check_row_map(who, "gather", a->gather, n, a->in_rows)) return rc;
    } else if (n > a->in_rows) {
        return fail(nullptr, "%s: %d documents without a gather leave the %d rows of in", who, n, a->in_rows);
    }
    if (lte && a->lte_gather) {
        if (int rc = check_row_map(who, "lte_gather", a->lte_gather, n, a->lte_rows)) return rc;
    } else if (lte && n > a->lte_rows) {
        return fail(nullptr, "%s: %d documents without an lte_gather leave the %d rows of lte_in", who, n, a->lte_rows);
    }
    HeadOutArgs ho{};
    ho.in = a->in; ho.ld = a->ld; ho.gather = a->gather; ho.W = a->W; ho.b = a->b; ho.H = a->H; ho.Ko = a->Ko;
    ho.n_docs_ptr = a->n_docs; ho.out = a->out;
    if (lte) {
        ho.lte_in = reinterpret_cast<const float*>(a->lte_in); ho.lte_ld = a->lte_ld; ho.lte_gather = a->lte_gather; ho.lte_split_inv = a->lte_split_inv;
        ho.lte_w = a->lte_w; ho.lte_b = a->lte_b; ho.lte_out = a->lte_out;
    }
    launch_head_out(ho, a->max_docs, s);
    return finish(who, s, nullptr, nullptr);
}

}  // extern "C"

namespace {

// ee_debug_exit_decide (qa null) and ee_debug_exit_quota (qa: the quota, its mode and the two arrays the ranking launches fill): the same
// checks of the stage, the same DecideArgs; the quota form runs the ranking launches and the QUOTA decide kernel in place of launch_decide.
// ee_debug_exit_audit (aa: the cut, the seed, the slot base and the caller's delivered array): launch_decide with its AuditArgs
int run_exit_decide(const char* who, const ee_debug_exit_decide_args* a, const ee_debug_exit_quota_args* qa, void* stream,
                    const ee_debug_exit_audit_args* aa = nullptr) {
    if (!a) return fail(nullptr, "%s: args must not be NULL", who);
    if (aa) {
        if (a->no_exit) return fail(nullptr, "%s: no_exit must be 0: dump-all calls ignore the audit and run the plain decide kernels (ee_debug_exit_decide)", who);
        if (aa->cut < 1 || aa->cut > (1ull << 32)) return fail(nullptr, "%s: cut %llu outside [1, 2^32]", who, (unsigned long long)aa->cut);
        if (aa->slot_base < 0) return fail(nullptr, "%s: slot_base %d is negative", who, aa->slot_base);
        if (!aa->delivered) return fail(nullptr, "%s: delivered must not be NULL", who);
    }
    if (qa) {
        if (a->mode != DECIDE_THRESHOLD || a->rule != RULE_PLAIN)
            return fail(nullptr, "%s: a rank is defined for the threshold criteria under the plain rule: mode must be 0 and rule MMEE_RULE_PLAIN, got mode %d, rule %d",
                        who, a->mode, a->rule);
        if (a->is_final || a->no_exit)
            return fail(nullptr, "%s: is_final and no_exit must be 0: the final exit and dump-all calls run the plain decide kernels (ee_debug_exit_decide)", who);
        if (qa->quota_mode != QUOTA_EXACT && qa->quota_mode != QUOTA_AT_LEAST)
            return fail(nullptr, "%s: unknown quota_mode %d (MMEE_QUOTA_EXACT = %d, MMEE_QUOTA_AT_LEAST = %d)", who, qa->quota_mode, QUOTA_EXACT, QUOTA_AT_LEAST);
        if (qa->quota < 0) return fail(nullptr, "%s: quota %d is negative", who, qa->quota);
        if (!qa->crit || !qa->rank) return fail(nullptr, "%s: crit and rank must not be NULL", who);
    }
    if (a->mode < DECIDE_THRESHOLD || a->mode > DECIDE_LTE || a->rule < RULE_PLAIN || a->rule > RULE_EITHER || (a->mode == DECIDE_PATIENCE && a->rule != RULE_PLAIN))
        return fail(nullptr, "%s: launch_decide has no kernel for mode %d with rule %d (modes 0 threshold, 1 patience, 2 LTE; rules 0 plain, 1 streak, 2 either; patience takes the plain rule only)",
                    who, a->mode, a->rule);
    // MMEE_CRIT_GATE is a criterion of this call only where the kernel can read two gate logits (mode 0, head_logits given, Kh == 2); without
    // them the criteria a call can name are the three functions of the policy row, and the refusal says so
    const bool gate_ok = a->criterion == CRIT_GATE && a->mode == DECIDE_THRESHOLD && a->head_logits && a->Kh == 2;
    if (a->criterion == CRIT_GATE && a->mode == DECIDE_PATIENCE)
        return fail(nullptr, "%s: MMEE_CRIT_GATE is a threshold criterion (mode 0), got mode %d", who, a->mode);
    if (a->mode != DECIDE_PATIENCE && a->criterion != CRIT_MAX_CONFIDENCE && a->criterion != CRIT_ENTROPY && a->criterion != CRIT_MARGIN && !gate_ok)
        return fail(nullptr, "%s: criterion %d is none of MMEE_CRIT_MAX_CONFIDENCE, _ENTROPY, _MARGIN", who, a->criterion);
    if (a->K < 1 || a->Kh < 1) return fail(nullptr, "%s: K %d or Kh %d is below 1", who, a->K, a->Kh);
    if (a->exit_index < 0 || a->exit_index > 255) return fail(nullptr, "%s: exit_index %d outside [0, 255]", who, a->exit_index);
    if (a->B < 1 || a->B > (1 << 20)) return fail(nullptr, "%s: B %d outside [1, 2^20]", who, a->B);
    if (a->patience < 0) return fail(nullptr, "%s: patience %d is negative", who, a->patience);
    if (!a->pol_logits || !a->counts || !a->doc_orig || !a->doc_off || !a->x_phys)
        return fail(nullptr, "%s: pol_logits and the current stage (counts, doc_orig, doc_off, x_phys) must not be NULL", who);
    if (!a->n_counts || !a->n_doc_orig || !a->n_doc_off || !a->n_x_src || !a->n_meta_src || !a->out_exit)
        return fail(nullptr, "%s: the next stage (n_counts, n_doc_orig, n_doc_off, n_x_src, n_meta_src) and out_exit must not be NULL", who);
    const bool stateful = a->mode == DECIDE_PATIENCE || a->rule != RULE_PLAIN;
    if (stateful && (!a->prev || !a->run)) return fail(nullptr, "%s: mode %d with rule %d keeps state per document: prev and run must be given", who, a->mode, a->rule);
    const bool compact = a->meta_old || a->meta_new || a->row_src;
    if (compact && (!a->meta_old || !a->meta_new || !a->row_src)) return fail(nullptr, "%s: meta_old, meta_new and row_src are given together or not at all", who);
    if (!have_device(who)) return 1;
    static_assert(sizeof(RowMeta) == 16 && sizeof(StageCounts) == 16, "the layouts include/mmee.h documents");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipStreamSynchronize(s) != hipSuccess) return fail(nullptr, "%s: the stream is in error", who);

    // ---- the stage on host copies: the table's rules, every original slot inside [0, B) ----
    StageCounts hc{};
    if (hipMemcpy(&hc, a->counts, sizeof(hc), hipMemcpyDeviceToHost) != hipSuccess) return fail(nullptr, "%s: copy of counts failed", who);
    const int n = hc.n_docs;
    if (n < 0 || n > a->B) return fail(nullptr, "%s: counts.n_docs = %d outside [0, B = %d]", who, n, a->B);
    DocTable stage;
    std::vector<int> dorig;
    if (!stage.read(a->doc_off, n) || !to_host(dorig, a->doc_orig, (size_t)n)) return fail(nullptr, "%s: copy of the document tables failed", who);
    if (stage.off[0] != 0) return fail(nullptr, "%s: doc_off[0] = %d, must be 0", who, stage.off[0]);
    for (int d = 0; d < n; ++d) {
        if (stage.len(d) < 1 || stage.off[d + 1] > (1 << 28)) return fail(nullptr, "%s: stage document %d has %d rows (or the stage more than 2^28)", who, d, stage.len(d));
        if (dorig[d] < 0 || dorig[d] >= a->B) return fail(nullptr, "%s: doc_orig[%d] = %d outside [0, B = %d)", who, d, dorig[d], a->B);
    }
    if (hc.n_rows != stage.rows) return fail(nullptr, "%s: counts.n_rows = %d, doc_off[n_docs] = %d", who, hc.n_rows, stage.rows);

    Scratch sc;
    DecideArgs d{};
    d.pol_logits = a->pol_logits; d.head_logits = a->head_logits; d.K = a->K; d.Kh = a->Kh;
    d.thr = a->thr; d.temp = a->temp;
    d.criterion = a->criterion; d.is_final = a->is_final ? 1 : 0; d.no_exit = a->no_exit ? 1 : 0; d.exit_index = a->exit_index; d.B = a->B;
    d.lte_score = a->lte_score;
    d.counts = reinterpret_cast<const StageCounts*>(a->counts); d.doc_orig = a->doc_orig; d.doc_off = a->doc_off; d.x_phys = a->x_phys;
    d.n_counts = reinterpret_cast<StageCounts*>(a->n_counts); d.n_doc_orig = a->n_doc_orig; d.n_doc_off = a->n_doc_off; d.n_x_src = a->n_x_src;
    d.n_meta_src = a->n_meta_src;
    d.out_logits = a->out_logits; d.out_exit = a->out_exit; d.out_conf = a->out_conf; d.out_all_logits = a->out_all_logits;
    d.out_all_crit = a->out_all_crit; d.out_head_logits = a->out_head_logits; d.out_head_crit = a->out_head_crit;
    PatienceArgs pa{};
    pa.t = a->patience; pa.prev = a->prev; pa.run = a->run;
    QuotaArgs q{};
    if (qa) { q.q = qa->quota; q.crit = qa->crit; q.rank = qa->rank; }
    if (a->by_pointer) {
        // as a replay reads them: exit e's threshold and temperature at [e] of device vectors, its patience (its quota) at [0] of the pointer handed over
        double *thr = nullptr, *temp = nullptr, *t = nullptr;
        const size_t e1 = (size_t)a->exit_index + 1;
        if (!get_dirty(sc, &thr, e1, s) || !get_dirty(sc, &temp, e1, s) || !get_dirty(sc, &t, 1, s)) return fail(nullptr, kScratchFailed, who);
        const double hv[3] = {a->thr, a->temp, qa ? (double)qa->quota : (double)a->patience};
        if (hipMemcpyAsync(thr + a->exit_index, &hv[0], sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(temp + a->exit_index, &hv[1], sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(t, &hv[2], sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return fail(nullptr, kUploadFailed, who);
        d.thr_ptr = thr; d.temp_ptr = temp; pa.t_ptr = t;
        d.thr = d.temp = __builtin_nan(""); pa.t = -1;             // the by-value forms must not be what the kernel reads
        if (qa) { q.q_ptr = t; q.q = -1; }
    }
    if (qa) {
        launch_exit_quota_crit(d, q, a->B, s);
        launch_exit_quota_rank(d, q, a->B, s);
        launch_decide_quota(d, q, qa->quota_mode, s);
    } else {
        AuditArgs au{};
        if (aa) { au.delivered = aa->delivered; au.cut = aa->cut; au.seed = aa->seed; au.slot_base = aa->slot_base; }
        launch_decide(d, stateful ? &pa : nullptr, a->mode, a->rule, s, aa ? &au : nullptr);
    }
    if (compact) {
        const int cus = device_cus(who);
        if (!cus) return 1;
        launch_compact_rows(d.n_counts, a->n_doc_off, a->n_x_src, a->n_meta_src, reinterpret_cast<const RowMeta*>(a->meta_old),
                            reinterpret_cast<RowMeta*>(a->meta_new), a->row_src, a->B, cus, s);
    }
    return finish(who, s, nullptr, nullptr);
}

}  // namespace

extern "C" {

int ee_debug_exit_decide(const ee_debug_exit_decide_args* a, void* stream) { return run_exit_decide("ee_debug_exit_decide", a, nullptr, stream); }

int ee_debug_exit_quota(const ee_debug_exit_quota_args* a, void* stream) {
    if (!a) return fail(nullptr, "ee_debug_exit_quota: args must not be NULL");
    return run_exit_decide("ee_debug_exit_quota", &a->decide, a, stream);
}

int ee_debug_exit_audit(const ee_debug_exit_audit_args* a, void* stream) {
    if (!a) return fail(nullptr, "ee_debug_exit_audit: args must not be NULL");
    return run_exit_decide("ee_debug_exit_audit", &a->decide, nullptr, stream, a);
}

int ee_debug_exit_ensemble(const ee_debug_exit_ensemble_args* a, void* stream) {
    const char* who = "ee_debug_exit_ensemble";
    if (!a) return fail(nullptr, "%s: args must not be NULL", who);
    if (!a->pol_logits || !a->counts || !a->doc_orig || !a->w || !a->state || !a->out)
        return fail(nullptr, "%s: pol_logits, counts, doc_orig, w, state and out must not be NULL", who);
    if (a->K < 1 || a->E1 < 1) return fail(nullptr, "%s: K %d or E1 %d is below 1", who, a->K, a->E1);
    if (a->exit_index < 0 || a->exit_index >= a->E1) return fail(nullptr, "%s: exit_index %d outside [0, E1 = %d)", who, a->exit_index, a->E1);
    if (a->B < 1 || a->B > (1 << 20)) return fail(nullptr, "%s: B %d outside [1, 2^20]", who, a->B);
    if ((long long)a->E1 * a->B * a->K > (1ll << 31)) return fail(nullptr, "%s: a state of E1 B K = %lld doubles is above 2^31", who, (long long)a->E1 * a->B * a->K);
    if (a->pol_rows < 0 || a->out_rows < 0) return fail(nullptr, "%s: pol_rows %d or out_rows %d is negative", who, a->pol_rows, a->out_rows);
    if (!have_device(who)) return 1;
    static_assert(sizeof(StageCounts) == 16, "the layout include/mmee.h documents");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipStreamSynchronize(s) != hipSuccess) return fail(nullptr, "%s: the stream is in error", who);
    StageCounts hc{};
    if (hipMemcpy(&hc, a->counts, sizeof(hc), hipMemcpyDeviceToHost) != hipSuccess) return fail(nullptr, "%s: copy of counts failed", who);
    const int n = hc.n_docs;
    if (n < 0 || n > a->B) return fail(nullptr, "%s: counts.n_docs = %d outside [0, B = %d]", who, n, a->B);
    if (n > a->pol_rows || n > a->out_rows) return fail(nullptr, "%s: %d documents leave the %d rows of pol_logits or the %d rows of out", who, n, a->pol_rows, a->out_rows);
    if (int rc = check_row_map(who, "doc_orig", a->doc_orig, n, a->B)) return rc;
    Scratch sc;
    EnsembleArgs en{};
    en.pol_logits = a->pol_logits; en.K = a->K; en.E1 = a->E1; en.exit_index = a->exit_index; en.B = a->B;
    en.temp = a->temp;
    en.counts = reinterpret_cast<const StageCounts*>(a->counts); en.doc_orig = a->doc_orig;
    en.w = a->w; en.b = a->b; en.state = a->state; en.out = a->out;
    if (a->by_pointer) {
        // as a replay reads it: the temperature of exit e at [e] of a device vector
        double* temp = nullptr;
        if (!get_dirty(sc, &temp, (size_t)a->exit_index + 1, s)) return fail(nullptr, kScratchFailed, who);
        if (hipMemcpyAsync(temp + a->exit_index, &a->temp, sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return fail(nullptr, kUploadFailed, who);
        en.temp_ptr = temp;
        en.temp = __builtin_nan("");                               // the by-value form must not be what the kernel reads
    }
    launch_exit_ensemble(en, s);
    return finish(who, s, nullptr, nullptr);
}

int ee_debug_audit_tally(const ee_debug_audit_tally_args* a, void* stream) {
    const char* who = "ee_debug_audit_tally";
    if (!a) return fail(nullptr, "%s: args must not be NULL", who);
    if (!a->pol_logits || !a->counts || !a->doc_orig || !a->delivered || !a->out_logits || !a->out_exit || !a->tally)
        return fail(nullptr, "%s: pol_logits, counts, doc_orig, delivered, out_logits, out_exit and tally must not be NULL", who);
    if (a->K < 1) return fail(nullptr, "%s: K %d is below 1", who, a->K);
    if (a->E1 < 2 || a->E1 > kCtlMaxE1) return fail(nullptr, "%s: E1 = %d, need 2 <= E1 <= %d", who, a->E1, kCtlMaxE1);
    if (a->B < 1 || a->B > (1 << 20)) return fail(nullptr, "%s: B %d outside [1, 2^20]", who, a->B);
    if (a->pol_rows < 0) return fail(nullptr, "%s: pol_rows %d is negative", who, a->pol_rows);
    if (a->cut < 1 || a->cut > (1ull << 32)) return fail(nullptr, "%s: cut %llu outside [1, 2^32]", who, (unsigned long long)a->cut);
    if (a->slot_base < 0) return fail(nullptr, "%s: slot_base %d is negative", who, a->slot_base);
    if (!(a->temp > 0.0)) return fail(nullptr, "%s: temp %g is not positive", who, a->temp);
    if (!have_device(who)) return 1;
    static_assert(sizeof(StageCounts) == 16, "the layout include/mmee.h documents");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipStreamSynchronize(s) != hipSuccess) return fail(nullptr, "%s: the stream is in error", who);
    StageCounts hc{};
    if (hipMemcpy(&hc, a->counts, sizeof(hc), hipMemcpyDeviceToHost) != hipSuccess) return fail(nullptr, "%s: copy of counts failed", who);
    const int n = hc.n_docs;
    if (n < 0 || n > a->B) return fail(nullptr, "%s: counts.n_docs = %d outside [0, B = %d]", who, n, a->B);
    if (n > a->pol_rows) return fail(nullptr, "%s: %d documents leave the %d rows of pol_logits", who, n, a->pol_rows);
    if (int rc = check_row_map(who, "doc_orig", a->doc_orig, n, a->B)) return rc;
    AuditTallyArgs t{};
    t.counts = reinterpret_cast<const StageCounts*>(a->counts); t.doc_orig = a->doc_orig; t.pol_logits = a->pol_logits; t.temp = a->temp;
    t.K = a->K; t.B = a->B; t.E1 = a->E1; t.delivered = a->delivered; t.out_logits = a->out_logits; t.out_exit = a->out_exit;
    t.cut = a->cut; t.seed = a->seed; t.slot_base = a->slot_base; t.tally = reinterpret_cast<long long*>(a->tally);
    launch_audit_tally(t, s);
    return finish(who, s, nullptr, nullptr);
}

int ee_debug_controller_step(const ee_debug_controller_step_args* a, void* stream) {
    const char* who = "ee_debug_controller_step";
    if (!a) return fail(nullptr, "%s: args must not be NULL", who);
    if (!a->path || !a->state || !a->tally || !a->thr) return fail(nullptr, "%s: path, state, tally and thr must not be NULL", who);
    if (a->E1 < 2 || a->E1 > kCtlMaxE1) return fail(nullptr, "%s: E1 = %d, need 2 <= E1 <= %d", who, a->E1, kCtlMaxE1);
    if (a->V < 2 || a->V > (1 << 20)) return fail(nullptr, "%s: V = %d vectors, a path needs 2 <= V <= 2^20", who, a->V);
    if (a->sign != 1.0 && a->sign != -1.0) return fail(nullptr, "%s: sign is +1 or -1", who);
    if (!(a->alpha > 0.0 && a->alpha < 1.0)) return fail(nullptr, "%s: alpha = %g, the risk level must lie in (0, 1)", who, a->alpha);
    if (!(a->gamma > 0.0) || !std::isfinite(a->gamma)) return fail(nullptr, "%s: gamma = %g, the step must be positive and finite", who, a->gamma);
    if (a->log_cap < 0 || (a->log_cap > 0 && !a->log)) return fail(nullptr, "%s: log_cap = %d rows without a log", who, a->log_cap);
    if (!have_device(who)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipStreamSynchronize(s) != hipSuccess) return fail(nullptr, "%s: the stream is in error", who);
    long long calls = 0;
    if (hipMemcpy(&calls, a->state + 1, sizeof(calls), hipMemcpyDeviceToHost) != hipSuccess) return fail(nullptr, "%s: copy of the state failed", who);
    if (calls < 0) return fail(nullptr, "%s: state.calls = %lld is negative (it picks the row of the log ring)", who, calls);
    ControllerStepArgs st{};
    st.path = a->path; st.V = a->V; st.E1 = a->E1; st.sign = a->sign; st.alpha = a->alpha; st.gamma = a->gamma;
    st.state = reinterpret_cast<long long*>(a->state); st.tally = reinterpret_cast<const long long*>(a->tally); st.thr = a->thr;
    st.log = reinterpret_cast<long long*>(a->log); st.log_cap = a->log ? a->log_cap : 0;
    launch_controller_step(st, s);
    return finish(who, s, nullptr, nullptr);
}

int ee_debug_deadline_check(const ee_debug_deadline_check_args* a, void* stream) {
    const char* who = "ee_debug_deadline_check";
    if (!a) return fail(nullptr, "%s: args must not be NULL", who);
    if (!a->state || !a->thr) return fail(nullptr, "%s: state and thr must not be NULL", who);
    if (a->E1 < 2 || a->E1 > kCtlMaxE1) return fail(nullptr, "%s: E1 = %d, need 2 <= E1 <= %d", who, a->E1, kCtlMaxE1);
    if (a->exit_index < 0 || a->exit_index >= a->E1) return fail(nullptr, "%s: exit_index %d outside [0, E1 = %d)", who, a->exit_index, a->E1);
    if (a->khz == 0) return fail(nullptr, "%s: khz is 0: ticks cannot be turned into ns", who);
    if (a->sign != 1.0 && a->sign != -1.0) return fail(nullptr, "%s: sign is +1 or -1", who);
    if (a->call == 0) return fail(nullptr, "%s: call is 0 (deadline calls are numbered from 1)", who);
    if (!have_device(who)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipStreamSynchronize(s) != hipSuccess) return fail(nullptr, "%s: the stream is in error", who);
    Scratch sc;
    unsigned long long* word = nullptr;                                  // the forward's is pinned host memory; the load is the same
    if (!sc.get(&word, 1)) return fail(nullptr, kScratchFailed, who);
    const unsigned long long w = a->host_word;
    if (hipMemcpy(word, &w, sizeof(w), hipMemcpyHostToDevice) != hipSuccess) return fail(nullptr, kUploadFailed, who);
    DeadlineCheckArgs k{};
    k.E1 = a->E1; k.exit_index = a->exit_index; k.khz = a->khz; k.sign = a->sign; k.call = a->call; k.budget = a->budget_ns; k.eta = a->eta_ns;
    k.host_word = word; k.state = reinterpret_cast<long long*>(a->state); k.thr = a->thr; k.row = reinterpret_cast<long long*>(a->row);
    k.now_set = 1; k.t0_set = 1; k.now = a->now; k.t0 = a->t0;
    launch_deadline_check(k, s);
    return finish(who, s, nullptr, nullptr);
}

int ee_debug_rows_out(const ee_debug_rows_out_args* a, void* stream) {
    const char* who = "ee_debug_rows_out";
    if (!a) return fail(nullptr, "%s: args must not be NULL", who);
    if (a->which != 0 && a->which != 1) return fail(nullptr, "%s: which %d is neither 0 (gather_cls) nor 1 (rows_to_padded)", who, a->which);
    if (!a->X || !a->out) return fail(nullptr, "%s: X and out must not be NULL", who);
    if (a->H < 4 || a->H > 4096 || a->H % 4 != 0) return fail(nullptr, "%s: hidden size %d is not a multiple of 4 in [4, 4096]", who, a->H);
    if (!(a->split_inv >= 0.f)) return fail(nullptr, "%s: split_inv must be 0 (f32 rows) or positive", who);
    if (a->split_inv != 0.f && a->H % 16 != 0) return fail(nullptr, "%s: split rows need a hidden size that is a multiple of 16 (got %d)", who, a->H);
    if (a->x_rows < 1 || a->out_rows < 0) return fail(nullptr, "%s: bad counts (x_rows >= 1, out_rows >= 0)", who);
    if (a->which == 0) {
        if (!a->x_phys || !a->n_docs) return fail(nullptr, "%s: gather_cls needs x_phys and n_docs", who);
        if (a->max_docs < 1 || a->max_docs > (1 << 20)) return fail(nullptr, "%s: max_docs %d outside [1, 2^20]", who, a->max_docs);
    } else {
        if (!a->doc_off) return fail(nullptr, "%s: rows_to_padded needs doc_off", who);
        if (a->B < 1 || a->T < 0 || a->Pv < 0 || a->T + (long long)a->Pv < 1 || (long long)a->B * ((long long)a->T + a->Pv) > (1ll << 28))
            return fail(nullptr, "%s: bad shape (B >= 1, T >= 0, Pv >= 0, T + Pv >= 1, B (T + Pv) <= 2^28), got B %d, T %d, Pv %d", who, a->B, a->T, a->Pv);
        if (!a->text_dst && a->T != 0) return fail(nullptr, "%s: without text_dst (image-only) T must be 0, got %d", who, a->T);
        if (a->text_dst && !a->ntext) return fail(nullptr, "%s: text_dst without ntext", who);
    }
    if (!have_device(who)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipStreamSynchronize(s) != hipSuccess) return fail(nullptr, "%s: the stream is in error", who);
    const float* X = reinterpret_cast<const float*>(a->X);
    if (a->which == 0) {
        int n = 0;
        if (int rc = read_n_docs(who, a->n_docs, a->max_docs, &n)) return rc;
        if (int rc = check_row_map(who, "x_phys", a->x_phys, n, a->x_rows)) return rc;
        if (a->doc_orig) {
            if (int rc = check_row_map(who, "doc_orig", a->doc_orig, n, a->out_rows)) return rc;
        } else if (n > a->out_rows) {
            return fail(nullptr, "%s: %d documents without doc_orig leave the %d rows of out", who, n, a->out_rows);
        }
        launch_gather_cls(X, a->H, a->x_phys, a->doc_orig, a->n_docs, a->out, a->max_docs, s, a->split_inv);
        return finish(who, s, nullptr, nullptr);
    }
    const int B = a->B, T = a->T, Pv = a->Pv;
    if ((long long)B * (T + Pv) > a->out_rows) return fail(nullptr, "%s: B (T + Pv) = %lld rows leave the %d rows of out", who, (long long)B * (T + Pv), a->out_rows);
    std::vector<int> off, td, nt;
    if (!to_host(off, a->doc_off, (size_t)B) || (a->text_dst && (!to_host(td, a->text_dst, (size_t)B * T) || !to_host(nt, a->ntext, (size_t)B))))
        return fail(nullptr, "%s: copy of the document tables failed", who);
    for (int d = 0; d < B; ++d) {
        const long long vis = (long long)off[d] + (a->text_dst ? nt[d] : 0);
        if (off[d] < 0 || (a->text_dst && nt[d] < 0) || vis + Pv > a->x_rows)
            return fail(nullptr, "%s: the visual rows of document %d (%lld .. %lld) leave the %d rows of X", who, d, vis, vis + Pv, a->x_rows);
        for (int p = 0; p < T; ++p) {
            const int t = td[(size_t)d * T + p];
            if (t >= 0 && (long long)off[d] + t >= a->x_rows)
                return fail(nullptr, "%s: text_dst[%d][%d] = %d leaves the %d rows of X", who, d, p, t, a->x_rows);
        }
    }
    launch_rows_to_padded(X, a->split_inv, a->H, B, T, Pv, a->text_dst, a->ntext, a->doc_off, a->out, s);
    return finish(who, s, nullptr, nullptr);
}

}  // extern "C"
