// Entry points of the device fits, none of which sees a handle: one-layer and two-layer exit heads from dumped CLS rows against labels
// (ee_head_fit, ee_mlp_head_fit), against the final classifier's logits (ee_head_fit_distill, ee_mlp_head_fit_distill), either with sample
// weights (ee_head_fit_weighted, ee_mlp_head_fit_weighted), the 2-way gate heads of either depth (ee_head_fit_gate; ee_mlp_head_fit_gate and
// ee_mlp_head_fit_gate_weighted), the learning-to-exit classifier (ee_lte_fit, with ee_lte_targets and ee_lte_scores) and the exit ensemble's weights (ee_ensemble_fit); their workspace queries, and the ee_debug_*_lossgrad hooks that run one evaluation of an
// objective on caller-provided buffers.  The L-BFGS is fit_lbfgs.hip.
//
// What a head is fitted against is one value, HeadObjective (mmee_kernels.h).  Each head entry point builds it from its own arguments
// (labelled, distilled, weighted, gate) and calls one of three bodies -- head_fit_call, mlp_head_fit_call, head_lossgrad_call -- which hand it
// down unchanged; objective_refuse holds the objective's own refusals, and error_word_fail is the one decoder of the error word, for the head
// fits, the LTE entry points and the debug hooks alike.
#include "capi_internal.h"

using namespace mmee;
using namespace mmee::capi;

static_assert(kHeadFitSlab == MMEE_HEAD_FIT_SLAB, "the kernel's slab height is the ABI's");
static_assert(kMlpHeadFitRows == MMEE_MLP_HEAD_FIT_ROWS, "the kernels' row tile is the ABI's");
static_assert(kLteFitRows == MMEE_LTE_FIT_ROWS, "the kernel's unit of rows is the ABI's");
static_assert(kLteLossMse == MMEE_LTE_LOSS_MSE && kLteLossBce == MMEE_LTE_LOSS_BCE, "the loss codes are the ABI's");

// ---- what the fits share -----------------------------------------------------------------------------------------------------------------
// the refusals of a fit's budget, in this order, behind those of its problem; need_bytes() is only asked about a valid history
template <typename Need>
static int budget_refuse(const char* who, double gtol, int32_t max_evals, int32_t history, size_t workspace_bytes, Need need_bytes) {
    if (!(gtol >= 0.0)) return fail(nullptr, "%s: gtol = %g, need gtol >= 0", who, gtol);
    if (max_evals < 1) return fail(nullptr, "%s: max_evals = %d, need max_evals >= 1", who, max_evals);
    if (history < 1 || history > kHeadFitMaxHistory) return fail(nullptr, "%s: history = %d, need 1 <= history <= %d", who, history, kHeadFitMaxHistory);
    const size_t need = need_bytes();
    if (workspace_bytes < need) return fail(nullptr, "%s: workspace of %zu bytes, needs %zu bytes", who, workspace_bytes, need);
    return 0;
}

// ---- the error word, decoded once ---------------------------------------------------------------------------------------------------------
// Which objective an entry point states.  For the head fits it is the family of entry points that built the HeadObjective, which the value
// alone does not say: a distilled entry point that was handed NULL teacher_logits is refused, a weighted one fits against labels then.
enum class Objective { kLabelled, kDistilled, kWeighted, kGate, kWeightedGate, kLte, kLteTargets, kEnsemble };

// bit 0: a bad label or target -- which, and so the message, is the objective's; bit 1: a teacher logit that is not finite (the distilled
// objectives); bit 2: a sample weight that is negative or not finite, bit 3: an exit whose weights sum to zero (launch_row_scale).  Bits 2 and 3
// are looked at first: labels and teacher rows mean nothing under them.  fit: a fit's call, which has then written no output and says so;
// else a debug hook's one evaluation.  -> 0 for a clean word
static int error_word_fail(const char* who, int err, Objective of, bool fit, int K) {
    const char* tail = fit ? "; no output was written" : "";
    if (err & 4) return fail(nullptr, "%s: a sample weight is negative or not finite%s", who, tail);
    if (err & 8) return fail(nullptr, "%s: an exit's weights sum to zero%s", who, tail);
    if (err & 1) switch (of) {
        default:
            return fail(nullptr, fit ? "%s: a label is outside [0, K = %d); no output was written" : "%s: a label is outside [0, K = %d)", who, K);
        case Objective::kGate:
        case Objective::kWeightedGate:
            return fit ? fail(nullptr, "%s: a target is not finite or lies outside [0, 1]%s", who, tail)
                       : fail(nullptr, "%s: a target is not finite or lies outside [0, 1] (K = %d)", who, K);
        case Objective::kLte:
            return fail(nullptr, fit ? "%s: a target is outside [0, 1] or NaN; no output was written" : "%s: a target is outside [0, 1] or NaN", who);
        case Objective::kLteTargets:
            return fail(nullptr, "%s: a label is outside [0, K = %d) or a logit is NaN (a row its document never reached); nothing was written", who, K);
    }
    if ((err & 2) && of == Objective::kEnsemble)
        return fail(nullptr, "%s: a logit is not finite (dump-all marks the rows a document never reached with NaN)%s", who, tail);
    if (err & 2)
        return fail(nullptr, "%s: a teacher logit is not finite (dump-all marks the rows a document never reached with NaN)%s", who, tail);
    return 0;
}

// The tail of a call that left an error word on the device: the launch status, the word read on the stream, one synchronise.
static int finish_call(const char* who, bool prepared, const void* err_word, hipStream_t s, Objective of, int K) {
    if (!prepared) return fail(nullptr, "%s: preparing the workspace (memset, copy of theta0) failed", who);
    if (launch_status(nullptr, who)) return 1;
    int err = 0;
    if (hipMemcpyAsync(&err, err_word, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return fail(nullptr, "%s: reading the error word failed: %s", who, hipGetErrorString(hipGetLastError()));
    return error_word_fail(who, err, of, true, K);
}

// One evaluation of an objective for a debug entry point: launch(scratch, err) gets n zeroed doubles and a zeroed error word.
template <typename Launch>
static int debug_lossgrad(const char* who, size_t n, hipStream_t s, Launch launch, Objective of, int K) {
    if (!have_device(who)) return 1;
    Scratch sc;
    double* scratch = nullptr;
    int* err_dev = nullptr;
    if (!sc.get(&scratch, n) || !sc.get(&err_dev, 1)) return fail(nullptr, "%s: hipMalloc of the scratch failed", who);
    launch(scratch, err_dev);
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(nullptr, "%s: launch failed: %s", who, hipGetErrorString(e));
    int err = 0;
    if (hipMemcpy(&err, err_dev, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail(nullptr, "%s: copy of the error word failed", who);
    if (launch_status(nullptr, who)) return 1;
    return error_word_fail(who, err, of, false, K);
}

// the refusals the head fits and their debug hooks share, before any device call
static int head_fit_refuse(const char* who, const float* features, int32_t E, int32_t N, int32_t H, int32_t K, double l2) {
    if (E < 1 || E > 65535) return fail(nullptr, "%s: E = %d, need 1 <= E <= 65535", who, E);
    if (N < 1) return fail(nullptr, "%s: N = %d, need N >= 1", who, N);
    if (K < 2 || K > 64) return fail(nullptr, "%s: K = %d, need 2 <= K <= 64 (ee_create's limit)", who, K);
    if (H < 4 || H > kHeadFitMaxH || H % 4 != 0)
        return fail(nullptr, "%s: H = %d, need 4 <= H <= %d and H %% 4 == 0 (a slab of %d rows stays in LDS)", who, H, kHeadFitMaxH, kHeadFitSlab);
    if (!(l2 > 0.0)) return fail(nullptr, "%s: l2 = %g, need l2 > 0 (the objective is strongly convex only then)", who, l2);
    if (reinterpret_cast<uintptr_t>(features) % 16 != 0) return fail(nullptr, "%s: features must be 16-byte aligned", who);
    return 0;
}
// the refusals of the LTE entry points that read feature rows, before any device call
static int lte_rows_refuse(const char* who, const float* features, int32_t E, int32_t N, int32_t H) {
    if (E < 1 || E > kLteFitMaxExits) return fail(nullptr, "%s: E = %d, need 1 <= E <= %d", who, E, kLteFitMaxExits);
    if (N < 1) return fail(nullptr, "%s: N = %d, need N >= 1", who, N);
    if (H < 4 || H > kHeadFitMaxH || H % 4 != 0) return fail(nullptr, "%s: H = %d, need 4 <= H <= %d and H %% 4 == 0", who, H, kHeadFitMaxH);
    if (reinterpret_cast<uintptr_t>(features) % 16 != 0) return fail(nullptr, "%s: features must be 16-byte aligned", who);
    return 0;
}
static int lte_objective_refuse(const char* who, int32_t loss, double l2) {
    if (loss != MMEE_LTE_LOSS_MSE && loss != MMEE_LTE_LOSS_BCE)
        return fail(nullptr, "%s: loss = %d, need MMEE_LTE_LOSS_MSE (0) or MMEE_LTE_LOSS_BCE (1)", who, loss);
    if (!(l2 > 0.0)) return fail(nullptr, "%s: l2 = %g, need l2 > 0", who, l2);
    return 0;
}

// ---- the head fits' entry points: each builds its HeadObjective and calls one of three bodies ------------------------------------------------
// what a head entry point asks for: the objective it built, and which family of entry points it belongs to
struct Asked {
    Objective by;
    HeadObjective o;
};
static const long long* int64_labels(const int64_t* labels) { return reinterpret_cast<const long long*>(labels); }
static Asked labelled(const int64_t* labels) { return {Objective::kLabelled, {int64_labels(labels), {}, nullptr, nullptr}}; }
static Asked distilled(const int64_t* labels, const float* teacher_logits, double alpha, double temperature) {
    return {Objective::kDistilled, {int64_labels(labels), {teacher_logits, alpha, temperature}, nullptr, nullptr}};
}
static Asked weighted(const int64_t* labels, const float* teacher_logits, double alpha, double temperature, const float* weights) {
    return {Objective::kWeighted, {int64_labels(labels), {teacher_logits, alpha, temperature}, weights, nullptr}};
}
static Asked gate(const double* targets) { return {Objective::kGate, {nullptr, {}, nullptr, targets}}; }
static Asked weighted_gate(const double* targets, const float* weights) { return {Objective::kWeightedGate, {nullptr, {}, weights, targets}}; }

// The refusals of the objective itself, with the body's NULL check among them, in the order they have always been tried: the weighted entry
// points' own, the NULL check, the distilled objective's.  missing: one of the body's other required pointers is NULL; null_fmt: the body's
// message for a NULL pointer, a format of (who, the name of the target the objective cannot do without).
static int objective_refuse(const char* who, const Asked& q, bool missing, const char* null_fmt) {
    const HeadObjective& o = q.o;
    const DistillTargets& soft = o.soft;
    const bool to_gate = q.by == Objective::kGate || q.by == Objective::kWeightedGate;
    if ((q.by == Objective::kWeighted || q.by == Objective::kWeightedGate) && !o.weights)
        return fail(nullptr, "%s: NULL argument (weights are required: (E,N) float32; the unweighted entry points take none)", who);
    if (q.by == Objective::kWeighted && !soft.teacher && soft.alpha != 0.0)                  // teacher_logits may be NULL here: labels alone
        return fail(nullptr, "%s: alpha = %g without teacher_logits: NULL teacher_logits select the labelled objective, alpha must be 0", who,
                    soft.alpha);
    const bool to_teacher = q.by == Objective::kDistilled || (q.by == Objective::kWeighted && soft.teacher);
    if (missing || (to_gate ? !o.gate_targets : !to_teacher && !o.labels))
        return fail(nullptr, null_fmt, who, to_gate ? "targets" : to_teacher ? "teacher_logits" : "labels");
    if (!to_teacher) return 0;
    if (!soft.teacher) return fail(nullptr, "%s: NULL argument (teacher_logits are required)", who);
    if (!(soft.alpha >= 0.0 && soft.alpha <= 1.0)) return fail(nullptr, "%s: alpha = %g, need 0 <= alpha <= 1", who, soft.alpha);
    if (!(soft.temperature > 0.0) || std::isinf(soft.temperature))
        return fail(nullptr, "%s: temperature = %g, need a finite temperature > 0", who, soft.temperature);
    if (soft.alpha < 1.0 && !o.labels) return fail(nullptr, "%s: NULL labels at alpha = %g: only alpha == 1 does without them", who, soft.alpha);
    return 0;
}

static int head_fit_call(const char* who, const Asked& q, const float* features, int32_t E, int32_t N, int32_t H, int32_t K,
                         double l2, double gtol, int32_t max_evals, int32_t history, void* workspace, size_t workspace_bytes, float* weight,
                         float* bias, double* weight64, double* bias64, double* loss, double* grad_norm, int32_t* evals, int32_t* status,
                         void* stream) {
    if (objective_refuse(who, q, !features || !workspace || !weight || !bias,
                         "%s: NULL argument (features, %s, workspace, weight and bias are required)") ||
        head_fit_refuse(who, features, E, N, H, K, l2))
        return 1;
    if (budget_refuse(who, gtol, max_evals, history, workspace_bytes, [&] { return head_fit_workspace_bytes(E, N, H, K, history, q.o.weights != nullptr); }))
        return 1;
    if (!have_device(who)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const HeadFitArgs a{{features, E, N, H, l2, gtol, max_evals, history, workspace, nullptr, nullptr, loss, grad_norm, evals, status},
                        q.o, K, weight, bias, weight64, bias64};
    return finish_call(who, launch_head_fit(a, s), workspace, s, q.by, K);
}

static int mlp_head_fit_call(const char* who, const Asked& q, const float* features, const double* theta0, int32_t E,
                             int32_t N, int32_t H, int32_t K, double l2, double gtol, int32_t max_evals, int32_t history, void* workspace,
                             size_t workspace_bytes, float* dense_weight, float* dense_bias, float* weight, float* bias, double* theta64,
                             double* loss, double* grad_norm, int32_t* evals, int32_t* status, void* stream) {
    if (objective_refuse(who, q, !features || !theta0 || !workspace || !dense_weight || !dense_bias || !weight || !bias,
                         "%s: NULL argument (features, %s, theta0, workspace, dense_weight, dense_bias, weight and bias are required; "
                         "theta = 0 is a saddle the iteration never leaves, so there is no default start)") ||
        head_fit_refuse(who, features, E, N, H, K, l2))
        return 1;
    if (budget_refuse(who, gtol, max_evals, history, workspace_bytes,
                      [&] { return mlp_head_fit_workspace_bytes(E, N, H, K, history, q.o.weights != nullptr); }))
        return 1;
    if (!have_device(who)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const MlpHeadFitArgs a{{features, E, N, H, l2, gtol, max_evals, history, workspace, theta0, theta64, loss, grad_norm, evals, status},
                           q.o, K, dense_weight, dense_bias, weight, bias};
    return finish_call(who, launch_mlp_head_fit(a, s), workspace, s, q.by, K);
}

// ONE evaluation of a head objective: mlp selects the two-layer head
static int head_lossgrad_call(const char* who, bool mlp, const Asked& q, const float* features, const double* theta64,
                              int32_t E, int32_t N, int32_t H, int32_t K, double l2, double* loss, double* grad, void* stream) {
    if (objective_refuse(who, q, !features || !theta64 || !loss || !grad, "%s: NULL argument") ||
        head_fit_refuse(who, features, E, N, H, K, l2))
        return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t n = (mlp ? mlp_head_fit_scratch_doubles(E, N, H, K) : head_fit_partial_bytes(E, N, H, K) / sizeof(double)) +
                     (q.o.weights ? (size_t)E * N : 0);                               // the row scales lie behind the unweighted scratch
    return debug_lossgrad(who, n, s, [&](double* scratch, int* err) {
        if (mlp) launch_mlp_head_lossgrad(features, q.o, theta64, E, N, H, K, l2, scratch, err, loss, grad, s);
        else launch_head_lossgrad(features, q.o, theta64, E, N, H, K, l2, scratch, err, loss, grad, s);
    }, q.by, K);
}

// the workspace queries' answer to arguments no fit accepts
static bool no_workspace(int32_t E, int32_t N, int32_t H, int32_t K, int32_t history) { return E < 1 || N < 1 || H < 1 || K < 1 || history < 1; }

extern "C" {

// ---- exit heads from CLS rows (head_fit.hip) ---------------------------------------------------------------------------------------------
size_t ee_head_fit_workspace_bytes(int32_t E, int32_t N, int32_t H, int32_t K, int32_t history) {
    return no_workspace(E, N, H, K, history) ? 0 : head_fit_workspace_bytes(E, N, H, K, history, false);
}

int ee_head_fit(const float* features, const int64_t* labels, int32_t E, int32_t N, int32_t H, int32_t K, double l2, double gtol,
                int32_t max_evals, int32_t history, void* workspace, size_t workspace_bytes, float* weight, float* bias, double* weight64,
                double* bias64, double* loss, double* grad_norm, int32_t* evals, int32_t* status, void* stream) {
    return head_fit_call("ee_head_fit", labelled(labels), features, E, N, H, K, l2, gtol, max_evals, history, workspace, workspace_bytes, weight,
                         bias, weight64, bias64, loss, grad_norm, evals, status, stream);
}

int ee_head_fit_distill(const float* features, const float* teacher_logits, const int64_t* labels, int32_t E, int32_t N, int32_t H, int32_t K,
                        double alpha, double temperature, double l2, double gtol, int32_t max_evals, int32_t history, void* workspace,
                        size_t workspace_bytes, float* weight, float* bias, double* weight64, double* bias64, double* loss, double* grad_norm,
                        int32_t* evals, int32_t* status, void* stream) {
    return head_fit_call("ee_head_fit_distill", distilled(labels, teacher_logits, alpha, temperature), features, E, N, H, K, l2, gtol, max_evals,
                         history, workspace, workspace_bytes, weight, bias, weight64, bias64, loss, grad_norm, evals, status, stream);
}

int ee_debug_head_lossgrad(const float* features, const int64_t* labels, const double* theta64, int32_t E, int32_t N, int32_t H, int32_t K,
                           double l2, double* loss, double* grad, void* stream) {
    return head_lossgrad_call("ee_debug_head_lossgrad", false, labelled(labels), features, theta64, E, N, H, K, l2, loss, grad, stream);
}

int ee_debug_head_distill_lossgrad(const float* features, const float* teacher_logits, const int64_t* labels, const double* theta64, int32_t E,
                                   int32_t N, int32_t H, int32_t K, double alpha, double temperature, double l2, double* loss, double* grad,
                                   void* stream) {
    return head_lossgrad_call("ee_debug_head_distill_lossgrad", false, distilled(labels, teacher_logits, alpha, temperature), features, theta64, E, N,
                              H, K, l2, loss, grad, stream);
}

// ---- 2-way gate heads from CLS rows: the gate objective (include/mmee.h) on the labelled fit's kernels at K = 2 ---------------------------------
int ee_head_fit_gate(const float* features, const double* targets, int32_t E, int32_t N, int32_t H, double l2, double gtol, int32_t max_evals,
                     int32_t history, void* workspace, size_t workspace_bytes, float* weight, float* bias, double* weight64, double* bias64,
                     double* loss, double* grad_norm, int32_t* evals, int32_t* status, void* stream) {
    return head_fit_call("ee_head_fit_gate", gate(targets), features, E, N, H, 2, l2, gtol, max_evals, history, workspace, workspace_bytes, weight,
                         bias, weight64, bias64, loss, grad_norm, evals, status, stream);
}

int ee_debug_head_gate_lossgrad(const float* features, const double* targets, const double* theta64, int32_t E, int32_t N, int32_t H, double l2,
                                double* loss, double* grad, void* stream) {
    return head_lossgrad_call("ee_debug_head_gate_lossgrad", false, gate(targets), features, theta64, E, N, H, 2, l2, loss, grad, stream);
}

// ---- two-layer exit heads from CLS rows (mlp_head_fit.hip) -------------------------------------------------------------------------------
size_t ee_mlp_head_fit_workspace_bytes(int32_t E, int32_t N, int32_t H, int32_t K, int32_t history) {
    return no_workspace(E, N, H, K, history) ? 0 : mlp_head_fit_workspace_bytes(E, N, H, K, history, false);
}

int ee_mlp_head_fit(const float* features, const int64_t* labels, const double* theta0, int32_t E, int32_t N, int32_t H, int32_t K, double l2,
                    double gtol, int32_t max_evals, int32_t history, void* workspace, size_t workspace_bytes, float* dense_weight,
                    float* dense_bias, float* weight, float* bias, double* theta64, double* loss, double* grad_norm, int32_t* evals,
                    int32_t* status, void* stream) {
    return mlp_head_fit_call("ee_mlp_head_fit", labelled(labels), features, theta0, E, N, H, K, l2, gtol, max_evals, history, workspace,
                             workspace_bytes, dense_weight, dense_bias, weight, bias, theta64, loss, grad_norm, evals, status, stream);
}

int ee_mlp_head_fit_distill(const float* features, const float* teacher_logits, const int64_t* labels, const double* theta0, int32_t E, int32_t N,
                            int32_t H, int32_t K, double alpha, double temperature, double l2, double gtol, int32_t max_evals, int32_t history,
                            void* workspace, size_t workspace_bytes, float* dense_weight, float* dense_bias, float* weight, float* bias,
                            double* theta64, double* loss, double* grad_norm, int32_t* evals, int32_t* status, void* stream) {
    return mlp_head_fit_call("ee_mlp_head_fit_distill", distilled(labels, teacher_logits, alpha, temperature), features, theta0, E, N, H, K, l2, gtol,
                             max_evals, history, workspace, workspace_bytes, dense_weight, dense_bias, weight, bias, theta64, loss, grad_norm, evals,
                             status, stream);
}

int ee_debug_mlp_head_lossgrad(const float* features, const int64_t* labels, const double* theta64, int32_t E, int32_t N, int32_t H, int32_t K,
                               double l2, double* loss, double* grad, void* stream) {
    return head_lossgrad_call("ee_debug_mlp_head_lossgrad", true, labelled(labels), features, theta64, E, N, H, K, l2, loss, grad, stream);
}

int ee_debug_mlp_head_distill_lossgrad(const float* features, const float* teacher_logits, const int64_t* labels, const double* theta64, int32_t E,
                                       int32_t N, int32_t H, int32_t K, double alpha, double temperature, double l2, double* loss, double* grad,
                                       void* stream) {
    return head_lossgrad_call("ee_debug_mlp_head_distill_lossgrad", true, distilled(labels, teacher_logits, alpha, temperature), features, theta64, E,
                              N, H, K, l2, loss, grad, stream);
}

// ---- the head fits with sample weights: weights (E,N); teacher_logits NULL selects the labelled objective ------------------------------------
size_t ee_head_fit_weighted_workspace_bytes(int32_t E, int32_t N, int32_t H, int32_t K, int32_t history) {
    return no_workspace(E, N, H, K, history) ? 0 : head_fit_workspace_bytes(E, N, H, K, history, true);
}

int ee_head_fit_weighted(const float* features, const int64_t* labels, const float* teacher_logits, const float* weights, int32_t E, int32_t N,
                         int32_t H, int32_t K, double alpha, double temperature, double l2, double gtol, int32_t max_evals, int32_t history,
                         void* workspace, size_t workspace_bytes, float* weight, float* bias, double* weight64, double* bias64, double* loss,
                         double* grad_norm, int32_t* evals, int32_t* status, void* stream) {
    return head_fit_call("ee_head_fit_weighted", weighted(labels, teacher_logits, alpha, temperature, weights), features, E, N, H, K, l2, gtol,
                         max_evals, history, workspace, workspace_bytes, weight, bias, weight64, bias64, loss, grad_norm, evals, status, stream);
}

int ee_debug_head_weighted_lossgrad(const float* features, const int64_t* labels, const float* teacher_logits, const float* weights,
                                    const double* theta64, int32_t E, int32_t N, int32_t H, int32_t K, double alpha, double temperature, double l2,
                                    double* loss, double* grad, void* stream) {
    return head_lossgrad_call("ee_debug_head_weighted_lossgrad", false, weighted(labels, teacher_logits, alpha, temperature, weights), features,
                              theta64, E, N, H, K, l2, loss, grad, stream);
}

size_t ee_mlp_head_fit_weighted_workspace_bytes(int32_t E, int32_t N, int32_t H, int32_t K, int32_t history) {
    return no_workspace(E, N, H, K, history) ? 0 : mlp_head_fit_workspace_bytes(E, N, H, K, history, true);
}

int ee_mlp_head_fit_weighted(const float* features, const int64_t* labels, const float* teacher_logits, const float* weights, const double* theta0,
                             int32_t E, int32_t N, int32_t H, int32_t K, double alpha, double temperature, double l2, double gtol,
                             int32_t max_evals, int32_t history, void* workspace, size_t workspace_bytes, float* dense_weight, float* dense_bias,
                             float* weight, float* bias, double* theta64, double* loss, double* grad_norm, int32_t* evals, int32_t* status,
                             void* stream) {
    return mlp_head_fit_call("ee_mlp_head_fit_weighted", weighted(labels, teacher_logits, alpha, temperature, weights), features, theta0, E, N, H, K,
                             l2, gtol, max_evals, history, workspace, workspace_bytes, dense_weight, dense_bias, weight, bias, theta64, loss,
                             grad_norm, evals, status, stream);
}

int ee_debug_mlp_head_weighted_lossgrad(const float* features, const int64_t* labels, const float* teacher_logits, const float* weights,
                                        const double* theta64, int32_t E, int32_t N, int32_t H, int32_t K, double alpha, double temperature,
                                        double l2, double* loss, double* grad, void* stream) {
    return head_lossgrad_call("ee_debug_mlp_head_weighted_lossgrad", true, weighted(labels, teacher_logits, alpha, temperature, weights), features,
                              theta64, E, N, H, K, l2, loss, grad, stream);
}

// ---- two-layer 2-way gate heads: the gate objective on the two-layer fit's launches at K = 2, with or without sample weights ------------------
int ee_mlp_head_fit_gate(const float* features, const double* targets, const double* theta0, int32_t E, int32_t N, int32_t H, double l2, double gtol,
                         int32_t max_evals, int32_t history, void* workspace, size_t workspace_bytes, float* dense_weight, float* dense_bias,
                         float* weight, float* bias, double* theta64, double* loss, double* grad_norm, int32_t* evals, int32_t* status,
                         void* stream) {
    return mlp_head_fit_call("ee_mlp_head_fit_gate", gate(targets), features, theta0, E, N, H, 2, l2, gtol, max_evals, history, workspace,
                             workspace_bytes, dense_weight, dense_bias, weight, bias, theta64, loss, grad_norm, evals, status, stream);
}

int ee_mlp_head_fit_gate_weighted(const float* features, const double* targets, const float* weights, const double* theta0, int32_t E, int32_t N,
                                  int32_t H, double l2, double gtol, int32_t max_evals, int32_t history, void* workspace, size_t workspace_bytes,
                                  float* dense_weight, float* dense_bias, float* weight, float* bias, double* theta64, double* loss,
                                  double* grad_norm, int32_t* evals, int32_t* status, void* stream) {
    return mlp_head_fit_call("ee_mlp_head_fit_gate_weighted", weighted_gate(targets, weights), features, theta0, E, N, H, 2, l2, gtol, max_evals,
                             history, workspace, workspace_bytes, dense_weight, dense_bias, weight, bias, theta64, loss, grad_norm, evals, status,
                             stream);
}

int ee_debug_mlp_head_gate_lossgrad(const float* features, const double* targets, const double* theta64, int32_t E, int32_t N, int32_t H, double l2,
                                    double* loss, double* grad, void* stream) {
    return head_lossgrad_call("ee_debug_mlp_head_gate_lossgrad", true, gate(targets), features, theta64, E, N, H, 2, l2, loss, grad, stream);
}

int ee_debug_mlp_head_gate_weighted_lossgrad(const float* features, const double* targets, const float* weights, const double* theta64, int32_t E,
                                             int32_t N, int32_t H, double l2, double* loss, double* grad, void* stream) {
    return head_lossgrad_call("ee_debug_mlp_head_gate_weighted_lossgrad", true, weighted_gate(targets, weights), features, theta64, E, N, H, 2, l2,
                              loss, grad, stream);
}

// ---- the LTE classifier from CLS rows (lte_fit.hip) --------------------------------------------------------------------------------------
size_t ee_lte_fit_workspace_bytes(int32_t E, int32_t N, int32_t H, int32_t history) {
    if (E < 1 || N < 1 || H < 1 || history < 1) return 0;
    return lte_fit_workspace_bytes(E, N, H, history);
}

int ee_lte_fit(const float* features, const double* targets, const double* theta0, int32_t E, int32_t N, int32_t H, int32_t loss, double l2,
               double gtol, int32_t max_evals, int32_t history, void* workspace, size_t workspace_bytes, float* weight, float* bias,
               double* theta64, double* loss_out, double* grad_norm, int32_t* evals, int32_t* status, void* stream) {
    const char* who = "ee_lte_fit";
    if (!features || !targets || !workspace || !weight || !bias)
        return fail(nullptr, "%s: NULL argument (features, targets, workspace, weight and bias are required)", who);
    if (lte_rows_refuse(who, features, E, N, H) || lte_objective_refuse(who, loss, l2)) return 1;
    if (budget_refuse(who, gtol, max_evals, history, workspace_bytes, [&] { return lte_fit_workspace_bytes(E, N, H, history); })) return 1;
    if (!have_device(who)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const LteFitArgs a{{features, E, N, H, l2, gtol, max_evals, history, workspace, theta0, theta64, loss_out, grad_norm, evals, status},
                       targets, loss, weight, bias};
    return finish_call(who, launch_lte_fit(a, s), workspace, s, Objective::kLte, 0);
}

int ee_debug_lte_lossgrad(const float* features, const double* targets, const double* theta64, int32_t E, int32_t N, int32_t H, int32_t loss,
                          double l2, double* loss_out, double* grad, void* stream) {
    const char* who = "ee_debug_lte_lossgrad";
    if (!features || !targets || !theta64 || !loss_out || !grad) return fail(nullptr, "%s: NULL argument", who);
    if (lte_rows_refuse(who, features, E, N, H) || lte_objective_refuse(who, loss, l2)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return debug_lossgrad(who, lte_fit_partial_doubles(E, N, H), s, [&](double* partial, int* err) {
        launch_lte_lossgrad(features, targets, theta64, E, N, H, loss, l2, partial, err, loss_out, grad, s);
    }, Objective::kLte, 0);
}

int ee_lte_targets(const float* logits, const int64_t* labels, int32_t E, int32_t N, int32_t K, double* targets, void* stream) {
    const char* who = "ee_lte_targets";
    if (!logits || !labels || !targets) return fail(nullptr, "%s: NULL argument", who);
    if (E < 1 || N < 1 || K < 1) return fail(nullptr, "%s: (E, N, K) = (%d, %d, %d), need each >= 1", who, E, N, K);
    if (!have_device(who)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Scratch sc;
    int* err_dev = nullptr;
    if (!sc.get(&err_dev, 1)) return fail(nullptr, "%s: hipMalloc of the error word failed", who);
    launch_lte_targets(logits, reinterpret_cast<const long long*>(labels), E, N, K, targets, err_dev, s);
    return finish_call(who, true, err_dev, s, Objective::kLteTargets, K);
}

// ---- the exit ensemble's weights from a dumped array (ensemble_fit.hip) ---------------------------------------------------------------------
static int ensemble_fit_refuse(const char* who, int32_t E1, int32_t N, int32_t K, double l2) {
    if (E1 < 1 || E1 > MMEE_MAX_ENCODER_EXITS + 4) return fail(nullptr, "%s: E1 = %d, need 1 <= E1 <= %d", who, E1, MMEE_MAX_ENCODER_EXITS + 4);
    if (N < 1) return fail(nullptr, "%s: N = %d, need N >= 1", who, N);
    if (K < 2 || K > 64) return fail(nullptr, "%s: K = %d, need 2 <= K <= 64 (ee_create's limit)", who, K);
    if (!ensemble_fit_supports(E1, K))
        return fail(nullptr, "%s: (E1, K) = (%d, %d): one document's rows and an exit-by-parameter table, E1 (3 K + E1 + 2) = %lld doubles, leave the 7680 "
                             "doubles of LDS the row kernel takes", who, E1, K, (long long)E1 * (3 * K + E1 + 2));
    if (!(l2 > 0.0)) return fail(nullptr, "%s: l2 = %g, need l2 > 0 (the objective is strongly convex only then)", who, l2);
    return 0;
}

size_t ee_ensemble_fit_workspace_bytes(int32_t E1, int32_t N, int32_t K, int32_t history) {
    if (E1 < 1 || N < 1 || K < 1 || history < 1) return 0;
    return ensemble_fit_workspace_bytes(E1, N, K, history);
}

int ee_ensemble_fit(const double* logits, const int64_t* labels, const double* w0, const double* b0, int32_t E1, int32_t N, int32_t K, double l2,
                    double gtol, int32_t max_evals, int32_t history, void* workspace, size_t workspace_bytes, double* w, double* b, double* loss,
                    double* grad_norm, int32_t* evals, int32_t* status, void* stream) {
    const char* who = "ee_ensemble_fit";
    if (!logits || !labels || !workspace || !w || !b) return fail(nullptr, "%s: NULL argument (logits, labels, workspace, w and b are required)", who);
    if (ensemble_fit_refuse(who, E1, N, K, l2)) return 1;
    if (budget_refuse(who, gtol, max_evals, history, workspace_bytes, [&] { return ensemble_fit_workspace_bytes(E1, N, K, history); })) return 1;
    if (!have_device(who)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const EnsembleFitArgs a{{nullptr, E1, N, 0, l2, gtol, max_evals, history, workspace, nullptr, nullptr, loss, grad_norm, evals, status},
                            logits, int64_labels(labels), w0, b0, K, w, b};
    return finish_call(who, launch_ensemble_fit(a, s), workspace, s, Objective::kEnsemble, K);
}

int ee_lte_scores(const float* features, const float* weight, const float* bias, int32_t E, int32_t N, int32_t H, double* scores, void* stream) {
    const char* who = "ee_lte_scores";
    if (!features || !weight || !bias || !scores) return fail(nullptr, "%s: NULL argument", who);
    if ((long long)E * N < 1 || E < 1 || N < 1) return fail(nullptr, "%s: (E, N) = (%d, %d), need each >= 1", who, E, N);
    if (H < 4 || H > kHeadFitMaxH || H % 4 != 0) return fail(nullptr, "%s: H = %d, need 4 <= H <= %d and H %% 4 == 0", who, H, kHeadFitMaxH);
    if (reinterpret_cast<uintptr_t>(features) % 16 != 0 || reinterpret_cast<uintptr_t>(weight) % 16 != 0)
        return fail(nullptr, "%s: features and weight must be 16-byte aligned", who);
    if (!have_device(who)) return 1;
    launch_lte_scores(features, weight, bias, E, N, H, scores, reinterpret_cast<hipStream_t>(stream));
    return launch_status(nullptr, who);
}

}  // extern "C"
