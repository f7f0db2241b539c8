/*
 * mmee.h — C-ABI of the MI355X-native early-exit document-classification path (libmmee_hip.so).
 *
 * The reference (Jordy-VL/multi-modal-early-exit) is pure Python and has no FFI layer; its boundary for this path is
 * two Python call surfaces.  Each entry point below names the reference interface it replaces:
 *
 *   ee_create / ee_load_tensor / ee_finalize   <- configs.build_model -> LayoutLMv3EEForSequenceClassification
 *                                                 .from_pretrained (EE/configs.py:389-411; model tree
 *                                                 EE/models/LayoutLMv3.py:308-356, 669-694).  Tensors are addressed by
 *                                                 their HF parameter names (EE/models/
 *                                                 EELayoutLM_exit_named_parameters-wotherexits.json).
 *   ee_forward                                  <- LayoutLMv3EEForSequenceClassification.forward
 *                                                 (EE/models/LayoutLMv3.py:696-749, 871-896) + the harness loop
 *                                                 utils.get_logits (EE/utils.py:169-193) + the early-exit decision of
 *                                                 Policy.max_confidence_global_thresholding_policy /
 *                                                 accuracy_calibration_heuristic (EE/policy.py:12-111) fused in,
 *                                                 per-exit temperature of EE/generic_scaling.py:54-61 applied first.
 *   ee_embedding_inputs                         <- the three pooled rows the embedding-level exit heads read, `visual_embeddings.mean(1)`,
 *                                                 `embedding_output.mean(1)` and `LayerNorm(cat).mean(1)` (EE/models/LayoutLMv3.py:466, 520, 582),
 *                                                 without the encoder behind them: the training set of those heads.
 *   ee_forward_vision                           <- no counterpart: the forward from the pixels alone up to the vision_avg exit (EE/models/LayoutLMv3.py:
 *                                                 465-483), phase 1 of a vision-first call -- what the reference prices with --benchmark_OCR
 *                                                 (EE/utils.py:127, 176) and never collects; definition below.
 *   ee_policy_scan                              <- Policy.* on a dumped (E+1, N, K) logits array (EE/policy.py:28-45,
 *                                                 87-104; called from EE/eval.py:87-98).
 *   ee_threshold_sweep                          <- thresh.opt1 / large_scale.opt0_2D vectorised exit-index search
 *   ee_threshold_search                         <- large_scale.generate_thresholds + the sweep + the Pareto front the reference stops short of
 *                                                 (EE/thresh.py:184-215, EE/large_scale.py:68-84).
 *   ee_threshold_search_cost                    <- the same search against the reference's efficiency figures: per-exit cost weighted by the exit
 *                                                 distribution ("GFLOPs reduction", "Latency reduction": EE/eval.py:62-84, EE/analysis.py:29-102).
 *   ee_threshold_refine                         <- no counterpart: a coordinate search on the same percentile grid that improves a search's vectors where
 *                                                 the grid (P^(E1-1) vectors) cannot be enumerated; semantics below.
 *   ee_set_patience / ee_patience_scan /        <- EarlyExitInference.PATIENCE, declared by the reference (EE/models/EE_modules.py:
 *   ee_patience_sweep                              123-124, PABEE: Zhou et al., NeurIPS 2020) but not implemented there; semantics below.
 *   ee_set_exit_rule / ee_set_patience_vector / <- no counterpart: the reference implements neither rule.  Patient-and-confident (PCEE-BERT, Zhang et al.,
 *   ee_rule_scan / ee_rule_sweep                   NAACL Findings 2022) and PABEE's patience-or-threshold hybrid, on the events and counters above; semantics below.
 *   ee_config.use_lte / ee_lte_scan             <- learning-to-exit (BERxiT's LTE): encoder.lte_classifier = nn.Linear(hidden_size, 1) + sigmoid on
 *                                                  the CLS row after every exit layer, `lte_output < lte_th[i]` leaves (EE/models/LayoutLMv3.py:
 *                                                  140-149, 229-268; switched on by EE_config["use_lte"]); semantics below.
 *
 * Conventions: every function returns 0 on success, non-zero on error (message via ee_last_error).  All pointers
 * marked "dev" are device (HBM) pointers borrowed from the caller for the duration of the enqueued work; kernels are
 * enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream); no call synchronises with the host
 * unless its comment says so.  One handle per device; a handle is not thread-safe.
 */
#ifndef MMEE_H
#define MMEE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMEE_ABI_VERSION 4
#define MMEE_MAX_ENCODER_EXITS 64

/* embedding-level exits, in the order the reference evaluates them (EE/models/LayoutLMv3.py:465-605) */
enum { MMEE_EXIT_VISION_AVG = 0, MMEE_EXIT_TEXT_AVG = 1, MMEE_EXIT_TEXT_VISUAL_CONCAT = 2 };
/* encoder_layer_strategy (EE/models/EE_modules.py:167-172) */
enum { MMEE_STRATEGY_RAMP = 0, MMEE_STRATEGY_GATE = 1 };
/* inference_strategy (EE/models/EE_modules.py:116-146): max_confidence exits on crit > thr, entropy on crit < thr, patience and margin as below */
enum { MMEE_CRIT_MAX_CONFIDENCE = 0, MMEE_CRIT_ENTROPY = 1, MMEE_CRIT_PATIENCE = 2, MMEE_CRIT_MARGIN = 3, MMEE_CRIT_GATE = 4 };
/*
 * MMEE_CRIT_GATE (the gate decides).  The reference's design note says what a gate head is for -- "binary gates on some encoder layers - if binary
 * gate confidence > threshold, exit" (EE/models/EE_modules.py:21-31) -- and trains gates with BCEWithLogitsLoss against the one-hot of
 * "classifier(gate input) is right here" (EE/models/LayoutLMv3.py:764-781), but its evaluation never lets one decide: under the gate strategy the
 * policy thresholds the max-softmax of classifier(gate input) (EE/utils.py:183-188), which MMEE_CRIT_MAX_CONFIDENCE on a gate handle still does.
 * Valid only with MMEE_STRATEGY_GATE.  Exit e below the final one has gate logits h = (h0, h1): float32, the head's raw output, exactly what
 * out_head_logits holds.  Column 1 is "correctly gated" (y[range, correctly_gated.long()] = 1, LayoutLMv3.py:772-773).  The gate score is
 *     g_e = 1 / (1 + exp((double)h0 - (double)h1))   in float64,
 * the 2-way softmax's probability of column 1 (h0 == h1: exactly 0.5; exp overflowing: exactly 0; exp underflowing: exactly 1).  Exit e fires
 * when g_e > thresholds[e]: strict, as under max_confidence; a NaN score never fires; if nothing fires the document leaves at the final exit.
 * temperatures[e] keeps scaling the policy logits that are written out, exactly as under every other criterion, and does not enter g_e: a
 * temperature on a two-way score only moves the threshold, and the threshold is already per exit.
 * What leaves is unchanged: the scaled classifier(gate input) row.  out_conf, out_all_crit and out_head_crit carry g_e (rounded once to float32)
 * at exits below the final one; at the final exit, which has no gate and where everybody leaves, out_conf and out_all_crit carry the max-softmax
 * of the scaled final logits.  Embedding-level exits have gate heads like any other exit and behave the same.  MMEE_RULE_STREAK / MMEE_RULE_EITHER
 * take g_e > thr_e as their event.  MMEE_FLAG_NO_EXIT, compaction, probes, MMEE_FLAG_LOW_LATENCY, the result stream and captured graphs (the
 * criterion is bound at capture) are as under the other threshold criteria.  The decision reads the two gate logits and nothing else.
 * Cost: the gate head's launches (dense layer of a 2-layer head, output projection) at every exit, which a gate handle under another criterion
 * issues only when out_head_logits / out_head_crit are asked for.  A handle that does not select the criterion launches what it launched before.
 * Refused, each with a message: the criterion on a MMEE_STRATEGY_RAMP handle (ee_create and ee_set_criterion) and together with use_lte.
 * On dumped arrays: ee_gate_table, ee_gate_scan.
 */
/*
 * MMEE_CRIT_MARGIN (top-1 minus top-2 softmax probability; the third confidence scoring function the reference names, CSF_dict in
 * EE/large_scale.py:12-18 and EE/thresh.py:55-61, whose own top12_margin_np subtracts the two SMALLEST raw logits and is never called: this
 * text, not that function, is the specification).  For one document at one exit, z the float32 policy logits and T the exit's temperature:
 *     x_k = (double)z_k / T,   m1 = max_k x_k,   m2 = the second largest value counting multiplicity (a maximum attained twice: m2 = m1),
 *     S = sum_k exp(x_k - m1) added in label order k = 0 .. K-1,   margin = (1 - exp(m2 - m1)) / S   in float64.
 * K = 1: the second probability is 0 and margin = 1.0.  In this form the margin is >= 0 exactly and exactly 0 on a tie; it lies in [0, 1] like the
 * max-softmax, so thresholds stay comparable.  The test is margin > thr, strict (higher is surer, as for max_confidence); a NaN criterion never
 * fires; if nothing fires the document leaves at the final exit.  The float32 form -- the same expression in float32 on the head's own logits, no
 * temperature -- is what the model reports as exit_states[j][1] and the handle as out_head_crit.  Everything else is as for the two other threshold
 * criteria: per-exit thresholds and temperatures, MMEE_FLAG_NO_EXIT, MMEE_RULE_STREAK / MMEE_RULE_EITHER with the margin test as their event,
 * use_lte (the criterion then only feeds out_head_crit), captured graphs (the criterion is bound at capture; thresholds and temperatures are read
 * from the vector of each launch).  It adds no launch: a margin forward issues exactly the launches of its max_confidence twin.
 */
/*
 * MMEE_CRIT_PATIENCE (patience-based early exit, PABEE).  Exits e = 0 .. E in the path's order (embedding exits vision, text, concat, then
 * encoder exits ascending, then the final classifier).  p_e(n) = argmax of document n's policy logits at exit e, taken on exactly the float32
 * values written to out_all_logits, (float)((double)z / T_e) (ramps: the head's logits; gates: classifier(gate input)); ties resolve to the
 * first maximal index (numpy argmax).  Run counter: c_0 = 0; c_e = c_{e-1} + 1 if p_e == p_{e-1}, else 0.  Document n leaves at the first e
 * with c_e >= t, or at E if there is none (t > E: every document runs to the final exit).  The patience t >= 1 is set by ee_set_patience, or per
 * exit by ee_set_patience_vector (c_e >= t_e).
 * Outputs keep their contract: out_logits = the scaled logits of the chosen exit, out_conf = the float64 max-softmax of those scaled logits
 * (rounded to float32), out_all_crit (dump-all) = the same max-softmax at every exit, out_head_crit = the max-softmax of the raw head logits.
 * Thresholds are ignored (may be NULL); temperatures act only through the scaled logits.
 */
/*
 * ee_config.use_lte (learning-to-exit, LTE).  The exit decision is a learned gate instead of a criterion on the logits.  Two more parameters
 * are expected, after all the others: layoutlmv3.encoder.lte_classifier.weight (1, H) and layoutlmv3.encoder.lte_classifier.bias (1,).
 * Score of encoder exit e and of the final classifier:  u_e(n) = 1 / (1 + exp(-(w . x_e(n) + b))),  x_e(n) = the float32 CLS row leaving that
 * layer, i.e. the row the exit's head reads and out_hidden_cls reports (split precision: rebuilt exactly as (hi + lo) / 16).  Arithmetic is
 * float64 throughout: the float32 inputs widened, a fixed summation order (lane l of one wave sums columns 4l + 256k + j in the order k, j;
 * the 64 lane sums are then added by a butterfly) that does not depend on which documents share the launch, exp and the comparison in float64;
 * the stored value is rounded to float32.  Document n leaves at the first encoder exit e with u_e(n) < thresholds[e] (strict, as
 * `lte_output < self.lte_th[i]`), else at the final exit.  Embedding-level exits have no CLS row: they are evaluated (their rows appear in the
 * dump-all outputs), never release anybody, and their criterion row holds 1.0f.  MMEE_FLAG_NO_EXIT and the final exit behave as without LTE.
 * out_all_crit[e] and out_conf carry the LTE score ("the criterion value, lower is surer", as under entropy); out_logits, out_all_logits,
 * out_head_logits and out_head_crit are exactly what they are without use_lte (out_head_crit stays ee_config.criterion on the raw head
 * logits); temperatures act on the returned logits only; the score does not look at the head (ramps, gates, 1- and 2-layer heads).
 * Refused: use_lte with MMEE_CRIT_PATIENCE (at ee_create or through ee_set_criterion) and with MMEE_ARCH_BEIT.  Bound at ee_create: captured
 * graphs keep reading the thresholds from the device vector of each ee_graph_launch.
 */
/*
 * Exit rules (ee_set_exit_rule): what a handle makes of its criterion / LTE test and PABEE's counter together.  Exits e = 0 .. E in the path's
 * order, E1 = E + 1.  A handle keeps its criterion and its use_lte setting.
 *   Event of exit e: today's test, unchanged.  max_confidence, margin: f_e = crit_e > thr_e; entropy: f_e = crit_e < thr_e; use_lte: f_e = u_e < thr_e
 *   (embedding exits never fire under LTE).  All compares strict; crit_e is the float64 criterion on the scaled logits, u_e the float64 score.
 *   Agreement: PABEE's counter exactly as under MMEE_CRIT_PATIENCE: c_0 = 0, c_e = c_{e-1} + 1 if argmax z_e == argmax z_{e-1}, else 0, the
 *   argmax taken on the scaled float32 logits as written out, the first maximum winning.
 *   Patience: a per-exit vector t_e >= 1, e = 0 .. E (ee_set_patience_vector; the final exit's entry is ignored).  ee_set_patience(h, t) is
 *   that value at every exit.
 *   MMEE_RULE_PLAIN  = 0  the test alone, as before: leave at the first e with f_e.  The default.
 *   MMEE_RULE_STREAK = 1  patient and confident (PCEE): s_e = f_e ? s_{e-1} + 1 : 0 with s_{-1} = 0; leave at the first e with s_e >= t_e.
 *                         With t = 1 this is MMEE_RULE_PLAIN exactly.
 *   MMEE_RULE_EITHER = 2  patience or threshold: leave at the first e with f_e or c_e >= t_e: the minimum of the PLAIN exit and the PABEE exit.
 * If no exit qualifies the document leaves at the final exit E.  MMEE_FLAG_NO_EXIT and the final exit behave as without a rule; every output
 * carries what it carries without one (out_conf: the criterion or LTE score of the exit the document leaves at): only WHICH exit changes.
 * Per document the decide kernels keep the streak (STREAK) or (previous argmax, c_e) (EITHER) where MMEE_CRIT_PATIENCE keeps its state: by the
 * document's slot in the call, rewritten at exit 0, nothing carried from one forward to the next, no launch added.
 * Refused, each with a message: a rule other than PLAIN under MMEE_CRIT_PATIENCE (PABEE has no threshold event; ee_set_exit_rule and
 * ee_set_criterion both check), a STREAK or EITHER forward without a patience set, any patience entry below 1, a patience vector whose length
 * is not E + 1.  MMEE_CRIT_PATIENCE itself also takes the vector: c_e >= t_e (per-exit patience).
 */
enum { MMEE_RULE_PLAIN = 0, MMEE_RULE_STREAK = 1, MMEE_RULE_EITHER = 2 };
/*
 * Budgeted exits (ee_set_quotas): every exit releases the most confident documents of THIS CALL, a chosen number of them -- the budgeted batch
 * classification setting of MSDNet (Huang et al., ICLR 2018).  THE definition (the forward, ee_quota_scan and the stand-alone hook refer to it).
 * Exit e below the final one has a quota q_e >= 0, an integer number of documents of this call.  For the n documents that reach exit e:
 *   c_i    the float64 criterion the decide kernel computes for active document i without quotas: the criterion of the scaled policy row,
 *          temperature included; under MMEE_CRIT_GATE the gate score of the document's two gate logits; with an ensemble set (ee_set_ensemble)
 *          the criterion of the ensemble row y_e.
 *   s_i    = sign * c_i, sign = -1 for MMEE_CRIT_ENTROPY and +1 otherwise: larger is more confident under every criterion.
 *   i PRECEDES j when s_i > s_j, or s_i == s_j and i's original slot (its index in the call) is lower.  A NaN criterion precedes nothing and
 *          is preceded by every number; NaNs order among themselves by slot.  (-0.0 == +0.0: a tie.)
 *   rank_i = the number of active documents that precede i: a permutation of 0 .. n-1.
 *   MMEE_QUOTA_EXACT    = 1  i leaves iff rank_i < q_e.  Thresholds are not read and may be NULL.  If fewer than q_e documents reach the exit
 *                            all of them leave and the later stages run empty, as in a forward at threshold 0.
 *   MMEE_QUOTA_AT_LEAST = 2  i leaves iff the threshold test fires (strict, as without quotas) or rank_i < q_e.  Firing is monotone in s, so
 *                            this is "the top max(q_e, #fired)": compute has an upper bound that holds for any data, and confident documents
 *                            still leave early.
 * What leaves is what leaves without quotas: the scaled policy row, confidence = (float)c_i.  The final exit takes everybody; under
 * MMEE_FLAG_NO_EXIT quotas are ignored like thresholds; the documents that stay keep their order (compaction stays stable).
 * A document's logits still do not depend on its batch mates.  Only WHERE IT LEAVES does: this is the first decision of the library with that
 * property, and it is so by definition -- the same page may leave at another exit in another batch, with that exit's logits.
 * Under MMEE_QUOTA_EXACT the size of every stage is known before the call, n_{e+1} = max(0, n_e - q_e), whatever the pages are: so are the
 * FLOPs of the forward, the chunk sizes of the result stream and the work of a captured graph.
 * Cost: two launches per exit below the final one (exit_quota_crit_kernel writes c_i, exit_quota_rank_kernel counts rank_i: 256 documents per
 * workgroup, the stage tiled through LDS, O(n^2) integer compares, deterministic to the bit) and the QUOTA form of the decide kernel in place
 * of the plain one; none at the final exit or in dump-all calls; a handle without quotas issues the launches it always did.
 * Refused, each with a message: MMEE_CRIT_PATIENCE, MMEE_RULE_STREAK / MMEE_RULE_EITHER and use_lte handles (their decisions carry
 * per-document state or another score; no rank is defined for them) -- by ee_set_quotas, and by ee_set_criterion / ee_set_exit_rule while
 * quotas are set.  Not built: quotas across micro-batches or ranks (each would rank alone), an "at most" mode.
 */
enum { MMEE_QUOTA_OFF = 0, MMEE_QUOTA_EXACT = 1, MMEE_QUOTA_AT_LEAST = 2 };
/*
 * Model cascades (ee_cascade_select / _gather / _merge; the Python CascadeEngine): the cheap model runs on every document and passes on only
 * the ones it is unsure about -- CascadeBERT (Li et al., Findings of EMNLP 2021).  THE definition (the three entry points and CascadeEngine
 * refer to it).
 * Stages s = 0 .. S-1, S >= 2, each a finalised handle on the same device with the same num_labels K.  Stage s has E1_s = E_s + 1 exits; its
 * offset is off_s = sum_{r < s} E1_r, the GLOBAL exit index of its local exit e is off_s + e, and SE1 = sum_s E1_s.
 * A stage runs its ordinary ee_forward on its documents, under its own thresholds, temperatures, criterion, rule, ensemble and quotas: that
 * code is not touched, and a handle outside a cascade issues the launches it always did.
 * A document of stage s < S-1 is DEFERRED when it left at the stage's final exit (exit_layer == E_s) and the deferral criterion does not fire
 * on the row the stage delivered for it:
 *   c      the criterion, in float64, of (double) of the delivered float32 logits row (temperature already applied by the forward), by the
 *          functions the criterion table of ee_csf_table is made of: the max-softmax 1 / sum_k exp(z_k - m) with m the first maximum and the
 *          sum in label order, the entropy log A - B / A, the margin of MMEE_CRIT_MARGIN.
 *   the document STAYS iff c passes thresholds_s[E_s] in the criterion's direction, strictly ('>'; entropy '<'): a NaN row never fires and is
 *          deferred.  The threshold is the stage's own final entry, which ee_forward carries and never reads.
 *   the criterion is the handle's own threshold criterion; handles under MMEE_CRIT_GATE, MMEE_CRIT_PATIENCE or use_lte take
 *          MMEE_CRIT_MAX_CONFIDENCE, which is what they report at the final exit anyway.  A caller may override it per stage.
 * Documents that left before the final exit are never deferred; the last stage defers nobody.
 * The deferred documents keep their order (ascending original slot) and are stage s+1's batch; their inputs are rows of the caller's arrays
 * for that stage.  A document's result is the result of the last stage it ran in: logits and confidence are that stage's, exit_layer is the
 * global index, stage the stage index.
 * The equivalence that makes the dumped-array tools apply.  When every stage is under one and the same plain threshold criterion, all
 * temperatures are 1 and the early-exit rows are the dump-all rows bit for bit (the K | V probe; not MMEE_FLAG_XPROBE), let D be the
 * (SE1, B, K) concatenation of the stages' dump-all out_all_logits over all B documents and t the (SE1) concatenation of their thresholds.
 * Then ee_criterion_scan(D, t, criterion) returns the cascade's global exit_layer for every document whose criteria are not within rounding
 * of a threshold: a cascade is ONE early-exit model whose exit list is the concatenation of its stages' exit lists, and ee_csf_table, the
 * scans, the sweeps, the searches (also with a cost), ee_threshold_refine, ee_exit_metrics and ee_quota_scan take D unchanged.  Choosing the
 * deferral threshold is the search that already exists.
 * Cost per stage boundary: three launches (select; gather, skipped when the caller supplies the deferred inputs itself; merge) and ONE host
 * read of 4 bytes, the number of deferred documents, because the next ee_forward takes its batch size by value.  Nothing else crosses.
 * Not built: a deferral quota (when fewer documents reach the final exit than the quota the count falls short: it needs a forward that takes
 * its batch size from the device), streaming across stages, captured cascades (a later stage's batch size depends on the data), stages on
 * different GPUs, a deferral that reads anything but the delivered row.
 */
/*
 * Audited exits (ee_set_audit; EarlyExitEngine.set_audit, audit.py): a deterministic, content-blind sample of the call's documents gets its
 * result exactly where and as the plain forward gives it, and then runs on to the final exit as a shadow, so that its columns of the
 * out_all_* / out_head_* arrays come back complete: an unbiased sampled dump-all table of the traffic that was served, from which the
 * agreement of the early answer with the full model's can be counted -- the consistency that CATs (Schuster et al., EMNLP 2021) and "Fast
 * yet Safe" (Jazbec et al., NeurIPS 2024) control.  THE definition (the decide kernels, ee_audit_selected, the stand-alone hook and the Python
 * mask refer to it).
 * Selection.  slot = the document's index in the caller's batch: its index in the call (doc_orig) plus the handle's slot_base.  In arithmetic
 * mod 2^32:
 *   x = (uint32)slot * 0x9E3779B1u ^ seed;
 *   x ^= x >> 16;  x *= 0x85EBCA6Bu;  x ^= x >> 13;  x *= 0xC2B2AE35u;  x ^= x >> 16;        (murmur3's fmix32)
 * The document is audited iff (uint64)x < cut, cut = floor(fraction 2^32 + 0.5) in [0, 2^32]: fraction 1 selects everybody, cut 0 is "audit
 * off".  (seed 0, slot 0) hashes to 0 and is selected under every cut > 0: callers vary the seed per call.  One __host__ __device__ function
 * (audit_selected, csrc/mmee_kernels.h) is the test of the kernels and of ee_audit_selected.
 * Semantics.  The audit is on when cut > 0 and the call is not MMEE_FLAG_NO_EXIT.  At an exit below the final one, a document whose decision
 * is `leave` -- under whatever criterion, rule, learning-to-exit score or ensemble the handle runs -- and which is selected gets out_logits /
 * out_exit / out_conf written exactly as without the audit, is marked delivered, and is KEPT in the next stage.  A delivered document at a
 * later exit always stays, never writes out_logits / out_exit / out_conf again (the final exit included), still writes its out_all_* /
 * out_head_* rows and still updates its patience / streak / ensemble state like any active document.  Documents that are not selected behave
 * exactly as without the audit.  Hence out_logits, out_exit and out_conf of an audited call are bit for bit those of the same call without
 * the audit.
 * Compute.  The documents active at exit e are #{exit_i >= e} + #{selected_i and exit_i < e}; ee_last_stage_counts and ee_last_flops report
 * that number: it is what ran.  With share p a forward costs about p x (dump-all - early-exit) more.
 * Cost in launches: none.  The AUDIT forms of the seven decide kernels (threshold, patience, LTE, streak, either, LTE + streak, LTE +
 * either) run in place of the plain ones at every exit of an audited call; the delivered marks live by original slot in max_docs ints of the
 * handle and are written, not read, at the call's first exit, so no launch zeroes them.  A handle without an audit issues the launches it
 * always did and returns the same bits.
 * Refused, each with a message: together with quotas, in either order (a rank would count the shadows, and n_{e+1} would no longer be
 * n_e - q_e); MMEE_FLAG_STREAM_RESULTS (emit_leavers infers who left from stage membership); ee_graph_capture while an audit is set and
 * ee_set_audit while graphs are held (the seed is per call and by value); cut > 2^32; slot_base < 0.  The Python CascadeEngine refuses a
 * stage handle with an audit set.
 * Not built: audit under quotas, with the result stream, in captured graphs, on cascade stages; a per-exit share; a selection that depends
 * on content; a confidence bound on the agreement rate (the audit counts; the bound, and thresholds certified on the sampled table, are
 * ee_binomial_bounds and ee_risk_control, "Risk control" below).
 */
/*
 * Online exit control (ee_set_controller; EarlyExitEngine.set_controller, risk.rolling_control): the thresholds of a handle follow the
 * disagreement its own audit observes, between forwards, on the device.  Rolling risk control -- Gibbs and Candes, "Adaptive conformal
 * inference under distribution shift" (NeurIPS 2021); Feldman, Ringel, Bates and Romano, "Achieving risk control in online learning settings"
 * (TMLR 2023).  THE definition (the forward's two launches, ee_rolling_control, the two stand-alone hooks and the numpy restatement of
 * tests/controller_ref.py refer to it).
 * A controller has a path[V][E1] of float64 threshold vectors, V >= 2, ordered from the most conservative (index 0) to the most aggressive (the
 * order of ee_risk_control's candidates); a position p (float64), started at p0 in [0, V - 1]; a risk level alpha in (0, 1); a step gamma > 0;
 * a base seed.  It needs an audit (ee_set_audit with cut > 0).
 * Thresholds of a call, computed on the device from p.  p < 0: every exit below the final one gets the value that never fires, +inf under the
 * `>` criteria and -inf under entropy.  Otherwise p' = min(p, V - 1), i = min(floor(p'), V - 2), t = p' - i and
 *   thr[e] = a + (b - a) t,   a = path[i][e], b = path[i + 1][e],
 * the product rounded before the add (no fused multiply-add).  thr[E1 - 1] is path[i][E1 - 1] (path[0]'s when p < 0); no forward reads it.
 * Loss of a call of B documents, all integers.  sampled = #{slot < B : selected(cut, seed_t, slot + slot_base)} by the audit's hash.
 * disagree = the shadows -- documents delivered below the final exit that ran on -- whose delivered row out_logits[slot], the float32 row as
 * written, has another argmax than their final-exit policy row, the row the final exit's decide launch read, scaled as that launch writes it.
 * The argmax takes the lowest index on ties; a row with a NaN counts as K - 1.  delivered[e] and agree[e] count the same per exit, by
 * out_exit[slot]: the numbers of audit.consistency, without the dump of every exit.
 * Step, by one thread.  sampled == 0: nothing changes.  Otherwise p <- min(V - 1, p - gamma ((double)disagree / (double)sampled - alpha)), the
 * product rounded before the subtraction.
 * Seed.  Call number t = 0, 1, ... since ee_set_controller audits under seed (seed + t) mod 2^32; the seed of ee_set_audit is not read.
 * Promise.  With l_t = disagree / sampled of the calls that sampled anybody, for every T:  sum_{t <= T} (l_t - alpha) <= p0 / gamma + 1 - alpha.
 * Why: while p < 0 nobody leaves early, so the loss is 0 and p rises by gamma alpha; from p >= 0 one step lowers p by at most gamma (1 - alpha);
 * so p >= -gamma (1 - alpha) always, and p_T = p0 - gamma sum (l_t - alpha) unless the clamp at V - 1 made it smaller still.  It is an
 * inequality on the observed sequence: it holds for any data, in any order, with no exchangeability assumed.
 * Limit.  The bound is on the AUDITED estimate: the true disagreement rate follows only up to the sampling error of the audit, and nothing
 * is promised for a single call.
 * Forward.  While a controller is set, every decide launch of a call that is not dump-all is the AUDIT form and reads its threshold from the
 * handle's device vector; behind the final exit run audit_tally_kernel and controller_step_kernel (profile role "controller"), which leave
 * the next call's thresholds in that vector and one row in a device ring log.  No host step, no synchronisation.  Dump-all calls and
 * MMEE_FLAG_NO_EXIT calls ignore the controller: no step is taken and no seed is used.  A handle without a controller issues the launches it
 * issued before and returns the same bits.
 * Log row, controller_log_words = 5 + 2 (E1 - 1) + E1 64-bit words: call index, p before, p after (float64 bits), sampled, disagree,
 * delivered[E1 - 1], agree[E1 - 1], thresholds[E1] the call ran with (float64 bits).
 * Allowed unchanged: the four threshold criteria (gate included), temperatures, an ensemble (the tally reads the row the decision read),
 * MMEE_FLAG_LOW_LATENCY, ramp, gate and DiT handles.
 * Refused, each with a message and nothing changed: no audit set; MMEE_CRIT_PATIENCE, an exit rule other than MMEE_RULE_PLAIN, use_lte; quotas (by
 * ee_set_quotas itself: a controller needs an audit, and an audit and quotas refuse each other);
 * MMEE_FLAG_STREAM_RESULTS and ee_graph_capture while a controller is set, ee_set_controller while graphs are held; a non-NULL thresholds
 * argument or a NULL out_logits on a controlled ee_forward; V < 2, E1 < 2 or E1 > 64, alpha outside (0, 1), gamma <= 0 or not finite, p0
 * outside [0, V - 1], a path entry that is not finite; ee_set_audit(h, 0, ...), a change of criterion and a non-plain exit rule while a
 * controller is set.  The Python MicroBatchedEngine and CascadeEngine refuse a controlled handle.
 * Not built: controllers under captured graphs, with the result stream, over micro-batches, on cascade stages; losses other than consistency
 * in the forward (ee_rolling_control takes any 0 / 1 table); a per-exit (conditional) risk; step-size schedules; one controller shared across
 * ranks.
 */
/*
 * Deadline exits (ee_set_deadline; EarlyExitEngine.set_deadline, request_cut, deadline_log): anytime prediction -- Huang et al., "Multi-scale
 * dense networks for resource efficient image classification" (ICLR 2018) -- next to the budgeted batch setting of the quotas: a clock on the
 * device, or the host, releases everybody who is still in the batch at the next exit.  THE definition (the forward's launches, the
 * stand-alone hook ee_debug_deadline_check and the numpy restatement of tests/deadline_ref.py refer to it).
 * A handle may carry a deadline: a budget in ns and eta_ns[E1], uint64.  A deadline call is an eager ee_forward on such a handle without
 * MMEE_FLAG_NO_EXIT; the handle numbers them k = 1, 2, ... over its lifetime.
 * Begin.  The call's first launch, deadline_begin_kernel, reads t0 from the 100 MHz counter s_memrealtime (one counter chip-wide: measured,
 * profiles/deadline.txt), copies the call's thresholds -- a kernel argument, E1 <= 64 -- into the device vector dl_thr[E1] and marks "no cut".
 * Every decide launch of the call reads its threshold at dl_thr[exit].
 * Check.  In front of the decide launch of every exit e runs deadline_check_kernel, one workgroup of one wave.  elapsed = ((now - t0) mod 2^64)
 * ticks in ns: with r kHz the runtime's wall-clock rate (hipDeviceAttributeWallClockRate), (d / r) 10^6 + (d % r) 10^6 / r in integers,
 * 2^64 - 1 where that would not fit.  It goes to the log.  At e < E1 - 1, if the call has not been cut yet, the kernel cuts when
 *   budget != MMEE_DEADLINE_NONE and sat_add(elapsed, eta_ns[e]) >= budget        (cut_by 1; sat_add saturates at 2^64 - 1), else when
 *   the host's request word >= k                                                  (cut_by 2; ee_request_cut).
 * A cut writes the value that fires for everybody into dl_thr[e .. E1 - 2] -- -inf under the `>` criteria, +inf under entropy, the mirror image
 * of the controller's never-fires value -- and records cut_exit = e.  It is sticky: later checks of the call only stamp.  The final exit's
 * check stamps and writes nothing else.
 * Result.  A cut call returns, bit for bit, what ee_forward returns under thresholds thr' with thr'[e] = thr[e] for e < cut_exit and the
 * always-fires value from cut_exit on: the cut documents leave through the ordinary decide launch, with the ordinary row of the exit they
 * stand at (ensembled row, temperature, confidence and result stream as ever).  The test is strict, so a NaN criterion does not fire under
 * -inf / +inf either: such a document runs to the final exit, as everywhere else.
 * Lookahead.  eta_ns[e] is the caller's estimate of the time from the decision at exit e to the end of the call IF NOBODY IS CUT THERE, so the
 * cut falls at the last exit the budget still allows, not at the first one after it has passed.  NULL means zeros.  deadline.eta_from_logs
 * builds the table from the logs of uncut calls.  budget = MMEE_DEADLINE_NONE: the clock never cuts; the calls are stamped and obey
 * ee_request_cut only.
 * Host cut.  ee_request_cut stores the number of deadline calls enqueued on the handle so far into a pinned, mapped host word, which the check
 * reads with a relaxed system-scope atomic load: every call already enqueued is cut at its next check, none enqueued later.  Any thread, no
 * HIP call; the word only ever grows (a compare-and-swap maximum), so concurrent requesters cannot take a request back.  A call that
 * ee_forward refuses is not numbered and writes no log row.  How many checks of a running call still see the old word is timing; that the call then equals thr' of its logged cut_exit is not.
 * Log.  A device ring of log_cap rows of 4 + E1 64-bit words: call number k, budget_ns, cut_exit (-1: none), cut_by (0, 1 clock, 2 host),
 * elapsed_ns[E1] at every check.  The stamps behind the cut are kept: elapsed[E1 - 1] - elapsed[cut_exit] is the tail of empty launches.
 * Dump-all calls (MMEE_FLAG_NO_EXIT) ignore the deadline: no launch is added, no row written, no call counted.  A handle without a deadline
 * issues the launches it issued before and returns the same bits.
 * Allowed unchanged: the four threshold criteria (gate included), temperatures, an ensemble, MMEE_FLAG_LOW_LATENCY, MMEE_FLAG_STREAM_RESULTS,
 * ramp, gate and DiT handles, 1- and 2-layer heads.
 * Refused, each with a message and nothing changed: E1 > 64; MMEE_CRIT_PATIENCE, an exit rule other than MMEE_RULE_PLAIN, use_lte (a cut must
 * fire at once, and their decisions carry state or another score); quotas in either mode; an audit or a controller (shadows would run past the
 * cut) -- each in either order of setting; ee_graph_capture while a deadline is set, ee_set_deadline while graphs are held;
 * ee_forward_vision; a device whose runtime reports a wall-clock rate of 0.  The Python MicroBatchedEngine and CascadeEngine refuse a deadline.
 * Not built: deadlines in captured graphs; an absolute deadline shared across calls (it needs a host <-> device clock correlation); deadlines
 * under quotas, audits or the patience rules; forcing out NaN documents; a learned eta.
 */
/* model family: LayoutLMv3 (text + layout + image, the reference's EE model) or BEiT / DiT (image only; BASELINE configs[4],
 * the reference's "dit" branch EE/configs.py:429-449 — exit heads there are this build's extrapolation) */
enum { MMEE_ARCH_LAYOUTLMV3 = 0, MMEE_ARCH_BEIT = 1 };
/* arithmetic of the encoder GEMMs */
/* MMEE_PREC_F32: v_mfma_f32_32x32x2_f32 on f32 operands.  MMEE_PREC_F32_SPLIT: the four big Linear layers of every encoder
 * layer run on the f16 matrix cores with every f32 operand split into two f16 planes (hi + lo, 22 significant bits) and
 * three MFMA terms per product, f32 accumulation — measured at least as accurate as the f32 MFMA chain, same
 * 1e-4 / bit-exact parity bar; needs hidden_size and intermediate_size to be multiples of 256.  Range: the f16 planes hold
 * 16 x LayerNorm outputs, 16 x Q/K/V, 64 x attention context, 16 x GELU outputs and 2^e x weights (e chosen per tensor at
 * ee_finalize); values beyond +-60000 / scale (|activation| > 3750, |context| > 937) are clamped, far outside what
 * LayoutLMv3 / DiT checkpoints produce — use MMEE_PREC_F32 for a model that exceeds it.  MMEE_PREC_BF16 is reserved and
 * rejected: plain bf16 cannot meet the tolerance. */
enum { MMEE_PREC_F32 = 0, MMEE_PREC_BF16 = 1, MMEE_PREC_F32_SPLIT = 2 };
/* ee_load_tensor dtypes */
enum { MMEE_DT_F32 = 0, MMEE_DT_F16 = 1, MMEE_DT_BF16 = 2 };
/* ee_forward flags */
enum {
    MMEE_FLAG_DENSE_ROWS = 1,  /* keep all T text rows per document (pad rows computed, masked as keys) instead of the
                                  ragged layout that drops pad rows; the two layouts agree to ROUNDING (<= 2e-5 on
                                  logits: the attention sums a row's keys in tiles whose boundaries differ), not
                                  to the bit; exit indices are equal.  This is the A/B switch                    */
    MMEE_FLAG_NO_EXIT = 2,     /* dump-all mode: evaluate every exit for every document, nobody leaves early
                                  (the reference's own behaviour, EE/utils.py:63-71 "impossible thresholds")        */
    MMEE_FLAG_WHOLE_LAYERS = 4,/* run every encoder layer whole before its exit decision (what the reference does,
                                  EE/models/LayoutLMv3.py:757-768), never "probe first" (ee_last_layer_plan)          */
    MMEE_FLAG_PROBE_ALWAYS = 8,/* probe first at every layer that ends in a decision, whatever ee_set_probe_mask pinned.  With neither flag
                                  and no pinned mask this is also the DEFAULT (round 5): the schedule is a function of the call, never of
                                  timing or of earlier forwards.  Whole layers, probe-first and any pinned mix give identical results bit for
                                  bit without MMEE_FLAG_XPROBE; the flags only pin the schedule, for A/B runs and tests          */
    MMEE_FLAG_ONE_TERM = 32,   /* REPORTED low-precision mode, never a parity path (SURVEY 8d config 2 "bf16 throughput mode reports its measured
                                  deviation separately"): the layer GEMMs and the attention of an MMEE_PREC_F32_SPLIT LayoutLMv3 handle run ONE f16
                                  MFMA term per MAC (hi planes only, f32 accumulate) instead of three; CLS probes and exit heads keep three.  Logits
                                  leave the 1e-4 bar and exit indices may flip: bench.py reports rate, max |dlogit| and flip rate as `lowprec` */
    MMEE_FLAG_XPROBE = 16,     /* probe-first layers take the CLS context in X space (csrc/xprobe.hip): score_j = (W_k^T q) . x_j + q . b_k,
                                  ctx = W_v (sum_j p_j x_j) + b_v.  No Q | K | V projection exists when the decision is taken: the layer's
                                  Q | K | V GEMM then runs for the documents that STAY only, and not at all in the last layer.  A
                                  re-association of the same arithmetic (~1e-6 on the CLS row): exit indices and the 1e-4 logit bar hold,
                                  bit-identity with MMEE_FLAG_WHOLE_LAYERS does not.  LayoutLMv3, MMEE_PREC_F32_SPLIT, no dump-all */
    MMEE_FLAG_LOW_LATENCY = 64,/* small batches (the reference's eval_batch_size = 1, EE/configs.py:36): in the rest of every LayoutLMv3 layer
                                  (attention, attention output, FFN) the attention-output and FFN-down GEMMs run as S-way split-K whenever
                                  ee_low_latency_k_splits gives S > 1 for this call's static row count B * (T + patches + 1): S workgroups per
                                  128 x 128 output tile, each over K / S, writing alpha * acc of its part and no bias.  The LayerNorm that
                                  follows completes the row from the S parts in the order p = 0, 1, ..., then the bias, then the residual.
                                  A re-association of the whole-layer arithmetic: within the 1e-4 bar of the goldens, with equal exit
                                  indices; NOT bit-identical to the same call without the flag, nor to the K | V probe (a flagged forward
                                  is bit-identical to its own dump-all rows under MMEE_FLAG_WHOLE_LAYERS).  The bits depend only on
                                  (B, T, flags, handle configuration), never on batch mates or on timing: S comes from the static row
                                  count, so the launch list stays a pure function of the call and a captured graph binds it.  Where the rule
                                  gives S = 1 for both GEMMs the flag changes nothing, neither a launch nor a bit.  Q | K | V, FFN-up,
                                  attention, probes and the exit tail are as without the flag.  Refused, each with a message: on an
                                  MMEE_PREC_F32 handle, on an MMEE_ARCH_BEIT handle, together with MMEE_FLAG_ONE_TERM */
    MMEE_FLAG_STREAM_RESULTS = 128 /* deliver the documents to the host as they leave: behind every exit's decide launch one more launch packs the
                                  rows of the documents that left there into a pinned buffer of the handle and an event is recorded; ee_stream_next
                                  (below) waits for the next exit's event and returns its rows.  out_logits and out_conf must be non-NULL; every
                                  out_* tensor is filled exactly as without the flag (same launches in front, same bits).  Adds E + 1 launches.
                                  Refused, each with a message: together with MMEE_FLAG_NO_EXIT (nobody leaves early: nothing to stream) and in
                                  ee_graph_capture (events between launches are not part of a captured launch list) */
};

typedef struct ee_handle ee_handle;

typedef struct ee_config {
    int32_t abi_version;            /* MMEE_ABI_VERSION */
    /* HF LayoutLMv3Config fields the path reads */
    int32_t hidden_size, num_hidden_layers, num_attention_heads, intermediate_size;
    int32_t vocab_size, max_position_embeddings, type_vocab_size, pad_token_id;
    int32_t max_2d_position_embeddings, coordinate_size, shape_size;
    int32_t rel_pos_bins, max_rel_pos, rel_2d_pos_bins, max_rel_2d_pos;
    int32_t input_size, patch_size, num_channels, num_labels;
    float layer_norm_eps;
    /* ExitConfig (EE/models/EE_modules.py:175-195) */
    int32_t n_embedding_exits;                      /* 0..3 */
    int32_t embedding_exits[3];                     /* MMEE_EXIT_*, evaluation order */
    int32_t n_encoder_exits;
    int32_t encoder_exit_layers[MMEE_MAX_ENCODER_EXITS];   /* 1-based, ascending; head k <-> encoder.early_exits.k */
    int32_t exit_head_num_layers;                   /* 1 or 2 */
    int32_t strategy;                               /* MMEE_STRATEGY_* */
    int32_t criterion;                              /* MMEE_CRIT_* */
    /* workspace sizing */
    int32_t max_docs;                               /* largest B one ee_forward call may pass */
    int32_t max_text_len;                           /* largest T */
    int32_t precision;                              /* MMEE_PREC_* */
    /* model family (appended in ABI version 2) */
    int32_t arch;                                   /* MMEE_ARCH_* */
    int32_t use_abs_pos;                            /* BEiT: use_absolute_position_embeddings */
    int32_t layer_scale;                            /* BEiT: layer_scale_init_value > 0 (lambda_1 / lambda_2 present) */
    int32_t use_mean_pooling;                       /* BEiT: must be 1 (DiT); pooled = LayerNorm(mean of patch tokens) */
    /* learning-to-exit (appended in ABI version 4) */
    int32_t use_lte;                                /* EE_config["use_lte"]: the exit test is the LTE score (semantics above) */
} ee_config;

int ee_create(const ee_config* cfg, ee_handle** out);
int ee_destroy(ee_handle* h);
const char* ee_last_error(const ee_handle* h);      /* h may be NULL: error of the last failed ee_create */

/* Copy one parameter into the handle (the library owns its weight memory and may re-layout it).  `name` is the HF
 * parameter name; `data` is a host pointer (is_device = 0) or a device pointer (is_device = 1) to a C-contiguous
 * tensor of `dtype`; shape is checked against the config.  Unknown names are an error. */
int ee_load_tensor(ee_handle* h, const char* name, const void* data, const int64_t* shape, int32_t ndim,
                   int32_t dtype, int32_t is_device);
/* Verify every parameter the config needs was loaded and build derived tables (relative-position value tables).
 * Synchronises with the device. */
int ee_finalize(ee_handle* h);
/* Number of parameters the config expects / name of the i-th one (for loaders and tests). */
int32_t ee_num_expected_tensors(const ee_handle* h);
const char* ee_expected_tensor_name(const ee_handle* h, int32_t i);

/*
 * One pass of the hot path over a batch of B documents with T text tokens each.
 *
 *   input_ids      dev int64 (B,T)        attention_mask  dev int64 (B,T) or NULL (= ones)
 *   bbox           dev int64 (B,T,4)      pixel_values    dev float (B,C,R,R)
 *   token_type_ids dev int64 (B,T) or NULL (= zeros)      position_ids dev int64 (B,T) or NULL (= pad-aware cumsum)
 *   thresholds     host double [E+1]: exit e leaves when sign(crit_e, thresholds[e]) (strict); entry E (final) unused.
 *                  Under ee_config.use_lte: encoder exit e leaves when u_e < thresholds[e] (strict); entries of embedding exits unused.
 *                  Ignored (may be NULL) under MMEE_CRIT_PATIENCE, which needs ee_set_patience before its first thresholded forward
 *   temperatures   host double [E+1] or NULL: logits of exit e are divided by temperatures[e] before the criterion
 *                  and in every returned logit (calibrated logits, EE/eval.py:321-323)
 * outputs (any may be NULL except out_exit):
 *   out_logits     dev float  (B,K)   logits at the exit the document left through   ("predictions")
 *   out_exit       dev int32  (B,)    index into the exit list, E = final classifier  ("exits_store")
 *   out_conf       dev float  (B,)    criterion value at that exit
 *   out_all_logits dev float  (E+1,B,K)  every evaluated exit's policy logits (ramp: exit_states[j][0]; gate:
 *                  gated_logits[j]); rows of exits a document never reached are left untouched
 *   out_all_crit   dev float  (E+1,B)    criterion of every evaluated exit on the policy logits
 *   out_head_logits dev float (E,B,Kh)   raw exit-head logits (Kh = K for ramps, 2 for gates) = exit_states[j][0]
 *   out_head_crit  dev float  (E,B)      criterion on the raw head logits = exit_states[j][1]
 *   out_hidden_cls dev float  (L+1,B,H)  CLS row entering layer 0 and leaving every layer (debug / parity)
 */
int ee_forward(ee_handle* h, const int64_t* input_ids, const int64_t* attention_mask, const int64_t* bbox,
               const float* pixel_values, const int64_t* token_type_ids, const int64_t* position_ids,
               int32_t B, int32_t T, const double* thresholds, const double* temperatures, uint32_t flags,
               float* out_logits, int32_t* out_exit, float* out_conf, float* out_all_logits, float* out_all_crit,
               float* out_head_logits, float* out_head_crit, float* out_hidden_cls, void* stream);

/*
 * The same forward as a captured launch list (hipGraph), for callers that keep the reference's small batches (eval_batch_size = 1,
 * EE/configs.py:36; the loop EE/utils.py:169-193 issues one forward per document): ~185 launches per forward become one graph launch.
 *
 * ee_graph_capture takes EXACTLY the arguments of ee_forward.  It runs the call once eagerly on `stream` (argument validation, one-time kernel
 * set-up; the outputs hold that call's results), synchronises, then captures the same launch list and instantiates it; *graph_id names it.
 * The graph is bound to the POINTERS it was captured with -- inputs and outputs are static buffers the caller refills / reads between
 * replays -- and to (B, T, flags, which outputs were non-NULL) and to the handle's exit-layer schedule at capture time (ee_set_probe_mask).
 * Thresholds and temperatures are NOT baked in: the decide kernels read them from a device vector that every ee_graph_launch refreshes.
 * Neither is the patience: under MMEE_CRIT_PATIENCE, MMEE_RULE_STREAK and MMEE_RULE_EITHER the decide kernel of exit e reads t_e from the
 * same vector (E + 1 entries behind the temperatures), which ee_graph_launch fills with the handle's CURRENT patience (ee_set_patience /
 * ee_set_patience_vector between replays take effect).  The criterion and the exit rule themselves are bound at capture.
 * Quotas (ee_set_quotas) likewise: whether they are on, and the mode, are bound at capture; the values are a fourth section of the vector
 * (E + 1 entries behind the patience), filled with the handle's CURRENT quotas by every ee_graph_launch.
 * `stream` must be a created stream (the legacy null stream cannot be captured).  Not capturable: the one-shot side inputs / outputs
 * (ee_set_inputs_embeds, ee_set_hidden_states_out, ee_set_head_mask, ee_set_attentions_out) and an armed ee_profile.
 *
 * ee_graph_launch replays it on `stream` (any stream, the null stream included) with this launch's thresholds (host double [E+1]; may be NULL
 * for a graph captured with MMEE_FLAG_NO_EXIT, under MMEE_CRIT_PATIENCE or under MMEE_QUOTA_EXACT) and temperatures (host double [E+1] or NULL = 1.0: a division by 1.0 is exact, so a graph
 * replayed without temperatures returns the bits of the eager call without them).  Same arithmetic, same launch order, same bits as
 * ee_forward on the same inputs (tests/test_gpu_round6.py).  Error reporting, ee_last_stage_counts, ee_last_flops and ee_last_layer_plan work
 * as after ee_forward.  Rows of out_all_* / out_head_* that a replay does not reach keep what the buffers held before (as ee_forward).
 * ee_graph_destroy releases the executable graph (ee_destroy releases all of them).
 */
int ee_graph_capture(ee_handle* h, const int64_t* input_ids, const int64_t* attention_mask, const int64_t* bbox,
                     const float* pixel_values, const int64_t* token_type_ids, const int64_t* position_ids,
                     int32_t B, int32_t T, const double* thresholds, const double* temperatures, uint32_t flags,
                     float* out_logits, int32_t* out_exit, float* out_conf, float* out_all_logits, float* out_all_crit,
                     float* out_head_logits, float* out_head_crit, float* out_hidden_cls, void* stream, int32_t* graph_id);
int ee_graph_launch(ee_handle* h, int32_t graph_id, const double* thresholds, const double* temperatures, void* stream);
int ee_graph_destroy(ee_handle* h, int32_t graph_id);

/*
 * The inputs of the embedding-level exit heads, from stage 0 of the forward alone: no encoder layer, no head, no exit stage.  Each output is a
 * dev float (B,H) or NULL (at least one must be given):
 *   out_vision   visual_embeddings.mean(1)          the row layoutlmv3.vision_exit_embeddings reads  (EE/models/LayoutLMv3.py:466)
 *   out_text     embedding_output.mean(1), text     the row layoutlmv3.text_exit_embeddings reads    (EE/models/LayoutLMv3.py:520)
 *   out_concat   LayerNorm(cat(text, visual)).mean(1)  the row layoutlmv3.concat_exit_embeddings reads  (EE/models/LayoutLMv3.py:582)
 * The means run over EVERY position of the call, padded text positions included, as in the reference: the same page padded to another T has
 * another text and concat row.  The launches are the ones ee_forward opens with (one definition serves both), so the rows are, bit for bit,
 * the rows the heads of a forward on the same handle and inputs read, and an output does not depend on which other outputs are asked for or
 * on which embedding exits the handle's configuration names.  The training set of these heads needs no encoder: this is the call that
 * collects it (heads.py collect_embedding_features).
 * Inputs and their checks are ee_forward's.  Refused with a message, nothing written: a MMEE_ARCH_BEIT handle (it has no such exits), all three
 * outputs NULL, B outside [1, max_docs], T outside [1, max_text_len], a missing input_ids / bbox / pixel_values.  An id, box, position or
 * token type out of range is flagged on the device and reported as after ee_forward -- by the next call on the handle or by
 * ee_last_stage_counts -- and the rows of that call are invalid.  An armed ee_set_inputs_embeds is consumed by this call as ee_forward
 * would consume it (its rows replace the word embeddings); the other one-shot side inputs / outputs stay armed for the next ee_forward.
 * Handle state: the call runs on `stream`, ordered behind the handle's previous call as a forward is, and only enqueues.  What the handle
 * records of its LAST FORWARD is untouched: ee_last_stage_counts, ee_last_flops, ee_last_k_splits, ee_last_layer_plan, ee_suggest_probe_mask
 * and ee_profile_read answer as if this call had not happened (an armed ee_profile stays armed and times nothing here).  It writes only
 * buffers that every forward and graph replay rewrites before reading them (the packed rows go to the handle's X rows as scratch), so
 * captured graphs stay valid and an undrained result stream keeps its chunks.
 */
int ee_embedding_inputs(ee_handle* h, const int64_t* input_ids, const int64_t* attention_mask, const int64_t* bbox,
                        const float* pixel_values, const int64_t* token_type_ids, const int64_t* position_ids,
                        int32_t B, int32_t T, float* out_vision, float* out_text, float* out_concat, void* stream);

/*
 * The vision-first call: OCR only for the documents the image keeps.  DEFINITION (engine.py, modeling.py, README and DESIGN refer to this one).
 * On a LayoutLMv3 handle whose exit list contains vision_avg that exit is exit 0, it reads visual_embeddings.mean(1) -- a function of the
 * document's own pixels -- and every later exit needs text.  A vision-first call over B documents has two phases.
 *   Phase 1, pixels only, all B documents (ee_forward_vision): the patch projection, the visual rows up to layoutlmv3.norm (LayerNorm, eps 1e-6)
 *     and their mean over the Pv positions (vision_pool_kernel + pool_finish: the bits of ee_embedding_inputs' out_vision), then exit 0 exactly
 *     as ee_forward runs it: the head (one or two layers; gate handles: classifier(gate input) and, under MMEE_CRIT_GATE, the gate head), the
 *     temperature, the ensemble row y_0 if an ensemble is set, the handle's criterion, its exit rule and patience entry 0, thresholds[0].
 *     A document that leaves gets out_logits / out_exit = 0 / out_conf with the bits the one-call ee_forward gives it; for a document that
 *     stays nothing is written, its slot goes into survivors (ascending; entries from the count on are not written) and their number to *count.
 *   Phase 2, survivors only: an ordinary ee_forward on the survivors' rows -- their pixel rows and the text the caller supplies NOW -- whose
 *     results go to the survivors' slots (ee_cascade_gather, ee_cascade_merge with exit offset 0 and stage 1).  Phase 2 evaluates exit 0
 *     again for its documents: a document's bits do not depend on its batch mates, so none of them leaves there, and the per-slot state
 *     (patience / streak run, ensemble state, audit marks) is rebuilt at exit 0 as in any forward.  The patch projection is 0.23 of 139 GFLOP
 *     per document, so phase 2 needs no new forward code, no stash of rows and no state handed over; ee_forward_vision keeps nothing that
 *     phase 2 needs, and phase 1 of the next batch may run while the text of this one is being read.
 *   The composition returns, bit for bit, what ee_forward returns on the full inputs (same flags); the text is needed for exactly the
 *   survivors, and not at all when nobody survives.  With MMEE_FLAG_LOW_LATENCY on phase 2 the bits are those of that flagged forward on
 *   the survivors' sub-batch, a pure function of its (B', T).  The text and concat means run over all T positions: pad phase 2 to the T
 *   deployment runs.
 * ee_forward_vision: pixel_values dev float (B,C,R,R); thresholds / temperatures host double [E+1] as in ee_forward (entry 0 is read);
 *   flags: the layer flags of ee_forward are accepted and read by nothing; out_logits dev float (B,K) or NULL, out_exit dev int32 (B),
 *   out_conf dev float (B) or NULL; survivors dev int32 (B); count dev int32 (1).  It only enqueues.  Launches: the error-word zeroing, the
 *   uniform layout of the decide kernel's bookkeeping, the patch projection, vision_pool_kernel, pool_finish, exit 0's head / ensemble /
 *   decide launches, one copy of the next stage's slots and count.
 *   Handle state: as ee_embedding_inputs.  What the handle records of its LAST FORWARD is untouched (ee_last_stage_counts, ee_last_flops,
 *   ee_last_k_splits, ee_last_layer_plan, ee_suggest_probe_mask, ee_profile_read; an armed ee_profile times nothing here); it writes only
 *   workspace that every forward and graph replay rewrites before reading it, so captured graphs stay valid and an undrained result stream
 *   keeps its chunks.
 *   Refused with a message, nothing written: a MMEE_ARCH_BEIT handle; a handle without vision_avg; B outside [1, max_docs]; a NULL
 *   pixel_values / out_exit / survivors / count; MMEE_FLAG_NO_EXIT, MMEE_FLAG_STREAM_RESULTS, MMEE_FLAG_DENSE_ROWS; quotas set (a rank over B
 *   and a second rank over the survivors are not the one-call ranking); an audit or a controller set (the audit hashes the slot in the
 *   call, which phase 2 renumbers); an armed one-shot side input / output (it stays armed); missing thresholds (unless MMEE_CRIT_PATIENCE)
 *   and the patience / exit-rule combinations ee_forward refuses.  Allowed unchanged: the four threshold criteria, patience, both exit
 *   rules, use_lte (nobody leaves at an embedding exit: correct and pointless), the gate criterion, temperatures, an ensemble, ramp and
 *   gate handles, 1- and 2-layer heads.
 *   NOT BUILT: a row stash between the phases; vision-first under audits / controllers / quotas / captured graphs / the result stream /
 *   micro-batches / as a cascade stage; the dump-all outputs (out_all_*, out_head_*, out_hidden_cls); a text-first counterpart for text_avg.
 */
int ee_forward_vision(ee_handle* h, const float* pixel_values, int32_t B, const double* thresholds, const double* temperatures, uint32_t flags,
                      float* out_logits, int32_t* out_exit, float* out_conf, int32_t* survivors, int32_t* count, void* stream);

/*
 * The result stream of the handle's most recent ee_forward with MMEE_FLAG_STREAM_RESULTS: one chunk per evaluated exit, in the path's order
 * e = 0 .. E (embedding exits, encoder exits ascending, the final classifier), E + 1 chunks per forward.  ee_stream_next BLOCKS the calling
 * thread until the next undelivered exit has been decided on the device (hipEventSynchronize on an event recorded behind that exit's launches:
 * no flag is polled, deeper layers keep running for the documents that stay), then returns *exit_index = e, *n_rows = the number of documents
 * that left at e (possibly 0) and *rows = host int32 (n_rows, K + 3): per document the K + 2 words of ee_pack_results -- the logits' float32 bit
 * patterns, the exit index, the confidence's bit pattern -- followed by the document's slot in the call (its row of out_*).  After the last
 * chunk it returns 0 with *exit_index = -1, *n_rows = 0, *rows = NULL.
 *   - rows within a chunk ascend by slot; every row of chunk e carries exit index e;
 *   - the union over the E + 1 chunks is every document of the call exactly once (n_rows sums to B);
 *   - the row's bits are the bits out_logits / out_exit / out_conf hold at that slot once the forward has finished;
 *   - the chunk sizes are the differences of ee_last_stage_counts' document counts.
 * The pointer addresses pinned memory of the handle, written by the device: read it, do not write it; it stays valid until the next
 * ee_forward with the flag on this handle.  That forward drops whatever the caller has not read yet (the earlier forward's out_* stay
 * complete) and, before it enqueues anything, waits on the host for the earlier flagged forward's last exit, so the buffer is never rewritten
 * under a reader.  A forward without the flag leaves the stream alone.  One caller thread per handle, as everywhere.
 * Error reporting is unchanged: out-of-range inputs and split-precision overflows are reported by ee_last_stage_counts or the next forward as
 * today; the chunks are what out_* will hold.  Refused with a message: a handle on which no flagged forward has run.
 */
int ee_stream_next(ee_handle* h, int32_t* exit_index, const int32_t** rows, int32_t* n_rows);

/* Per-stage statistics of the last ee_forward (synchronises with `stream`): active documents and packed rows entering
 * each of the E+1 exit stages.  n_stages_out receives E+1. */
int ee_last_stage_counts(ee_handle* h, int32_t* docs_out, int32_t* rows_out, int32_t cap, int32_t* n_stages_out,
                         void* stream);
/* FLOPs (2*M*N*K counting) the GEMM and attention kernels of the last ee_forward executed (synchronises). */
int ee_last_flops(ee_handle* h, double* gemm_flops, double* attn_flops, void* stream);
/* How the last ee_forward ran each encoder layer (synchronises).  A layer that ends in a decision (an exit head, or the final
 * classifier) is run "probe first" in split precision: Q|K|V for every row of the stage, then the layer's output for the CLS row of
 * every document only (the one row the head reads, EE/models/LayoutLMv3.py:757-768), the decision, and the rest of the layer for
 * the documents that stay.  Per layer l < cap: rows whose Q|K|V was projected, rows the attention / attention-out / FFN ran on
 * (0: none, the last layer), documents probed (0: the layer was run whole).  probe_flops: FLOPs of all the probes, which
 * ee_last_flops leaves out. */
int ee_last_layer_plan(ee_handle* h, int32_t* rows_qkv, int32_t* rows_main, int32_t* docs_probe, int32_t cap, double* probe_flops,
                       void* stream);

/* The split-K rule of MMEE_FLAG_LOW_LATENCY: how many parts S the k-loop of a residual GEMM with N output columns and inner size K is divided
 * into when the call has max_rows = B * (T + patches + 1) rows, on a chip of num_cus compute units.  A pure function: no handle, no GPU.
 * S is the largest of {8, 4, 2} that divides the K / 32 k-stages, leaves every part at least 3 stages (the depth of the kernel's stage ring) and
 * keeps ceil(max_rows / 128) * (N / 128) * S <= 2 * num_cus -- the 128 x 128 tiles of the launch times S still fit the chip at two workgroups
 * per CU -- else 1.  Non-increasing in max_rows.  Arguments outside the kernel's shapes (N % 128, K % 32, anything < 1) give 1.
 * (Measured against the bound <= num_cus at B = 1, 2, 4, T = 512, LayoutLMv3-base: profiles/low_latency_ab.txt.) */
int32_t ee_low_latency_k_splits(int32_t max_rows, int32_t N, int32_t K, int32_t num_cus);
/* The S the handle's most recent forward (or graph launch) used for the attention-output and the FFN-down GEMMs of its layers: 1 / 1 when
 * MMEE_FLAG_LOW_LATENCY was off or the rule declined.  Either pointer may be NULL.  Does not synchronise. */
int ee_last_k_splits(ee_handle* h, int32_t* attn_out, int32_t* ffn_down);

/* The exit criterion of every LATER ee_forward (MMEE_CRIT_*; ee_config.criterion is its initial value).  The reference's evaluation driver
 * overrides `model.config.exit_config["inference_strategy"]` after the model has been built (EE/utils.py:62-78); the Python mirror forwards that
 * write here so that those lines run unchanged. */
int ee_set_criterion(ee_handle* h, int32_t criterion);
/* The patience t (>= 1; smaller values are rejected) of every later forward and graph launch under MMEE_CRIT_PATIENCE.  Part of the handle's
 * state until changed.  Per document, the decide kernels keep (argmax at the previous exit, run counter) in the handle's workspace, indexed
 * by the document's slot in the call and rewritten at exit 0, which every document reaches: nothing carries over from one forward to the next. */
int ee_set_patience(ee_handle* h, int32_t t);
/* The per-exit patience t[0 .. E] (n must be E + 1, every entry >= 1; the final exit's entry is ignored) of every later forward and graph launch
 * under MMEE_CRIT_PATIENCE, MMEE_RULE_STREAK and MMEE_RULE_EITHER.  Copied: the caller's array need not outlive the call.  ee_set_patience stays
 * the broadcast and replaces the vector. */
int ee_set_patience_vector(ee_handle* h, const int32_t* t, int32_t n);
/* The exit rule (MMEE_RULE_*, semantics above) of every LATER ee_forward and ee_graph_capture; MMEE_RULE_PLAIN after ee_create. */
int ee_set_exit_rule(ee_handle* h, int32_t rule);

/* Exit ensemble (Zero Time Waste, Wolczyk et al., NeurIPS 2021): the decision at exit m sees a weighted geometric ensemble of the exits the
 * document has passed, instead of exit m's row alone.  No backbone work is added: a document that reaches exit m has run every head below it.
 * THE definition (the forward, ee_ensemble_logits and the stand-alone hook all refer to it).  Exits e = 0 .. E in the path's order,
 * E1 = E + 1, K labels:
 *   x_e[k] = (float)((double)z_e[k] / T_e)          the scaled row of exit e as the path writes it out (what dump-all stores in all_logits);
 *   l_e[k] = (x_e[k] - M) - log(S)                   in float64: M = max_k x_e[k], S = sum_k exp(x_e[k] - M) over k = 0 .. K-1 in label order
 *                                                    (the max-shifted log-softmax);
 *   a_m[k] = b[m][k] + sum_{j = 0 .. m} w[m][j] l_j[k]   in float64, accumulated with fma, j ascending, starting from b[m][k];
 *   y_m[k] = (float)a_m[k]                           the ensemble row.
 * w is (E1, E1) lower triangular in float64 (an entry with j > m must be 0), b is (E1, K) in float64, NULL meaning 0.
 * With an ensemble set, y_m takes the place of the scaled policy row everywhere behind it: the decision sees y_m with temperature 1 (every
 * threshold criterion, MMEE_CRIT_PATIENCE and the two rules, whose argmax is y_m's); out_logits, out_all_logits and the result stream carry
 * y_m; out_conf and out_all_crit are the criterion of y_m; out_head_logits and out_head_crit stay the head's own raw values.  The final exit
 * is ensembled like any other.  On gate-strategy handles under the threshold criteria the ensemble is over classifier(gate input).
 * Special cases: w = I, b = 0 gives y_m = logsoftmax(x_m), the plain exit up to one rounding (the same decisions for max-confidence, entropy
 * and margin up to that rounding; not the same bits); w[m][j] = 1 / (m + 1) is the running geometric mean of the exits' distributions.
 * One launch per exit (exit_ensemble_kernel, between the head's and the decision's); per-document state l_e in the handle's workspace,
 * indexed by the document's slot in the call, written at every exit the document reaches: nothing carries over from one forward to the next.
 *
 * ee_set_ensemble: w host (E1 * E1) doubles, b host (E1 * K) doubles or NULL; both are copied.  w == NULL clears the ensemble: the handle then
 * issues the launches and returns the bits it did before one was ever set.  Applies to every later ee_forward and ee_graph_capture; the first
 * call allocates E1 * max_docs * K doubles of state.  Refused, with a message and nothing changed: an entry that is not finite; a non-zero entry
 * of w above the diagonal; a handle under MMEE_CRIT_GATE or with use_lte (their decision does not read the policy row; not built); a handle
 * that holds captured graphs when the call would switch the ensemble on or off (a graph's launch list is the one of its capture; new weights for
 * a set ensemble are fine, replays read them).  While an ensemble is set, ee_set_criterion refuses MMEE_CRIT_GATE.  Synchronises the device.
 * ee_has_ensemble: 1 when an ensemble is set, else 0. */
int ee_set_ensemble(ee_handle* h, const double* w, const double* b);
int ee_has_ensemble(const ee_handle* h);

/* The quotas (budgeted exits, semantics above) of every LATER ee_forward, ee_graph_capture and ee_graph_launch: quotas[0 .. n-1] host int32,
 * n must equal E, the number of exits below the final one; mode MMEE_QUOTA_EXACT or MMEE_QUOTA_AT_LEAST.  Copied; part of the handle's state
 * until changed, like ee_set_patience_vector.  quotas == NULL switches quotas off (n and mode are then ignored).  The first call allocates
 * max_docs doubles and max_docs ints of stage scratch.
 * Captured graphs: whether quotas are on, and in which mode, is bound at capture; the quota VALUES are not -- ee_graph_launch writes the
 * handle's current quotas into the device vector it refreshes anyway (a fourth section behind thresholds, temperatures and patience), so
 * ee_set_quotas between two replays takes effect.  A graph captured under MMEE_QUOTA_EXACT replays without thresholds (NULL is accepted).
 * Refused, with a message and nothing changed: n != E; a negative entry; an unknown mode; a handle under MMEE_CRIT_PATIENCE, under
 * MMEE_RULE_STREAK / MMEE_RULE_EITHER or with use_lte; a call that would switch quotas on or off, or change the mode, while the handle holds
 * captured graphs (ee_graph_destroy them first).
 * ee_has_quotas: the mode (MMEE_QUOTA_EXACT / MMEE_QUOTA_AT_LEAST) when quotas are set, else 0. */
int ee_set_quotas(ee_handle* h, const int32_t* quotas, int32_t n, int32_t mode);
int ee_has_quotas(const ee_handle* h);

/* The audit (audited exits, definition above, behind the cascades) of every LATER ee_forward: cut = floor(fraction 2^32 + 0.5) in [0, 2^32],
 * 0 switches the audit off; seed: vary it per call; slot_base >= 0: the index of the call's document 0 in the caller's batch (0 unless the
 * call is a slice of a larger batch).  Part of the handle's state until changed, passed by value to the decide launches.  The first call with
 * cut > 0 allocates max_docs ints (the delivered marks).  MMEE_FLAG_NO_EXIT calls ignore the audit.
 * Refused, with a message and nothing changed: cut > 2^32; slot_base < 0; cut > 0 while quotas are set (and ee_set_quotas while an audit is
 * set); cut > 0 while the handle holds captured graphs.  ee_forward refuses MMEE_FLAG_STREAM_RESULTS, and ee_graph_capture refuses, while an
 * audit is set.
 * ee_has_audit: 1 while cut > 0.  ee_audit_selected: the selection test itself, 1 or 0; no handle, no device. */
int ee_set_audit(ee_handle* h, uint64_t cut, uint32_t seed, int32_t slot_base);
int ee_has_audit(const ee_handle* h);
int ee_audit_selected(uint64_t cut, uint32_t seed, int32_t slot);

/* The controller (online exit control, definition above, behind the audit's) of every LATER ee_forward.  path HOST float64 (V,E1), most
 * conservative first, copied; NULL switches the controller off (the other arguments are then not read).  p0: the starting position; seed: call
 * t audits under seed + t; log_cap: rows of the device ring log, 0 for none.  Setting a controller restarts the call count, the position
 * and the log.  Synchronises the device.  Refusals: the definition's list.
 * ee_has_controller: 1 while one is set.
 * ee_controller_state: synchronises the stream and reads the position, the controlled calls so far, those that sampled anybody (steps), the
 * sums of sampled and disagree over them, and (thr_out HOST float64 [E1], or NULL) the thresholds the NEXT call will run with.  Any output
 * may be NULL.
 * ee_controller_log: synchronises the stream; *n = rows the ring holds (min(calls, log_cap)); the latest min(*n, cap) of them, oldest first,
 * into rows_out HOST int64 (cap, controller_log_words).  The one download. */
int ee_set_controller(ee_handle* h, const double* path, int32_t V, double alpha, double gamma, double p0, uint32_t seed, int32_t log_cap);
int ee_has_controller(const ee_handle* h);
int ee_controller_state(ee_handle* h, double* p, int64_t* calls, int64_t* steps, int64_t* sampled_sum, int64_t* disagree_sum, double* thr_out,
                        void* stream);
int ee_controller_log(ee_handle* h, int64_t* rows_out, int32_t cap, int32_t* n, void* stream);
/* The same loop replayed on dumped arrays in one launch (no handle): table dev float64 (E1,N), a criterion table (ee_csf_table, ee_gate_table)
 * and its sign (+1: leave on c > thr, -1: on c < thr; strict, a NaN never fires); bad dev uint8 (E1,N), row e: delivering document n at exit e
 * is a loss; path dev float64 (V,E1).  Consecutive groups of G documents play the calls: group t audits its slots 0 .. G-1 under seed + t,
 * the exit of a document is the first e < E1 - 1 whose test fires under the group's thresholds, else E1 - 1.  exits dev int32 (N); log dev
 * int64 (ceil(N / G), controller_log_words), one row per group; p_out dev float64 [1] or NULL: the position after the last group.
 * Refused: E1 outside [2, 64], N outside [1, 2^28), G < 1, V < 2, a sign that is not +-1, cut outside [1, 2^32], alpha, gamma, p0 as for
 * ee_set_controller. */
int ee_rolling_control(const double* table, double sign, const uint8_t* bad, int32_t E1, int32_t N, const double* path, int32_t V, uint64_t cut,
                       uint32_t seed, double alpha, double gamma, double p0, int32_t G, int32_t* exits, int64_t* log, double* p_out, void* stream);

/* The deadline (deadline exits, definition above, behind the controller's) of every LATER ee_forward.  budget_ns: the budget of a call from its
 * begin launch; MMEE_DEADLINE_NONE: stamp and obey ee_request_cut, never cut by the clock; MMEE_DEADLINE_OFF: remove the deadline (eta_ns is
 * then not read).  eta_ns HOST uint64 [E1], copied, or NULL for zeros.  Budget and eta travel as kernel arguments, so a handle that has a
 * deadline takes a new one without synchronising (EarlyExitEngine.forward(deadline_ms=) does); the first ee_set_deadline of a handle
 * allocates (ee_set_deadline_log with MMEE_DEADLINE_LOG_DEFAULT rows).  Refusals: the definition's list.
 * ee_set_deadline_log: log_cap rows for the device ring log, 0 for none; restarts the log.  Synchronises the device.  On a handle without a
 * deadline it refuses what ee_set_deadline refuses, in its words.
 * ee_has_deadline: 1 while one is set.
 * ee_request_cut: cut every deadline call enqueued on h so far at its next check, none enqueued later.  Any thread; no HIP call; returns 1
 * (and does nothing) on a handle that never had a deadline.
 * ee_deadline_log: synchronises the stream; *n = rows the ring holds (min(deadline calls since the log's restart, log_cap)); the latest
 * min(*n, cap) of them, oldest first, into rows_out HOST int64 (cap, 4 + E1).  The log outlives ee_set_deadline(h, MMEE_DEADLINE_OFF, NULL). */
#define MMEE_DEADLINE_NONE 0xFFFFFFFFFFFFFFFFull
#define MMEE_DEADLINE_OFF 0xFFFFFFFFFFFFFFFEull
#define MMEE_DEADLINE_LOG_DEFAULT 1024
int ee_set_deadline(ee_handle* h, uint64_t budget_ns, const uint64_t* eta_ns);
int ee_set_deadline_log(ee_handle* h, int32_t log_cap);
int ee_has_deadline(const ee_handle* h);
int ee_request_cut(ee_handle* h);
int ee_deadline_log(ee_handle* h, int64_t* rows_out, int32_t cap, int32_t* n, void* stream);

/* Pin the exit-layer schedule.  DEFAULT (enabled == 0): every layer that ends in a decision is probed first.  Rounds 2-4 chose per layer
 * from the stage populations of "the handle's most recent FINISHED forward" -- a timing-dependent host decision, and under MMEE_FLAG_XPROBE
 * (whose probe is a re-association) the same inputs could return different low bits from run to run.  Round 5: the library never picks a
 * schedule by itself; the same call always issues the same launches and returns the same bits (the reference's policy is deterministic,
 * EE/policy.py:28-45).  enabled != 0: bit l of `mask` says whether encoder layer l (0-based) is probed first; layers without an exit ignore
 * their bit, the last layer is always probed, and MMEE_FLAG_WHOLE_LAYERS / MMEE_FLAG_PROBE_ALWAYS still override.  The mask stays until it is
 * changed: it is part of the handle's configuration, like the thresholds are part of the call. */
int ee_set_probe_mask(ee_handle* h, int32_t enabled, uint64_t mask);
/* The priced alternative to "probe everywhere": which exit layers are worth probing first, judged by a cost model from the
 * stage populations of the LAST ee_forward on this handle, which must have been a thresholded one (synchronises).  `flags`: the flags the
 * caller is going to run with (MMEE_FLAG_XPROBE changes the probe's price).  A pure function of those populations: the caller decides whether
 * to pin the result with ee_set_probe_mask (bench.py and EarlyExitEngine.pin_schedule() do, once, after a warm-up forward). */
int ee_suggest_probe_mask(ee_handle* h, uint32_t flags, uint64_t* mask_out, void* stream);
/* Shader-clock stamps: out_dev (dev uint64[MMEE_CLOCK_STAMP_WORDS], 16-byte aligned) receives one (s_memtime = shader clocks, s_memrealtime =
 * 100 MHz) pair PER CU, slot = XCC_ID * 256 + HW_ID[15:8], as seen by one-wave workgroups enqueued on `stream`; slots no workgroup reached stay 0.
 * Two stamps around a region give the clock the chip HELD over it: mean over the slots filled in both of d(out[2s]) / d(out[2s + 1]) x 0.1 GHz
 * (the counters of different CUs are not aligned with each other: only same-slot differences mean anything).  bench.py
 * `docs_per_sec_per_ghz`: the boxes of a pool hold different clocks under the same load. */
#define MMEE_CLOCK_STAMP_WORDS 4096
int ee_clock_stamp(uint64_t* out_dev, void* stream);

/* `inputs_embeds` of the reference signature (EE/models/LayoutLMv3.py:383, 414-417 -> LayoutLMv3TextEmbeddings.forward, HF:185-186:
 * "if inputs_embeds is None: inputs_embeds = self.word_embeddings(input_ids)").  embeds: dev float (B,T,H) of the NEXT ee_forward call, read
 * in place of the word-embedding rows; consumed by that call (pass it again for the next one), NULL clears it.  ee_forward still takes
 * input_ids -- validated and used for the default, padding-aware position ids; a caller without token ids passes pad-free dummies (any valid
 * id != pad_token_id) together with the sequential position_ids of HF:148-158 (pad_token_id + 1 + t), which is what the host mirror does. */
int ee_set_inputs_embeds(ee_handle* h, const float* embeds);

/* `output_hidden_states=True` of the reference signature (EE/models/LayoutLMv3.py:386, 396-400; the encoder collects the hidden state
 * entering every layer and the last layer's output, :164, 182-183, 284-285).  out: dev float (L+1, B, T+Pv, H) -- (L+1, B, Pv, H) for the
 * image-only model -- filled by the NEXT ee_forward, which must carry MMEE_FLAG_NO_EXIT | MMEE_FLAG_WHOLE_LAYERS (nobody leaves, every layer
 * runs on every document, as in the reference's forward); consumed by that call, NULL clears it.  Positions the attention mask drops hold
 * the values the reference computes for them under MMEE_FLAG_DENSE_ROWS and zeros in the ragged layout (their rows do not exist there).
 * In MMEE_PREC_F32_SPLIT the values are the hi + lo planes the next layer actually reads (22 significant bits). */
int ee_set_hidden_states_out(ee_handle* h, float* out);
/* `head_mask` of the reference signature (EE/models/LayoutLMv3.py:382, 631-641: get_head_mask -> one factor per layer and head, applied as
 * `attention_probs = attention_probs * head_mask` in LayoutLMv3SelfAttention.forward of transformers 4.26).  mask: dev float (L, heads) of the NEXT ee_forward,
 * which must carry MMEE_FLAG_NO_EXIT | MMEE_FLAG_WHOLE_LAYERS (what `model.forward` runs); consumed by that call, NULL clears it.  LayoutLMv3 only.
 * Applied by a side kernel to the context rows behind the fused attention kernel (probs * m @ V == m * (probs @ V)): the hot path is untouched. */
int ee_set_head_mask(ee_handle* h, const float* mask);
/* `output_attentions=True` (EE/models/LayoutLMv3.py:157, 219-220, 301: one (B, heads, S, S) tensor of attention probabilities per layer, after the head
 * mask).  out: dev float (L, B, heads, S, S), S = T + patches + 1, filled by the NEXT ee_forward, which must carry MMEE_FLAG_NO_EXIT |
 * MMEE_FLAG_WHOLE_LAYERS | MMEE_FLAG_DENSE_ROWS (every position, masked keys with probability 0, as the reference computes them); S <= 1280.
 * 24 MB per document and layer at S = 709: a debugging / analysis output recomputed by a side kernel, never materialised on the hot path. */
int ee_set_attentions_out(ee_handle* h, float* out);

/*
 * The policy on a dumped logits array.  logits dev double (E1,N,K); thresholds host double [E1]
 * (global threshold: repeat it).  exits dev int32 (N,), predictions dev double (N,K), confidence dev double (N,) or
 * NULL, counts dev int32 [E1] or NULL (documents per exit).  Strict '>' on float64 max-softmax, last exit fallback.
 */
int ee_policy_scan(const double* logits, int32_t E1, int32_t N, int32_t K, const double* thresholds,
                   int32_t* exits, double* predictions, double* confidence, int32_t* counts, void* stream);
/*
 * The same policy under any threshold criterion: criterion is MMEE_CRIT_MAX_CONFIDENCE, MMEE_CRIT_ENTROPY or MMEE_CRIT_MARGIN (patience --
 * ee_patience_scan -- and unknown codes are refused with a message), computed in float64 from the row as ee_csf_table computes it.  exit(n) = the
 * first e < E1-1 whose criterion passes thresholds[e] in the criterion's direction (strict: '>' for max_confidence and margin, '<' for entropy),
 * else E1-1.  Arguments as ee_policy_scan (1 <= E1 <= 256); confidence = the criterion at the chosen exit.  With MMEE_CRIT_MAX_CONFIDENCE it is
 * ee_policy_scan bit for bit.  Needs no table workspace.
 */
int ee_criterion_scan(const double* logits, int32_t E1, int32_t N, int32_t K, int32_t criterion, const double* thresholds, int32_t* exits,
                      double* predictions, double* confidence, int32_t* counts, void* stream);
/*
 * The patience policy (MMEE_CRIT_PATIENCE semantics) on a dumped logits array: logits dev double (E1,N,K), patience >= 1.  p_e is the argmax
 * of the float64 row (first maximum).  exits dev int32 (N,), predictions dev double (N,K) or NULL (the row of the chosen exit), confidence
 * dev double (N,) or NULL (its float64 max-softmax), counts dev int32 [E1] or NULL (documents per exit).
 */
int ee_patience_scan(const double* logits, int32_t E1, int32_t N, int32_t K, int32_t patience, int32_t* exits, double* predictions,
                     double* confidence, int32_t* counts, void* stream);
/*
 * The LTE policy (ee_config.use_lte semantics) on dumped arrays: scores dev double (E1,N) (the LTE score of every exit; rows of embedding
 * exits hold 1.0, which no threshold <= 1 releases), logits dev double (E1,N,K) or NULL with predictions NULL, thresholds host double [E1]
 * (entry E1-1 unused).  exit(n) = the first e < E1-1 with scores[e,n] < thresholds[e] (strict), else E1-1.  exits dev int32 (N,),
 * predictions dev double (N,K) or NULL (the logits row of the chosen exit), counts dev int32 [E1] or NULL (documents per exit).
 */
int ee_lte_scan(const double* scores, const double* logits, int32_t E1, int32_t N, int32_t K, const double* thresholds, int32_t* exits,
                double* predictions, int32_t* counts, void* stream);
/*
 * The gate policy (MMEE_CRIT_GATE semantics) on dumped arrays: scores dev double (E1,N) (ee_gate_table: the gate score of every exit below the
 * final one; row E1-1 is never tested), logits dev double (E1,N,K) or NULL with predictions NULL (the policy logits, classifier(gate input)),
 * thresholds host double [E1] (entry E1-1 unused).  exit(n) = the first e < E1-1 with scores[e,n] > thresholds[e] (strict), else E1-1.  exits
 * dev int32 (N,), predictions dev double (N,K) or NULL (the logits row of the chosen exit), confidence dev double (N,) or NULL (the table entry
 * of the chosen exit), counts dev int32 [E1] or NULL (documents per exit).  The scan loop of ee_lte_scan with the other sign.
 */
int ee_gate_scan(const double* scores, const double* logits, int32_t E1, int32_t N, int32_t K, const double* thresholds, int32_t* exits,
                 double* predictions, double* confidence, int32_t* counts, void* stream);
/*
 * MMEE_RULE_STREAK / MMEE_RULE_EITHER on dumped arrays.  criterion dev double (E1,N): the criterion table (ee_csf_table; max-softmax: ee_msp_table)
 * or the LTE scores; sign +1: the event is criterion > threshold (max_confidence), -1: criterion < threshold (entropy, LTE; rows of embedding
 * exits hold 1.0 under LTE, which no threshold <= 1 releases).  logits dev double (E1,N,K) for the agreement counter (argmax of the float64
 * row, first maximum) and the predictions; may be NULL under MMEE_RULE_STREAK with predictions NULL.  thresholds host double [E1], patience
 * host int32 [E1] (every entry >= 1; entries E1-1 unused); 1 <= E1 <= 256.  exits dev int32 (N,), predictions dev double (N,K) or NULL (the logits row of the
 * chosen exit), confidence dev double (N,) or NULL (the criterion entry of the chosen exit), counts dev int32 [E1] or NULL.
 */
int ee_rule_scan(const double* criterion, double sign, const double* logits, int32_t E1, int32_t N, int32_t K, const double* thresholds,
                 const int32_t* patience, int32_t rule, int32_t* exits, double* predictions, double* confidence, int32_t* counts, void* stream);
/*
 * V threshold vectors x P patience values at once (the rule counterpart of ee_threshold_sweep at its search scale, EE/large_scale.py:42-84), with
 * the POLICY's semantics, as ee_patience_sweep follows its policy's: the event is conf[e,n] > thr[v,e] (strict; a NaN threshold never fires; for
 * a '<' criterion pass the negated table and thresholds, which is exact), exit(v,p,n) as ee_rule_scan with the scalar patience patiences[p] at
 * every exit, the final exit when nothing qualifies.  conf dev double (E1,N), logits dev double (E1,N,K), references dev int64 (N,), thr dev
 * double (V,E1), patiences HOST int32 [P] (each >= 1); E1 <= 64, N < 2^24, P <= 128.  Outputs dev: acc double (V,P) = #{n : argmax
 * logits[exit, n] == references[n]} / N, mean_exit double (V,P), exit_hist int32 (V,P,E1) or NULL; integer sums, then one division: deterministic.
 * A document's streak is walked once per threshold vector and every patience value is a lookup.  Two kernels give the same integers: E1 = 7,
 * P <= 8, no histogram and 8 V >= N (the reference's search shape; enough vectors to pay for the O(N^2) ranking pass, the condition
 * ee_threshold_sweep uses) runs on integer ranks, one thread per threshold vector; every other call, and a call whose rank workspace
 * (104 N + 28 V bytes) cannot be allocated, runs one workgroup per threshold vector on the float64 table.
 */
int ee_rule_sweep(const double* conf, const double* logits, const int64_t* references, int32_t E1, int32_t N, int32_t K, const double* thr, int32_t V,
                  const int32_t* patiences, int32_t P, int32_t rule, double* acc, double* mean_exit, int32_t* exit_hist, void* stream);
/*
 * V patience values at once over one dumped array (the patience counterpart of ee_threshold_sweep / EE/eval.py:186-210): logits dev double
 * (E1,N,K) with E1 <= 128, references dev int64 (N,), patiences dev int32 (V,).  exit(v,n) as ee_patience_scan with t = patiences[v];
 * acc[v] = #{n : argmax logits[exit(v,n), n] == references[n]} / N, mean_exit[v] = sum_n exit(v,n) / N (integer sums, then one division:
 * deterministic).  Outputs dev: acc double (V,), mean_exit double (V,), exit_hist int32 (V,E1) or NULL.
 */
int ee_patience_sweep(const double* logits, const int64_t* references, int32_t E1, int32_t N, int32_t K, const int32_t* patiences, int32_t V,
                      double* acc, double* mean_exit, int32_t* exit_hist, void* stream);

/*
 * The row of the north star's ONE all-gather, for hosts that call RCCL themselves (the Python host does the same with tensor views, dist.py):
 * per document K + 2 int32 words = [logits (K) as their float32 bit patterns | exit_layer | confidence bit pattern].  ee_pack_results builds
 * rows (dev int32 (n, K+2)) from the three ee_forward outputs; after `ncclAllGather(rows, all_rows, n * (K + 2), ncclInt32, comm, stream)`
 * (shards padded to one size, rank r's local row i = document r + i * world) ee_unpack_results splits rows back (any output may be NULL).
 * Integer words are never flushed, canonicalised or rounded on the way.
 */
int ee_pack_results(const float* logits, const int32_t* exit_layer, const float* confidence, int32_t n, int32_t K,
                    int32_t* rows, void* stream);
int ee_unpack_results(const int32_t* rows, int32_t n, int32_t K, float* logits, int32_t* exit_layer, float* confidence,
                      void* stream);

/*
 * Many threshold vectors at once over a confidence table (EE/thresh.py:184-215 / EE/large_scale.py:42-84 semantics:
 * exit(v,n) = argmax_e(conf[e,n] >= thr[v,e]) = first exit whose confidence reaches its threshold, 0 when none does;
 * accuracy = mean(correct[exit(v,n), n]), average exit = mean(exit(v,n)), EE/large_scale.py:87-96).
 * conf dev double (E1,N) (float64 like the reference's CSF table), correct dev uint8 (E1,N), thr dev double (V,E1).
 * Outputs dev: acc double (V,), mean_exit double (V,), exit_hist int32 (V,E1) or NULL.
 */
int ee_threshold_sweep(const double* conf, const uint8_t* correct, int32_t E1, int32_t N, const double* thr, int32_t V,
                       double* acc, double* mean_exit, int32_t* exit_hist, void* stream);
/* The confidence table of the sweep: conf[e,n] = max softmax (float64) of logits[e,n,:] (CSF "msp", EE/thresh.py:55-57),
 * correct[e,n] = (argmax_k logits[e,n,k] == references[n]).  logits dev double (E1,N,K); references dev int64 (N,) or NULL
 * with correct NULL. */
int ee_msp_table(const double* logits, const int64_t* references, int32_t E1, int32_t N, int32_t K, double* conf,
                 uint8_t* correct, void* stream);
/* The table of any of the three confidence scoring functions (CSF_dict, EE/thresh.py:55-61), for ee_threshold_sweep, ee_rule_scan and
 * ee_rule_sweep: criterion MMEE_CRIT_MAX_CONFIDENCE (ee_msp_table bit for bit), MMEE_CRIT_ENTROPY (the reference's expression log A - B / A with
 * A = sum e^z, B = sum z e^z, no max shift, EE/thresh.py:41-45; LOWER is surer: sweep it negated, scan it with sign -1) or MMEE_CRIT_MARGIN (above,
 * T = 1).  Patience and unknown codes are refused with a message.  logits dev double (E1,N,K), table dev double (E1,N), correct dev uint8 (E1,N) or
 * NULL, references dev int64 (N,) (may be NULL with correct NULL). */
int ee_csf_table(const double* logits, const int64_t* references, int32_t E1, int32_t N, int32_t K, int32_t criterion, double* table,
                 uint8_t* correct, void* stream);
/* The criterion table of MMEE_CRIT_GATE, for ee_gate_scan, ee_threshold_sweep, ee_rule_scan / ee_rule_sweep (sign +1), ee_threshold_search and
 * ee_exit_metrics' table form: head_logits dev float32 (E,N,2) (out_head_logits of a dump-all forward), final_logits dev double (N,K) (the
 * final exit's policy logits), E >= 0, N >= 1, K >= 1.  table dev double (E+1,N): rows 0 .. E-1 the gate score g_e by the device function the
 * decide kernels use (the bits of the forward's decision), row E the max-softmax of final_logits as ee_msp_table writes it.  The `correct`
 * table that goes with it is ee_msp_table's on the policy logits: what leaves under the gate is the classifier(gate input) row. */
int ee_gate_table(const float* head_logits, const double* final_logits, int32_t E, int32_t N, int32_t K, double* table, void* stream);
/* The exit ensemble (definition at ee_set_ensemble) on a dumped array: logits dev double (E1,N,K), the UN-ensembled scaled rows x_e as a
 * dump-all forward returns them in out_all_logits; w dev double (E1,E1), b dev double (E1,K) or NULL; out dev double (E1,N,K), which may not
 * overlap logits.  out[m][n] = y_m of document n by the two device functions the forward's launch calls, so for float32-valued input every
 * output value is exactly a float32 and has the forward's bits.  A NaN input row (an exit the document never reached) gives NaN from that exit
 * on.  The result is a logits array like any other: it goes unchanged into ee_csf_table, the scans, the sweeps, the searches and
 * ee_exit_metrics.  Refused: a NULL logits / w / out, E1, N or K below 1. */
int ee_ensemble_logits(const double* logits, int32_t E1, int32_t N, int32_t K, const double* w, const double* b, double* out, void* stream);
/* Budgeted exits (definition at MMEE_QUOTA_*) on a criterion table: table dev double (E1,N), the criterion c of every document at every exit
 * (ee_csf_table / ee_gate_table / the table of an ensembled array); sign +1 or -1 (-1: entropy); quotas host int32 [E1 - 1], every entry >= 0;
 * mode MMEE_QUOTA_EXACT or MMEE_QUOTA_AT_LEAST; thresholds host double [E1], needed by AT_LEAST (the event is sign * c > sign * thr[e],
 * strict), ignored and may be NULL under EXACT; G >= 1 the group size.  Consecutive groups of G documents are ranked independently, as
 * ceil(N / G) forwards of G documents would be (the last group may be short; a document's slot is its index in the table); the documents
 * that stay at exit e are the ones ranked at exit e + 1; the last exit takes everybody.  exits dev int32 (N).  cuts dev double
 * (groups, E1 - 1, 2) or NULL: the criterion of the last leaver (the leaver every other leaver precedes) and of the first stayer (the stayer
 * that precedes every other stayer) of every group at every exit, NaN where there is none (and where that document's criterion is NaN).
 * workspace dev int32 (N) of scratch.  Two launches per exit below the last one.  With G = N the midpoints of a row of cuts are MSDNet's
 * thresholds: a plain thresholded forward then releases that share of a like batch.  Refused: a NULL table / quotas / exits / workspace,
 * E1 below 1 or above 256, N below 0, G below 1, a sign that is not +-1, an unknown mode, AT_LEAST without thresholds, a negative quota. */
int ee_quota_scan(const double* table, double sign, int32_t E1, int32_t N, const int32_t* quotas, int32_t mode, const double* thresholds,
                  int32_t G, int32_t* exits, double* cuts, int32_t* workspace, void* stream);
/* Model cascades (definition above, behind MMEE_QUOTA_*): the three launches of a stage boundary, handle-free like the other tools; every
 * pointer is a device pointer unless it says host.
 * ee_cascade_select: which of a stage's n documents are deferred.  logits float (n,K) and exit_layer int32 (n): what the stage's forward
 *   delivered, by the stage's document index; orig int32 (n): the documents' original slots, ascending, or NULL: the identity (stage 0);
 *   final_exit = E_s; criterion MMEE_CRIT_MAX_CONFIDENCE, _ENTROPY or _MARGIN; threshold = thresholds_s[E_s].  Writes next_orig int32 (n):
 *   the original slots of the deferred documents in their order (entries past the count are not written), count_dev int32 (1): their
 *   number, and crit_out double (n) or NULL: c of EVERY document.  One workgroup, one launch.
 * ee_cascade_gather: dst[j] <- src[slots[j]] for j < *count_dev, for n_arrays <= 8 arrays at once.  descs HOST array of n_arrays
 *   descriptors; a row is row_bytes bytes, a multiple of 4; src and dst 4-byte aligned and not overlapping; copied in 16-byte pieces when
 *   src, dst and row_bytes are all multiples of 16, else in 8- or 4-byte ones.  slots int32 (cap) with slots[j] a row of every src;
 *   cap >= *count_dev is the static bound that sizes the grid (cap == 0: nothing is launched).  Rows of dst from *count_dev on are not
 *   written.
 * ee_cascade_merge: a later stage's results into the cascade's outputs.  logits float (n,K), exit_layer int32 (n), confidence float (n) by
 *   the stage's document index, slots int32 (n) their original slots; writes out_logits (B,K), out_exit (B) = exit_layer + exit_offset,
 *   out_confidence (B) and out_stage (B) = stage at those slots and nowhere else.  n == 0: nothing is launched.
 * Refused: n or cap below 0, K below 1, final_exit / exit_offset / stage below 0, a criterion that is not one of the three, n_arrays outside
 *   0 .. 8, a row_bytes that is below 4 or no multiple of 4, a misaligned src / dst, NULL pointers where n (cap, n_arrays) is above 0. */
typedef struct ee_cascade_desc {
    const void* src;
    void* dst;
    int64_t row_bytes;
} ee_cascade_desc;
int ee_cascade_select(const float* logits, const int32_t* exit_layer, const int32_t* orig, int32_t n, int32_t K, int32_t final_exit,
                      int32_t criterion, double threshold, int32_t* next_orig, int32_t* count_dev, double* crit_out, void* stream);
int ee_cascade_gather(const ee_cascade_desc* descs, int32_t n_arrays, const int32_t* slots, const int32_t* count_dev, int32_t cap, void* stream);
int ee_cascade_merge(const float* logits, const int32_t* exit_layer, const float* confidence, const int32_t* slots, int32_t n, int32_t K,
                     int32_t exit_offset, int32_t stage, float* out_logits, int32_t* out_exit, float* out_confidence, int32_t* out_stage,
                     void* stream);

/*
 * The threshold search: which thresholds should a deployment run?  Candidate thresholds from the percentiles of the confidence table, V candidate
 * vectors scored as ee_threshold_sweep / ee_rule_sweep score them, and the accuracy / mean-exit Pareto front of the scores, in one call on the
 * device (EE/large_scale.py:46-65 builds the candidates on the host and stops at a dump of every vector's result).  No threshold is uploaded and
 * no per-vector result has to come back.
 *
 * Inputs: conf dev double (E1,N) (for a '<' criterion pass the negated table, which is exact; the thresholds that come back are then negated too),
 * correct dev uint8 (E1,N), P = thresholds per exit; 2 <= E1 <= 64, 1 <= N < 2^24, 2 <= P <= 64.
 *
 * Percentile table, dev double (E1,P): table[e][j] = np.percentile(conf[e], linspace(0, 100, P)[j]) (linear method) for e < E1-1, bit for bit:
 *   q_j = (j * (100 / (P-1))) / 100, the last one 100 / 100; virtual index x = (N-1) * q_j in double; x >= N-1: lo = hi = N-1, t = x + 1; else
 *   lo = floor(x), hi = lo + 1, t = x - lo (functions of N and P only, computed once on the host).  With a = sorted[e][lo], b = sorted[e][hi]:
 *   table = a + (b - a) * t, and b - (b - a) * (1 - t) where t >= 0.5 -- numpy's two-branch lerp, every product rounded before it is added (no fma).
 *   Row E1-1 is 0.0, as generate_thresholds leaves it.
 * Rank table trank[e][j] (internal): the rank of table[e][j] in the sorted row e by the sweeps' rule -- #{m : conf[e][m] < table[e][j]} under
 *   MMEE_SEARCH_REFERENCE, #{m : conf[e][m] <= table[e][j]} under MMEE_SEARCH_POLICY -- so that the integers of a search are exactly those
 *   ee_threshold_sweep / the policy give for the reported vectors.
 *
 * Candidate vectors: V of them, vector v = E1 digits d_e(v) in [0, P), its thresholds table[e][d_e(v)]; the final exit's digit is unused.
 *   MMEE_SEARCH_GRID      the whole grid: V = P^(E1-1) (the argument V is ignored), d_e(v) = (v / P^e) % P.  Refused when V >= 2^32.
 *   MMEE_SEARCH_SAMPLED   1 <= V < 2^32 draws: d_e(v) = ((splitmix64(seed + (v * E1 + e + 1) * 0x9E3779B97F4A7C15) >> 32) * P) >> 32 in 64-bit
 *                         wrap-around arithmetic, splitmix64(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *                         z ^ z >> 31.  A pure function of (seed, v, e).
 *   MMEE_SEARCH_MIXTURES  mixtures dev uint8 (V,E1), 1 <= V < 2^32: the caller's digits (the reference's np.random.seed(42) draw, for one).  A
 *                         digit >= P is the caller's error: it is clamped to P-1 so that nothing is read out of bounds.
 *
 * Exit rule per (vector, document):
 *   MMEE_SEARCH_REFERENCE  ee_threshold_sweep's: the first e with conf[e,n] >= threshold, exit 0 when none fires (the zero last row fires for
 *                          every confidence >= 0).
 *   MMEE_SEARCH_POLICY     what a forward does: the first e < E1-1 with conf[e,n] > threshold (strict), else the final exit E1-1; the last
 *                          threshold is unused.
 * Per vector: hits(v) = sum_n correct[exit, n], exit_sum(v) = sum_n exit, integers; acc / mean_exit dev double (V,) or NULL = sum / N.
 *
 * Front: over exit_sum = 0 .. N (E1-1) (N (E1-1) + 1 buckets, refused above 2^26), bucket[exit_sum] = max_v (hits << 32 | (0xFFFFFFFF - v)):
 * the most hits among the vectors of one exit sum, ties to the LOWEST v.  A bucket is on the front iff some vector has its exit sum and its hits
 * exceed the hits of every bucket of lower exit sum: the strict Pareto front of (fewer exits, more hits).  Deterministic; no sort.  Outputs dev,
 * ascending by exit sum: front_count int32 [1], front_exit_sum int32, front_hits int32, front_vector uint32 (N+1 entries each) and
 * front_thresholds double (N+1, E1) = table[e][d_e(v)] of the entry's vector (column E1-1: 0.0).  Hits rise strictly along the front, so N+1
 * entries always suffice; entries past front_count are not written.
 */
enum { MMEE_SEARCH_GRID = 0, MMEE_SEARCH_SAMPLED = 1, MMEE_SEARCH_MIXTURES = 2 };
enum { MMEE_SEARCH_REFERENCE = 0, MMEE_SEARCH_POLICY = 1 };
int ee_threshold_search(const double* conf, const uint8_t* correct, int32_t E1, int32_t N, int32_t P, int32_t source, int64_t V, uint64_t seed,
                        const uint8_t* mixtures, int32_t semantics, double* table, double* acc, double* mean_exit, int32_t* front_count,
                        int32_t* front_exit_sum, int32_t* front_hits, uint32_t* front_vector, double* front_thresholds, void* stream);

/*
 * The cost-weighted threshold search: the same candidates, scored the same way, but the front is the one of accuracy against COST.  The mean exit
 * index is not what a forward pays: exits sit behind different numbers of layers, and in the packed layout a long document pays many times what a
 * short one pays for the same layer.
 *
 * Inputs: those of ee_threshold_search plus cost, dev uint32 (E1,N): cost[e][n] is what document n costs when it leaves at exit e, in units the
 * caller chooses (sweep.exit_costs gives the path's algorithmic FLOPs).  No monotonicity in e is assumed.  The percentile table, the three digit
 * sources and both exit rules (MMEE_SEARCH_REFERENCE / MMEE_SEARCH_POLICY) are exactly those of ee_threshold_search.
 *
 * Per vector: hits(v) and exit_sum(v) as above, and cost_sum(v) = sum_n cost[exit(v, n)][n] as an exact uint64 (N < 2^24 and 32-bit entries keep it
 * below 2^56: nothing can overflow).  acc / mean_exit dev double (V,) or NULL as above; cost_sum dev uint64 (V,) or NULL.
 *
 * Front: the strict Pareto front of (cost_sum down, hits up).  Vector v is on it iff no vector has cost_sum <= and hits >= with one of the two
 * strict; among vectors of equal (cost_sum, hits) the LOWEST index is the one reported.  As it is computed: over hits = 0 .. N (N + 1 buckets, so
 * ee_threshold_search's bucket limit does not apply), best[h] = the minimum over {v : hits(v) = h} of (cost_sum, v) compared lexicographically;
 * bucket h is on the front iff it is not empty and its cost_sum is below that of every non-empty bucket with MORE hits.  Deterministic: the result
 * does not depend on the launch shape, on the order in which atomics arrive, or on a sort.  Outputs dev, ascending in cost_sum -- which is also
 * strictly ascending in hits --, at most N + 1 entries: front_count int32 [1], front_cost_sum uint64, front_exit_sum int32 (the exit sum of the
 * entry's vector: NOT monotone along this front), front_hits int32, front_vector uint32 (N+1 entries each) and front_thresholds double (N+1, E1) as
 * above; entries past front_count are not written.
 *
 * With cost[e][n] = e the front equals ee_threshold_search's entry for entry: cost_sum = exit_sum, the same hits, vectors and threshold bits.
 *
 * Refusals: every one of ee_threshold_search except the bucket limit, plus a NULL cost and a NULL front_cost_sum; all before any device call.  The
 * call only enqueues on `stream`: nothing is uploaded or downloaded.
 */
int ee_threshold_search_cost(const double* conf, const uint8_t* correct, const uint32_t* cost, int32_t E1, int32_t N, int32_t P, int32_t source,
                             int64_t V, uint64_t seed, const uint8_t* mixtures, int32_t semantics, double* table, double* acc, double* mean_exit,
                             uint64_t* cost_sum, int32_t* front_count, uint64_t* front_cost_sum, int32_t* front_exit_sum, int32_t* front_hits,
                             uint32_t* front_vector, double* front_thresholds, void* stream);

/*
 * The threshold refinement: a local search on the device that IMPROVES candidate threshold vectors, for the models whose grid no search can
 * enumerate (E1 = 24, P = 10: 10^23 vectors).  S independent chains of steepest-ascent coordinate search on the percentile grid, each from its
 * own start, with no host round trip between rounds.  Starts are typically the front of a sampled ee_threshold_search_cost, or the vector under
 * which nobody leaves early.
 *
 * Inputs: those of ee_threshold_search_cost -- conf dev double (E1,N) (for a '<' criterion pass the negated table, which is exact), correct dev
 * uint8 (E1,N), cost dev uint32 (E1,N) or NULL for cost[e][n] = e, P thresholds per exit; 2 <= E1 <= 64, 1 <= N < 2^24, 2 <= P <= 64.
 * Percentile table (E1,P): ee_threshold_search's, bit for bit; row E1-1 is 0.0.
 * Exit rule: MMEE_SEARCH_POLICY only, what a forward does: exit(d, n) = the first e < E1-1 with conf[e][n] > table[e][d_e] (strict), else E1-1.
 * MMEE_SEARCH_REFERENCE is not offered: nothing deploys it.
 *
 * Chains: 1 <= S <= 4096.  Chain s has a start, start[s] dev uint8 (E1,) digits in [0, P) (a digit >= P is clamped to P-1 as in the search; the
 * last digit is unused), a hit value w_s, hit_value dev uint64 (S,), taken as min(w_s, 2^32 - 1): what one more correct document is worth in cost
 * units, and a budget B_s, budget dev uint64 (S,); a NULL budget array means no budget.
 *
 * Score of a digit vector d: hits(d) = sum_n correct[exit(d,n)][n], exit_sum(d) = sum_n exit(d,n), cost_sum(d) = sum_n cost[exit(d,n)][n], an
 * exact uint64 below 2^56, and J(d) = w hits(d) - cost_sum(d) as a signed 64-bit integer (|w hits| < 2^56: it cannot overflow).
 *
 * One round of a live chain at d: the neighbours of d are all d' that differ from d in exactly one digit (e in [0, E1-1), p in [0, P), d'_e = p);
 * a neighbour is admissible iff cost_sum(d') <= B; the best neighbour is the admissible one with the largest J, ties to the lowest e, then the
 * lowest p.  If J(best) > J(d) the chain moves there; otherwise it stops with status 0: no admissible single-exit change improves J.  A chain
 * that has moved in every one of max_rounds rounds (1 <= max_rounds <= 4096) ends with status 1.  A chain whose start already has
 * cost_sum > B ends with status 2, rounds 0, and its outputs describe the start.  J rises strictly with every move, so a chain cannot cycle.
 *
 * As it is computed: for a document with exit x0 under d and next firing exit x1 behind it (E1-1 when none), changing exit e < x0 moves it to e
 * for exactly the digits whose threshold it beats -- a prefix of p, the table ascends --, changing e = x0 moves it on to x1 for the digits whose
 * threshold it does not beat -- a suffix --, and changing e > x0 does nothing: all (E1-1) P neighbour scores come out of one pass of O(E1) work per
 * document, as differences accumulated by integer atomics.  Where a prefix ends is decided by the strict compare of the values (through the
 * searches' rank words), duplicated table values and confidences equal to a threshold included.
 *
 * Outputs, all dev; the first five describe the FINAL vector: digits uint8 (S,E1) (last column 0; required: it holds the chains' vectors while
 * the call runs), thresholds double (S,E1) = table[e][d_e] (last column 0.0), hits int32 (S,), exit_sum int32 (S,), cost_sum uint64 (S,); rounds
 * int32 (S,) = moves made, status int32 (S,) as above, start_hits int32 (S,), start_cost_sum uint64 (S,), table double (E1,P).  Every output but
 * digits is optional (may be NULL).
 *
 * Everything is integers or copied doubles: the result is a pure function of the inputs and does not depend on the launch shape, on the order in
 * which atomics arrive or on which other chains share the call.  The call only enqueues on `stream` -- a fixed list of max_rounds x 2 launches, in
 * which the workgroups of a finished chain return at once --: nothing is uploaded, downloaded or waited for.  Its workspace holds
 * S (E1-1) (P+1) x 16 bytes of difference arrays (ee_threshold_refine_workspace_bytes: all of it).
 *
 * Refusals, all before any device call: NULL conf / correct / start / hit_value / digits, the search's range checks of E1, N and P, S, max_rounds.
 */
int ee_threshold_refine(const double* conf, const uint8_t* correct, const uint32_t* cost, int32_t E1, int32_t N, int32_t P, int32_t S,
                        const uint8_t* start, const uint64_t* hit_value, const uint64_t* budget, int32_t max_rounds, uint8_t* digits,
                        double* thresholds, int32_t* hits, int32_t* exit_sum, uint64_t* cost_sum, int32_t* rounds, int32_t* status,
                        int32_t* start_hits, uint64_t* start_cost_sum, double* table, void* stream);
/* The bytes ee_threshold_refine allocates for its rounds (0 for arguments it would refuse): a pure function, no device. */
size_t ee_threshold_refine_workspace_bytes(int32_t E1, int32_t N, int32_t P, int32_t S);

/*
 * Risk control: which of a list of candidate threshold vectors may be deployed with a PROMISE.  The sweeps, the searches and the refinement
 * return the point that looks best on the table they were given; ee_risk_control returns the cheapest candidate whose risk is at most alpha
 * with probability at least 1 - delta over the draw of the calibration table: Learn-then-Test (Angelopoulos et al. 2021) with fixed-sequence
 * testing, as CATs (Schuster et al., EMNLP 2021) and "Fast yet Safe" (Jazbec et al., NeurIPS 2024) use it; along a front found on OTHER data
 * it is Pareto testing (Laufer-Goldshtein et al. 2023).  THE definition (csrc/risk_control.hip, risk.py and tests/risk_ref.py refer to it).
 *
 * Candidates: thr dev double (V,E1), real thresholds of the criterion, in the caller's order, most conservative first.  conf dev double (E1,N) is
 * the criterion table itself (not negated), sign +1 or -1 (-1: entropy, a learning-to-exit score).
 * Exit of document n under vector v: the first e < E1-1 with sign conf[e][n] > sign thr[v][e], else E1-1.  The test is strict, a NaN criterion
 * never fires, thr[v][E1-1] is not read: the decide kernels' and ee_criterion_scan's rule, for one vector.
 * Loss: loss_q dev uint32 (E1,N) in units of 2^-30: loss_q[e][n] is what it costs in risk that document n leaves at exit e.  A binary loss is
 * exactly 0 or 2^30; a real loss l in [0,1] is min(2^30, ceil(l 2^30)), so that rounding never understates a risk.  Alternatively loss_f64 dev
 * double (E1,N), which the call quantises by that rule into its workspace; a value that is not finite or outside [0,1], and under
 * MMEE_RISK_BINOMIAL a value that is neither 0 nor 1, fails the call with no output written (one synchronise of the stream, as the fits do for a
 * bad label).  Exactly one of the two is given.  The values of a loss_q the caller built are the caller's duty (<= 2^30; 0 or 2^30 under
 * MMEE_RISK_BINOMIAL); whatever they are, nothing is read out of bounds.
 * Per vector, all integers: loss_sum(v) = sum_n loss_q[exit][n] (uint64), exit_sum(v) = sum_n exit (int64), cost_sum(v) = sum_n cost[exit][n]
 * (uint64) with cost dev uint32 (E1,N) as ee_threshold_search_cost takes it, = exit_sum when cost is NULL, and hist(v,e) = #{n : exit = e} (int32
 * (V,E1), optional).  No floating-point atomics: the integers do not depend on the launch shape or on the order in which anything arrives.
 * p-value of H0: R(v) > alpha, n = N.  F(k) = sum_{i <= k} exp(lgamma(n+1) - lgamma(i+1) - lgamma(n-i+1) + i log(alpha) + (n-i) log1p(-alpha)),
 * summed ascending in float64 and clamped to 1: the binomial distribution function, one table of n + 1 entries per call.
 *   MMEE_RISK_BINOMIAL (binary tables only)   p = F(loss_sum / 2^30)
 *   MMEE_RISK_HB (Hoeffding-Bentkus, any table)   r = loss_sum / (n 2^30);  p_H = exp(-n h(r, alpha)) if r < alpha, else 1, with
 *       h(a,b) = a log(a/b) + (1-a) log((1-a)/(1-b)) and 0 log 0 = 0;  p_B = min(1, e F(ceil(loss_sum / 2^30))), the ceil in integers;
 *       p = min(p_H, p_B)
 * Certification at level delta:  MMEE_RISK_FIXED_SEQUENCE: v is certified iff p_u <= delta for every u <= v;  MMEE_RISK_BONFERRONI: iff
 * p_v <= delta / V.  Selected: the certified vector of smallest cost_sum, ties to the lowest v; -1 when none is certified.
 * What is promised, and no more: if the calibration documents are exchangeable with the documents served, and the candidate list was fixed
 * without looking at the calibration table, then P(risk of the selected vector <= alpha) >= 1 - delta.  A front searched on the same table
 * does not qualify: split the table, search on one part, certify on the other.  The risk is marginal over all documents; a document that runs
 * to the final exit contributes its final-exit loss.
 * Outputs, all dev: loss_sum uint64 (V,), exit_sum int64 (V,), cost_sum uint64 (V,), hist int32 (V,E1) or NULL, pvalue double (V,), certified uint8
 * (V,), n_certified int32 [1], selected int32 [1].  The floating-point sums are taken in an order fixed by the launch, which is fixed by (N, V):
 * the outputs are a pure function of the inputs.
 * As it runs: risk_count_kernel (the shape of ee_threshold_sweep's direct kernel, a workgroup's threads striding over a vector's documents; with
 * few vectors several workgroups share one vector and add their integer sums with integer atomics; a call has 10^2 .. 10^4 vectors, the ranked
 * route of the big sweeps is not built here), a lgamma table, risk_cdf_kernel (one workgroup), risk_select_kernel (one workgroup).
 * Refused, each with a message and before any device call: a NULL pointer (cost and hist may be NULL), both or neither of loss_f64 / loss_q,
 * E1 < 1 or > 64, N < 1 or >= 2^24, V < 1 or > 65536, alpha or delta outside (0,1), a sign other than +-1, unknown bound / method codes.
 * Not built: the WSR betting bound, conditional (per-exit) risk control, several risks at once, the ranked scorer for millions of vectors,
 * patience / rule / learning-to-exit / gate decisions (a gate or LTE table can be passed as conf with plain-threshold semantics only).
 *
 * ee_binomial_bounds: one-sided Clopper-Pearson bounds, each at delta, of Q counts: n, k HOST int32 (Q,) (k events in n trials), upper and lower
 * dev double (Q,).  upper = 1 if k = n, else the theta with F(k; n, theta) = delta;  lower = 0 if k = 0, else the theta with
 * 1 - F(k-1; n, theta) = delta, where F(.; n, theta) is the sum above with theta in place of alpha (a term with a zero count times log 0 is the
 * term without it).  Each by exactly 64 bisections of [0,1], every tail one block sum in a fixed order, and the midpoint of the last bracket
 * is returned: a pure function of (n, k, delta).  Refused: NULL pointers, Q < 1 or > 65536, delta outside (0,1), n < 1 or >= 2^24, k < 0 or
 * k > n in any query.
 */
enum { MMEE_RISK_BINOMIAL = 0, MMEE_RISK_HB = 1 };
enum { MMEE_RISK_FIXED_SEQUENCE = 0, MMEE_RISK_BONFERRONI = 1 };
int ee_risk_control(const double* conf, double sign, const double* loss_f64, const uint32_t* loss_q, const uint32_t* cost, int32_t E1, int32_t N,
                    const double* thr, int32_t V, double alpha, double delta, int32_t bound, int32_t method, uint64_t* loss_sum, int64_t* exit_sum,
                    uint64_t* cost_sum, int32_t* hist, double* pvalue, uint8_t* certified, int32_t* n_certified, int32_t* selected, void* stream);
int ee_binomial_bounds(const int32_t* n, const int32_t* k, int32_t Q, double delta, double* upper, double* lower, void* stream);

/*
 * The evaluation report: the seven metrics the reference scores every exit and every policy's predictions with (METRICS of evaluate_checkpoint,
 * EE/eval.py:175-181; calc_metrics, EE/utils.py:226-237) plus the average confidence, on the device, from a dumped array that never leaves it.
 *
 * Inputs, all dev.  The logits form: logits double (E1,N,K), references int64 (N,) with values in [0,K) (a value outside is the caller's error: it
 * is clamped for the lookups and never counts as correct).  The table form (logits == NULL): conf double (E1,N) with values in [0,1], correct uint8
 * (E1,N), as ee_csf_table / ee_msp_table write them; K is not read.  temperatures double (E1,) or NULL (logits form).  exits int32 (N,) or NULL: one
 * exit per document, from a policy scan, a forward or a threshold vector.  n_bins: the ECE bins, <= 0: max(1, min(N - 1, 100)); at most 1024.
 * 1 <= E1 <= 256, 1 <= N <= 2^20 (refused above: the counting sort is O(N^2) per row), K >= 1.
 *
 * Outputs, dev: out double (R, MMEE_METRIC_COUNT), R = E1 + (exits ? 1 : 0), one row per exit and, with exits, row E1 = the OPERATING POINT:
 * document n scored on logits[exits[n]][n] (table form: conf / correct[exits[n]][n]), what eval_model reports for a policy's predictions
 * (EE/eval.py:87-112).  An exit outside [0,E1) is clamped for the lookup, never dereferenced, and not counted in exit_hist.  confusion int64
 * (R,K,K) or NULL: confusion[r][ref][pred] (logits form only; refused in the table form).  exit_hist int64 (E1,) or NULL: the count of exits == e
 * (needs exits).
 *
 * Per (row, document), float64 throughout as the reference evaluates the float64 store; integer quantities keep integer types:
 *   z = logits / T_e when temperatures are given (the operating point: the temperature of the document's own exit); p = softmax(z), max-subtracted
 *   pred = the FIRST maximum of z (np.argmax);  conf = max p = 1 / sum_k exp(z_k - max);  correct = (pred == ref)
 *   brier = sum_k (p_k - [k == ref])^2;   nll = log sum_k exp(z_k - max) - (z_ref - max)
 * Per row:
 *   accuracy = hits / N.   f1_micro: the same number (single-label multiclass: sklearn's micro F1 is the accuracy).
 *   f1_macro from the integer confusion counts: per class 2TP / (2TP + FP + FN), 0 where the denominator is 0, averaged over the classes that occur
 *     in the references or the predictions (sklearn's unique_labels), not over all K.
 *   brier, nll, avg_conf: means over N.
 *   ece: calibration.expected_calibration_error with its defaults, the arguments of ece_logits (EE/metrics.py:479-498).  ONLY this scheme:
 *     equal-mass edges sorted_conf[(k N) / n_bins], k = 0 .. n_bins-1, plus 1.0; bin = searchsorted(edges, conf, side="right") - 1, clipped to
 *     [0, n_bins); integer document / hit counts per bin; sum_b (cnt_b / N) |hit_b / cnt_b - edges[b+1]| (upper-edge proxy, p = 1), bins in order.
 *   aurc: StatsCache.rc_curve_stats + aurc (EE/metrics.py:346-424; AURC_DISPLAY_SCALE = 1).  The documents in ascending conf, TIES IN DOCUMENT
 *     ORDER (a stable sort: the order of ee_threshold_sweep's ranking pass); r_i = 1 - correct_i in that order, S_i = sum_{j >= i} r_j (integers).
 *     risks = [S_0 / N]; t = 0; for i = 0 .. N-2: t += 1, and if i == 0 or c_i != c_{i-1}: append risk S_{i+1} / (N-1-i) and weight t / N, t = 0.
 *     If t > 0 at the end: append the last risk again, with weight t / N.  AURC = sum_j (risk_j + risk_{j+1}) / 2 * w_j; N = 1: no weights, 0.
 *     The reference sorts with numpy's unstable argsort and its result DOES depend on the order inside a tie; the document-order rule is this
 *     library's contract.
 *   In the table form brier, nll and f1_macro are not computed: their entries are NaN.
 * Deviations from the reference, deliberate: (1) its nll passes the logits to sklearn's log_loss, which current sklearn refuses for values above 1;
 * on softmax probabilities it is the plain mean of -log p_ref, which is what is computed here.  (2), (3) its brier_loss and aurc_logits guess from
 * isclose(sum(x), N) whether an input is already probabilities / correctness; here the inputs are always logits and labels.
 *
 * Deterministic: integer atomics for the counts, every float sum in a fixed order; two calls on the same input give the same bits.  The call only
 * enqueues on `stream` (workspace from the stream's pool); nothing is uploaded or downloaded.  Refusals, all before any device call: out NULL,
 * logits without references, the table form without conf / correct or with confusion, exit_hist without exits, E1, N, K, n_bins out of range.
 */
#define MMEE_METRIC_ACCURACY 0
#define MMEE_METRIC_BRIER    1
#define MMEE_METRIC_NLL      2
#define MMEE_METRIC_F1_MICRO 3
#define MMEE_METRIC_F1_MACRO 4
#define MMEE_METRIC_ECE      5
#define MMEE_METRIC_AURC     6
#define MMEE_METRIC_AVG_CONF 7
#define MMEE_METRIC_COUNT    8
int ee_exit_metrics(const double* logits, const int64_t* references, const double* conf, const uint8_t* correct, const double* temperatures,
                    const int32_t* exits, int32_t E1, int32_t N, int32_t K, int32_t n_bins, double* out, int64_t* confusion, int64_t* exit_hist,
                    void* stream);

/*
 * Per-exit temperature fit on the device (TemperatureScaler.set_temperature, EE/generic_scaling.py:64-111, as driven per
 * exit by calibrate(), EE/eval.py:313-337): for every exit e, T[e] = argmin_T mean NLL(softmax(logits[e] / T), labels),
 * starting from T = 1, by Newton iterations on 1/T (the objective is convex in 1/T).  logits dev double (E1,N,K),
 * labels dev int64 (N,) with values in [0,K).  Outputs dev (E1,): temperature; optional nll / accuracy /
 * avg_confidence of the scaled logits and the iteration count.  The ECE that calibrate() also records comes from a
 * remote metric (evaluate.load("jordyvl/ece"), EE/metrics.py:479-498) that is not available offline and is not built.
 */
int ee_temperature_fit(const double* logits, const int64_t* labels, int32_t E1, int32_t N, int32_t K, int32_t max_iter,
                       double* temperature, double* nll, double* accuracy, double* avg_confidence, int32_t* iterations,
                       void* stream);

/*
 * Exit heads fitted on the device from a frozen backbone's CLS rows (the two-stage strategies of the reference train only the heads,
 * EE/models/EE_modules.py:91, 108-113 with the backbone frozen at EE/IC_only.py:189-207; a one-layer ramp head, exit_head_num_layers = 1,
 * EE/models/LayoutLMv3.py:84-93, is one Linear).  Solved per exit e, independently:
 *
 *     L_e(theta) = (1/N) sum_n [ logsumexp(z_n) - z_n[y_n] ] + (l2 / 2) (||W||^2 + ||b||^2),      z_n = W x_n + b
 *
 * with the features X_e (N,H) float32, the labels y (N,) int64 in [0,K) and theta_e = (W_e (K,H), b_e (K,)).  The bias is penalised too:
 * without that the optimum is unique only up to a common shift of b.  With l2 > 0 the objective is l2-strongly convex; l2 <= 0 is refused.
 * All arithmetic is float64 on the float32 features (widening is exact), the logsumexp is max-shifted.
 *
 * ee_head_fit: L-BFGS (`history` pairs, 1 <= history <= 32) from theta = 0 as a fixed launch list of max_evals ticks of [loss / gradient,
 *   controller]; no host round trip between them.  The controller accepts a trial point by the Armijo test (c1 = 1e-4, halving; step 1
 *   except the very first, 1 / ||g||), skips a pair with s.y <= 0 and writes the next trial point.  The test reads
 *   L(trial) <= L + c1 step g.d + 8 eps |L|: the last term allows for the rounding of L, without which nothing passes once a good step's
 *   decrease is below the resolution of L (gradient norms of a few 1e-9).  An exit stops with
 *   status 0 when ||grad L||_2 <= gtol, 1 after max_evals evaluations, 2 after 30 halvings without progress; a stopped exit costs nothing
 *   more.  features dev (E,N,H), 16-byte aligned, H % 4 == 0, 4 <= H <= 1024; 2 <= K <= 64; workspace dev of
 *   ee_head_fit_workspace_bytes(E,N,H,K,history) bytes.  Outputs dev: weight (E,K,H), bias (E,K) float32; optional weight64 / bias64 (the
 *   float64 solution the float32 pair is rounded from), loss, grad_norm (of the returned point), evals, status (E,).
 *   A label outside [0,K) raises the error word at the head of the workspace: the call then fails with a message and has written no
 *   output.  To know that, the call waits for its stream before it returns.
 *   The sums are taken in a fixed order that depends on N alone: two calls return the same bits, and an exit fitted together with others
 *   gets the bits it gets alone.
 * ee_debug_head_lossgrad: ONE evaluation of L_e and grad L_e (the launch a tick makes) at theta64 dev (E, K*H + K): W_e then b_e;
 *   loss dev (E,), grad dev (E, K*H + K).
 * MMEE_HEAD_FIT_SLAB: the rows a workgroup keeps on chip between its logits and its gradient pass.
 */
#define MMEE_HEAD_FIT_SLAB 32
int ee_head_fit(const float* features, const int64_t* labels, int32_t E, int32_t N, int32_t H, int32_t K, double l2, double gtol,
                int32_t max_evals, int32_t history, void* workspace, size_t workspace_bytes, float* weight, float* bias, double* weight64,
                double* bias64, double* loss, double* grad_norm, int32_t* evals, int32_t* status, void* stream);
size_t ee_head_fit_workspace_bytes(int32_t E, int32_t N, int32_t H, int32_t K, int32_t history);
int ee_debug_head_lossgrad(const float* features, const int64_t* labels, const double* theta64, int32_t E, int32_t N, int32_t H, int32_t K,
                           double l2, double* loss, double* grad, void* stream);

/*
 * Two-layer exit heads fitted on the device from the same CLS rows: the reference's default head, exit_head_num_layers = 2
 * (LayoutLMv3Exit, EE/models/LayoutLMv3.py:70-93): dense (H,H) -> tanh -> out_proj (K,H); dropout is the identity (eval).  Solved per
 * exit e, independently, float64 throughout on the float32 features:
 *
 *     a_n = tanh(W1 x_n + b1)                                      W1 (H,H) [out,in], b1 (H,)
 *     z_n = W2 a_n + b2                                            W2 (K,H), b2 (K,)
 *     L(theta) = (1/N) sum_n [ logsumexp(z_n) - z_n[y_n] ] + (l2 / 2) ||theta||^2
 *     theta = W1 row-major, b1, W2 row-major, b2                   P = H*H + H + K*H + K
 *
 * Every block is penalised, the biases included; l2 <= 0 (and NaN) is refused; the logsumexp is max-shifted.  The objective is not convex:
 * the fit promises a stationary point reached by descent from the stated start, not a unique optimum.
 *
 * ee_mlp_head_fit: the L-BFGS of ee_head_fit (the same controller: Armijo test with c1 = 1e-4 and the 8 eps |L| allowance, halving, first
 *   step 1 / ||g||, a pair with s.y <= 0 skipped, restart from steepest descent when the direction is no descent, status 2 after 30 halvings)
 *   from theta0, dev (E,P) float64, which is required: theta = 0 is a saddle the iteration never leaves (with W1 = W2 = 0 only b2 has a
 *   gradient).  A fixed launch list of max_evals ticks of [loss / gradient, controller], no host round trip between them; a stopped exit's
 *   workgroups return at once.  Stopping rules and status codes are those of ee_head_fit: 0 when ||grad L||_2 <= gtol, 1 after max_evals
 *   evaluations, 2 when the line search made no progress.  Limits are those of ee_head_fit: features dev (E,N,H), 16-byte aligned,
 *   H % 4 == 0, 4 <= H <= 1024; 2 <= K <= 64; 1 <= history <= 32.  workspace dev of ee_mlp_head_fit_workspace_bytes(E,N,H,K,history) bytes:
 *   8 E P (5 + 2 history) for the controller's vectors + 8 E N (H + K + 1) for the hidden rows, the logits and the rows' losses (+ < 2 KB
 *   of control words) -- at N = 40 000, H = 768, K = 16, history = 8: 100 MB + 251 MB an exit.
 *   Outputs dev: dense_weight (E,H,H), dense_bias (E,H), weight (E,K,H), bias (E,K) float32; optional theta64 (E,P), the float64 point they
 *   are rounded from; optional loss, grad_norm (of the returned point), evals, status (E,).
 *   A label outside [0,K) fails the call with no output written; the call learns of it by the one wait after the last launch.
 *   No floating-point atomics: every sum runs in an order that depends on (N, H, K) alone, so two calls return the same bits and an exit
 *   fitted together with others gets the bits it gets alone.
 * ee_debug_mlp_head_lossgrad: ONE evaluation of L_e and grad L_e (the launches a tick makes) at theta64 dev (E,P); loss dev (E,), grad dev
 *   (E,P) in the layout of theta.
 * MMEE_MLP_HEAD_FIT_ROWS: the largest number of rows any of the fit's kernels treats as one tile (the row tile of its two GEMM kernels).
 */
#define MMEE_MLP_HEAD_FIT_ROWS 64
int ee_mlp_head_fit(const float* features, const int64_t* labels, const double* theta0, int32_t E, int32_t N, int32_t H, int32_t K, double l2,
                    double gtol, int32_t max_evals, int32_t history, void* workspace, size_t workspace_bytes, float* dense_weight,
                    float* dense_bias, float* weight, float* bias, double* theta64, double* loss, double* grad_norm, int32_t* evals,
                    int32_t* status, void* stream);
size_t ee_mlp_head_fit_workspace_bytes(int32_t E, int32_t N, int32_t H, int32_t K, int32_t history);
int ee_debug_mlp_head_lossgrad(const float* features, const int64_t* labels, const double* theta64, int32_t E, int32_t N, int32_t H, int32_t K,
                               double l2, double* loss, double* grad, void* stream);

/*
 * Exit heads fitted by distillation from the final classifier, for CLS rows that have no labels (self-distillation with the backbone frozen,
 * as FastBERT trains its exits; the reference declares the knobs -- EETrainingArguments(alpha = 1, temperature = 1), EE/models/EE_modules.py:
 * 288-298 -- and implements nothing behind them).  Both head types, per exit e, independently; t (N,K) float32 are the final classifier's
 * logits on the same documents, the same for every exit:
 *
 *     z_n = head_theta(x_n)                  one Linear (ee_head_fit), or dense -> tanh -> out_proj (ee_mlp_head_fit)
 *     q_n = softmax(t_n / T)                 p_n = softmax(z_n)                 pT_n = softmax(z_n / T)
 *     L_e(theta) = (1/N) sum_n [ (1 - alpha) (logsumexp(z_n) - z_n[y_n]) + alpha T^2 KL(q_n || pT_n) ] + (l2 / 2) ||theta||^2
 *     KL(q || p) = sum_k q_k (log q_k - log p_k)
 *     dL/dz_n = (1/N) [ (1 - alpha) (p_n - onehot(y_n)) + alpha T (pT_n - q_n) ]
 *
 * All arithmetic is float64 on the float32 inputs.  Every softmax and log-softmax is max-shifted; log q and log pT are the shifted logits
 * minus the log of their sum of exponentials, never the log of a probability, so a q_k that underflows to 0 contributes exactly 0.  The sum
 * q log q is kept: L's soft term is a true KL, >= 0 up to rounding.  0 <= alpha <= 1; the temperature T is finite and > 0; l2 > 0 as for the
 * fits above (every parameter is penalised, and for 0 <= alpha <= 1 the one-layer objective stays l2-strongly convex).  At alpha = 1 the
 * labels are ignored entirely: the pointer may be NULL and is not range-checked.  At alpha < 1 labels are required and checked as above.
 * At alpha = 0 the objective is ee_head_fit's (ee_mlp_head_fit's); the teacher is still required and checked.
 *
 * ee_head_fit_distill / ee_mlp_head_fit_distill: limits, workspaces (ee_head_fit_workspace_bytes / ee_mlp_head_fit_workspace_bytes), outputs,
 *   the L-BFGS, stopping rules and status codes are those of ee_head_fit / ee_mlp_head_fit (theta0 required for the two-layer head).
 *   The error word at the head of the workspace: bit 0 a label outside [0,K), bit 1 a teacher logit that is not finite (a dump-all forward
 *   marks the rows a document never reached with NaN).  Either fails the call with a message and leaves no output written; the call learns
 *   of it by the one wait after its last launch.  Sums run in the fixed orders of ee_head_fit / ee_mlp_head_fit: two calls return the same
 *   bits, and an exit fitted together with others gets the bits it gets alone.
 * ee_debug_head_distill_lossgrad / ee_debug_mlp_head_distill_lossgrad: ONE evaluation of L_e and grad L_e at theta64 dev (E,P), as
 *   ee_debug_head_lossgrad / ee_debug_mlp_head_lossgrad.
 */
int ee_head_fit_distill(const float* features, const float* teacher_logits, const int64_t* labels, int32_t E, int32_t N, int32_t H, int32_t K,
                        double alpha, double temperature, double l2, double gtol, int32_t max_evals, int32_t history, void* workspace,
                        size_t workspace_bytes, float* weight, float* bias, double* weight64, double* bias64, double* loss, double* grad_norm,
                        int32_t* evals, int32_t* status, void* stream);
int ee_debug_head_distill_lossgrad(const float* features, const float* teacher_logits, const int64_t* labels, const double* theta64, int32_t E,
                                   int32_t N, int32_t H, int32_t K, double alpha, double temperature, double l2, double* loss, double* grad,
                                   void* stream);
int ee_mlp_head_fit_distill(const float* features, const float* teacher_logits, const int64_t* labels, const double* theta0, int32_t E, int32_t N,
                            int32_t H, int32_t K, double alpha, double temperature, double l2, double gtol, int32_t max_evals, int32_t history,
                            void* workspace, size_t workspace_bytes, float* dense_weight, float* dense_bias, float* weight, float* bias,
                            double* theta64, double* loss, double* grad_norm, int32_t* evals, int32_t* status, void* stream);
int ee_debug_mlp_head_distill_lossgrad(const float* features, const float* teacher_logits, const int64_t* labels, const double* theta64, int32_t E,
                                       int32_t N, int32_t H, int32_t K, double alpha, double temperature, double l2, double* loss, double* grad,
                                       void* stream);

/*
 * The four head fits above with a weight per (exit, document): exit e under an early-exit policy only sees the documents no earlier exit
 * released ("train by exiting already when CSF is high enough", EE/models/EE_modules.py:33-37), a class-imbalanced set wants balanced
 * classes, and a held-out fold is a 0/1 mask over features that stay where they are.  Per exit e, independently, with w (E,N) float32,
 * w[e][n] >= 0 and finite, W_e = sum_n w[e][n] > 0:
 *
 *     L_e(theta) = (1 / W_e) sum_n w[e][n] l_n(theta) + (l2 / 2) ||theta||^2
 *
 * l_n is the row loss of the unweighted fit: logsumexp(z_n) - z_n[y_n] (ee_head_fit, ee_mlp_head_fit), or the mixed
 * (1 - alpha) CE + alpha T^2 KL row loss of the distilled fits.  The penalty, the L-BFGS, the stopping rules, the status codes and the
 * limits are those of the unweighted fits; the one-layer problem stays l2-strongly convex.  All-ones weights are the unweighted fit bit
 * for bit, and w and c w with c a power of two return the same bits.
 *
 * teacher_logits == NULL selects the labelled objective: alpha must then be 0, temperature is ignored and labels are required.  Otherwise
 * the arguments are those of the distilled fits (labels may be NULL at alpha == 1).  weights dev (E,N) float32 is required.
 * How: one kernel per call sums W_e in float64 in a fixed order and writes scale[e][n] = (double) w[e][n] * ((double) N / W_e) into the
 * workspace (8 bytes per (exit, row) on top of the unweighted workspace: ee_head_fit_weighted_workspace_bytes /
 * ee_mlp_head_fit_weighted_workspace_bytes); the row step multiplies the row's N dL/dz and its loss by it, as one last multiplication, and
 * everything behind the row step is the unweighted fit's, division by N included.  A row with w[e][n] == 0 contributes zeros: neither its
 * label nor its teacher row is read or checked, so they may hold anything.  Its FEATURES still pass through the gradient sums as 0 * x
 * and must be finite: 0 * NaN is not defended against.
 * The error word: bits 0 and 1 as above (on rows of positive weight), bit 2 a weight that is negative or not finite, bit 3 an exit whose
 * weights sum to zero.  Each fails the call with a message and leaves no output written; the call learns of it by the one wait after its
 * last launch.  Determinism as above: no floating-point atomics, every sum in an order that depends on (N, H, K) alone, nothing depends
 * on E, two calls return the same bits.
 * ee_debug_head_weighted_lossgrad / ee_debug_mlp_head_weighted_lossgrad: ONE evaluation of L_e and grad L_e at theta64 dev (E,P), as the
 *   hooks above; the row scales are made inside the call.
 */
int ee_head_fit_weighted(const float* features, const int64_t* labels, const float* teacher_logits, const float* weights, int32_t E, int32_t N,
                         int32_t H, int32_t K, double alpha, double temperature, double l2, double gtol, int32_t max_evals, int32_t history,
                         void* workspace, size_t workspace_bytes, float* weight, float* bias, double* weight64, double* bias64, double* loss,
                         double* grad_norm, int32_t* evals, int32_t* status, void* stream);
size_t ee_head_fit_weighted_workspace_bytes(int32_t E, int32_t N, int32_t H, int32_t K, int32_t history);
int ee_debug_head_weighted_lossgrad(const float* features, const int64_t* labels, const float* teacher_logits, const float* weights,
                                    const double* theta64, int32_t E, int32_t N, int32_t H, int32_t K, double alpha, double temperature, double l2,
                                    double* loss, double* grad, void* stream);
int ee_mlp_head_fit_weighted(const float* features, const int64_t* labels, const float* teacher_logits, const float* weights, const double* theta0,
                             int32_t E, int32_t N, int32_t H, int32_t K, double alpha, double temperature, double l2, double gtol,
                             int32_t max_evals, int32_t history, void* workspace, size_t workspace_bytes, float* dense_weight, float* dense_bias,
                             float* weight, float* bias, double* theta64, double* loss, double* grad_norm, int32_t* evals, int32_t* status,
                             void* stream);
size_t ee_mlp_head_fit_weighted_workspace_bytes(int32_t E, int32_t N, int32_t H, int32_t K, int32_t history);
int ee_debug_mlp_head_weighted_lossgrad(const float* features, const int64_t* labels, const float* teacher_logits, const float* weights,
                                        const double* theta64, int32_t E, int32_t N, int32_t H, int32_t K, double alpha, double temperature,
                                        double l2, double* loss, double* grad, void* stream);

/*
 * The learning-to-exit classifier (ee_config.use_lte) fitted on the device from the CLS rows of a frozen backbone.  The reference trains it
 * inside EETrainer (EE/models/LayoutLMv3.py:795-857: lte_loss_fct = MSELoss against 1 - lte_gold, one MSE per exit, summed); here it is one
 * deterministic batch problem.  ONE classifier theta = (w (H,), b) is shared by all encoder exits, as in the reference (init_lte: one
 * nn.Linear(H, 1)).  With x_{e,n} the float32 CLS row leaving encoder exit e (out_hidden_cls), a = w . x + b, s = 1 / (1 + exp(-a)) and
 * targets t_{e,n} in [0, 1] ("exit e is wrong on document n"):
 *
 *     L(theta) = sum_e (1/N) sum_n l(a_{e,n}, t_{e,n}) + (l2 / 2) (||w||^2 + b^2)
 *     MMEE_LTE_LOSS_MSE = 0:  l = (s - t)^2                               dl/da = 2 (s - t) s (1 - s)
 *     MMEE_LTE_LOSS_BCE = 1:  l = max(a, 0) + log1p(exp(-|a|)) - t a      dl/da = s - t
 *
 * MSE is the reference's loss.  It is not convex: status 0 promises a stationary point reached by descent from the start, not a unique
 * optimum.  BCE is the convex alternative: l2-strongly convex, one optimum.  All arithmetic is float64 on the float32 rows (widening is exact);
 * the softplus of BCE is shifted, so |a| of several hundred is finite.  l2 <= 0 (and NaN) is refused.  The bias is penalised, as in ee_head_fit.
 * Deviation from the reference, deliberate: an exit at the last layer is not special-cased (the reference substitutes the final logits there);
 * its rows and targets enter like any other exit's.  Per-exit loss weights, embedding-level exits, BEiT handles and an unfrozen backbone are out
 * of scope; so are gates (under the gate strategy the policy reads classifier(gate input): the 2-logit gate head decides nothing here).
 *
 * ee_lte_fit: the L-BFGS of ee_head_fit -- the same controller kernel on one vector of H + 1 parameters: Armijo test with c1 = 1e-4 and the
 *   8 eps |L| allowance, halving, first step 1 / ||g||, a pair with s.y <= 0 skipped -- from theta0, dev (H + 1,) float64: w then b; NULL = 0.
 *   A fixed launch list of max_evals ticks of [loss / gradient, reduce, controller], no host round trip between them; once stopped, the
 *   remaining workgroups return at once.  Stopping rules and status codes are ee_head_fit's: 0 when ||grad L||_2 <= gtol, 1 after max_evals
 *   evaluations, 2 after 30 halvings without progress.  features dev (E,N,H) float32, 16-byte aligned, H % 4 == 0, 4 <= H <= 1024; targets dev
 *   (E,N) float64; 1 <= E <= 64; 1 <= history <= 32; workspace dev of ee_lte_fit_workspace_bytes(E,N,H,history) bytes.  Outputs dev: weight
 *   (1,H), bias (1,) float32 -- the tensors layoutlmv3.encoder.lte_classifier.weight / .bias; optional theta64 (H + 1,), the float64 point
 *   they are rounded from; optional loss_out, grad_norm (of the returned point), evals, status (one element each).
 *   A target outside [0, 1] or NaN fails the call with no output written; the call learns of it by the one wait after the last launch.
 *   One evaluation reads every feature row from HBM once: a wave holds a row in registers (lane l: columns 4l + 256k + j, the order of the
 *   forward's score) between its dot product and its contribution dl/da * x to the gradient.  No floating-point atomics: a workgroup adds
 *   its waves in LDS in wave order and writes one partial (dw, db, loss) per row chunk; the chunking is a function of N alone; the partials
 *   are added in chunk order, the exits in ascending order, then the penalty.  Two calls return the same bits.
 * ee_debug_lte_lossgrad: ONE evaluation of L and grad L (the launches a tick makes) at theta64 dev (H + 1,); loss_out dev one double, grad dev
 *   (H + 1,).  A bad target fails the call.
 * ee_lte_targets: from the policy logits dev float32 (E,N,K) (out_all_logits of the encoder exits) and labels dev int64 (N,):
 *   targets[e,n] = 1 - [argmax_k logits[e,n,k] == labels[n]], the first maximum winning, dev float64 (E,N).  A label outside [0,K) or a NaN
 *   logit (a row its document never reached) fails the call with nothing written.  Waits for the stream once.
 * ee_lte_scores: scores[e,n] = 1 / (1 + exp(-(w . x_{e,n} + b))) dev float64 (E,N) from a float32 weight (1,H) (16-byte aligned) and bias (1,):
 *   the expression and summation order of ee_config.use_lte, unrounded -- the rows sweep.lte_sweep and ee_lte_scan take.
 * MMEE_LTE_FIT_ROWS: the rows a workgroup of the loss / gradient kernel treats as a unit (four waves, four rows in flight each).
 */
#define MMEE_LTE_LOSS_MSE 0
#define MMEE_LTE_LOSS_BCE 1
#define MMEE_LTE_FIT_ROWS 16
int ee_lte_fit(const float* features, const double* targets, const double* theta0, int32_t E, int32_t N, int32_t H, int32_t loss, double l2,
               double gtol, int32_t max_evals, int32_t history, void* workspace, size_t workspace_bytes, float* weight, float* bias,
               double* theta64, double* loss_out, double* grad_norm, int32_t* evals, int32_t* status, void* stream);
size_t ee_lte_fit_workspace_bytes(int32_t E, int32_t N, int32_t H, int32_t history);
int ee_debug_lte_lossgrad(const float* features, const double* targets, const double* theta64, int32_t E, int32_t N, int32_t H, int32_t loss,
                          double l2, double* loss_out, double* grad, void* stream);
int ee_lte_targets(const float* logits, const int64_t* labels, int32_t E, int32_t N, int32_t K, double* targets, void* stream);
int ee_lte_scores(const float* features, const float* weight, const float* bias, int32_t E, int32_t N, int32_t H, double* scores, void* stream);

/*
 * The exit ensemble's weights (definition at ee_set_ensemble) from a dumped array, on the device.  Per exit m, in float64,
 *     L_m(w_m, b_m) = (1/N) sum_n [logsumexp(a_m,n) - a_m,n[y_n]] + (l2/2) (|w_m - e_m|^2 + |b_m|^2)
 * with a_m,n the ensemble row of document n before its rounding to float32 and e_m the unit vector of the plain exit: the penalty pulls toward
 * "no ensemble".  Entries j > m of w_m have zero gradient and stay exactly 0.  l2 > 0 makes every L_m strongly convex: one optimum.  The start
 * is w_m = e_m, b_m = 0 (or w0 / b0, dev double (E1,E1) / (E1,K), each or NULL; entries of w0 above the diagonal are ignored).  Because the
 * penalty vanishes at the default start and the driver only accepts descent steps, loss[m] never exceeds the plain exit's mean NLL.
 *   logits dev double (E1,N,K): UN-ensembled scaled rows, as a dump-all forward returns them; labels dev int64 (N,).
 *   Outputs, dev: w double (E1,E1), b double (E1,K) -- what ee_set_ensemble and ee_ensemble_logits take, after a copy to the host for the
 *   former; loss, grad_norm double (E1,), evals, status int32 (E1,), each or NULL, as ee_head_fit reports them (status 0: converged to gtol).
 * The L-BFGS driver, its budget (gtol, max_evals, history), the workspace convention and the error convention are ee_head_fit's: a label outside
 * [0,K) or a logit that is not finite (a NaN row: an exit a document never reached) fails the call and no output is written.  Deterministic to the
 * bit (no floating-point atomics, every sum in a fixed order), and an exit gets the same bits whatever E1 is: alone, in a table cut behind it, or
 * among all.  Refused: E1 outside [1, MMEE_MAX_ENCODER_EXITS + 4], K outside [2, 64], E1 (3 K + E1 + 2) > 7680 (a workgroup holds one
 * document's rows of every exit in LDS), l2 <= 0.  Not built: sample or reach weights, per-class weights. */
size_t ee_ensemble_fit_workspace_bytes(int32_t E1, int32_t N, int32_t K, int32_t history);
int ee_ensemble_fit(const double* logits, const int64_t* labels, const double* w0, const double* b0, int32_t E1, int32_t N, int32_t K, double l2,
                    double gtol, int32_t max_evals, int32_t history, void* workspace, size_t workspace_bytes, double* w, double* b, double* loss,
                    double* grad_norm, int32_t* evals, int32_t* status, void* stream);

/*
 * 2-way gate heads from a frozen backbone's CLS rows: the heads MMEE_CRIT_GATE scores (one-layer gates, exit_head_num_layers == 1).  The
 * reference trains gates with nn.BCEWithLogitsLoss() against the one-hot of "classifier(gate input) is right here"
 * (EE/models/LayoutLMv3.py:764-781); on a frozen backbone that is, per exit e, with targets c[e][n] in [0, 1] (hard 0 / 1, or soft) and
 * z = W x + b in R^2,
 *     L_e(W, b) = (1 / (2N)) sum_n [ bce(z_1, c) + bce(z_0, 1 - c) ] + (l2 / 2)(||W||^2 + ||b||^2),     bce(z, t) = softplus(z) - t z,
 * the mean over the 2N elements of the (N, 2) logits that BCEWithLogitsLoss takes; column 1 is "correctly gated".  Arithmetic is float64 on the
 * float32 rows; softplus(z) = max(z, 0) + log1p(exp(-|z|)) does not overflow.  Strongly convex for l2 > 0: one optimum.  The two columns do
 * not interact: column j is ee_lte_fit's MMEE_LTE_LOSS_BCE problem on one exit with targets t_j and 2 l2 (the objectives differ by the factor 1/2).
 * ee_head_fit_gate: features dev float32 (E,N,H), targets dev double (E,N); everything else -- l2, gtol, max_evals, history, the workspace
 *   (ee_head_fit_workspace_bytes(E, N, H, 2, history)), the outputs weight (E,2,H) / bias (E,2) and their float64 forms, loss, grad_norm, evals,
 *   status -- is ee_head_fit's at K = 2, and so are the kernels (the same slab walk with another row step), the L-BFGS driver and the launch
 *   list: no floating-point atomics, every sum in a fixed order that is a function of N alone, deterministic to the bit, an exit fitted
 *   alone gets the bits it gets among others.  A target that is not finite or lies outside [0, 1] fails the call through the error word; no
 *   output is written then.  Limits: 4 <= H <= 1024, H % 4 == 0.
 * ee_debug_head_gate_lossgrad: ONE evaluation at theta64 dev double (E, 2H + 2) (W row-major, then b): loss dev double (E,), grad (E, 2H + 2).
 */
int ee_head_fit_gate(const float* features, const double* targets, int32_t E, int32_t N, int32_t H, double l2, double gtol, int32_t max_evals,
                     int32_t history, void* workspace, size_t workspace_bytes, float* weight, float* bias, double* weight64, double* bias64,
                     double* loss, double* grad_norm, int32_t* evals, int32_t* status, void* stream);
int ee_debug_head_gate_lossgrad(const float* features, const double* targets, const double* theta64, int32_t E, int32_t N, int32_t H, double l2,
                                double* loss, double* grad, void* stream);

/*
 * Two-layer 2-way gate heads (exit_head_num_layers == 2, the reference's default depth: dense (H,H) -> tanh -> out_proj (2,H)) from the same
 * CLS rows and the same targets: the gate objective above on ee_mlp_head_fit's head.  Per exit e, independently, with x_n the float32 CLS row,
 * c = targets[e][n] in [0, 1] and theta = (W1 (H,H), b1 (H,), W2 (2,H), b2 (2,)) in ee_mlp_head_fit's layout at K = 2 (P = H*H + 3H + 2):
 *
 *     z_n = W2 tanh(W1 x_n + b1) + b2                              in R^2; column 1 is "correctly gated"
 *     L_e(theta) = (1 / (2N)) sum_n [ bce(z_1, c) + bce(z_0, 1 - c) ] + (l2 / 2) ||theta||^2
 *     bce(z, t) = max(z, 0) + log1p(exp(-|z|)) - t z               dL/dz_j = (sigmoid(z_j) - t_j) / (2N),  t_1 = c, t_0 = 1 - c
 *
 * nn.BCEWithLogitsLoss() on the (N, 2) gate logits, as for ee_head_fit_gate.  Arithmetic is float64 on the float32 rows; the softplus does not
 * overflow (logits of several hundred stay finite).  Every block is penalised; l2 <= 0 (and NaN) is refused.  The objective is NOT convex:
 * status 0 promises ||grad L||_2 <= gtol at a point reached by descent from theta0, as for ee_mlp_head_fit, not a unique optimum.
 *
 * ee_mlp_head_fit_gate: features dev float32 (E,N,H), targets dev double (E,N), theta0 dev double (E,P), required (theta = 0 is a saddle).
 *   Everything else -- l2, gtol, max_evals, history, the workspace (ee_mlp_head_fit_workspace_bytes(E, N, H, 2, history)), the outputs
 *   dense_weight (E,H,H), dense_bias (E,H), weight (E,2,H), bias (E,2), theta64 (E,P), loss, grad_norm, evals, status, the L-BFGS, the stopping
 *   rules and the status codes -- is ee_mlp_head_fit's at K = 2, and so are six of the seven launches of an evaluation: one row kernel takes the
 *   softmax kernel's place.  Limits: 4 <= H <= 1024, H % 4 == 0, features 16-byte aligned, 1 <= history <= 32.
 *   A target that is not finite or lies outside [0, 1] raises bit 0 of the error word: the call fails with a message and has written no
 *   output; it learns of it by the one wait after its last launch.
 * ee_mlp_head_fit_gate_weighted: the same with weights dev float32 (E,N), required (the unweighted entry point takes none), w[e][n] >= 0 and
 *   finite, W_e = sum_n w[e][n] > 0: the data term becomes (1 / (2 W_e)) sum_n w[e][n] [ ... ].  How: scale[e][n] = w[e][n] N / W_e, made once
 *   per call as for ee_mlp_head_fit_weighted, multiplies the row's loss and its N dL/dz as the last multiplication; the workspace is
 *   ee_mlp_head_fit_weighted_workspace_bytes(E, N, H, 2, history).  A row of weight zero contributes zeros and its target is not read or
 *   checked (it may be NaN); its features must be finite.  Error-word bit 2 a weight that is negative or not finite, bit 3 an exit whose
 *   weights sum to zero, both looked at before bit 0.  All-ones weights are the unweighted fit bit for bit; w and c w with c a power of two
 *   return the same bits.
 *   Determinism, both: no floating-point atomics, every sum in an order that depends on (N, H) alone, nothing depends on E -- two calls return
 *   the same bits, and an exit fitted together with others gets the bits it gets alone.
 * ee_debug_mlp_head_gate_lossgrad / ee_debug_mlp_head_gate_weighted_lossgrad: ONE evaluation of L_e and grad L_e at theta64 dev (E,P): loss dev
 *   (E,), grad dev (E,P) in the layout of theta; the weighted hook makes the row scales inside the call.
 */
int ee_mlp_head_fit_gate(const float* features, const double* targets, const double* theta0, int32_t E, int32_t N, int32_t H, double l2, double gtol,
                         int32_t max_evals, int32_t history, void* workspace, size_t workspace_bytes, float* dense_weight, float* dense_bias,
                         float* weight, float* bias, double* theta64, double* loss, double* grad_norm, int32_t* evals, int32_t* status,
                         void* stream);
int ee_mlp_head_fit_gate_weighted(const float* features, const double* targets, const float* weights, const double* theta0, int32_t E, int32_t N,
                                  int32_t H, double l2, double gtol, int32_t max_evals, int32_t history, void* workspace, size_t workspace_bytes,
                                  float* dense_weight, float* dense_bias, float* weight, float* bias, double* theta64, double* loss,
                                  double* grad_norm, int32_t* evals, int32_t* status, void* stream);
int ee_debug_mlp_head_gate_lossgrad(const float* features, const double* targets, const double* theta64, int32_t E, int32_t N, int32_t H, double l2,
                                    double* loss, double* grad, void* stream);
int ee_debug_mlp_head_gate_weighted_lossgrad(const float* features, const double* targets, const float* weights, const double* theta64, int32_t E,
                                             int32_t N, int32_t H, double l2, double* loss, double* grad, void* stream);

/*
 * Device-side input feed (replaces the host image processor + collator in front of the model, EE/data/RVL_CDIP.py:246-262
 * and EE/utils.py:93-98, 173).
 *
 * ee_preprocess_images: B raw page images -> pixel_values (B,3,R,R) float32.  `images` dev uint8: the images packed back to
 *   back, each HWC RGB (c = 3) or HW greyscale (c = 1, replicated to 3 channels like Image.convert("RGB")); `desc` dev array
 *   of B records {int64 offset; int32 h, w, c, pad}.  Resize = Pillow Image.resize(BILINEAR) bit for bit, then HF rescale
 *   (1/255) and normalise (mean = std = 0.5).  `workspace` dev scratch of
 *   ee_preprocess_workspace_bytes(B, R, max_h) bytes (max_h = largest image height).  resized_u8 (B,R,R,3) optional.
 *   The caller's duty: every side h, w of every image is in [1, 31 R], every h <= max_h, and every image lies inside `images` (any byte
 *   offset; no alignment is needed).  The descriptors are on the device, so the entry point cannot check them; a side above 31 R needs
 *   more than the 64 filter taps the tables hold per output pixel, the taps are cut off and the pixels are wrong WITHOUT an error (the
 *   package's feed.preprocess_images / DeviceFeeder check the sides on the host and raise).  max_h <= 31 R is checked here.
 * ee_collate_pad: ragged token streams (ids dev int64 [total], boxes dev int64 [total,4], offsets dev int64 [B+1]) ->
 *   max_length tensors (B,T): input_ids padded with pad_id, attention_mask, bbox padded with zeros; longer inputs truncated.
 */
int ee_preprocess_images(const uint8_t* images, const void* desc, int32_t B, int32_t R, int32_t max_h, void* workspace,
                         size_t workspace_bytes, float* pixel_values, uint8_t* resized_u8, void* stream);
size_t ee_preprocess_workspace_bytes(int32_t B, int32_t R, int32_t max_h);
int ee_collate_pad(const int64_t* ids, const int64_t* boxes, const int64_t* offsets, int32_t B, int32_t T, int64_t pad_id,
                   int64_t* out_ids, int64_t* out_mask, int64_t* out_bbox, void* stream);

/* Per-kernel timing of subsequent ee_forward calls with HIP events recorded on the launch stream (adds two event
 * records per launch; keep it off in timed runs).  ee_profile(h, 1) arms it and clears old records; every ee_forward
 * replaces the records.  ee_profile_read synchronises the device and returns, for kernel role idx = 0,1,..., the
 * role name as "role|hip_kernel_symbol(s)", the summed milliseconds and the number of timed launches of the last
 * ee_forward; it returns 2 when idx is past the last role. */
int ee_profile(ee_handle* h, int32_t enable);
int ee_profile_read(ee_handle* h, int32_t idx, char* name_out, int32_t name_cap, double* total_ms, int32_t* launches);

/* Micro-benchmark / unit-test hook: ONE launch of the path's GEMM kernel, Cout[M,N] = epi(A[M,K] W[N,K]^T + bias (+ resid)),
 * epi 0 = bias, 1 = GELU(erf), 2 = + residual, 3 = tanh; all pointers dev float; N % 128 == 0, K % 32 == 0.  epi | 256 selects the
 * LDS-DMA staging kernel (the one the path launches); a bare epi runs the register-staged kernel.  epi | 16 = static grid stride
 * instead of the work queues.
 * wgs_per_cu sizes the persistent grid (0 = default).  row_src (dev int32 [M] or NULL) gathers the A (and residual) rows as
 * the layer after an exit stage does.  clk_probe (dev, 2 x grid uint64, or NULL): per workgroup
 * {shader cycles, 100 MHz real-time ticks} spent in the kernel, i.e. the clock the chip held (diagnostic). */
int ee_debug_gemm(const float* A, const float* W, const float* bias, const float* resid, float* Cout, int32_t M, int32_t N,
                  int32_t K, int32_t epi, int32_t wgs_per_cu, const int32_t* row_src, uint64_t* clk_probe, void* stream);

/* Unit-test / micro-benchmark hook of the split-precision GEMM (MMEE_PREC_F32_SPLIT): the f32 inputs A [rows_A, K] and
 * W [N, K] are converted to split-f16 rows with the given power-of-two scales, then `iters` launches of the kernel compute
 * Cout = epi(A[row_src ? row_src[r] : r] W^T + bias (+ resid)).  out_split != 0: Cout receives split-f16 rows (64-byte
 * groups [hi 16 f16 | lo 16 f16]) scaled by out_scale instead of f32.  ms_out (host float[2], may be NULL): [0] = average
 * milliseconds per launch, [1] = shader clock in GHz when a diagnostic bit is set in epi (bits 4..: timing diagnostics).  N % 256 == 0, K % 32 == 0
 * (gemm_split_supports).  row_src must be non-decreasing: the kernel addresses the gathered A rows of a tile as offsets from its first one. */
int ee_debug_gemm_split(const float* A, const float* W, const float* bias, const float* resid, float* Cout, int32_t M, int32_t N,
                        int32_t K, int32_t epi, int32_t out_split, float a_scale, float w_scale, float out_scale,
                        const int32_t* row_src, int32_t rows_A, int32_t iters, float* ms_out, void* stream);

/* The same hook for the residual epilogue as the layers launch it (attention output, FFN down): f32 output, a residual of its own rows.
 * resid is f32 [rows_resid, N]; resid_scale > 0 (a power of two) converts it to split-f16 rows of that scale first, as the layers' residual
 * (a LayerNorm output) is kept, resid_scale == 0 passes it on as f32.  Cout[r] = A[row_src ? row_src[r] : r] W^T + bias +
 * resid[resid_row_src ? resid_row_src[r] : r]; row_src must be non-decreasing, resid_row_src may be any rows; both are checked against
 * rows_A / rows_resid.  route: 0 = the tile configuration the row count selects, as in a forward; 1 = the 128 x 128 configuration (small
 * launches, probes), which reads the residual straight into registers; 2 = the 256 x 256 configuration, which takes a split residual
 * through LDS.  All compute the same bits.  ms_out (host float[1], may be NULL): average milliseconds per launch. */
int ee_debug_gemm_split_resid(const float* A, const float* W, const float* bias, const float* resid, float* Cout, int32_t M, int32_t N,
                              int32_t K, float a_scale, float w_scale, float resid_scale, const int32_t* row_src, int32_t rows_A,
                              const int32_t* resid_row_src, int32_t rows_resid, int32_t route, int32_t iters, float* ms_out, void* stream);

/* The hook the two above are wrappers of: one call of launch_gemm_split with every operand a forward can set, so that each of its routes can be
 * launched alone (tests/test_gpu_gemm_routes.py).  The operands of ee_debug_gemm_split and ee_debug_gemm_split_resid keep their meaning (A, W,
 * bias, resid f32 on the device; resid_scale > 0 converts the residual to split-f16 rows of that scale, 0 passes it on as f32; out_scale is
 * read with out_split only; row_src non-decreasing, resid_row_src any rows, both checked against rows_A / rows_resid).  Beyond them:
 *   k_splits, split_stride   S > 1: split-K as MMEE_FLAG_LOW_LATENCY and the X-space probe launch it -- part p of C = alpha * acc over k-stages
 *                            [p K / 32 / S, (p + 1) K / 32 / S) is written as f32 rows at Cout + p * split_stride (floats); no bias: the LayerNorm
 *                            kernel behind it (ee_debug_ln_rows, pre_parts = S) adds the parts in order, the bias and the residual
 *   probe                    != 0: the CLS-probe launches of a forward (128 x 128 tiles under their own kernel name, static tile assignment,
 *                            three terms whatever `terms` says)
 *   terms                    3, or 1 = MMEE_FLAG_ONE_TERM (hi x hi only; the pairs GELU -> split, bias -> split, residual -> f32 have such a kernel,
 *                            every other pair runs the three terms)
 *   role_tag                 0, or 2 / 3: the kernel names of the attention-output / FFN-down GEMM (residual epilogue)
 *   route                    as ee_debug_gemm_split_resid's (residual epilogue, f32 output), else 0
 *   scale_cols, scale        columns [0, scale_cols) are multiplied by `scale` behind the bias (Q / sqrt(d) of the fused Q | K | V GEMM)
 *   col_scale                NULL, or f32 [N]: a factor per column on (acc + bias), in front of the residual (BEiT's lambda)
 *   max_m, m_on_device       m_on_device != 0: the launch is sized by max_m and the kernel reads M from a device word the hook uploads, as in
 *                            every forward; Cout and the row maps still hold M rows.  m_on_device == 0: max_m is not read.
 * Refused before any device work: k_splits outside {1, 2, 4, 8} or not a divisor of the K / 32 k-stages (the kernel's integer division would
 * drop the tail); k_splits > 1 with anything but the bias epilogue, an f32 output, three terms and no bias pointer (launch_gemm_split would
 * write ONE part); terms outside {1, 3}; M > max_m; scale_cols no multiple of 64 in [0, N].  ms_out as ee_debug_gemm_split's.
 *   err_flag_out             NULL: the launches get no error word (as ee_debug_gemm_split and ee_debug_gemm_split_resid run them).  Otherwise a
 *                            zeroed device word is the err_flag of the GEMM launch and of the launch_split_rows calls that convert A, W and
 *                            the residual, and its value after the last launch is written here. */
typedef struct ee_debug_gemm_routes_args {
    const float *A, *W, *bias, *resid;
    float* Cout;
    int32_t M, N, K, epi, out_split;
    float a_scale, w_scale, out_scale, resid_scale;
    const int32_t* row_src;
    int32_t rows_A;
    const int32_t* resid_row_src;
    int32_t rows_resid;
    int32_t route, role_tag, probe, terms;
    int32_t k_splits;
    size_t split_stride;
    int32_t scale_cols;
    float scale;
    const float* col_scale;
    int32_t max_m, m_on_device, iters;
    int32_t* err_flag_out;      /* NULL, or host int32: the error word of the launches (16 = a value left the split planes' range, or is a NaN) */
} ee_debug_gemm_routes_args;
int ee_debug_gemm_routes(const ee_debug_gemm_routes_args* args, float* ms_out, void* stream);

/* The f32 counterpart of ee_debug_gemm_routes: ONE call of launch_gemm_f32 (csrc/gemm_f32.hip) with every operand a forward can set, so that the
 * kernel can be launched alone as Forward::qkv, layer_rest, beit_rest and run_head launch it (tests/test_gpu_gemm_f32_routes.py).  The arguments
 * are those every GEMM of a forward starts from (scale 1, the static priority of the odd wave slots) plus the caller's; lda = K, ldc = ldr = N.
 * Cout[r] = epi((A[row_src ? row_src[r] : r] W^T + bias) * (column < scale_cols ? scale : 1)) * col_scale (+ resid[resid_row_src ? resid_row_src[r] : r]).
 *   A, W, bias, resid        dev f32: A [rows_A][K], W [N][K], bias [N] or NULL, resid [rows_resid][N] (residual epilogue) or NULL
 *   Cout                     dev f32 [>= max(M, max_m)][N]; rows >= M keep their bytes
 *   epi                      0 = bias, 1 = GELU(erf), 2 = + residual, 3 = tanh; no flag bits (ee_debug_gemm keeps the diagnostic ones)
 *   staging                  0 = the LDS-DMA kernel (what the path runs), 1 = the register-staged kernel
 *   use_queue                != 0: XCD-local work queues (the hook zeroes the heads), 0: static grid stride
 *   row_src, rows_A          NULL (dense), or dev int32 [M] into the rows_A rows of A: any order, repeats allowed
 *   resid_row_src, rows_resid  the same for the residual, independent of row_src (read with the residual epilogue only)
 *   scale_cols, scale        columns [0, scale_cols) are multiplied by `scale` behind the bias (Q / sqrt(d) of the fused Q | K | V GEMM)
 *   col_scale                NULL, or f32 [N]: a factor per column behind the epilogue function, in front of the residual (BEiT's lambda)
 *   max_m, m_on_device       m_on_device != 0: the launch is sized by max_m and the kernel reads M from a device word the hook uploads, as in
 *                            every forward; the row maps still hold M entries.  m_on_device == 0: max_m is not read, the launch is sized by M.
 *   wgs_per_cu               workgroups per CU of the persistent grid, 0 = default
 * M = 0 is legal: the kernel returns without touching anything.  Refused on the host before any device call, each with its own message: args,
 * A, W or Cout NULL; N or K below 1, N % 128, K % 32; M < 0; epi outside 0 .. 3; staging outside {0, 1}; the residual epilogue without resid, or
 * resid with another epilogue; scale_cols no multiple of 128 in [0, N] (the kernel decides per 128-column tile side); m_on_device with
 * max_m < 1 or M > max_m; wgs_per_cu < 0; M rows without a row map and fewer than M rows of A / of the residual.  The row maps are checked
 * against rows_A / rows_resid on host copies.  Synchronises the stream. */
typedef struct ee_debug_gemm_f32_args {
    const float *A, *W, *bias, *resid;
    float* Cout;
    int32_t M, N, K, epi;
    int32_t staging;
    int32_t use_queue;
    const int32_t* row_src;
    int32_t rows_A;
    const int32_t* resid_row_src;
    int32_t rows_resid;
    int32_t scale_cols;
    float scale;
    const float* col_scale;
    int32_t max_m, m_on_device;
    int32_t wgs_per_cu;
} ee_debug_gemm_f32_args;
int ee_debug_gemm_f32(const ee_debug_gemm_f32_args* args, void* stream);

/* Unit-test hook of the fused attention kernels: ONE launch of one kernel of the path on caller-provided DEVICE buffers; no handle.
 *   qkv            f32 [qkv_rows][3 H], H = 64 * heads: Q (already divided by sqrt(d)) | K | V of every row
 *   doc_off        int32 [n_docs + 1], doc_off[0] = 0: the ragged documents; row r of document d is context row doc_off[d] + r
 *   qkv_doc_off    NULL, or int32 [n_docs]: first Q | K | V row of every document when those rows lie elsewhere (probe-first layers)
 *   pos, x0, y1    int32 per row: the 1-D position index in [0, max_pos], bbox x0 / y1 in [0, max_coord]; masked: != 0 = not an attention key
 *   w1, wx, wy     f32 [heads][bins1], [heads][bins2], [heads][bins2]: rel_pos_bias / rel_pos_x_bias / rel_pos_y_bias (NULL for _IDX_NOBIAS)
 *   kernel         MMEE_ATTN_KERNEL_*; use_queue: != 0 work queues, 0 static grid stride; q_limit > 0: the first q_limit queries of every document
 *   terms          3, or 1 (MMEE_ATTN_KERNEL_IDX only): the f16 MFMA terms per product (MMEE_FLAG_ONE_TERM)
 *   ctx            out, [rows][H] exactly as the kernel writes it: f32 rows (MMEE_ATTN_KERNEL_F32) or split-f16 rows (64-byte groups
 *                  [hi 16 f16 | lo 16 f16]) scaled by 64; rows the kernel does not write keep their bytes
 *   err_flag_out   host int32: the kernel's error word after the launch (16 = a value left the range of the split planes)
 * The operands are built by the path's own code: row metadata, bucket LUTs, value tables, split Q | K | V rows (scale 16), pair index,
 * stage counts, zeroed queue counters; max_len = the longest document.  What the kernels' *_supports() predicates refuse is refused here.
 * Synchronises the stream. */
#define MMEE_ATTN_KERNEL_F32 0          /* attention_f32.hip */
#define MMEE_ATTN_KERNEL_PAIR 1         /* attention_pair.hip (bucket tables beyond 64 bins) */
#define MMEE_ATTN_KERNEL_IDX 2          /* attention_idx.hip with the 32-bit pair index */
#define MMEE_ATTN_KERNEL_IDX_NOBIAS 3   /* attention_idx.hip without a pair index: no bias, no key mask (image-only models) */
int ee_debug_attention(const float* qkv, int32_t qkv_rows, const int32_t* doc_off, int32_t n_docs, const int32_t* qkv_doc_off, const int32_t* pos,
                       const int32_t* x0, const int32_t* y1, const int32_t* masked, const float* w1, const float* wx, const float* wy, int32_t heads,
                       int32_t bins1, int32_t bins2, int32_t max_rel_pos, int32_t max_rel_2d_pos, int32_t max_pos, int32_t max_coord, int32_t kernel,
                       int32_t use_queue, int32_t q_limit, int32_t terms, void* ctx, int32_t* err_flag_out, void* stream);

/* Unit-test hooks of the row kernels (csrc/prep_embed.hip), the counterparts of ee_debug_attention: the path's own launchers on
 * caller-provided DEVICE buffers; no handle.  Each synchronises the stream and writes the kernels' error word to the host int32
 * err_flag_out (1 token id, 2 bbox, 4 position id, 8 token_type id out of range; 16 a value left the range of the split planes).  Every
 * table and output must be as large as the shapes say: the hooks check shapes, not buffer sizes.  Refused, not launched: a hidden size
 * that is no multiple of 128 or above 1024, 4 cs + 2 ss != H, split rows where H % 256 != 0.
 *
 * ee_debug_prep: doc_prep / doc_scan / row_meta.  input_ids, attention_mask (or NULL), position_ids (or NULL), token_type_ids (or NULL)
 *   int64 (B,T); bbox int64 (B,T,4); G = patches per side (Pv = G G + 1 visual rows per document); the range limits pad_id, vocab,
 *   max_2d, max_pos, type_vocab; dense_rows != 0 keeps trailing pad rows (MMEE_FLAG_DENSE_ROWS).  Outputs, int32: text_dst (B,T) the row
 *   inside the document or -1, emb_pos (B,T), ntext (B), doc_off (B + 1), x_src (B), doc_orig (B), meta (rows,4) = {4 pos, 4 x0, 4 y1,
 *   float bits of the key mask} per packed row, counts = 16 bytes {int32 n_docs, int32 n_rows, uint64 sum_len_sq}.
 *
 * ee_debug_embed: prep, embed_text, embed_visual (embed_visual_rows when neither vis_part nor cat_part is given), then pool_finish for
 *   every partial-sum buffer given.  Tables: word (vocab,H), type (type_vocab,H), pos (max_pos,H), xtab / ytab (max_2d,cs), htab / wtab
 *   (max_2d,ss); inputs_embeds (B,T,H) or NULL; vis_raw (B,Pv - 1,H) = the patch projection's output, cls_token (H), pos_embed (Pv,H).
 *   LayerNorms: text_ln_* / text_eps = embeddings.LayerNorm, vis_ln_* / vis_eps = layoutlmv3.norm, ln2_* / eps2 = layoutlmv3.LayerNorm.
 *   Exactly one of X (f32 rows) and Xs (split-f16 rows scaled by split_scale) receives the B (T + Pv) packed rows at most.  text_part
 *   (B,ceil(T/32),H), vis_part (B,ceil(Pv/32),H), cat_part (B,ceil(T/32) + ceil(Pv/32),H): scratch, each with its pooled_* (B,H) output.
 *
 * ee_debug_ln_rows: one launch_ln_rows.  dst[r] = LayerNorm(src[row_src ? row_src[r] : r]) for r < *n_rows (a DEVICE word, <= max_rows);
 *   dst may be src or NULL; dst_split (or NULL) receives the rows as split-f16 planes scaled by split_scale.  pre_parts >= 1: the row is
 *   first completed from pre_parts split-K planes (src + p pre_stride), pre_bias (or NULL) and the residual row pre_resid_rows[r] (or r)
 *   of pre_resid (split-f16 rows scaled by 1 / pre_resid_inv, or NULL).  The grid is sized by max_rows and the device's CU count. */
typedef struct ee_debug_embed_args {
    const int64_t *input_ids, *attention_mask, *bbox, *position_ids, *token_type_ids;
    int32_t B, T, G, pad_id, vocab, max_2d, max_pos, type_vocab, dense_rows, H, cs, ss;
    const float *word, *type, *pos, *xtab, *ytab, *htab, *wtab, *inputs_embeds;
    const float *text_ln_g, *text_ln_b, *vis_ln_g, *vis_ln_b, *ln2_g, *ln2_b;
    float text_eps, vis_eps, eps2, split_scale;
    const float *cls_token, *pos_embed, *vis_raw;
    float* X;
    void* Xs;
    float *text_part, *vis_part, *cat_part;
    float *pooled_text, *pooled_vis, *pooled_cat;
} ee_debug_embed_args;
int ee_debug_prep(const int64_t* input_ids, const int64_t* attention_mask, const int64_t* bbox, const int64_t* position_ids,
                  const int64_t* token_type_ids, int32_t B, int32_t T, int32_t G, int32_t pad_id, int32_t vocab, int32_t max_2d, int32_t max_pos,
                  int32_t type_vocab, int32_t dense_rows, int32_t* text_dst, int32_t* emb_pos, int32_t* ntext, int32_t* doc_off, int32_t* x_src,
                  int32_t* doc_orig, int32_t* meta, void* counts, int32_t* err_flag_out, void* stream);
int ee_debug_embed(const ee_debug_embed_args* args, int32_t* err_flag_out, void* stream);
int ee_debug_ln_rows(const float* src, float* dst, const int32_t* row_src, const int32_t* n_rows, int32_t max_rows, int32_t H, const float* gamma,
                     const float* beta, float eps, void* dst_split, float split_scale, int32_t pre_parts, size_t pre_stride,
                     const float* pre_bias, const void* pre_resid, const int32_t* pre_resid_rows, float pre_resid_inv, int32_t* err_flag_out,
                     void* stream);
/* ee_debug_vision_pool: the phase-1 kernel of a vision-first call (csrc/vision_first.hip) alone, as ee_forward_vision launches it behind the
 *   patch projection: vision_pool_kernel, then pool_finish; no handle.  vis_raw dev float (B,Pv - 1,H) = the patch projection's output,
 *   cls_token (H), pos_embed (Pv,H), ln_g / ln_b (H) and eps = layoutlmv3.norm; vis_part dev float (B,ceil(Pv/32),H) scratch that receives
 *   the partial sums per (document, 32-row chunk); pooled dev float (B,H) = the mean over the Pv rows.  Refused, not launched: a NULL
 *   pointer, a hidden size that is not a multiple of 4 in [4, 1024], B < 1, Pv < 2, B Pv > 2^24, eps <= 0.  Synchronises the stream. */
int ee_debug_vision_pool(const float* vis_raw, const float* cls_token, const float* pos_embed, const float* ln_g, const float* ln_b, float eps,
                         int32_t B, int32_t Pv, int32_t H, float* vis_part, float* pooled, void* stream);

/* Unit-test hook of the X-space CLS probe (csrc/xprobe.hip), the counterpart of ee_debug_attention: the three kernels of launch_xprobe on
 * caller-provided DEVICE buffers, fed as layer_probe() of the forward feeds them; no handle.
 *   The stage-0 batch the pair index is built from: n_orig documents, orig_doc_off int32 [n_orig + 1] (first entry 0), and per row pos, x0,
 *     y1, masked (int32) with the meaning and ranges of ee_debug_attention.
 *   The stage the probe runs on: n_docs documents (0 allowed), max_docs >= max(n_docs, 1) sizes the grids and the scratch as the forward's
 *     batch size does; doc_off int32 [n_docs + 1] (first entry 0; the context row of document d is row doc_off[d] of ctx), doc_orig [n_docs]
 *     the original document (pair-index slab; equal length required), x_phys [n_docs] the first row of the document in xs.
 *   xs     split-f16 rows [x_rows][H] scaled by 16 (64-byte groups [hi 16 f16 | lo 16 f16]): the LayerNorm rows
 *   qc     f32 [n_docs][H]: Q of the CLS rows, already divided by sqrt(d);  wk, wv f32 [H][H] (rows = outputs), bk, bv f32 [H]; wv is split here
 *          with ee_finalize's per-tensor power-of-two scale
 *   w1, wx, wy   f32 [heads][bins1], [heads][bins2], [heads][bins2]
 *   index_form   0: the 32-bit pair index (launch_pair_index); 1: the query-block-0 output of the 16-bit form, which only the diagnostic
 *                library builds -- the release library refuses it
 *   cus          0: the device's CU count, else the num_cus handed to launch_xprobe (the probe's grid is min(max_docs, cus) workgroups)
 *   ctx          out, split-f16 rows [ctx_rows][H] scaled by 64: row doc_off[d] of every stage document is written, every other row keeps its bytes
 *   u_out [n_docs][heads][H], s0_out [n_docs][heads][2] (q . b_k, plane scale of u), cvec_out [n_docs][heads][H] f32, order_out int32
 *                [n_docs] (documents by falling length, ties by rising index): copies of the intermediates, each may be NULL
 *   err_flag_out host int32: the kernels' error word (16 = a context value left the range of the split planes)
 * The probe's scratch is filled with a non-zero byte pattern first, as a workspace that is not zeroed between forwards may hold anything.
 * Refused, not launched: what xprobe_supports() refuses (anything but 12 heads x 768 and 16 x 1024, more than 255 bins, a longest document
 * whose LDS layout exceeds 160 KB), a stage document whose length differs from its original's, rows outside xs or ctx, integers outside
 * their ranges.  Synchronises the stream. */
typedef struct ee_debug_xprobe_args {
    int32_t n_orig;
    const int32_t *orig_doc_off, *pos, *x0, *y1, *masked;
    int32_t n_docs, max_docs;
    const int32_t *doc_off, *doc_orig, *x_phys;
    const void* xs;
    int32_t x_rows, ctx_rows;
    const float *qc, *wk, *bk, *bv, *wv, *w1, *wx, *wy;
    int32_t H, heads, bins1, bins2, max_rel_pos, max_rel_2d_pos, max_pos, max_coord, index_form, cus;
    void* ctx;
    float *u_out, *s0_out, *cvec_out;
    int32_t* order_out;
} ee_debug_xprobe_args;
int ee_debug_xprobe(const ee_debug_xprobe_args* args, int32_t* err_flag_out, void* stream);

/* Unit-test hooks of the exit stage (csrc/exit_stage.hip), the counterparts of ee_debug_attention: the path's own launchers on
 * caller-provided DEVICE buffers; no handle.  Each synchronises the stream; these kernels have no error word.  Every buffer must be as
 * large as the shapes say: the hooks check shapes and the index arrays they can read, not buffer sizes.
 *
 * ee_debug_head_out: one launch_head_out.  out[i][o] = <in[gather ? gather[i] : i], W[o]> + b[o] for i < *n_docs (a DEVICE word,
 *   <= max_docs, which sizes the grid), o < Ko; in f32 [in_rows][ld], W f32 [Ko][H], b f32 [Ko].  With lte_out (double [n_docs]) the same
 *   launch scores every document: sigmoid(<lte_in[lte_gather ? lte_gather[i] : i], lte_w> + lte_b[0]) in float64, lte_in [lte_rows][lte_ld]
 *   f32 rows (lte_split_inv 0) or split-f16 rows (64-byte groups [hi 16 f16 | lo 16 f16], lte_split_inv = 1 / plane scale).  Refused: H
 *   outside [4, 1024] or no multiple of 4, ld / lte_ld below H or no multiple of 4, Ko < 1, a gather entry outside its rows.
 *
 * ee_debug_exit_decide: one exit of one stage through launch_decide, and launch_compact_rows behind it when meta_old, meta_new and
 *   row_src are given (all three or none).  mode: 0 threshold criterion, 1 patience, 2 LTE; rule: MMEE_RULE_*; criterion: MMEE_CRIT_*
 *   (ignored under mode 1; MMEE_CRIT_GATE: mode 0 only, and a criterion of the call only with head_logits given and Kh == 2: refused otherwise).  pol_logits f32 [n_docs][K]; head_logits f32 [n_docs][Kh] or NULL; lte_score double [n_docs] or NULL (an
 *   exit without a score: nobody leaves).  thr, temp, patience: this exit's; by_pointer != 0 hands them to the kernel as a captured
 *   graph's replay does, at [exit_index] of device vectors (the patience at [0] of its own).  The current stage: counts (16 bytes
 *   {int32 n_docs, int32 n_rows, uint64 sum_len_sq}), doc_orig [n_docs] (slots in [0, B)), doc_off [n_docs + 1], x_phys [n_docs].
 *   prev, run int32 [B]: the caller's per-document state by original slot, needed by mode 1 and by every rule but PLAIN; exit 0 does not
 *   read it.  Outputs: the next stage n_counts, n_doc_orig, n_doc_off (one more entry than survivors), n_x_src, n_meta_src; out_exit
 *   [B]; and, each or NULL, out_logits (B,K), out_conf (B), out_all_logits (E1,B,K), out_all_crit (E1,B), out_head_logits (E1,B,Kh),
 *   out_head_crit (E1,B), written at exit_index.  Rows: meta_old / meta_new int32 (rows,4), row_src int32 (rows).  Refused: a (mode, rule)
 *   pair launch_decide has no kernel for, K or Kh < 1, a stateful pair without prev / run, exit_index < 0, a document table that does not
 *   start at 0 or holds an empty document, counts.n_rows != doc_off[n_docs], doc_orig outside [0, B).
 *
 * ee_debug_rows_out: which = 0, launch_gather_cls: out[doc_orig ? doc_orig[i] : i] = X[x_phys[i]] for i < *n_docs (DEVICE word, <=
 *   max_docs); which = 1, launch_rows_to_padded: out (B, T + Pv, H), position p < T of document d = X row doc_off[d] + text_dst[d][p]
 *   (zeros when text_dst[d][p] < 0), position T + v = X row doc_off[d] + ntext[d] + v; text_dst NULL (image-only): T = 0 and no ntext.
 *   X [x_rows][H] f32 rows (split_inv 0) or split-f16 rows (split_inv = 1 / plane scale); out f32 [out_rows][H].  Refused: a row index
 *   outside X or out.
 *
 * ee_debug_exit_ensemble: one launch_exit_ensemble (the exit ensemble's launch; definition at ee_set_ensemble) for exit exit_index of E1.
 *   pol_logits f32 [pol_rows][K], the head's rows of the stage's documents; temp: this exit's temperature (by_pointer != 0: read at
 *   [exit_index] of a device vector, as a replay does); counts and doc_orig as for ee_debug_exit_decide (slots in [0, B)); w dev double
 *   (E1,E1), b dev double (E1,K) or NULL; state dev double (E1,B,K), the caller's per-document rows l_e by original slot: row exit_index of
 *   every active slot is written, rows 0 .. exit_index-1 of those slots are read, nothing else is touched; out f32 [out_rows][K] receives
 *   y of document i at row i.  Refused: K, E1 or B below 1 (B above 2^20), exit_index outside [0, E1), n_docs outside [0, B] or above
 *   pol_rows / out_rows, doc_orig outside [0, B), E1 * B * K above 2^31. */
typedef struct ee_debug_exit_ensemble_args {
    const float* pol_logits;
    int32_t pol_rows, K, E1, exit_index, B;
    double temp;
    int32_t by_pointer;
    const void* counts;
    const int32_t* doc_orig;
    const double *w, *b;
    double* state;
    float* out;
    int32_t out_rows;
} ee_debug_exit_ensemble_args;
int ee_debug_exit_ensemble(const ee_debug_exit_ensemble_args* args, void* stream);
typedef struct ee_debug_head_out_args {
    const float* in;
    int32_t in_rows, ld;
    const int32_t* gather;
    const float *W, *b;
    int32_t H, Ko;
    const int32_t* n_docs;
    int32_t max_docs;
    float* out;
    const void* lte_in;
    int32_t lte_rows, lte_ld;
    const int32_t* lte_gather;
    float lte_split_inv;
    const float *lte_w, *lte_b;
    double* lte_out;
} ee_debug_head_out_args;
typedef struct ee_debug_exit_decide_args {
    int32_t mode, rule, criterion;
    const float *pol_logits, *head_logits;
    int32_t K, Kh;
    const double* lte_score;
    double thr, temp;
    int32_t patience, by_pointer, exit_index, is_final, no_exit, B;
    const void* counts;
    const int32_t *doc_orig, *doc_off, *x_phys;
    int32_t *prev, *run;
    void* n_counts;
    int32_t *n_doc_orig, *n_doc_off, *n_x_src, *n_meta_src;
    float* out_logits;
    int32_t* out_exit;
    float *out_conf, *out_all_logits, *out_all_crit, *out_head_logits, *out_head_crit;
    const int32_t* meta_old;
    int32_t *meta_new, *row_src;
} ee_debug_exit_decide_args;
typedef struct ee_debug_rows_out_args {
    int32_t which;
    const void* X;
    int32_t x_rows, H;
    float split_inv;
    const int32_t *x_phys, *doc_orig, *n_docs;
    int32_t max_docs, B, T, Pv;
    const int32_t *text_dst, *ntext, *doc_off;
    float* out;
    int32_t out_rows;
} ee_debug_rows_out_args;
int ee_debug_head_out(const ee_debug_head_out_args* args, void* stream);
int ee_debug_exit_decide(const ee_debug_exit_decide_args* args, void* stream);
int ee_debug_rows_out(const ee_debug_rows_out_args* args, void* stream);
/* ee_debug_exit_quota: one exit of one stage under a quota (budgeted exits, definition at MMEE_QUOTA_*): the two ranking launches
 *   (launch_exit_quota_rank) and the QUOTA form of the decide kernel (launch_decide_quota), then launch_compact_rows as ee_debug_exit_decide.
 *   decide: the stage, the logits, this exit's thr / temp and every output exactly as for ee_debug_exit_decide; mode must be 0 and rule
 *   MMEE_RULE_PLAIN (prev / run / patience / lte_score are not read), is_final and no_exit must be 0 (the forward runs the plain kernels
 *   there).  quota >= 0: this exit's q_e; quota_mode MMEE_QUOTA_EXACT or MMEE_QUOTA_AT_LEAST.  by_pointer != 0 hands thr, temp and the quota
 *   to the kernels as a captured graph's replay does.  crit dev double [n_docs] and rank dev int32 [n_docs] receive c_i and rank_i by the
 *   stage's document index; nothing behind n_docs entries is written.  doc_orig may list the slots in any order: the tie-break is by slot.
 *   Refused: what ee_debug_exit_decide refuses, a NULL crit / rank, a negative quota, an unknown quota_mode, a mode / rule / is_final /
 *   no_exit other than above. */
typedef struct ee_debug_exit_quota_args {
    ee_debug_exit_decide_args decide;
    int32_t quota, quota_mode;
    double* crit;
    int32_t* rank;
} ee_debug_exit_quota_args;
int ee_debug_exit_quota(const ee_debug_exit_quota_args* args, void* stream);
/* ee_debug_exit_audit: one exit of one stage of an audited call (audited exits, definition behind the cascades): launch_decide with its
 *   AuditArgs -- the AUDIT form of the (mode, rule) kernel -- then launch_compact_rows as ee_debug_exit_decide.  decide: everything exactly as
 *   for ee_debug_exit_decide, is_final included; no_exit must be 0 (a dump-all call runs the plain kernels).  cut in [1, 2^32], seed and
 *   slot_base >= 0 as for ee_set_audit.  delivered dev int32 [B] by original slot goes in and comes out: at exit_index 0 the entries of the
 *   stage's documents are written without being read; at a later exit they are read, and written where a document is delivered here; entries
 *   of slots outside the stage are never touched.
 *   Refused: what ee_debug_exit_decide refuses, no_exit != 0, a cut outside [1, 2^32], a negative slot_base, a NULL delivered. */
typedef struct ee_debug_exit_audit_args {
    ee_debug_exit_decide_args decide;
    uint64_t cut;
    uint32_t seed;
    int32_t slot_base;
    int32_t* delivered;
} ee_debug_exit_audit_args;
int ee_debug_exit_audit(const ee_debug_exit_audit_args* args, void* stream);
/* ee_debug_audit_tally / ee_debug_controller_step: the two launches a controlled forward adds behind its final exit (online exit control,
 *   definition behind the audit's), each alone.
 *   tally: the final stage (counts dev StageCounts, doc_orig dev int32 [n_docs], every entry in [0, B)), pol_logits dev float [pol_rows][K] the
 *   rows the final decide launch read and temp what it scaled them by, delivered dev int32 [B] the audit's marks, out_logits dev float (B,K),
 *   out_exit dev int32 (B), the audit's cut in [1, 2^32], seed and slot_base >= 0.  tally dev int64 [2 + 2 (E1 - 1)] is written: sampled,
 *   disagree, delivered[E1 - 1], agree[E1 - 1]; a shadow whose out_exit lies outside [0, E1 - 1) counts in disagree only.
 *   step: path dev float64 (V,E1); state dev int64 [5]: p (float64 bits), calls, steps, sampled_sum, disagree_sum, updated; tally as above,
 *   read; thr dev float64 [E1]: the thresholds the call ran with go in (they are logged), the next call's come out; log dev int64
 *   (log_cap, controller_log_words) or NULL: row calls % log_cap is written.
 *   Refused: NULL pointers, E1 outside [2, 64], counts or slots outside the buffers, and the parameter ranges of ee_set_controller. */
typedef struct ee_debug_audit_tally_args {
    const float* pol_logits;
    int32_t pol_rows, K, B, E1;
    double temp;
    const int32_t *counts, *doc_orig, *delivered;
    const float* out_logits;
    const int32_t* out_exit;
    uint64_t cut;
    uint32_t seed;
    int32_t slot_base;
    int64_t* tally;
} ee_debug_audit_tally_args;
int ee_debug_audit_tally(const ee_debug_audit_tally_args* args, void* stream);
typedef struct ee_debug_controller_step_args {
    const double* path;
    int32_t V, E1;
    double sign, alpha, gamma;
    int64_t* state;
    const int64_t* tally;
    double* thr;
    int64_t* log;
    int32_t log_cap;
} ee_debug_controller_step_args;
int ee_debug_controller_step(const ee_debug_controller_step_args* args, void* stream);
/* ee_debug_deadline_check: the check launch of a deadline call (deadline exits, definition behind the controller's) alone, with the clock
 *   injected: the kernel takes `now` and `t0` (ticks of a counter at khz kHz) instead of reading s_memrealtime and state[0], so every branch
 *   runs without timing.  state dev int64 [3]: t0 (not read here), cut_exit (-1: not cut yet), cut_by, updated; thr dev float64 [E1]:
 *   entries exit_index .. E1 - 2 receive the always-fires value of `sign` when this check cuts; row dev int64 [4 + E1] or NULL: a log row,
 *   elapsed_ns[exit_index] and, at a cut, cut_exit / cut_by are written; host_word: the value the host's request word holds.
 *   Refused: NULL pointers, E1 outside [2, 64], exit_index outside [0, E1), khz == 0, a sign that is not +-1, call == 0. */
typedef struct ee_debug_deadline_check_args {
    int32_t E1, exit_index;
    uint32_t khz;
    double sign;
    uint64_t call, budget_ns, eta_ns, host_word, now, t0;
    int64_t* state;
    double* thr;
    int64_t* row;
} ee_debug_deadline_check_args;
int ee_debug_deadline_check(const ee_debug_deadline_check_args* args, void* stream);

/* Unit-test hook of the patch projection (Conv2d with kernel = stride = patch as a GEMM over flattened patches), the counterpart of
 * ee_debug_attention: what patch_projection() of the forward launches, on caller-provided DEVICE buffers; no handle.
 *   pixel_values   f32 [B][C][R][R]; weight f32 [H][C P P] (k = (c, ky, kx), as Conv2d's weight flattens); bias f32 [H]
 *   form           0 = the f32 GEMM with the LDS-DMA kernel (what an MMEE_PREC_F32 forward runs), 1 = the f32 GEMM with the register-staged
 *                  kernel, 2 = split precision: launch_patch_split writes the patches as split-f16 rows scaled by 16, the weight becomes split
 *                  rows with ee_finalize's per-tensor scale, and the split GEMM multiplies them
 *   out            f32 [B (R / P)^2][H]: row b (R / P)^2 + gy (R / P) + gx = patch (gy, gx) of image b; rows past that keep their bytes
 *   a_split_out    NULL, or (form 2) [B (R / P)^2][C P P] 32-bit words: the split rows (64-byte groups [hi 16 f16 | lo 16 f16]) are
 *                  written here instead of into scratch, and the GEMM reads them from here
 *   err_flag_out   host int32: the kernels' error word (16 = a pixel left the range of the split planes)
 * Refused, not launched: NULL pointers, B < 1; a geometry ee_create refuses (R % P, P % 4, R % 4, C P P % 32); more than 2^24 rows;
 * H % 128 or H > 1024; form outside 0..2; form 2 with H % 256; a_split_out with form 0 or 1.  Synchronises the stream. */
typedef struct ee_debug_patch_project_args {
    const float *pixel_values, *weight, *bias;
    int32_t B, C, R, P, H, form;
    float* out;
    void* a_split_out;
    int32_t* err_flag_out;
} ee_debug_patch_project_args;
int ee_debug_patch_project(const ee_debug_patch_project_args* args, void* stream);

/* Unit-test hooks of the split-f16 encoders (csrc/mmee_common.h "Split-f16 operand rows"), on caller-provided DEVICE buffers; no handle
 * (tests/test_gpu_split.py compares their words with tests/split_ref.py bit for bit).
 * ee_debug_split_rows: ONE launch_split_rows call (the clamp form of the encoder) with a zeroed error word.
 *   src            f32 [rows][K]; dst_words [rows][K] 32-bit words: the split rows scaled by `scale` (64-byte groups [hi 16 f16 | lo 16 f16])
 *   err_flag_out   host int32: the kernel's error word (16 = |scale * x| left the planes' range, or x is a NaN)
 * Refused, not launched: NULL pointers, rows < 0, K no positive multiple of 16, rows K > 2^30, a scale that is not positive and finite.
 * ee_debug_split_weight: the weight split of ee_finalize (the maximum of |w| on the device, the per-tensor power-of-two scale that puts it
 * in [2^12, 2^13) capped at 2^8, the clamp-form encoder), as build_split calls it.
 *   w              f32 [N][K]; dst_words [N][K] 32-bit words; inv_out host float: 1 / scale
 * Refused, not launched: NULL pointers, N < 1, K no positive multiple of 16, N K > 2^30.  A tensor that holds inf / nan is refused with
 * ee_finalize's words ("a weight tensor holds inf/nan") and dst_words keeps its bytes.  Both synchronise the stream. */
int ee_debug_split_rows(const float* src, int32_t rows, int32_t K, float scale, void* dst_words, int32_t* err_flag_out, void* stream);
int ee_debug_split_weight(const float* w, int32_t N, int32_t K, void* dst_words, float* inv_out, void* stream);

/* Diagnostic of the two-heads-per-item attention kernel (attention_pair.hip): with MMEE_ATTN_STAMPS=1 in the environment the
 * launches run a build with in-kernel s_memtime stamps; this call synchronises, copies the eight phase sums (shader cycles summed over
 * waves: 0 wait for the tile's LDS-DMA, 1 DMA issue, 2 bias gathers, 3 Q K^T MFMAs, 4 / 5 softmax + P V of head A / B, 6 item prologue,
 * 7 barrier) to out8 and clears them.  Timing shares only; never part of the path. */
int ee_debug_attn_stamps(uint64_t* out8);

/* Host-only helper (no GPU needed): the relative_position_bucket LUT (HF modeling_layoutlmv3.py:392-413) over
 * delta in [-max_delta, max_delta]; out_host has 2*max_delta+1 entries, index = delta + max_delta.  Exposed so the LUT
 * the kernels use can be pinned against the HF-generated golden table. */
int ee_bucket_lut(int32_t num_buckets, int32_t max_distance, int32_t max_delta, uint8_t* out_host);

#ifdef __cplusplus
}
#endif
#endif /* MMEE_H */
