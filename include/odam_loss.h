/*
 * odam_loss.h -- C ABI of the detector's validation loss: the matching cost, the assignment and the losses of the reference's
 * HungarianMatcher and SetCriterion on B frames whose outputs are already on the device.
 *
 * Replaces, of the reference (likojack/ODAM):
 *   src/models/matcher.py:49-73        the cost matrix of HungarianMatcher.forward                 -> odam_detr_match_cost
 *   src/models/matcher.py:75-76        scipy.optimize.linear_sum_assignment, once per frame        -> odam_lsap_batch
 *   src/models/detr.py:286-384         loss_labels (with class_error), loss_cardinality, loss_boxes, loss_size, loss_depth,
 *                                      loss_angle, loss_offset                                     -> odam_detr_criterion
 *   src/utils/box_utils.py:8-21, 147-166, 490-494   box_iou, generalized_box_iou, box_cxcywh_to_xyxy_pytorch (both of the above)
 *   src/utils/misc.py:415-431          accuracy (top-1)                                            -> odam_detr_criterion
 *   src/models/detr.py:465-481         the same again for every entry of aux_outputs               -> odam_detr_match_cost_layers,
 *                                                                                                     odam_detr_criterion_layers
 * SetCriterion.forward without aux_outputs (:441-463) is the first three calls in a row; with aux_outputs (:465-481) the layered
 * cost, ONE odam_lsap_batch over L B problems and the layered criterion (odam_amd/criterion.py).  No gradients.
 *
 * Conventions as in odam_sq.h: int return codes (0 = OK), odam_last_error(), [dev] / [host] pointers, stream-ordered on the
 * caller's hipStream_t, no synchronisation, no allocation, caller-owned buffers.  Plain vector stores; no floating-point
 * atomics; no call writes a word that no frame, problem, row or entry owns.  Offsets that live on the device are checked
 * against the sizes of the call before they index anything.  (csrc/det_loss.hip, arithmetic in csrc/det_loss_core.h,
 * restated in numpy by tests/criterion_ref.py.)
 *
 * Targets of a batch: objects [dev] float32 [n_obj][W], W >= 12, and obj_off [dev] int32 [B+1]: frame b owns the rows
 * obj_off[b] .. obj_off[b+1]-1 (G_b of them).  Columns as the reference lays them out: 0 label, 1:5 box (cx, cy, w, h), 5:8
 * size, 8:10 offset, W-2 depth, W-1 angle bin.  n_obj is the host's copy of obj_off[B].
 *
 * Frame status words (int32, [B]) are written by odam_detr_match_cost and odam_detr_criterion, 0 when all is well, else a sum of
 *   ODAM_LOSS_ST_DEGENERATE  a box with x1 < x0 or y1 < y0 (or a NaN): generalized_box_iou's AssertionError.  The cost kernel tests
 *                            every query and every target of the frame, the criterion every matched pair
 *   ODAM_LOSS_ST_CLASS       a label outside 0 .. n_logit-1, or an angle bin outside 0 .. n_angle-1: where torch raises an IndexError
 *   ODAM_LOSS_ST_OFFSETS     obj_off[b], obj_off[b+1] not ascending inside [0, n_obj], or an assignment outside -1 .. G_b-1
 * A frame with a non-zero status has no meaning in its other outputs (what is written stays inside the frame's own words).
 *
 * odam_detr_match_cost -- for every frame b the [Q][G_b] float32 block
 *     C = cost_bbox * L1(box_q, box_g) + cost_class * (-softmax(logits_q)[label_g]) + cost_giou * (-GIoU(xyxy_q, xyxy_g))
 * in float32, added in that order.  ONE launch: one workgroup per frame, lanes over queries; the target rows are staged in LDS
 * ODAM_LOSS_STAGE at a time, the maximum and the sum of a query's softmax are computed once.
 *   logits       [dev] float32 [B][Q][n_logit]   (n_logit = classes + 1: the no-object column is last)
 *   boxes        [dev] float32 [B][Q][4]
 *   cost_out     [dev] float32 [Q * n_obj]: frame b's block starts at Q * obj_off[b], row-major [Q][G_b]
 *   B, Q, n_obj >= 0, n_logit >= 2, W >= 12, else ODAM_E_INVALID.  B == 0 is ODAM_OK without a launch.
 *
 * odam_lsap_batch -- scipy.optimize.linear_sum_assignment of n_prob cost blocks in ONE launch, one wavefront per problem: the
 * rectangular shortest-augmenting-path solver (Crouse 2016) with scipy's transposition of a tall matrix and scipy's tie order,
 * float32 costs widened to binary64 as scipy widens them.
 *   cost         [dev] float32 [n_cost]; problem p is the row-major [rows[p]][cols[p]] block at element cost_off[p]
 *   rows, cols   [dev] int32 [n_prob]     cost_off, match_off [dev] int64 [n_prob]
 *   max_small, max_large   [host] the largest min(rows, cols) and max(rows, cols) of any problem: more than ODAM_LSAP_MAX_SMALL /
 *                ODAM_LSAP_MAX_LARGE is ODAM_E_LIMIT before anything is launched (the caller solves on the host from the block)
 *   col_of_row   [dev] int32 [n_match]: words match_off[p] .. match_off[p] + rows[p] - 1, the matched column of every row, -1 if none
 *   n_pairs      [dev] int32 [n_prob]     min(rows, cols) when the status is 0
 *   status       [dev] int32 [n_prob]     0 ok; 1 infeasible, or a NaN / -inf entry (where scipy raises ValueError): col_of_row
 *                is all -1 and n_pairs 0; 3 the shape on the device is negative or beyond the limits, or a block does not lie inside
 *                [0, n_cost) / [0, n_match): nothing else is written
 *   scipy's (row_ind, col_ind) are the rows with a column, ascending, and their columns.
 *
 * odam_detr_criterion -- the losses under a given assignment, TWO launches: one wavefront per frame writes the frame's partial
 * sums, one wavefront adds them over the frames in index order and writes the table.  Per element float32, as the reference;
 * every sum in binary64 in a fixed order (a lane's queries in ascending order, then the lanes by a fixed exchange tree; frames
 * 0 .. B-1): two calls on the same inputs return the same bits, and a frame's partial sums do not depend on the batch it is in.
 *   logits [B][Q][n_logit], boxes [B][Q][4], angle [B][Q][n_angle], offset [B][Q][2], size [B][Q][3], depth [B][Q][1]   [dev] float32
 *   match        [dev] int32 [B][Q]: index inside its frame of the target a query is assigned, -1 for none (odam_lsap_batch's
 *                col_of_row with match_off[b] = b Q)
 *   num_boxes    divisor of the pair losses (> 0, else ODAM_E_INVALID); eos_coef the weight of the no-object class, rounded to float32
 *   weights      [host] double [ODAM_LOSS_N_WEIGHTS]: loss_ce, loss_bbox, loss_giou, loss_size, loss_offset, loss_depth, loss_angle
 *   out_partial  [dev] float64 [B][ODAM_LOSS_N_PARTIAL], per frame:
 *                0 sum of w nll   1 sum of w   2 matched queries whose arg-max class is the target   3 matched queries
 *                4 |#{q: max over the object classes of softmax > 0.7} - G_b|   5 sum L1 box   6 sum (1 - GIoU)   7 sum L1 size
 *                8 sum L1 offset   9 sum L1 depth   10 sum of the angle cross entropy
 *   out_table    [dev] float64 [ODAM_LOSS_N_ENTRIES]:
 *                0 loss_ce = S0 / S1   1 class_error = 100 - 100 S2 / S3 (100 when S3 == 0)   2 cardinality_error = S4 / B
 *                3 loss_bbox   4 loss_giou   5 loss_size   6 loss_offset   7 loss_depth   8 loss_angle = S5 .. S10 / num_boxes
 *                9 total = sum of weight * loss over the seven weights, in the order of `weights`, skipping a weight of 0
 *   out_status   [dev] int32 [B]
 *   B >= 1 (F.cross_entropy of no query is NaN and the reference's mean over no frame too: ODAM_E_INVALID), Q >= 0,
 *   n_logit >= 2, n_angle >= 1, W >= 12.
 *
 * odam_detr_match_cost_layers, odam_detr_criterion_layers -- the two entries above with a leading layer dimension L >= 1 on every
 * prediction tensor ([L][B][Q][.], e.g. the blocks odam_detr_forward_aux fills); the targets of frame b serve every layer.
 *   cost_out     [dev] float32 [L][Q * n_obj]: layer l's frame b at l Q n_obj + Q obj_off[b]
 *   match        [dev] int32 [L][B][Q]   (odam_lsap_batch over the L B problems with match_off[l B + b] = (l B + b) Q)
 *   out_partial  [dev] float64 [L][B][ODAM_LOSS_N_PARTIAL]     out_table [dev] float64 [L][ODAM_LOSS_N_ENTRIES]
 *   out_status   [dev] int32 [L][B]   (both entries)
 * The cost is ONE launch, one workgroup per (layer, frame); the criterion TWO, one wavefront per (layer, frame), then one per
 * layer.  The kernels are instantiations of the single-layer ones with the layer in a further grid dimension: layer l of a layered
 * call holds the bits of the single-layer call on that layer's tensors (cost block, partial sums, table, status), wherever the
 * layer stands and whatever L is.  L < 1 is ODAM_E_INVALID (more than 65535 layers ODAM_E_LIMIT); every other argument is checked
 * as by the single-layer entry, before anything is launched.
 */
#ifndef ODAM_LOSS_H
#define ODAM_LOSS_H
#include "odam_sq.h"
#ifdef __cplusplus
extern "C" {
#endif

#define ODAM_LOSS_STAGE 32
#define ODAM_LSAP_MAX_SMALL 32
#define ODAM_LSAP_MAX_LARGE 128
#define ODAM_LOSS_N_PARTIAL 11
#define ODAM_LOSS_N_ENTRIES 10
#define ODAM_LOSS_N_WEIGHTS 7
#define ODAM_LOSS_ST_DEGENERATE 1
#define ODAM_LOSS_ST_CLASS 2
#define ODAM_LOSS_ST_OFFSETS 4

int odam_detr_match_cost(const float* logits, const float* boxes, int B, int Q, int n_logit, const float* objects,
                         const int* obj_off, int n_obj, int W, float cost_class, float cost_bbox, float cost_giou,
                         float* cost_out, int* out_status, void* stream);

int odam_lsap_batch(const float* cost, long long n_cost, const long long* cost_off, const int* rows, const int* cols, int n_prob,
                    int max_small, int max_large, const long long* match_off, long long n_match, int* col_of_row, int* n_pairs,
                    int* status, void* stream);

int odam_detr_criterion(const float* logits, const float* boxes, const float* angle, const float* offset, const float* size,
                        const float* depth, int B, int Q, int n_logit, int n_angle, const float* objects, const int* obj_off,
                        int n_obj, int W, const int* match, double num_boxes, float eos_coef, const double* weights,
                        double* out_partial, double* out_table, int* out_status, void* stream);

int odam_detr_match_cost_layers(const float* logits, const float* boxes, int L, int B, int Q, int n_logit, const float* objects,
                                const int* obj_off, int n_obj, int W, float cost_class, float cost_bbox, float cost_giou,
                                float* cost_out, int* out_status, void* stream);

int odam_detr_criterion_layers(const float* logits, const float* boxes, const float* angle, const float* offset, const float* size,
                               const float* depth, int L, int B, int Q, int n_logit, int n_angle, const float* objects,
                               const int* obj_off, int n_obj, int W, const int* match, double num_boxes, float eos_coef,
                               const double* weights, double* out_partial, double* out_table, int* out_status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
