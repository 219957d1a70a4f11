/*
 * odam_eval.h -- C ABI of the evaluation of a finished map: oriented-box 3D IoU and Scan2CAD matching, all scenes in one launch each.
 *
 * Replaces, of the reference (likojack/ODAM):
 *   src/utils/box_utils.py:98-120            box3d_iou (polygon_clip :24-83, poly_area / qhull, box3d_vol)   -> odam_box3d_iou_batch
 *   src/scripts/run_merge.py:105-110         the class gate of the merge cost                                -> gate = 2
 *   src/scripts/eval_scan2cad.py:249-267     match_sequence, once per scene in Python                        -> odam_box3d_match_batch
 * get_f1 (:270-295) is a few divisions on the summed counts and stays on the host (odam_amd/evaluate.py::f1_table).
 *
 * Conventions as in odam_sq.h: int return codes (0 = OK), odam_last_error(), [dev] / [host] pointers, the first argument is the
 * odam_sq_ctx of the device (odam_sq_create); stream-ordered on the caller's hipStream_t, no synchronisation, no allocation.
 * ONE launch per call (csrc/box_iou.hip, arithmetic in csrc/box_iou_core.h); binary64.  Plain vector stores; no call writes a
 * word that no pair, box or scene owns.  The offsets live on the device, so the two sizes a launch is shaped by come from the
 * caller, who built the offsets: n_pairs and max_gt.
 *
 * Scenes: scene s owns the rows a_off[s] .. a_off[s+1]-1 of A (n_s boxes), b_off[s] .. b_off[s+1]-1 of B (m_s boxes) and the
 * n_s x m_s pair words pair_off[s] .. pair_off[s+1]-1, row-major [n_s][m_s] (pair_off[0] = 0, pair_off[s+1] = pair_off[s] + n_s m_s).
 *   a_off, b_off [dev] [n_scene+1] int32     pair_off [dev] [n_scene+1] int64
 *
 * odam_box3d_iou_batch -- 3D IoU and bird's-eye IoU of every pair (a, b) inside every scene:
 *   n_pairs      pair_off[n_scene] (host copy); n_scene == 0 or n_pairs == 0 returns ODAM_OK without a launch
 *   A, B         [dev] [sumN][8][3], [sumM][8][3]   corners in the get_3d_box / compute_oriented_bbox layout (top face 0-3, bottom
 *                4-7).  A is the reference's corners1 (the clipped box), B its corners2 (the clipper): a B whose top face winds
 *                clockwise gives 0, as the reference does; the value is that of odam_amd/merge.py::box3d_iou_pairs(A_row, B_row),
 *                operation for operation
 *   cls_a, cls_b [dev] [sumN], [sumM] int32, nullable when gate == 0
 *   gate         0 = all pairs; 1 = pairs of equal class; 2 = the merge rule: equal class, or both in {4, 5} (sofa, chair).  A
 *                gated-off pair is written as exactly 0 in both outputs.  gate outside 0..2, or gate != 0 with a null class
 *                pointer, is ODAM_E_INVALID
 *   out_iou3d    [dev] [n_pairs]     out_bev  [dev] [n_pairs], nullable
 *   A degenerate box is not an error: the value is what the arithmetic gives (0 / 0 = NaN for two boxes without volume).
 *
 * odam_box3d_match_batch -- match_sequence for all scenes: one wavefront per scene, predictions in their given order; prediction p
 * claims ground-truth box i when cls_gt[i] == cls_pred[p], iou3d[p][i] > threshold (a NaN never is) and i is not yet claimed.
 * There is no `break` in the reference: one prediction may claim several boxes and every claim counts as a true positive.
 *   iou3d        [dev] [n_pairs]     rows = predictions (A), columns = ground truth (B), as odam_box3d_iou_batch wrote it
 *   cls_pred, cls_gt  [dev] [sumN], [sumM] int32; an id outside 0 .. n_class-1 is counted nowhere and matches nothing
 *   n_class      1 .. 64, else ODAM_E_INVALID
 *   max_gt       largest m_s of any scene (host copy); more than 4096 is ODAM_E_LIMIT, before any launch
 *   out_counts   [dev] [n_scene][3][n_class] int32   ground-truth boxes, predictions, true positives per class
 *   out_claimed  [dev] [sumN] int32   how many ground-truth boxes each prediction claimed
 *   out_gt_match [dev] [sumM] int32   index inside the scene of the claiming prediction, else -1
 *   A scene whose m_s on the device exceeds max_gt gets -1 in its whole count row and nothing else.
 */
#ifndef ODAM_EVAL_H
#define ODAM_EVAL_H
#include "odam_sq.h"
#ifdef __cplusplus
extern "C" {
#endif

int odam_box3d_iou_batch(odam_sq_ctx* ctx, int n_scene, const int* a_off, const int* b_off, const long long* pair_off,
                         long long n_pairs, const double* A, const double* B, const int* cls_a, const int* cls_b, int gate,
                         double* out_iou3d, double* out_bev, void* stream);
int odam_box3d_match_batch(odam_sq_ctx* ctx, int n_scene, const int* a_off, const int* b_off, const long long* pair_off,
                           const double* iou3d, const int* cls_pred, const int* cls_gt, double threshold, int n_class, int max_gt,
                           int* out_counts, int* out_claimed, int* out_gt_match, void* stream);

/*
 * odam_det_ap -- average precision of score-ranked predictions, every class and every image in one call: the reference's
 * src/utils/eval_utils.py voc_ap (:43-74) and eval_det_cls (:86-176) for all classes at once (csrc/det_ap.hip, arithmetic in
 * csrc/det_ap_core.h, restated by tests/det_ap_ref.py).  An image is a scene or a frame.  SIX launches per call, whatever the
 * sizes (overlap, count, rank, claim, flag, curve); stream-ordered, no synchronisation, no allocation, binary64.
 *
 *   kind         how a pair's overlap is found
 *                0  axis-aligned boxes of 8 corners, as eval_det_cls:147-152 computes it (min / max per axis, box_utils.iou_3d)
 *                1  read from `iou`, as odam_box3d_iou_batch wrote it with gate = 1: predictions are rows (A), ground truth columns
 *                   (B), pred_off / gt_off / pair_off / n_pairs are that call's a_off / b_off / pair_off / n_pairs
 *                2  detection rows [n_image][30][15] float32 as odam_detr_select_pack writes them, 3D: the box t_co -+ dims / 2
 *                   (columns 9-11, 6-8; DETR.nms_3d's box) in binary64, then iou_3d
 *                3  detection rows, 2D: columns 2-5 with box_utils.iou_2d
 *   n_image, n_pred, n_gt, n_class   the sizes every launch is shaped by (host copies).  n_class 1 .. 64.  n_pred counts SLOTS:
 *                for kinds 2, 3 n_pred == n_gt == 30 n_image (ODAM_AP_ROW_SLOTS), else ODAM_E_INVALID.  n_pred above
 *                ODAM_AP_MAX_PRED is ODAM_E_LIMIT, before any launch: the ranking counts pairs of predictions
 *   pred_off, gt_off  [dev] int32.  Kinds 0, 1: [n_image+1] offsets, image i owns the rows off[i] .. off[i+1]-1.  Kinds 2, 3:
 *                [n_image] counts, frame f owns the slots 30 f .. 30 f + count[f] - 1; a slot past the count is owned by nobody,
 *                is never read and gets no output word
 *   pred_box, gt_box  [dev] kind 0: float64 [n][8][3]; kinds 2, 3: the float32 blocks (class = column 1, score = column 14; a class
 *                word that is not in [0, 64) is no class); kind 1: not read, may be null
 *   cls_pred, cls_gt [dev] int32 [n_pred], [n_gt], score [dev] float64 [n_pred]: kinds 0, 1; not read for kinds 2, 3
 *   pair_off [dev] int64 [n_image+1], iou [dev] float64 [n_pairs], n_pairs: kind 1 only
 *   scratch      [dev] int32 [2 n_pred + 2 n_gt]; every word of it may be written, none past it
 *
 * Per prediction d (out_* [dev] [n_pred]):
 *   out_ovmax    float64: the largest IoU with a ground-truth box of ITS image and ITS class, boxes in their given order, replaced
 *                when `iou > ovmax` from -inf: the first of equal maxima wins, a NaN never; -inf when there is no such box
 *   out_jmax     int32: that box's index among ALL ground truth of the image (classes mixed, as given), -1 when none
 *   out_rank     int32: position inside its class by descending score; equal scores keep their input order and a NaN score ranks
 *                after every number (np.argsort(-confidence) leaves the order of equal keys open: this is a deviation)
 *   out_is_tp    int32: 1 when ovmax > ovthresh and no prediction of the class ranked before it has the same image, the same
 *                jmax and ovmax > ovthresh; else 0
 * Per ground-truth box (out_gt_claim [dev] [n_gt] int32): the index d of the true positive on it, else -1.
 * Per class c (out_npos, out_npred, out_ap [dev] [n_class]; out_cls_off [dev] [n_class+1] int32, cls_off[c+1] - cls_off[c] = npred[c]):
 *   out_order    [dev] int32, words cls_off[c] + r: the prediction of rank r
 *   out_tp, out_fp   [dev] int32, out_rec, out_prec [dev] float64, same words: inclusive prefix sums in rank order,
 *                rec = tp / npos, prec = tp / max(tp + fp, eps).  These five are [n_pred] long; words from cls_off[n_class] on are
 *                not written
 *   out_ap       voc_ap: the 11-point form when use_07_metric != 0, else the area under the precision envelope, summed in the
 *                order tests/det_ap_ref.py::ap_area restates.  npos == 0: NaN in both forms (the reference's 11-point form would
 *                give 0), with rec NaN and prec as computed; leave such a class out of a mean.  npos > 0, npred == 0: 0.
 * A prediction or box counts under NO class when its class id is outside 0 .. n_class-1, or (offsets that contradict the sizes
 * are not trusted) when no image's range off[i] <= d < off[i+1], inside [0, n], holds it, or, for a prediction, when its image's
 * ground-truth range or pair block does not lie inside [0, n_gt] / [0, n_pairs].  It is counted nowhere, matches nothing and has
 * no rank: out_ovmax NaN, out_jmax -1, out_rank -1, out_is_tp -1; out_gt_claim -1.  A frame count outside 0 .. 30 owns no slot.
 * n_pred == 0 (and n_image == 0) is ODAM_OK: the per-class words are still written.
 */
#define ODAM_AP_MAX_PRED 32768
#define ODAM_AP_ROW_SLOTS 30
int odam_det_ap(odam_sq_ctx* ctx, int kind, int n_image, int n_pred, int n_gt, int n_class, const int* pred_off, const int* gt_off,
                const void* pred_box, const void* gt_box, const int* cls_pred, const int* cls_gt, const double* score,
                const long long* pair_off, const double* iou, long long n_pairs, double ovthresh, int use_07_metric, int* scratch,
                double* out_ovmax, int* out_jmax, int* out_rank, int* out_is_tp, int* out_gt_claim, int* out_order, int* out_npos,
                int* out_npred, int* out_cls_off, double* out_ap, int* out_tp, int* out_fp, double* out_rec, double* out_prec,
                void* stream);

#ifdef __cplusplus
}
#endif
#endif
