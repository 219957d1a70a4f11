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

#ifdef __cplusplus
}
#endif
#endif
