/*
 * odam_merge.h -- C ABI of the track merge between the two fit passes, for every scene of a call at once.
 *
 * Replaces, of the reference (likojack/ODAM):
 *   src/scripts/run_merge.py:119-124   AgglomerativeClustering(n_clusters=None, distance_threshold, affinity="precomputed",
 *                                      linkage="average").fit(cost).labels_                              -> odam_merge_cluster
 *   src/scripts/run_merge.py:24-58     merge_tracks: per image the row of the longest member, class = mode   -> odam_merge_assemble
 * The pair costs come from odam_box3d_iou_batch with gate = 2 (odam_eval.h); the host path is odam_amd/merge.py::merge_process,
 * and both kernels are restated in numpy by tests/merge_ref.py.
 *
 * Conventions as in odam_sq.h: int return codes (0 = OK), odam_last_error(), [dev] / [host] pointers, the first argument is the
 * odam_sq_ctx of the device; stream-ordered on the caller's hipStream_t, no synchronisation, no allocation: every word of working
 * memory is the caller's `scratch`.  binary64, plain vector stores (csrc/track_merge.hip, arithmetic in csrc/track_merge_core.h).
 * Argument checks come before any device work; what only the device can see (offsets, costs, rows) is answered by a status word
 * per scene, never by a fault: a scene with a non-zero status has no other output a caller may use.
 *
 * Scenes as in odam_eval.h with A = B: scene s owns the tracks a_off[s] .. a_off[s+1]-1 (n_s of them) and the n_s x n_s words
 * pair_off[s] .. pair_off[s+1]-1 of the IoU block, row-major.
 *   a_off [dev] [n_scene+1] int32     pair_off [dev] [n_scene+1] int64
 *
 * odam_merge_cluster -- average-linkage clustering of every scene, ONE launch, one workgroup per scene.
 *   n_tracks     a_off[n_scene] (host copy)        n_pairs   pair_off[n_scene] (host copy)
 *   max_tracks   largest n_s of any scene (host copy); more than ODAM_MERGE_MAX_TRACKS is ODAM_E_LIMIT, before any launch
 *   iou3d        [dev] [n_pairs]  as odam_box3d_iou_batch wrote it.  cost(i, j) = cost(j, i) = 1 - iou3d[i][j] is taken from the UPPER
 *                triangle i < j only (the clipper is not symmetric), the diagonal is 0: odam_amd/merge.py::cost_matrix
 *   threshold    the distance threshold (0.95 in run_merge.py)
 *   scratch      [dev] [n_pairs] float64: the working copy of the costs; every word may be written, none past it
 *   out_linkage  [dev] [n_tracks][4] float64: rows a_off[s] .. a_off[s] + n_s - 2 are scene s's linkage matrix exactly as
 *                scipy.cluster.hierarchy.linkage(condensed cost, "average") returns it (children, distance, count), bit for bit; the
 *                row a_off[s] + n_s - 1 is not written
 *   out_labels   [dev] [n_tracks] int32: sklearn's labels_ (positions in _hc_cut's heap)
 *   out_n_cluster, out_status  [dev] [n_scene] int32
 * The algorithm is scipy's nearest-neighbour chain: the chain restarts at the lowest live index; the nearest neighbour of the chain's
 * top is the lowest index with the strictly smallest distance, the previous chain element winning an exact tie; merging x < y leaves
 * the cluster at y with D[i][y] = (n_x D[i][x] + n_y D[i][y]) / (n_x + n_y), each operation rounded on its own; the merges are sorted
 * stably by distance and relabelled by scipy's union-find; n_cluster = #(distance >= threshold) + 1; the labels come from CPython's
 * heapq on negated node ids as sklearn's _hc_cut uses it.
 *
 * odam_merge_assemble -- merge_tracks for every cluster of every scene: THREE launches (select: one workgroup per cluster; scan;
 * gather) after two memsets.
 *   labels, n_cluster, cluster_status   [dev] as odam_merge_cluster wrote them
 *   row_off      [dev] [n_tracks+1] int32: track t (numbered across scenes) owns the rows row_off[t] .. row_off[t+1]-1
 *   rows         [dev] [n_rows][14] float64, as odam_sq_prepare_batch takes them; columns 0 (frame id) and 1 (class) are read
 *   n_rows       row_off[n_tracks] (host copy)
 *   max_cand     the most rows the tracks of one scene have together (host copy): sizes the sort; a cluster whose members have more
 *                than min(max_cand rounded up to a power of two, ODAM_SQ_PREPARE_MAX_ROWS) rows sets ODAM_MERGE_TOO_MANY_ROWS
 *   img_off      [dev] [n_scene+1] int32: scene s owns the entries img_off[s] .. img_off[s+1]-1 of the two image tables
 *   img_ids      [dev] int64, ascending inside a scene     img_order  [dev] int32: the image index (position in img_names) of img_ids[i]
 *   n_imgs       img_off[n_scene] (host copy)
 *   scratch      [dev] int32 [n_rows + 4 n_tracks + 4]
 *   out_off      [dev] [n_tracks+1] int32: merged track o (numbered across scenes, scene after scene, clusters in label order, a
 *                cluster without a row left out) owns the words out_off[o] .. out_off[o+1]-1 of out_src; out_off[0] = 0, no gaps
 *   out_src      [dev] [n_rows] int32: the source row of every merged row, per merged track in image order
 *   out_cls      [dev] [n_tracks] int32: the class of merged track o
 *   out_rows14   [dev] [n_rows][14] float64, nullable: rows[out_src[k]] with column 1 replaced by the merged class
 *   out_n_out    [dev] [n_scene] int32: merged tracks of scene s        out_status  [dev] [n_scene] int32
 *   out_total    [dev] [2] int32: merged tracks and merged rows of the whole call
 * Members of a cluster are taken in track order; the class is scipy.stats.mode of column 1 over all rows of all members (the
 * smallest of the most frequent values); a row is a view of image k only if its column 0 EQUALS that frame id as a binary64 number;
 * for each image the row of the member with the most rows wins (all rows count), the first such member in track order on a tie.
 * A scene with a non-zero status contributes no merged track.
 */
#ifndef ODAM_MERGE_H
#define ODAM_MERGE_H
#include "odam_sq.h"
#ifdef __cplusplus
extern "C" {
#endif

#define ODAM_MERGE_MAX_TRACKS 1024
/* status words of both calls */
#define ODAM_MERGE_BAD_OFFSETS 1      /* a_off / pair_off / row_off / img_off of the scene contradict each other or the sizes given */
#define ODAM_MERGE_BAD_COST 2         /* a cost that is not a finite number */
#define ODAM_MERGE_NOT_CLUSTERED 3    /* assemble: the scene's cluster_status is not 0 */
#define ODAM_MERGE_BAD_CLASS 4        /* a class value that is not an integer in 0..63 */
#define ODAM_MERGE_REPEATED_FRAME 5   /* a frame id that occurs twice in one track (the reference asserts) */
#define ODAM_MERGE_TOO_MANY_ROWS 6    /* more candidates in one cluster than the sort holds */

int odam_merge_cluster(odam_sq_ctx* ctx, int n_scene, const int* a_off, const long long* pair_off, int n_tracks, long long n_pairs,
                       int max_tracks, const double* iou3d, double threshold, double* scratch, double* out_linkage, int* out_labels,
                       int* out_n_cluster, int* out_status, void* stream);
int odam_merge_assemble(odam_sq_ctx* ctx, int n_scene, const int* a_off, int n_tracks, const int* labels, const int* n_cluster,
                        const int* cluster_status, const int* row_off, const double* rows, int n_rows, int max_cand, const int* img_off,
                        const long long* img_ids, const int* img_order, int n_imgs, int* scratch, int* out_off, int* out_src,
                        int* out_cls, double* out_rows14, int* out_n_out, int* out_status, int* out_total, void* stream);

#ifdef __cplusplus
}
#endif
#endif
