/*
 * odam_sq.h -- C ABI of the MI355X (gfx950) super-quadric multi-view fit.
 *
 * Drop-in boundary for the reference's (likojack/ODAM) SQ path:
 *   src/scripts/run_multi_view.py:22-76       optim_process       (per-object driver, host Python)
 *   src/super_quadric/sq_libs.py:432-475      SuperQuadricOptimizer.run   -> odam_sq_fit_batch
 *   src/super_quadric/sq_libs.py:577-595      compute_ellipsoid_points    -> odam_sq_points_batch
 *   learnable_primitives/fast_sampler/sampling.hpp:5-15  sample_on_batch  -> odam_sq_sample
 *
 * Conventions: plain pointers and sizes, no exceptions across the boundary, int return code
 * (0 = OK, otherwise an ODAM_E_* value; odam_last_error() returns a static message), caller-owned
 * buffers, work is enqueued on the caller's hipStream_t (passed as void*).  All scratch lives in the handle: the
 * *_batch calls neither synchronise nor allocate, except that odam_sq_fit_batch grows the handle's exchange
 * buffer (hipMalloc) the first time a larger problem is seen and, for a call with more objects than the device has CUs, reads the
 * view counts back (one small copy and a synchronisation of the caller's stream) to fit the objects longest first.  A handle serves one launch at a time (use one
 * per stream / thread).
 * Pointers marked [dev] are device pointers, [host] host pointers.
 */
#ifndef ODAM_SQ_H
#define ODAM_SQ_H
#ifdef __cplusplus
extern "C" {
#endif

#define ODAM_OK 0
#define ODAM_E_INVALID 1   /* bad argument (null pointer, size out of range) */
#define ODAM_E_HIP 2       /* a HIP runtime call failed */
#define ODAM_E_LIMIT 3     /* problem exceeds a compiled limit (views per object, iterations) */

#define ODAM_SQ_POINTS 1000      /* surface samples per super-quadric   (sq_libs.py:545) */
#define ODAM_SQ_MAX_VIEWS 1024   /* views one workgroup reduces; an object split over k workgroups may have k times as many
                                    (k <= 32, odam_config sq.split, and k * padded object count <= number of CUs; odam_sq_fit_batch takes at most
                                    16 * ODAM_SQ_MAX_VIEWS views per object) */

/* representation codes, sq_libs.py:362-386 */
#define ODAM_SQ_SUPER_QUADRIC 0  /* 9 parameters optimised */
#define ODAM_SQ_CUBE 1           /* shapes frozen (caller passes -10000), 7 optimised */
#define ODAM_SQ_QUADRIC 2        /* shapes frozen at -0, 7 optimised */

typedef struct odam_sq_ctx odam_sq_ctx;

const char* odam_last_error(void);

/* Creates the per-device context: uploads the sampler's constant random draws
 * (std::mt19937(0), _sampler.pyx:438) and the Adam bias-correction tables for up to max_iters
 * steps (lr 0.01 / 0.1 for the shape logits, sq_libs.py:373-387). */
int odam_sq_create(int max_iters, odam_sq_ctx** out);
int odam_sq_destroy(odam_sq_ctx* ctx);

/*
 * Fits n_obj super-quadrics, n_iters Adam steps each, entirely on device: one 1024-thread workgroup per object,
 * or -- when the grid would leave most CUs idle -- up to thirty-two per object that split the views of the per-view
 * extent search by residue class and exchange one sub-tree root each per step (results are bit-identical either way).
 *   init_params  [dev] [n_obj][9]   translate[3], angle, scales[3] (= sqrt(dims/2)), shapes[2]
 *   class_id     [dev] [n_obj]      0..7 selects the scale prior row; < 0 = no prior (prior=False)
 *   view_offsets [dev] [n_obj+1]    object o owns views view_offsets[o] .. view_offsets[o+1]-1
 *   P            [dev] [sumF][12]   row-major 3x4 projection K @ inv(T_wc)[:3,:] as float32
 *   tgt          [dev] [sumF][4]    bbox edge in pixels per direction x_min,x_max,y_min,y_max
 *                                   (the reference stores gt = -pixel and compares with -gt)
 *   mask         [dev] [sumF][4]    1 = edge is a constraint, 0 = dropped (near the image border)
 *   prior_icov   [dev] [8][9]       row-major 3x3 inverse covariances, CLASS_MAPPER order
 *   out_params   [dev] [n_obj][9]
 *   out_points   [dev] [n_obj][1000][3]  surface of the fitted SQ (compute_ellipsoid_points); nullable
 *   loss_log     [dev] [n_obj][n_iters]  loss_2d per step (sq_libs.py:471); nullable
 *   traj         [dev] [n_obj][n_iters][9] parameters after every step; nullable (parity tests)
 *   max_views    largest view count of any object (host-known; sizes the workgroup's LDS); up to 16 * ODAM_SQ_MAX_VIEWS
 *                when few enough objects are fitted per call for the view split to cover it, else ODAM_E_LIMIT
 */
int odam_sq_fit_batch(odam_sq_ctx* ctx, int n_obj, const float* init_params, const int* class_id,
                      const int* view_offsets, const float* P, const float* tgt, const float* mask,
                      const float* prior_icov, int n_iters, int representation, int max_views,
                      float* out_params, float* out_points, float* loss_log, float* traj,
                      void* stream);

/*
 * The resumable fit.  odam_sq_fit_batch loses the Adam moments, the step count and the scales the prior is measured from when its
 * launch ends; this entry point takes and returns them, so that a fit of n steps equals a fit of k steps followed by a resumed fit
 * of n - k steps on the same views, bit for bit, on every output.  Arguments as odam_sq_fit_batch, and:
 *   state_in   [dev]  [n_obj][ODAM_SQ_STATE_FLOATS]  nullable.  Null: a cold start from init_params, exactly as odam_sq_fit_batch.
 *                     Given: EVERY object starts from its row and init_params is ignored (may be null).  An object that starts
 *                     cold inside such a call gets the row of a fit that has not begun: its initial parameters, zero moments,
 *                     scales_init = its initial scales, 0 steps.
 *   t0         [host] [n_obj]  steps each object has taken so far = word 30 of its row, as the caller knows it on the host.
 *                     Required with state_in, ignored without.  All checks are made on it before anything is enqueued, so neither
 *                     path reads the device back: a negative entry is ODAM_E_INVALID; t0[i] + n_iters > max_iters of the context
 *                     is ODAM_E_LIMIT with both numbers in the message.  (The kernel takes the count from the row and clamps it to
 *                     the table; a row that disagrees with t0 is the caller's error and gives a defined, wrong, result.)
 *   state_out  [dev]  [n_obj][ODAM_SQ_STATE_FLOATS]  nullable; may be the buffer of state_in (a workgroup reads its row before the
 *                     first step, one stores it after the last; but not where the view split is taken -- several workgroups read).
 * State row (float32 words):
 *    0 ..  8  parameters (= out_params)
 *    9 .. 17  Adam first moments  (exp_avg)
 *   18 .. 26  Adam second moments (exp_avg_sq)
 *   27 .. 29  scales_init: the scales of the FIRST launch's init_params, which the scale prior is measured from (sq_libs.py:454,465)
 *   30        steps taken so far, an exact small integer
 *   31        representation code of the launch that wrote the row (checked by the caller: odam_amd/sq.py refuses a mismatch)
 * Step i of the launch uses row t0 + i of the bias-correction table odam_sq_create uploaded.  loss_log and traj hold this launch's
 * n_iters rows only.  class_id is passed again with every call: an object without prior (class_id < 0) resumes as it started.
 * Scheduling (view split, two workgroups per CU, longest object first) is that of odam_sq_fit_batch for the same views; with several
 * workgroups per object all of them load the row and the one that writes out_params stores it.
 */
#define ODAM_SQ_STATE_FLOATS 32
int odam_sq_fit_resume(odam_sq_ctx* ctx, int n_obj, const float* init_params, const int* class_id,
                       const int* view_offsets, const float* P, const float* tgt, const float* mask,
                       const float* prior_icov, int n_iters, int representation, int max_views,
                       float* out_params, float* out_points, float* loss_log, float* traj,
                       const float* state_in, const int* t0, float* state_out, void* stream);

/* Shape of the newest fit launch of this context (host-side note, no device work): shape4 [host][4] = workgroups in the grid, threads
 * per workgroup (1024, or 512 for two workgroups per CU), workgroups per object of the view split (1 = off), 1 if the objects were
 * dealt longest first. */
int odam_sq_last_launch(odam_sq_ctx* ctx, int* shape4);

/* Surface points of n super-quadrics: params [dev][n][9] -> out_points [dev][n][1000][3]. */
int odam_sq_points_batch(odam_sq_ctx* ctx, int n, const float* params, float* out_points, void* stream);

/* Projected extent of n super-quadric surfaces in one camera -- what OdamProcess._prepare_tracks (src/processor.py:181-207)
 * computes per live track and frame: params [dev][n][9] -> surface points (as odam_sq_points_batch) -> float64
 * [p, 1] T_cw^T K^T, divide by depth, min / max.  T_cw12_K9 [host][21]: rows 0..2 of inv(T_wc) (12 values, row-major), then K
 * (9, row-major); out_px [dev][n][4] float64 = x_min, y_min, x_max, y_max.  Stream-ordered. */
int odam_sq_project_extents(odam_sq_ctx* ctx, int n, const float* params, const double* T_cw12_K9, double* out_px, void* stream);

/* The reference's one native symbol under its own name and signature
 * (learnable_primitives/fast_sampler/sampling.hpp:5-15; bound by _sampler.pyx:430-439, which passes
 * buffer_size = 201, seed = 0):  shapes [host][B][M][3], epsilons [host][B][M][2] -> etas, omegas [host][B][M][N].
 * One std::mt19937(seed) stream over all primitives in (b, m) order.  void, no error path, re-entrant -- as upstream. */
void sample_on_batch(float* shapes, float* epsilons, float* etas, float* omegas, int B, int M, int N,
                     int buffer_size, int seed);

/* sample_on_batch for the call the pipeline makes (B = M = 1, N = 1000, buffer_size = 201, seed = 0) with this
 * library's return-code convention:  a[3], e[2] -> etas[1000], omegas[1000]  (all [host]). */
int odam_sq_sample(const float* a, const float* e, float* etas, float* omegas);

/* Result extraction of a fit pass (run_multi_view.py:66-67): the reference's compute_oriented_bbox (src/utils/box_utils.py:319-410)
 * for n_obj surfaces -- qhull's 2-D hull of the xy projection walked as an OPEN polygon from qhull's own start vertex, the
 * smallest rectangle over the edge directions, the z extent.  points [host][n_obj][n_pts][3] float32 (the fit's out_points,
 * downloaded) -> corners [host][n_obj][8][3] float64, status [host][n_obj]: 0 = done; 1 = this object sits inside qhull's
 * round-off tolerance band (or two candidate rectangles tie to 1e-9) and must be recomputed with scipy / qhull itself, which is
 * what the reference calls -- odam_amd/multi_view.py does.  Host code, multi-threaded, no device call. */
int odam_sq_oriented_bbox(const float* points, int n_obj, int n_pts, double* corners, int* status);
/* the hull alone (tests): hull [host][n_pts] <- point indices in the order of scipy's ConvexHull(points[:, :2]).vertices */
int odam_sq_hull2d(const float* points, int n_pts, int* hull, int* n_hull, int* status);

/*
 * The reference's second object model, QuadricOptimizer.run (src/super_quadric/sq_libs.py:194-241): the dual quadric
 * Q = T diag((scale_factor * h)^2, -1) T^T, T = [rotz(angle) | translate], fitted to the bbox edges of its projected conics
 * C = M Q M^T by n_iters Adam steps (lr 0.01, no prior).  ONE launch for all objects, one wavefront per object, views strided
 * over the lanes; stream-ordered, and no allocation except that the handle's bias-correction table for this path grows
 * (hipMalloc, a synchronisation of the caller's stream if an older table is replaced) the first time more steps are asked for.
 * Nothing odam_sq_create uploaded is touched; n_iters is NOT bounded by the context's max_iters.
 *   init5        [dev] [n_obj][5]   translate[3], angle, scale_factor (the reference starts at 1)
 *   half_dims    [dev] [n_obj][3]   h = dims / 2 as float32 (constant)
 *   view_offsets, P, tgt, mask      as odam_sq_fit_batch (tgt in pixels, order x_min, x_max, y_min, y_max)
 *   max_views    largest view count of any object, 1 .. 16 * ODAM_SQ_MAX_VIEWS, else ODAM_E_LIMIT
 *   out5         [dev] [n_obj][5]
 *   out_Q        [dev] [n_obj][16]  row-major params2mat of out5 (float32, not symmetrised: as the reference's product)
 *   loss_log     [dev] [n_obj][n_iters]     loss_2d per step; nullable
 *   traj         [dev] [n_obj][n_iters][5]  parameters after every step; nullable
 *   status       [dev] [n_obj][2]   code, step:  0, -1 = fitted;  1, s = a view's discriminant 4 C_i2^2 - 4 C_ii C_22 was
 *                negative (or NaN) at step s (0-based) -- where the reference asserts (sq_libs.py:129,136): the object keeps the
 *                parameters it had before that step, its loss_log rows from s on are NaN and its traj rows repeat them;
 *                2, 0 = the object's view count is outside 1 .. max_views (nothing fitted).  Other objects are unaffected.
 * odam_dq_set_group_waves: objects per workgroup (1, 2, 4 or 8; default 4) -- scheduling only, every result is bit-identical.
 * DualQuadric.get_srt / compute_ellipsoid_points (sq_libs.py:257-348) are NOT in this library: LAPACK's geev decides the
 * eigenvector bits in the reference (scipy.linalg.eig), so odam_amd/sq.py calls the same scipy routine on the host.
 */
int odam_dq_fit_batch(odam_sq_ctx* ctx, int n_obj, const float* init5, const float* half_dims, const int* view_offsets,
                      const float* P, const float* tgt, const float* mask, int n_iters, int max_views, float* out5,
                      float* out_Q, float* loss_log, float* traj, int* status, void* stream);
int odam_dq_set_group_waves(odam_sq_ctx* ctx, int waves);

/*
 * The closed-form dual quadric of an object from the planes through its 2D box edges -- no 3D guess, float64 throughout:
 *   src/super_quadric/sq_libs.py:30-36           compute_quadric_svd  (A = Sigma^T Sigma, eigenvector of the smallest eigenvalue)
 *   src/utils/tracking_gt_utils.py:198-205       load_pred_object's plane_vecs: bbox_to_lines, normalize_plane(line @ P), plane_2vect
 *   src/super_quadric/quadric_helper.py:16-48    quadric_2mat, plane_2vect
 * ONE launch for all objects, one wavefront per object, views strided over the lanes, odam_dq_set_group_waves objects per
 * workgroup; stream-ordered, no synchronisation, no allocation.  The accumulation order of A and the Jacobi pivot order are fixed
 * (csrc/dq_svd.hip), so every result is bit-identical from launch to launch and for every group size.
 *   view_offsets [dev] [n_obj+1]    object o owns rows view_offsets[o] .. view_offsets[o+1]-1
 *   P            [dev] [sumF][12]   row-major 3x4 projection K @ inv(T_wc)[:3,:] as float64
 *   edges        [dev] [sumF][4]    bbox edge in pixels (float64), order x_min, x_max, y_min, y_max
 *   mask         [dev] [sumF][4]    != 0: the edge is a constraint; 0: dropped (its edge value is not read)
 *   max_views    largest view count of any object, 1 .. 16 * ODAM_SQ_MAX_VIEWS, else ODAM_E_LIMIT
 *   out_Q        [dev] [n_obj][16]  row-major symmetric 4x4, normalised Q <- -Q / Q[3][3] (so Q[3][3] = -1)
 *   out_eig      [dev] [n_obj][3]   eigenvalues of A: the smallest, the second smallest, the largest
 *   status       [dev] [n_obj]      0 = an ellipsoid (the three eigenvalues of Q[:3,:3] + t t^T, t = -Q[:3,3], are > 0, the test of
 *                DualQuadric.get_srt, sq_libs.py:257-280);  1 = not an ellipsoid, or Q[3][3] = 0 (then out_Q is the matrix of the
 *                unit eigenvector, not normalised), or a Jacobi iteration reached its sweep limit (out_Q, out_eig from the last
 *                iterate);  2 = fewer than 9 unmasked edges, or a view count outside 1 .. max_views: nothing computed, out_Q and
 *                out_eig are NaN.  Other objects are unaffected.
 */
int odam_dq_svd_batch(odam_sq_ctx* ctx, int n_obj, const int* view_offsets, const double* P, const double* edges,
                      const float* mask, int max_views, double* out_Q, double* out_eig, int* status, void* stream);

/*
 * Reprojection: the 2D box a fitted object predicts in every one of its views, and how far that is from the detections.  The forward
 * half of the reference's two box predictions, which it evaluates inside its fits only and never returns per view:
 *   src/super_quadric/sq_libs.py:395-430   SuperQuadricOptimizer.constraint_2d   -> odam_sq_reproject_batch + odam_reproject_score_f32
 *   src/super_quadric/sq_libs.py:289-314   DualQuadric.get_bbox                  -> odam_dq_reproject_batch + odam_reproject_score_f64
 * ONE launch per call for all objects and all views (csrc/reproject.hip, arithmetic in csrc/reproject_core.h); stream-ordered, no
 * synchronisation, no allocation.  view_offsets [dev][n_obj+1] as above; an object whose view count is outside 1 .. max_views owns
 * no view.  max_views: 1 .. 16 * ODAM_SQ_MAX_VIEWS, else ODAM_E_LIMIT.  No call writes a word that no view or object owns.
 *
 * odam_sq_reproject_batch, float32 -- any of the three super-quadric representations, from surface points:
 *   points       [dev] [n_obj][n_pts][3]  surface points (odam_sq_points_batch, or the fit's out_points); n_pts 1 .. 4096, else
 *                ODAM_E_LIMIT
 *   P            [dev] [sumF][12]   projections as float32, as the fit saw them
 *   out_ext      [dev] [sumF][4]    x_min, x_max, y_min, y_max over the points with depth > 0.5, each u = q_x / (|q_z| + 1e-6); start
 *                values +1e6 / -1e6, so a view without such a point holds exactly (1e6, -1e6, 1e6, -1e6); a NaN coordinate of such a
 *                point makes that extent NaN (torch.min / torch.max); a zero is stored as +0
 *   out_nvalid   [dev] [sumF]       points with depth > 0.5
 * odam_dq_reproject_batch, float64 -- a dual quadric, fitted or closed-form:
 *   Q            [dev] [n_obj][16]  row-major 4x4
 *   P            [dev] [sumF][12]   projections as float64
 *   out_ext      [dev] [sumF][4]    x_min, x_max, y_min, y_max of the conic C = (P Q) P^T
 *   out_status   [dev] [sumF]       0; 1 = a discriminant 4 C_i2^2 - 4 C_ii C_22 is negative or NaN, or C_22 = 0: the four extents of
 *                that view are NaN, every other view is unaffected
 * odam_reproject_score_f32 / _f64 (T = float / double) -- per view and per object, from either of the above:
 *   ext          [dev] [sumF][4]    predicted edges
 *   bad          [dev] [sumF]       nullable; != 0: the view has no prediction (out_nvalid == 0, or out_status)
 *   boxes        [dev] [sumF][4]    detected edges in pixels, x_min, x_max, y_min, y_max
 *   mask         [dev] [sumF][4]    != 0: the edge is a constraint
 *   img_w, img_h > 0, else ODAM_E_INVALID: the predicted box is clipped to the image for the IoU (detections are clipped already)
 *   out_res      [dev] [sumF][4]    |ext - box| of a constrained edge, NaN -> 0; 0 of any other
 *   out_iou      [dev] [sumF]       IoU of the detected box with the clipped predicted box; 0 for a bad view or an empty union
 *   out_obj      [dev] [n_obj][4]   loss_2d = sum over the four directions of (sum of residuals / F), what the fits log;  mean_abs_px =
 *                sum of residuals / n_edges (NaN without an edge);  mean_iou;  min_iou
 *   out_obj_i    [dev] [n_obj][3]   worst_view (index inside the object of the first view with the smallest IoU), n_edges
 *                (constrained edges), n_bad (bad views)
 *   An object without views gets NaN x 4 and -1, 0, 0.  Sums run in the order of odam_dq_fit_batch (lane partials, XOR butterfly),
 *   so every result is bit-identical from launch to launch and for every odam_dq_set_group_waves.
 */
int odam_sq_reproject_batch(odam_sq_ctx* ctx, int n_obj, const float* points, int n_pts, const int* view_offsets, const float* P,
                            int max_views, float* out_ext, int* out_nvalid, void* stream);
int odam_dq_reproject_batch(odam_sq_ctx* ctx, int n_obj, const double* Q, const int* view_offsets, const double* P, int max_views,
                            double* out_ext, int* out_status, void* stream);
int odam_reproject_score_f32(odam_sq_ctx* ctx, int n_obj, const int* view_offsets, const float* ext, const int* bad,
                             const float* boxes, const float* mask, float img_w, float img_h, int max_views, float* out_res,
                             float* out_iou, float* out_obj, int* out_obj_i, void* stream);
int odam_reproject_score_f64(odam_sq_ctx* ctx, int n_obj, const int* view_offsets, const double* ext, const int* bad,
                             const double* boxes, const float* mask, double img_w, double img_h, int max_views, double* out_res,
                             double* out_iou, double* out_obj, int* out_obj_i, void* stream);

/*
 * The prelude of a fit pass on the device: what run_multi_view.py:44-62 does per track before it fits -- the views, constraint rows
 * and initial shape of EVERY track in one launch (csrc/sq_prepare.hip), one workgroup per track, no device-wide barrier.  Replaces, for
 * sequences whose frame ids are all different:
 *   src/utils/tracking_gt_utils.py:145-211, 59-66   load_pred_object (views of a track in image order, first row of a frame id wins;
 *                                                   class = median; t_wo = mean) and averaging_T_wos
 *   src/super_quadric/quadric_helper.py:69-109      bbox_to_lines (an edge is a constraint when it is farther than thr from the border)
 *   src/scripts/run_multi_view.py:44-62             the views with at least one constrained edge, get_3d_box of the detector's pose
 *   src/super_quadric/sq_libs.py:353-371, 41-58     SuperQuadricOptimizer.__init__ / QuadricOptimizer.__init__ (the initial parameters)
 * Every rotation averaged is a rotz(a), quaternion (0, 0, sin a/2, cos a/2), so the mean rotation of averaging_T_wos (the leading
 * eigenvector of sum q q^T) is rotz(yaw) with yaw = atan2(sum sin a, sum cos a): no eigen-solver.
 * Stream-ordered, no synchronisation, no allocation.
 *   row_off      [dev] [n_obj+1]    track o owns rows row_off[o] .. row_off[o+1]-1
 *   rows         [dev] [R][14]      float64: the first 14 columns of every track row (frame id, class, x_min, y_min, x_max, y_max,
 *                                   dims[3], t_wo[3], yaw, one more), track after track
 *   max_rows     largest row count of any track as the caller knows it on the host: sizes the workgroup and its LDS (8 bytes per row of
 *                the next power of two).  A value above ODAM_SQ_PREPARE_MAX_ROWS is taken as that.  A track with more rows than the
 *                launch was sized for gets status 3, whatever else is true of it; < 1 is ODAM_E_INVALID.
 *   img_ids      [dev] [n_img]      int64 frame ids of the images, ascending, all different, |id| < 2^31
 *   img_order    [dev] [n_img]      image index of img_ids[i] (an entry outside 0 .. n_img-1 is an image no row can be a view of)
 *   P_cws        [dev] [n_img][12]  float64 projection of every image
 *   img_w, img_h, thr               edge e of a view is a constraint when thr < value < lim - thr (both strict, float64),
 *                                   lim = img_w, img_w, img_h, img_h for the order x_min, x_max, y_min, y_max (columns 2, 4, 3, 5)
 *   representation                  ODAM_SQ_SUPER_QUADRIC / _CUBE / _QUADRIC, or ODAM_SQ_DUAL_QUADRIC
 * Per track (o):
 *   cls          [dev] [n_obj]      int(median of column 1 over ALL rows), an even count averaging the two middle values; -1 when a class
 *                                   value is not an integer in 0..63 (or the track has no row)
 *   n_obs        [dev] [n_obj]      views: rows whose frame id (column 0 truncated to int32; a value outside int32 is no id) is in
 *                                   img_ids, the lowest row of each id, in ascending image index
 *   n_valid      [dev] [n_obj]      views with at least one constrained edge
 *   init         [dev] [n_obj][9]   float32 of (translation[3], yaw, sqrt(scales / 2)[3], shapes[2] = -0.0 or, for the cube, -10000);
 *                                   for ODAM_SQ_DUAL_QUADRIC [n_obj][5] = (translation[3], yaw, 1)
 *   half_dims    [dev] [n_obj][3]   ODAM_SQ_DUAL_QUADRIC only (else nullable, not written): float32(scales / 2)
 *   pose         [dev] [n_obj][7]   float64 translation[3], yaw, scales[3].  t_wo = (row-order sum of columns 9..11 over ALL rows) / rows;
 *                                   translation = (t_wo + ... + t_wo, n_obs terms added one after the other) / n_obs, the mean of n_obs
 *                                   equal poses that averaging_T_wos takes, and what init and bboxes_dl use; scales = (view-order sum of
 *                                   columns 6..8 over the views) / n_obs; yaw = atan2(sum sin, sum cos) of column 12 over the views
 *   bboxes_dl    [dev] [n_obj][8][3] float64 get_3d_box(scales, rotz(yaw), translation)
 *   status       [dev] [n_obj]      0;  ODAM_SQ_PREPARE_NO_VIEW (1): no view -- cls, n_obs = n_valid = 0 and status are written, nothing
 *                                   else;  ODAM_SQ_PREPARE_BAD_CLASS (2): a class value is not an integer in 0..63 -- cls = -1, everything
 *                                   else as for status 0;  ODAM_SQ_PREPARE_TOO_MANY_ROWS (3): decided from row_off alone, no row is read --
 *                                   cls = -1, n_obs = n_valid = 0, nothing else written.  1 goes before 2.
 * Per view, written from row_off[o] on in image order; the words of a track beyond its n_obs views are not touched:
 *   view_img     [dev] [R]          image index
 *   view_row     [dev] [R]          row inside the track (0-based) the view came from
 *   tgt          [dev] [R][4]       float32 edge value where it is a constraint, else 0
 *   mask         [dev] [R][4]       1 / 0
 *   P            [dev] [R][12]      float32(P_cws[image])
 *   valid        [dev] [R]          1: at least one constrained edge
 */
#define ODAM_SQ_DUAL_QUADRIC 3
#define ODAM_SQ_PREPARE_MAX_ROWS 16384
#define ODAM_SQ_PREPARE_NO_VIEW 1
#define ODAM_SQ_PREPARE_BAD_CLASS 2
#define ODAM_SQ_PREPARE_TOO_MANY_ROWS 3
int odam_sq_prepare_batch(odam_sq_ctx* ctx, int n_obj, const int* row_off, const double* rows, int max_rows, int n_img,
                          const long long* img_ids, const int* img_order, const double* P_cws, double img_w, double img_h,
                          double thr, int representation, int* cls, int* n_obs, int* n_valid, float* init, float* half_dims,
                          double* pose, double* bboxes_dl, int* status, int* view_img, int* view_row, float* tgt, float* mask,
                          float* P, int* valid, void* stream);

/*
 * odam_sq_prepare_batch for the tracks of MANY scenes in one launch: the single image table and image size become one per scene.
 * Still one workgroup per track; it finds its scene in trk_off (a binary search on the workgroup's index) and searches that scene's
 * slice of img_ids only.  Every output word is the word odam_sq_prepare_batch writes when it is called on that scene alone; view_img
 * stays the image index INSIDE the scene, per-view words still start at row_off[o], status codes and their precedence are the same.
 * Stream-ordered, no synchronisation, no allocation, no device-wide barrier.
 *   n_scene                         scenes (>= 1 where there is a track)
 *   trk_off      [dev] [n_scene+1]  scene s owns tracks trk_off[s] .. trk_off[s+1]-1 (trk_off[0] = 0, trk_off[n_scene] = n_obj, not
 *                                   decreasing; an empty scene is legal).  A track no scene owns has no image: status 1
 *   img_off      [dev] [n_scene+1]  scene s owns entries img_off[s] .. img_off[s+1]-1 of img_ids, img_order and P_cws, the scenes' tables
 *                                   one after the other; a slice that does not lie inside 0 .. n_img is taken as empty
 *   n_img                           entries of the concatenated tables
 *   img_ids      [dev] [n_img]      ascending and all different inside every scene's slice; the same id may appear in several scenes
 *   img_order    [dev] [n_img]      image index of img_ids[i] inside its scene, 0 .. (images of the scene) - 1
 *   P_cws        [dev] [n_img][12]  projection of image j of scene s at entry img_off[s] + j
 *   img_wh       [dev] [n_scene][2] float64 (img_w, img_h) of every scene
 *   scene_rows   [dev] [n_scene]    nullable.  The max_rows odam_sq_prepare_batch would be given for scene s alone.  That call sizes its
 *                                   workgroups from max_rows, the size decides how a track's sorted rows are dealt to the threads, and that
 *                                   the order of the sin / cos sums behind the yaw; with scene_rows a workgroup deals them as the launch
 *                                   for its scene would (and refuses tracks as it would: status 3 beyond the power of two that holds
 *                                   scene_rows[s]), so the yaw has that launch's bits.  Values above max_rows are taken as max_rows.  Null:
 *                                   every scene as a launch with this call's max_rows
 * Everything else as odam_sq_prepare_batch.
 */
int odam_sq_prepare_scenes(odam_sq_ctx* ctx, int n_obj, const int* row_off, const double* rows, int max_rows, int n_scene,
                           const int* trk_off, const int* img_off, int n_img, const long long* img_ids, const int* img_order,
                           const double* P_cws, const double* img_wh, const int* scene_rows, double thr, int representation, int* cls,
                           int* n_obs,
                           int* n_valid, float* init, float* half_dims, double* pose, double* bboxes_dl, int* status,
                           int* view_img, int* view_row, float* tgt, float* mask, float* P, int* valid, void* stream);

#ifdef __cplusplus
}
#endif
#endif
