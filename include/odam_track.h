/*
 * odam_track.h -- C ABI of the network-free association: the reference's IoU tracker, the frame loop of whole sequences in one launch.
 *
 * Replaces, of the reference (likojack/ODAM):
 *   src/scripts/run_tracking.py:37-52      convert_det_to_list (clip of the pixel box, t_wo = T_wc t_co)       -> odam_track_iou_step
 *   src/scripts/run_tracking.py:106-170    match_tracks (score order, ordered scan of the tracks, attach)     -> odam_track_iou_step
 *   src/scripts/run_tracking.py:55-103     init_tracks without its ORB / depth side data (:61-63, :76-98)     -> odam_track_iou_step
 *   src/utils/box_utils.py:123-144         iou_2d                                                             -> odam_track_iou_step
 *   src/utils/box_utils.py:424-447         iou_3d                                                             -> odam_track_iou_step
 * match_tracks_feature (:173-242; ORB keypoints, depth maps) is not here.
 *
 * Conventions as in odam_eval.h: int return codes (0 = OK), odam_last_error(), [dev] / [host] pointers, the first argument is the
 * odam_sq_ctx of the device (odam_sq_create); stream-ordered on the caller's hipStream_t, no synchronisation, no allocation.
 * ONE launch per call (csrc/track_iou.hip), one wavefront per sequence; binary64 without contraction, IEEE division.  Plain vector
 * stores from the lanes that own a slot; no call writes a word that no slot, sequence or state block owns.
 *
 * The rule, per frame with detections (restated in numpy by tests/track_iou_ref.py, which the kernel equals bit for bit):
 *   1. detections are taken by descending score; equal scores by descending index (numpy's default argsort, which the reference
 *      calls, is not stable: the reference's order of equal scores is unspecified; this is det_select.hip's rule, i.e.
 *      np.argsort(kind="stable")[::-1]).  A NaN score sorts as the largest, as numpy sorts it;
 *   2. pixel box = float32 normalised box, widened, x (img_w, img_h), clipped to [0, img_w] x [0, img_h];
 *      t_wo[r] = ((x T[r][0] + y T[r][1]) + z T[r][2]) + T[r][3]; the detection's 3D box is (-dims) / 2 + t_wo .. dims / 2 + t_wo;
 *   3. the tracks are scanned in index order from max_iou_2d = max_iou_3d = -1, best = -1; a track matched earlier in this frame
 *      is skipped.  A track's 3D box comes from the mean of dims and t_wo over all its observations (running sums / count), its
 *      2D box is that of its last observation.  A track last seen within max_gap frame ids updates the state when
 *      iou_2d > max_iou_2d and iou_3d > max_iou_3d and the classes are equal (both maxima and best change); one seen longer ago
 *      when iou_3d > max_iou_3d and the classes are equal (max_iou_3d and best change, max_iou_2d does not).  Not an arg-max:
 *      the result depends on the track order;
 *   4. the detection joins `best` when max_iou_2d > match_threshold or max_iou_3d > iou3d_threshold (and best != -1, which the
 *      reference asserts and which always holds for thresholds >= -1); that track is then out of this frame's scans;
 *   5. after all matching, every unmatched detection whose score is not below track_threshold starts a track, in detection
 *      index order, with id = number of tracks.
 * The IoUs are box_utils.iou_2d(track, detection) and iou_3d(detection, track), operation for operation: Python's max / min (the
 * second argument wins only when strictly greater / less), max(0, .), products left to right, one division.  Where the reference
 * asserts on a NaN or out-of-range IoU, here a NaN compares false and never matches.
 *
 * State: caller-owned device memory, odam_track_iou_state_bytes(max_tracks) bytes per sequence, sequence s at
 * state + s * that.  odam_track_iou_reset starts a sequence; the state persists across calls, so a sequence fed in chunks of
 * frames continues where it stopped.  Per sequence: a header of 8 int32 (n_tracks, the overflow record of the last call,
 * max_tracks, 5 spare), then per track and structure-of-arrays over max_tracks: running sums of dims and t_wo (6 doubles), the 3D
 * box of their means (6 doubles; formed when the track changes, i.e. at most once per frame), the clipped pixel box of the last
 * observation (4 doubles), class (float32), observation count and last frame id (int32).
 *
 * odam_track_iou_state_bytes   max_tracks 1 .. 65536 (the kernel's matched-in-this-frame flags are 8 KiB of LDS bits), else -1
 * odam_track_iou_reset         n_seq state blocks of capacity max_tracks become empty sequences (one small launch)
 * odam_track_iou_step
 *   n_seq, seq_off   [dev] [n_seq+1] int32: sequence s owns the frames seq_off[s] .. seq_off[s+1]-1 (clamped to 0 .. n_frames)
 *   n_frames         rows of the frame arrays (host copy); n_seq == 0 returns ODAM_OK without a launch
 *   det_block        [dev] [n_frames][30][15] float32, parallel.pack_detections' layout (frame id, class, normalised box 4, dims 3,
 *                    camera-frame centre 3, sin, cos, score)      det_count [dev] [n_frames] int32: the first count rows, at most 30
 *   frame_ids        [dev] [n_frames] int32        T_wc [dev] [n_frames][4][4] float64, row-major
 *   img_w, img_h, match_threshold, track_threshold, iou3d_threshold, max_gap    the reference's defaults are 0.5, 0.8, 0.2 and 5
 *   out_ids          [dev] [n_frames][30] int32    track id of every detection slot; -1 = dropped (unmatched and below the track
 *                    threshold) or an unused slot
 *   out_iou2d/3d     [dev] [n_frames][30] float64  max_iou_2d / max_iou_3d when the detection's scan ended: -1 where it never
 *                    updated (and in unused slots)
 *   out_n_tracks     [dev] [n_seq] int32           tracks of the sequence after the call; -1 when the state block was not reset
 *                    for this max_tracks (header[1] = -2; nothing else is written)
 *   All 30 slots of every frame the call processed are written.  If a frame would take a sequence past max_tracks, the kernel
 *   stops BEFORE that frame: the state is as after the frame before it, header[1] holds the frame's index in the frame arrays
 *   (-1 otherwise), and the slots of that and of every later frame of the sequence are not touched -- pre-fill them.
 */
#ifndef ODAM_TRACK_H
#define ODAM_TRACK_H
#include "odam_sq.h"
#ifdef __cplusplus
extern "C" {
#endif

#define ODAM_TRACK_MAX_TRACKS 65536
#define ODAM_TRACK_DETS 30
#define ODAM_TRACK_HEADER_WORDS 8

long long odam_track_iou_state_bytes(int max_tracks);
int odam_track_iou_reset(odam_sq_ctx* ctx, void* state, int n_seq, int max_tracks, void* stream);
int odam_track_iou_step(odam_sq_ctx* ctx, int n_seq, const int* seq_off, int n_frames, const float* det_block, const int* det_count,
                        const int* frame_ids, const double* T_wc, double img_w, double img_h, double match_threshold,
                        double track_threshold, double iou3d_threshold, int max_gap, void* state, int max_tracks, int* out_ids,
                        double* out_iou2d, double* out_iou3d, int* out_n_tracks, void* stream);

#ifdef __cplusplus
}
#endif
#endif
