/*
 * odam_rows.h -- C ABI of the device-resident track-row store: grouping a row log by track, and the row gather.
 *
 * A store keeps the first 14 columns of every track row in ARRIVAL order: a log rows[N][14] float64 and tid[N] int32, the track of
 * each row.  odam_sq_prepare_batch (odam_sq.h), odam_merge_assemble (odam_merge.h) and the fits take rows track after track.  The two
 * calls below make that order on the device; together they replace, of the host code,
 *   odam_amd/multi_view.py::_device_prelude   np.concatenate([a[:, :14] for a in arrs]) and its upload        -> group + gather14
 *   odam_amd/merge.py::_device_merge          np.concatenate([t for k in picked for t in scenes[k][1]]), same  -> group + gather14
 * for a caller that appended only the NEW rows to the log (odam_amd/track_store.py::TrackRows).  Both kernels are restated in numpy by
 * tests/track_rows_ref.py.
 *
 * Conventions as in odam_sq.h: int return codes (0 = OK), odam_last_error(), [dev] pointers; stream-ordered on the caller's
 * hipStream_t, no host synchronisation, no allocation: every word of working memory is the caller's `work`.  There is no context
 * argument: nothing is kept between calls.  Argument checks come before any device work; what only the device can see (the ids, the
 * offsets) is answered by the status word, never by a fault.  Plain launches that each run to completion (csrc/track_rows.hip).
 *
 * odam_rows_group_workspace -- bytes of `work` the group call needs for N rows of n_tracks tracks (0 for an empty call).
 *
 * odam_rows_group -- the stable order of the log by track: np.argsort(tid, kind="stable").
 *   tid        [dev] [N] int32: the track of every log row
 *   N          rows in the log, <= ODAM_ROWS_MAX_ROWS          n_tracks   <= ODAM_ROWS_MAX_TRACKS; beyond either: ODAM_E_LIMIT,
 *              before anything is enqueued.  N == 0 or n_tracks == 0: returns 0 with no launch (status is not written)
 *   row_off    [dev] [n_tracks+1] int32: the offsets the HOST expects -- the store counts rows per track as it appends, so nothing is
 *              read back to size anything.  Read by the check only; never used as an index
 *   src_out    [dev] [N] int32: src_out[row_off[t] + k] = log index of the k-th row of track t in arrival order
 *   status     [dev] [1] int32: ODAM_ROWS_OK, ODAM_ROWS_BAD_ID (a tid outside [0, n_tracks)) or ODAM_ROWS_BAD_COUNT (no bad id, but
 *              row_off[0] != 0 or a track whose row count is not row_off[t+1] - row_off[t]).  Where it is non-zero src_out is
 *              unspecified; every store stays inside src_out[0 .. N-1] and work[0 .. work_bytes-1] all the same: an id is checked
 *              before it is used as an index (a bad one sorts as track 0), and positions come from counts of the log alone
 *   work       [dev] work_bytes >= odam_rows_group_workspace's answer, 16-byte aligned
 * Shape: an LSD radix sort on the id with 8-bit digits -- ONE pass for n_tracks <= 256, TWO beyond -- each pass a stable counting
 * sort over chunks of ODAM_ROWS_CHUNK rows: digit histogram per chunk, scan per digit over the chunks, stable scatter (the four
 * waves of a chunk own consecutive quarters; the rank inside a wave comes from a ballot match); a log of one chunk is one launch
 * per pass.  Integer LDS atomics make the COUNTS only, so the result is the same on every run.
 *
 * odam_rows_gather14 -- out[i] = log[src[i]] for i < N on whole 112-byte rows, as seven 16-byte words: every bit is preserved (NaN
 * payloads, -0.0).  log and out hold N rows each, 16-byte aligned, and do not overlap; an index outside [0, N) leaves its row of
 * `out` unwritten.  N <= ODAM_ROWS_MAX_ROWS (ODAM_E_LIMIT); N == 0 returns 0 with no launch.
 *
 * Feeding the log from the IoU tracker (csrc/track_emit.hip, restated in numpy by tests/track_emit_ref.py).  These two
 * replace, of the host code, odam_amd/processor.py::_track_frames_iou's copy back of the detection block and the ids, its
 * _track_rows per frame and its grouping of one-row slices, and the upload TrackRows.load then makes of the result.
 *
 * odam_rows_emit_workspace -- bytes of `work` the emit call needs for N frames (0 for N == 0).
 *
 * odam_rows_emit_tracked -- appends the track rows of N frames' detections to the log at position base.
 *   det_block  [dev] [N][30][15] float32, det_count [dev] [N] int32: odam_track.h's detection block and counts
 *   ids        [dev] [N][30] int32: the tracker's out_ids          T_wc [dev] [N][4][4] float64, row-major
 *   cam_azi    [dev] [N] float64: the camera's azimuth per frame (processor.get_cam_azi of the pose, made on the host)
 *   N          frames; N * 30 <= ODAM_ROWS_MAX_ROWS and n_tracks <= ODAM_ROWS_MAX_TRACKS, beyond either: ODAM_E_LIMIT before
 *              anything else is looked at.  N == 0 returns 0 with no launch (nothing is written)
 *   rows, tid  [dev] the log, rows[cap][14] float64 (16-byte aligned) and tid[cap] int32; 0 <= base <= cap
 *   Slot (k, d) is EMITTED iff d < min(max(det_count[k], 0), 30) and 0 <= ids[k][d] < n_tracks.  Its row goes to position
 *   base + rank, rank = the emitted slots in front of it in (k, d) lexicographic order, and tid there becomes its id.  The row, with
 *   r the slot's 15 float32 and T = T_wc[k], all binary64 without contraction:
 *     columns 0, 1, 6-8   r[0], r[1], r[6..8] widened
 *     columns 2-5         widened r[2..5] times (img_w, img_h, img_w, img_h), one multiplication each, NOT clipped
 *     columns 9-11        ((x T[q][0] + y T[q][1]) + z T[q][2]) + T[q][3] for q = 0, 1, 2 with (x, y, z) = widened r[9..11]
 *     column 12           atan2(widened r[12], widened r[13]) + cam_azi[k]           column 13   r[14] widened
 *   n_emitted  [dev] [1] int32: the emitted slots (where status has ODAM_ROWS_EMIT_OVERFLOW: the slots that would have been)
 *   counts, first_pos, last_pos   [dev] [n_tracks] int32 each: per track the rows this call wrote and the smallest and largest log
 *              position among them (-1 where it wrote none)
 *   status     [dev] [1] int32, a sum of ODAM_ROWS_EMIT_BAD_ID -- a live slot (d inside the clamped count) whose id is >= n_tracks:
 *              the slot is not emitted and nothing is stored for it -- and ODAM_ROWS_EMIT_OVERFLOW -- base + n_emitted > cap: NO
 *              row, id, count or position is stored (counts are 0, positions -1); decided from the counts before the first store
 *   work       [dev] work_bytes >= odam_rows_emit_workspace's answer, 16-byte aligned
 * Shape: chunks of ODAM_ROWS_CHUNK slots; a count per chunk, ONE workgroup scanning the chunk counts, a scatter that makes the
 * flags again and ranks by ballot.  Vector stores only; integer atomics make the per-track counts and position minima / maxima
 * only: every output has the same bits on every run.
 *
 * odam_rows_marks -- one small block for the host: out [n_tracks + 1][4] float64.  Row t < n_tracks: counts[t], the frame id
 * (column 0) of the log row at first_pos[t], the frame id and the world x (column 9) of the log row at last_pos[t]; -1 for a position
 * outside [0, n_log).  Row n_tracks: n_emitted, status, 0, 0.  With the emit call's outputs that is per track the rows added and the
 * (first, last, last x) marks of them; a track's first row in the WHOLE log is this call's only where the track had none before, which
 * the host knows.  n_tracks <= ODAM_ROWS_MAX_TRACKS (ODAM_E_LIMIT); one launch.
 */
#ifndef ODAM_ROWS_H
#define ODAM_ROWS_H
#include <stddef.h>
#include "odam_sq.h"
#ifdef __cplusplus
extern "C" {
#endif

#define ODAM_ROWS_MAX_ROWS 16777216      /* 2^24 */
#define ODAM_ROWS_MAX_TRACKS 65536
#define ODAM_ROWS_CHUNK 4096             /* rows one workgroup sorts: 4 waves x 16 steps x 64 lanes */
/* status word of odam_rows_group */
#define ODAM_ROWS_OK 0
#define ODAM_ROWS_BAD_ID 1
#define ODAM_ROWS_BAD_COUNT 2

int odam_rows_group_workspace(int N, int n_tracks, size_t* bytes);
int odam_rows_group(const int* tid, int N, int n_tracks, const int* row_off, int* src_out, int* status, void* work, size_t work_bytes,
                    void* stream);
int odam_rows_gather14(const double* log, const int* src, int N, double* out, void* stream);

#define ODAM_ROWS_EMIT_DETS 30           /* detection slots of a frame (ODAM_TRACK_DETS) */
/* status word of odam_rows_emit_tracked: a sum of */
#define ODAM_ROWS_EMIT_BAD_ID 1
#define ODAM_ROWS_EMIT_OVERFLOW 2

int odam_rows_emit_workspace(int N, size_t* bytes);
int odam_rows_emit_tracked(const float* det_block, const int* det_count, const int* ids, const double* T_wc, const double* cam_azi,
                           int N, double img_w, double img_h, int n_tracks, double* rows, int* tid, int base, int cap, int* n_emitted,
                           int* counts, int* first_pos, int* last_pos, int* status, void* work, size_t work_bytes, void* stream);
int odam_rows_marks(const double* rows, int n_log, const int* counts, const int* first_pos, const int* last_pos, const int* n_emitted,
                    const int* status, int n_tracks, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
