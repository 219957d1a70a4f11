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

#ifdef __cplusplus
}
#endif
#endif
