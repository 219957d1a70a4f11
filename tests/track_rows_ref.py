"""numpy restatement of include/odam_rows.h: the stable order of a row log by track and the row gather, with the two status rules.
tests/test_track_rows_gpu.py asks the device for exactly this."""
import numpy as np

OK, BAD_ID, BAD_COUNT = 0, 1, 2
FILL_I = -7


def group(tid, n_tracks, row_off):
    """-> (status, src): src = np.argsort(tid, kind="stable") where the status is 0, None otherwise (unspecified)"""
    tid = np.asarray(tid, np.int64)
    row_off = np.asarray(row_off, np.int64)
    if ((tid < 0) | (tid >= n_tracks)).any():
        return BAD_ID, None
    if row_off[0] != 0 or not np.array_equal(np.bincount(tid, minlength=n_tracks), np.diff(row_off)):
        return BAD_COUNT, None
    return OK, np.argsort(tid, kind="stable").astype(np.int32)


def gather14(log, src):
    return np.ascontiguousarray(log)[np.asarray(src, np.int64)]


def offsets(tid, n_tracks):
    off = np.zeros(n_tracks + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(np.asarray(tid, np.int64), minlength=n_tracks))
    return off


def bit_rows(n, seed=0):
    """[n, 14] float64 rows whose 64-bit words are all different and include NaNs with payloads, -0.0, denormals and infinities"""
    rs = np.random.RandomState(seed)
    w = rs.randint(0, 2 ** 63 - 1, size=(n, 14), dtype=np.int64).astype(np.uint64)
    w = (w & ~np.uint64(0xFFFFFF)) | (np.arange(n * 14, dtype=np.uint64).reshape(n, 14) & np.uint64(0xFFFFFF))      # (distinct up to 2^24 words)
    if n:
        k = np.arange(n)
        w[k % 5 == 0, 3] = np.uint64(0x7FF0000000000000) | (w[k % 5 == 0, 3] & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(1)      # NaN, payload kept
        w[k % 5 == 1, 4] = np.uint64(0xFFF8000000000000) | (w[k % 5 == 1, 4] & np.uint64(0x0007FFFFFFFFFFFF))                      # negative quiet NaN
        w[k % 5 == 2, 5] = np.uint64(0x8000000000000000)                                                                           # -0.0
        w[k % 5 == 3, 6] = w[k % 5 == 3, 6] & np.uint64(0x800FFFFFFFFFFFFF) | np.uint64(1)                                          # denormal
        w[k % 7 == 0, 7] = np.uint64(0xFFF0000000000000)                                                                           # -inf
    return w.view(np.float64)


def scan_log(n_tracks=700, n_rows=70000, seed=3):
    """an interleaved "scan": rows in frame order, at most one row per track per frame -> (tid [n_rows] int32, frame [n_rows])"""
    rs = np.random.RandomState(seed)
    per_frame = 100
    tid, frame = [], []
    f = 0
    while len(tid) < n_rows:
        live = min(n_tracks, 50 + f * n_tracks // (n_rows // per_frame))      # tracks are born as the scan goes on
        seen = np.sort(rs.choice(live, min(per_frame, live, n_rows - len(tid)), replace=False))
        tid.extend(seen.tolist())
        frame.extend([f] * len(seen))
        f += 1
    tid = np.asarray(tid, np.int32)
    # every track of the list has at least one row: number the tracks in order of first appearance, as association does
    first = {}
    for t in tid.tolist():
        first.setdefault(t, len(first))
    return np.asarray([first[t] for t in tid.tolist()], np.int32), np.asarray(frame, np.float64), len(first)
