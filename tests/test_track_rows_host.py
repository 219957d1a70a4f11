"""The device-resident row store without a device: the entry points of include/odam_rows.h against what odam_amd.track_store gives
ctypes and their argument checks (which come before any device work), TrackRows.sync's decisions on a stub that records what would be
uploaded, and merge.tracks_from_packed against merge_scenes' own result on the merge golden.  CPU only."""
import ctypes
import os
import re

import numpy as np
import pytest

import track_rows_ref as R
from conftest import REPO

C_TO_CTYPES = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "odam_rows.h")).read(), flags=re.S)


def _header_args(txt, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, f"{name} is not declared in include/odam_rows.h"
    names, want = [], []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        names.append(arg.split()[-1].lstrip("*"))
        want.append(ctypes.c_void_p if "*" in arg else C_TO_CTYPES[arg.replace("const ", "").rsplit(" ", 1)[0]])
    return names, want


def test_prototypes_are_the_headers():
    from odam_amd import _lib, track_store as ts
    txt = _header()
    for name in ("odam_rows_group_workspace", "odam_rows_group", "odam_rows_gather14"):
        names, want = _header_args(txt, name)
        assert ts.ROWS_ARGTYPES[name] == want, name
        assert hasattr(_lib.lib(), name)
        f = ts._entry(name)
        assert list(f.argtypes) == want and f.restype is ctypes.c_int
    assert _header_args(txt, "odam_rows_group")[0] == ["tid", "N", "n_tracks", "row_off", "src_out", "status", "work", "work_bytes", "stream"]
    assert _header_args(txt, "odam_rows_gather14")[0] == ["log", "src", "N", "out", "stream"]
    for name, value in (("ODAM_ROWS_MAX_ROWS", ts.MAX_ROWS), ("ODAM_ROWS_MAX_TRACKS", ts.MAX_TRACKS), ("ODAM_ROWS_CHUNK", ts.CHUNK),
                        ("ODAM_ROWS_OK", R.OK), ("ODAM_ROWS_BAD_ID", R.BAD_ID), ("ODAM_ROWS_BAD_COUNT", R.BAD_COUNT)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, txt).group(1)) == value, name
    assert (ts.STATUS_OK, ts.STATUS_BAD_ID, ts.STATUS_BAD_COUNT) == (R.OK, R.BAD_ID, R.BAD_COUNT)
    assert ts.MAX_ROWS == 2 ** 24 and ts.MAX_TRACKS == 65536


def test_argument_checks_come_before_any_device_work():
    from odam_amd import _lib, track_store as ts
    L = _lib.lib()
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    size = ctypes.c_size_t(12345)
    ps = ctypes.cast(ctypes.byref(size), ctypes.c_void_p)
    fw = ts._entry("odam_rows_group_workspace")
    assert fw(10, 3, None) == 1 and b"odam_rows_group_workspace" in L.odam_last_error()      # ODAM_E_INVALID
    assert fw(-1, 3, ps) == 1 and fw(10, -1, ps) == 1
    assert fw(2 ** 24 + 1, 3, ps) == 3 and fw(10, 65537, ps) == 3                              # ODAM_E_LIMIT
    assert fw(0, 3, ps) == 0 and size.value == 0 and fw(10, 0, ps) == 0 and size.value == 0
    chunks = lambda n: -(-n // ts.CHUNK)
    for n, t in ((1, 1), (ts.CHUNK, 256), (ts.CHUNK + 1, 256), (ts.CHUNK + 1, 257), (2 ** 24, 65536)):
        assert fw(n, t, ps) == 0
        ints = 256 * chunks(n) + 256 + (n if t > ts.ONE_PASS_TRACKS else 0)      # histograms, digit totals, the order between two passes
        assert size.value == -(-4 * ints // 16) * 16, (n, t)
    assert ts.group_workspace(100, 7) == 4 * 512

    fg = ts._entry("odam_rows_group")
    ok = lambda **kw: [kw.get("tid", p), kw.get("N", 4), kw.get("n_tracks", 2), kw.get("row_off", p), kw.get("src", p), kw.get("status", p),
                       kw.get("work", p), kw.get("bytes", 4 * 512), None]
    for k in ("tid", "row_off", "src", "status", "work"):
        assert fg(*ok(**{k: None})) == 1 and b"odam_rows_group" in L.odam_last_error(), k
    assert fg(*ok(N=-1)) == 1 and fg(*ok(n_tracks=-1)) == 1
    assert fg(*ok(bytes=4 * 512 - 1)) == 1 and b"workspace" in L.odam_last_error()
    assert fg(*ok(N=2 ** 24 + 1)) == 3 and b"2^24" in L.odam_last_error()
    assert fg(*ok(n_tracks=65537)) == 3 and b"65536" in L.odam_last_error()
    assert fg(*ok(N=2 ** 24 + 1, tid=None)) == 3      # the limit is answered before anything else is looked at
    assert fg(*ok(N=0)) == 0 and fg(*ok(n_tracks=0)) == 0 and fg(*ok(N=0, tid=None, work=None)) == 0      # the empty call launches nothing

    fa = ts._entry("odam_rows_gather14")
    oka = lambda **kw: [kw.get("log", p), kw.get("src", p), kw.get("N", 4), kw.get("out", p), None]
    for k in ("log", "src", "out"):
        assert fa(*oka(**{k: None})) == 1 and b"odam_rows_gather14" in L.odam_last_error(), k
    assert fa(*oka(N=-1)) == 1 and fa(*oka(N=2 ** 24 + 1)) == 3 and fa(*oka(N=0)) == 0 and fa(*oka(N=0, log=None)) == 0
    assert fa(*oka(log=ctypes.c_void_p(p.value + 8))) == 1 and b"aligned" in L.odam_last_error()


def test_the_restatement_itself():
    tid = np.array([2, 0, 2, 1, 0, 2], np.int32)
    st, src = R.group(tid, 4, [0, 2, 3, 6, 6])
    assert st == R.OK and src.tolist() == [1, 4, 3, 0, 2, 5]
    assert R.group(tid, 2, [0, 2, 3])[0] == R.BAD_ID and R.group([0, -1], 2, [0, 1, 2])[0] == R.BAD_ID
    assert R.group(tid, 4, [0, 2, 4, 6, 6])[0] == R.BAD_COUNT and R.group(tid, 4, [1, 3, 4, 7, 7])[0] == R.BAD_COUNT
    rows = R.bit_rows(50)
    w = rows.view(np.uint64)
    assert len(np.unique(w[:, 0])) == 50 and np.isnan(rows).any() and (w == 0x8000000000000000).any()
    assert ((w & 0x7FF0000000000000 == 0) & (w & 0x000FFFFFFFFFFFFF != 0)).any()      # denormals
    nan = w[np.isnan(rows)]
    assert len(np.unique(nan)) > 5                                                         # payloads
    tid, frame, n = R.scan_log()
    assert n == 700 and len(tid) == 70000 and (np.diff(frame) >= 0).all()
    assert max(np.bincount(tid[frame == f]).max() for f in (0, 100, 699)) == 1             # at most one row per track per frame
    assert (np.diff(np.unique(tid, return_index=True)[1]) > 0).all()                       # numbered in order of first appearance


# ---- TrackRows.sync: what goes up, decided on the host ------------------------------------------------------------------------------------

class _Fitter:
    device = "cpu"


def _stub():
    from odam_amd.track_store import TrackRows

    class Stub(TrackRows):
        """records what would be uploaded instead of touching a device"""

        def __init__(self):
            self.uploads = []
            super().__init__(_Fitter())

        def _reserve(self, n_rows):
            while self.capacity < n_rows:
                self.capacity *= 2

        def _upload(self, pieces, ids, at):
            self.uploads.append((at, [int(i) for i in ids], np.concatenate([np.asarray(p)[:, :14] for p in pieces])))
    return Stub()


def _tracks(lens, seed=0, width=82):
    rs = np.random.RandomState(seed)
    out = []
    for n in lens:
        t = rs.uniform(size=(n, width))
        t[:, 0] = np.sort(rs.choice(1000, n, replace=False))
        out.append(t)
    return out


def test_sync_uploads_appended_rows_only():
    full = _tracks([30, 12, 25, 40])
    s = _stub()
    assert s.sync([t[:10] for t in full[:3]]) == 30 and s.loads == 1 and s.rows_uploaded == 30
    at, ids, rows = s.uploads[-1]
    assert at == 0 and ids == [0, 1, 2] and np.array_equal(rows, np.concatenate([t[:10, :14] for t in full[:3]]))
    assert s._grouped and s.lengths == [10, 10, 10]
    # rows appended to two tracks, the third as it was
    nxt = [full[0][:17], full[1][:10], full[2][:11]]
    assert s.sync(nxt) == 8 and s.loads == 1 and s.rows_uploaded == 38 and not s._grouped
    at, ids, rows = s.uploads[-1]
    assert at == 30 and ids == [0, 2] and np.array_equal(rows, np.concatenate([full[0][10:17, :14], full[2][10:11, :14]]))
    assert s.lengths == [17, 10, 11] and s.n_rows == 38
    # a new track and more rows
    nxt = [full[0][:17], full[1][:12], full[2][:11], full[3][:5]]
    assert s.sync(nxt) == 7 and s.loads == 1
    at, ids, rows = s.uploads[-1]
    assert at == 38 and ids == [1, 3] and np.array_equal(rows, np.concatenate([full[1][10:12, :14], full[3][:5, :14]]))
    # nothing new: nothing goes up
    n_up = len(s.uploads)
    assert s.sync([t.copy() for t in nxt]) == 0 and len(s.uploads) == n_up and s.loads == 1 and s.lengths == [17, 12, 11, 5]
    assert np.array_equal(s.marks, np.array([[t[0, 0], t[-1, 0], t[-1, 9]] for t in nxt]))


@pytest.mark.parametrize("case", ["shortened", "first row replaced", "last stored row replaced", "fewer tracks", "empty list", "not float64",
                                  "an empty track"])
def test_sync_falls_back_to_a_load(case):
    full = _tracks([30, 12, 25])
    s = _stub()
    assert s.sync(full) == 67 and s.loads == 1
    nxt = [t.copy() for t in full]
    want = 67
    if case == "shortened":
        nxt[1] = nxt[1][:11]
        want = 66
    elif case == "first row replaced":
        nxt[2][0, 0] += 1
    elif case == "last stored row replaced":
        nxt[0] = np.concatenate([nxt[0], nxt[0][-1:]])
        nxt[0][29, 9] += 0.5
        want = 68
    elif case == "fewer tracks":
        nxt = nxt[:2]
        want = 42
    elif case == "empty list":
        nxt, want = [], 0
    elif case == "not float64":
        nxt[1] = nxt[1].astype(np.float32)
        want = None
    elif case == "an empty track":
        nxt[1] = nxt[1][:0]
        want = None
    assert s.sync(nxt) == want
    if want is None:      # refused: the caller falls back, the store is empty
        assert s.loads == 1 and s.n_rows == 0 and s.lengths == []
        assert s.sync(full) == 67 and s.loads == 2
        return
    assert s.loads == 2 and s.rows_uploaded == 67 + want and s._grouped and s.n_rows == want and s.lengths == [len(t) for t in nxt]
    if want:
        at, ids, rows = s.uploads[-1]
        assert at == 0 and ids == list(range(len(nxt))) and np.array_equal(rows, np.concatenate([t[:, :14] for t in nxt]))
    s.reset()
    assert s.n_rows == 0 and s.lengths == [] and s.loads == 2


def test_growth_doubles_the_capacity():
    from odam_amd.track_store import TrackRows
    s = _stub()
    assert s.capacity == 65536 and TrackRows(_Fitter(), capacity_rows=64).capacity == 64
    s.capacity = 64
    full = _tracks([100, 100])
    s.sync([t[:20] for t in full])
    assert s.capacity == 64
    s.sync([t[:40] for t in full])
    assert s.capacity == 128
    s.sync(full)
    assert s.capacity == 256


# ---- merge.tracks_from_packed ----------------------------------------------------------------------------------------------------------------

def test_tracks_from_packed_equals_merge_scenes_on_the_golden(golden):
    """the block is made here from the host merge's own decisions (tests/merge_ref.py, which test_track_merge_host.py holds against
    merge._merge_cluster): offsets, source rows and classes as odam_merge_assemble hands them out, as CPU tensors"""
    import torch
    import merge_ref
    from odam_amd import merge
    z = golden("sq_merge.npz")
    tracks = [z[f"track{i}"].copy() for i in range(int(z["n_tracks"]))]
    img_names = [int(x) for x in z["img_names"]]
    data = {"tracks": tracks, "bboxes_qc": list(z["bboxes_qc"])}
    want = merge.merge_process(data, img_names)
    cost = merge.cost_matrix(tracks, data["bboxes_qc"])
    labels, n_cl = merge_ref.labels_from_linkage(merge_ref.linkage_average(cost), len(tracks), 0.95)
    st, out = merge_ref.assemble_scene(tracks, labels, n_cl, img_names)
    assert st == 0
    off = np.concatenate([[0], np.cumsum([len(s) for _, s in out])])
    block = {"row_offsets": torch.from_numpy(off.astype(np.int32)), "src": torch.from_numpy(np.concatenate([s for _, s in out]).astype(np.int32)),
             "cls": torch.from_numpy(np.array([c for c, _ in out], np.int32))}
    before = [t.copy() for t in tracks]
    got = merge.tracks_from_packed(block, data)
    assert len(got) == len(want) == int(z["n_merged"])
    for a, b, c in zip(got, want, [z[f"merged{i}"] for i in range(int(z["n_merged"]))]):
        assert a.shape == b.shape and np.array_equal(a, b) and np.array_equal(a, c)
    assert all(np.array_equal(a, b) for a, b in zip(tracks, before))      # the caller's tracks stay as they were
