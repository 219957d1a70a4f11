"""The fit prelude, host side: the numpy restatement of odam_sq_prepare_batch (tests/sq_prepare_ref.py, closed-form yaw) against the
host path multi_view.optim_process runs per track -- _object_constraints + averaging_T_wos_batch (scipy Rotation.mean's operations) +
as_euler + init_params / init_dual + get_3d_box -- over 420 synthetic tracks, and the C declaration against what odam_amd.sq gives
ctypes.  tests/test_sq_prepare_gpu.py asks the device for what the restatement gives.

Bit for bit: class, views, view_row, counts, tgt, mask, P, the translate and scale entries of the init rows, half_dims.  The yaw and
bboxes_dl are two float64 evaluations of one quantity: their largest gap over these tracks is measured, printed, and held against
sq_prepare_ref.YAW_GAP / BOX_GAP, the figures DESIGN 6l quotes and the GPU test takes its tolerance from."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import sq_prepare_ref as R
from conftest import REPO

N_TRACKS = 420


@pytest.fixture(scope="module")
def scene():
    return R.random_tracks(5, N_TRACKS)


@pytest.fixture(scope="module")
def host(scene):
    """the host path of optim_process (multi_view.py, the prelude loop), per track, for both families of init rows"""
    from odam_amd import multi_view as mv, sq
    tracks, img_names, P_cws, img_h, img_w = scene
    assert mv._UniqueFrames.applies(img_names)
    fi = mv._frame_index(img_names)
    cons = [mv._object_constraints(np.asarray(t), fi, img_h, img_w, with_rows=True) for t in tracks]
    assert all(len(c[4]) for c in cons)
    T_wos = mv.averaging_T_wos_batch([c[4] for c in cons], [c[5] for c in cons])
    yaws = Rotation.from_matrix(T_wos[:, :3, :3]).as_euler("zxy")[:, 0]
    out = []
    for o, (cls, img_ids, tgt, mask, _, _, dims, rows) in enumerate(cons):
        scales = np.mean(np.asarray(dims), axis=0)
        T = T_wos[o]
        out.append(dict(cls=cls, img=img_ids, rows=rows, tgt=tgt, mask=mask, P=P_cws[img_ids].astype(np.float32).reshape(-1, 12),
                        valid=mask.any(axis=1), yaw=yaws[o], box=mv.get_3d_box(scales, T[:3, :3], T[:3, 3]),
                        init={rep: sq.init_params(T[:3, 3], yaws[o], scales, rep) for rep in ("super_quadric", "cube", "quadric")},
                        dual=sq.init_dual(T[:3, 3], yaws[o], scales)))
    return out


@pytest.fixture(scope="module")
def restated(scene):
    tracks, img_names, P_cws, img_h, img_w = scene
    rows, offs = R.pack(tracks)
    return {rep: R.prepare_ref(rows, offs, img_names, P_cws, img_h, img_w, rep) for rep in ("super_quadric", "cube", "quadric", "dual_quadric")}, offs


def test_inputs_cover_the_branches(scene):
    from odam_amd import multi_view as mv
    tracks, img_names, P_cws, img_h, img_w = scene
    assert len(tracks) >= 400 and sorted(img_names) != list(img_names)
    ids = set(img_names)
    dup = absent = unordered = frac = 0
    order = {f: i for i, f in enumerate(img_names)}
    for t in tracks:
        f = t[:, 0].astype(np.int32)
        dup += len(np.unique(f)) < len(f)
        absent += any(int(x) not in ids for x in f)
        frac += bool((t[:, 0] != f).any())
        seen = [order[int(x)] for x in f if int(x) in ids]
        unordered += seen != sorted(seen)
        a = t[np.unique(f, return_index=True)[1]]
        a = a[[int(x) in ids for x in a[:, 0].astype(np.int32)], 12]
        assert np.hypot(np.sin(a).sum(), np.cos(a).sum()) / len(a) >= 0.1      # the mean rotation is defined
    assert min(dup, absent, unordered, frac) >= 40, (dup, absent, unordered, frac)
    lens = [len(t) for t in tracks]
    assert min(lens) == 1 and max(lens) > 256


def test_discrete_and_exact_outputs_equal_the_host_path(scene, host, restated):
    ref, offs = restated
    r = ref["super_quadric"]
    assert not r["status"].any()
    n_masked_out = n_band = 0
    tracks = scene[0]
    for o, h in enumerate(host):
        k, g = len(h["img"]), slice(int(offs[o]), int(offs[o]) + len(h["img"]))
        assert r["cls"][o] == h["cls"] and r["n_obs"][o] == k and r["n_valid"][o] == int(h["valid"].sum())
        assert np.array_equal(r["view_img"][g], h["img"]) and np.array_equal(r["view_row"][g], h["rows"])
        assert np.array_equal(r["valid"][g], h["valid"].astype(np.int32))
        for key in ("tgt", "mask", "P"):
            assert r[key][g].dtype == np.float32 and np.array_equal(r[key][g].view(np.uint32), h[key].view(np.uint32)), (o, key)
        # nothing is written beyond the views
        rest = slice(int(offs[o]) + k, int(offs[o + 1]))
        assert (r["view_img"][rest] == R.FILL_I).all() and np.isnan(r["P"][rest]).all()
        n_masked_out += int((~h["valid"]).sum())
        v = tracks[o][h["rows"]][:, 2:6]
        n_band += int(((v == 20) | (v[:, 2:3] == 620) | (v[:, 3:4] == 460)).sum())
    assert n_masked_out > 20 and n_band > 100      # views without any constrained edge, edges exactly on the band


def test_init_rows_translate_scales_bitwise_yaw_one_ulp(host, restated):
    ref, _ = restated
    worst = 0
    for rep in ("super_quadric", "cube", "quadric"):
        for o, h in enumerate(host):
            a, b = ref[rep]["init"][o], h["init"][rep]
            keep = [0, 1, 2, 4, 5, 6, 7, 8]
            assert np.array_equal(a[keep].view(np.uint32), b[keep].view(np.uint32)), (rep, o, a, b)
            worst = max(worst, int(R.ulps32(a[3], b[3])))
        shapes = ref[rep]["init"][:, 7:9]
        assert (shapes.view(np.uint32) == np.float32(-10000.0 if rep == "cube" else -0.0).view(np.uint32)).all()
    for o, h in enumerate(host):
        a5, ah = ref["dual_quadric"]["init"][o], ref["dual_quadric"]["half_dims"][o]
        assert np.array_equal(a5[[0, 1, 2, 4]].view(np.uint32), h["dual"][0][[0, 1, 2, 4]].view(np.uint32))
        assert np.array_equal(ah.view(np.uint32), h["dual"][1].view(np.uint32))
        worst = max(worst, int(R.ulps32(a5[3], h["dual"][0][3])))
    print("float32 yaw entry: largest distance to the host path %d ulp" % worst)
    assert worst <= 1


def test_yaw_and_box_gap_to_the_scipy_path(host, restated):
    ref, _ = restated
    r = ref["super_quadric"]
    d = r["pose"][:, 3] - np.array([h["yaw"] for h in host])
    d = np.abs((d + np.pi) % (2 * np.pi) - np.pi)
    yaw_gap = float(d.max())
    box_gap = float(max(np.abs(r["bboxes_dl"][o] - h["box"]).max() for o, h in enumerate(host)))
    print("closed-form yaw against scipy's mean rotation over %d tracks: largest gap %.3e rad; bboxes_dl %.3e" % (len(host), yaw_gap, box_gap))
    assert yaw_gap <= R.YAW_GAP and box_gap <= R.BOX_GAP


def test_status_codes_of_the_restatement():
    tracks, img_names, P_cws, img_h, img_w = R.random_tracks(2, 6, n_img=20, max_rows=12)
    tracks[1][:, 0] = 5.0                      # no frame id of the sequence
    tracks[2][0, 1] = 3.5                      # not an integer
    tracks[3][-1, 1] = 64                      # outside 0..63
    tracks[4][:, 0] = 5.0
    tracks[4][0, 1] = np.nan                   # no view goes before the class
    rows, offs = R.pack(tracks)
    r = R.prepare_ref(rows, offs, img_names, P_cws, img_h, img_w, cap=8)
    want = [0, R.NO_VIEW, R.BAD_CLASS, R.BAD_CLASS, R.NO_VIEW, 0]
    want = [R.TOO_MANY_ROWS if len(t) > 8 else w for t, w in zip(tracks, want)]
    assert r["status"].tolist() == want
    r = R.prepare_ref(rows, offs, img_names, P_cws, img_h, img_w)
    assert r["status"].tolist() == [0, R.NO_VIEW, R.BAD_CLASS, R.BAD_CLASS, R.NO_VIEW, 0]
    assert r["cls"].tolist()[1:5] == [int(np.median(tracks[1][:, 1])), -1, -1, -1]
    assert r["n_obs"][2] > 0 and not np.isnan(r["init"][2]).any() and np.isnan(r["init"][1]).all()
    # the even-count median of two classes truncates
    t = tracks[0][:2].copy()
    t[:, 1] = [5, 4]
    r = R.prepare_ref(t, [0, 2], img_names, P_cws, img_h, img_w)
    assert r["cls"].tolist() == [4]


C_TO_CTYPES = {"int": ctypes.c_int, "double": ctypes.c_double}


def test_prepare_ctypes_signature_matches_the_header():
    """the argument list odam_amd.sq gives ctypes for odam_sq_prepare_batch is the header's, argument by argument; the symbol is
    exported; argument checks come before any device work"""
    from odam_amd import _lib, sq
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "odam_sq.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+odam_sq_prepare_batch\s*\(([^)]*)\)\s*;", txt)
    assert m, "odam_sq_prepare_batch is not declared in include/odam_sq.h"
    names, want = [], []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        names.append(arg.split()[-1].lstrip("*"))
        want.append(ctypes.c_void_p if "*" in arg else C_TO_CTYPES[arg.replace("const ", "").rsplit(" ", 1)[0]])
    assert names == ["ctx", "n_obj", "row_off", "rows", "max_rows", "n_img", "img_ids", "img_order", "P_cws", "img_w", "img_h", "thr",
                     "representation", "cls", "n_obs", "n_valid", "init", "half_dims", "pose", "bboxes_dl", "status", "view_img", "view_row",
                     "tgt", "mask", "P", "valid", "stream"]
    assert sq.PREPARE_ARGTYPES == want
    for name, value in (("ODAM_SQ_PREPARE_MAX_ROWS", sq.PREPARE_MAX_ROWS), ("ODAM_SQ_PREPARE_NO_VIEW", sq.PREPARE_NO_VIEW),
                        ("ODAM_SQ_PREPARE_BAD_CLASS", sq.PREPARE_BAD_CLASS), ("ODAM_SQ_PREPARE_TOO_MANY_ROWS", sq.PREPARE_TOO_MANY_ROWS),
                        ("ODAM_SQ_DUAL_QUADRIC", sq.REPRESENTATIONS["dual_quadric"])):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, txt).group(1)) == value, name
    assert (R.MAX_ROWS, R.NO_VIEW, R.BAD_CLASS, R.TOO_MANY_ROWS) == (sq.PREPARE_MAX_ROWS, sq.PREPARE_NO_VIEW, sq.PREPARE_BAD_CLASS, sq.PREPARE_TOO_MANY_ROWS)
    assert hasattr(_lib.lib(), "odam_sq_prepare_batch")
    f = sq._prepare_entry()
    assert list(f.argtypes) == want and f.restype is ctypes.c_int
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = lambda **kw: [kw.get("ctx", p), kw.get("n", 1), p, p, kw.get("max_rows", 4), 3, p, p, p, 640.0, 480.0, 20.0, kw.get("rep", 0)] + \
        [p] * 4 + [kw.get("half", p)] + [p] * 9 + [None]
    assert f(*ok(ctx=None)) == 1 and b"odam_sq_prepare_batch" in _lib.lib().odam_last_error()      # ODAM_E_INVALID
    assert f(*ok(n=-1)) == 1 and f(*ok(max_rows=0)) == 1 and f(*ok(rep=4)) == 1 and f(*ok(rep=3, half=None)) == 1
    assert f(*ok(rep=2, half=None, n=0)) == 0 and f(*ok(n=0)) == 0      # the empty call launches nothing
