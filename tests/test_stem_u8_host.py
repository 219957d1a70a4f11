"""The host side of the uint8 stem, without a GPU: the folded filters and the centres (odam_amd/csrc/stem_u8_fold.h) and the producer's
pixel / frame layout, compiled by the host compiler (tests/native/stem_u8_check.cpp), against numpy float64 (tests/stem_u8_ref.py); and
odam_cg::choose with the new field -- the stem's argument block gets the new mode, and nothing else changes."""
import os
import subprocess

import numpy as np
import pytest

import cg_choice_rows as T
import stem_u8_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN = np.asarray((0.485, 0.456, 0.406), np.float32)
STD = np.asarray((0.229, 0.224, 0.225), np.float32)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("stem_u8") / "stem_u8_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", os.path.join(REPO, "tests", "native", "stem_u8_check.cpp"), "-o", out])
    return out


def _fold(exe, tmp, w, mean, std):
    path = os.path.join(tmp, "fold.bin")
    np.concatenate([mean, std, w.reshape(-1)]).astype(np.float32).tofile(path)
    lines = subprocess.run([exe, "fold", path], capture_output=True, text=True, check=True).stdout.split("\n")
    c = [int(v) for v in lines[0].split()]
    rows = np.array([float.fromhex(v) for v in lines[1:1 + 64 * 224]]).reshape(64, 7, 8, 4)
    return c, rows


def test_centres_are_lrint_of_255_mean(exe, tmp_path):
    """the model's mean, a mean whose 255-fold is a tie in binary (0.5 / 255 rounds to even), the ends"""
    w = np.zeros((64, 3, 7, 7), np.float32)
    assert _fold(exe, str(tmp_path), w, MEAN, STD)[0] == [124, 116, 104]
    for mean in ([0.0, 1.0, 0.5], [0.498, 0.502, 0.0019], [2.5 / 255, 3.5 / 255, 0.999]):
        m = np.asarray(mean, np.float32)
        want = [int(v) for v in np.rint(255.0 * m.astype(np.float64))]
        assert _fold(exe, str(tmp_path), w, m, STD)[0] == want == R.centres(m).tolist()


def test_fold_equals_float64_rounded_once(exe, tmp_path):
    rng = np.random.default_rng(1)
    w = (rng.standard_normal((64, 3, 7, 7)) * 0.05).astype(np.float32)
    w[0] = 0.0; w[1, :, 3, 3] = [1.0, -1.0, 2.0 ** -20]
    c, rows = _fold(exe, str(tmp_path), w, MEAN, STD)
    want = R.fold(w, MEAN, STD)
    assert np.array_equal(rows, want.astype(np.float32).astype(np.float64))      # bit for bit: one rounding of the same double
    assert not rows[:, :, 7, :].any() and not rows[0].any()
    # ... and it IS the normalisation: sum_k w'_k (u_k - c_k) + w'_3 = sum_k w_k (u_k / 255 - mean_k) / std_k for every byte value
    u = np.arange(256, dtype=np.float64)[:, None]
    m64, s64 = MEAN.astype(np.float64), STD.astype(np.float64)
    for o, ky, kx in ((1, 3, 3), (5, 0, 6), (63, 6, 0)):
        lhs = ((u - np.asarray(c)) * want[o, ky, kx, :3]).sum(1) + want[o, ky, kx, 3]
        rhs = ((u / 255.0 - m64) / s64 * w[o, :, ky, kx].astype(np.float64)).sum(1)
        assert np.abs(lhs - rhs).max() <= 1e-14 * max(1.0, np.abs(rhs).max())


def test_frame_layout_of_an_odd_sized_image(exe, tmp_path):
    """indicator 1 inside, four zeros in the frame (3 rows above / below, 3 + 5 columns), the differences exact in bf16, both extremes"""
    H, W = 7, 9
    img = np.random.default_rng(2).integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[0, 0] = 0; img[H - 1, W - 1] = 255; img[3, 4] = [124, 116, 104]
    path = str(tmp_path / "img.bin")
    img.tofile(path)
    out = subprocess.run([exe, "frame", str(H), str(W), "124", "116", "104", path], capture_output=True, text=True, check=True).stdout
    got = np.array([[int(v, 16) for v in ln.split()] for ln in out.split("\n") if ln], np.uint32).reshape(H + 6, W + 8, 2)
    want = R.frame(img, [124, 116, 104])
    assert np.array_equal(got, want)
    inside = np.zeros((H + 6, W + 8), bool); inside[3:H + 3, 3:W + 3] = True
    assert not got[~inside].any() and ((got[inside][:, 1] >> 16) == 0x3f80).all()
    vals = np.stack([got[..., 0] & 0xffff, got[..., 0] >> 16, got[..., 1] & 0xffff], -1)[inside].astype(np.uint32)
    back = (vals << 16).view(np.float32).reshape(H, W, 3)      # the bf16 values read back are the integers themselves
    assert np.array_equal(back, img.astype(np.float32) - np.asarray([124, 116, 104], np.float32))
    assert got[3 + 3, 3 + 4, 0] == 0 and got[3 + 3, 3 + 4, 1] == 0x3f80 << 16      # a pixel at the centres: zero but for the indicator


def _choose(exe, tmp, rows, settings):
    np.savetxt(os.path.join(tmp, "rows.txt"), np.asarray(rows), fmt="%d")
    np.savetxt(os.path.join(tmp, "settings.txt"), np.asarray(settings), fmt="%d")
    p = subprocess.run([exe, "choose", os.path.join(tmp, "rows.txt"), os.path.join(tmp, "settings.txt")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = []
    for ln in p.stdout.split("\n")[:-1]:
        head, text = ln.split(" | ", 1) if not ln.endswith(" | ") else (ln[:-3], "")
        v = head.split(" ")
        out.append(dict(family=v[0], code=int(v[1]), mode=int(v[2]), bm=int(v[3]), bn=int(v[4]), waves=int(v[5]), pool=int(v[6]),
                        plane_ok=int(v[7]), text=text))
    return out


def _stem_row(B, ih, iw, pool, a_bf16=1, **kv):
    a = T.stem_rows(0, B, ih, iw, pool)
    a.update(kv)
    return [a[f] for f in T.FIELDS] + [a_bf16]


def _setting(**kv):
    return [dict(T.SWITCH_DEFAULTS, **kv)[k] for k in T.SWITCHES]


def test_choose_gives_the_stem_the_new_mode(exe, tmp_path):
    cases = [   # (row, setting, token or None = refused)
        (_stem_row(32, 800, 1066, 1), _setting(), "f32.ring.m5.512x64.pool"),
        (_stem_row(32, 800, 1066, 0), _setting(), "f32.ring.m5.512x64"),
        (_stem_row(2, 230, 310, 1), _setting(pin=1), "f32.ring.m5.512x64.pool"),
        (_stem_row(1, 40, 72, 1), _setting(pin=1), "f32.ring.m5.512x64.pool"),
        (_stem_row(2, 230, 310, 1), _setting(), None),                       # too few rows for the sixteen-wave tile, not pinned
        (_stem_row(32, 800, 1066, 1), _setting(stem_pool=0), None),          # pooled form asked for with the pool switched off
        (_stem_row(32, 800, 1066, 0), _setting(stem_pool=0), "f32.ring.m5.512x64"),
        (_stem_row(32, 800, 1066, 1), _setting(f32=0), None),
        (_stem_row(32, 800, 1066, 1), _setting(mfma16=0), None),             # the 16x16x32 loop only
        (_stem_row(32, 800, 1066, 1), _setting(presplit=0), None),
        (_stem_row(32, 800, 1066, 1), _setting(tiles=23), None),             # sixteen-wave tiles switched off
        (_stem_row(32, 800, 1066, 1), _setting(ring=0), None),
        (_stem_row(32, 800, 1066, 1, Wt3=0), _setting(), None),              # no pre-split filters
        (_stem_row(32, 800, 1065, 1), _setting(), None),                     # odd row pitch: rows off the 16-byte boundary
        (_stem_row(32, 800, 1066, 1, res=1), _setting(), None),
    ]
    got = _choose(exe, str(tmp_path), [c[0] for c in cases], [c[1] for c in cases])
    for (row, setting, tok), g in zip(cases, got):
        if tok is None:
            assert g["family"] == "Refused" and g["code"] == 1 and not g["plane_ok"] and "bf16_plane_ok" in g["text"], (g, setting)
        else:
            assert g["family"] == "RingF32" and g["text"] == tok and g["plane_ok"], (g, setting)
            assert (g["mode"], g["bm"], g["bn"], g["waves"], g["pool"]) == (5, 512, 64, 16, int(tok.endswith(".pool")))


def test_nothing_else_changes(exe, tmp_path):
    """every row of the table under the default, pinned and forced-ring settings with the new field at 0: mode 5 never appears, and the
    answers are those of tests/native/cg_choice_check.cpp (the program the recorded fixture is held to) for the same calls"""
    rows = T.all_rows()
    settings = [_setting(), _setting(pin=1), _setting(ring=2)]
    R_, S_ = [], []
    for r in rows:
        for s in settings:
            R_.append(list(r) + [0]); S_.append(s)
    got = _choose(exe, str(tmp_path), R_, S_)
    assert len(got) == len(R_) and not [g for g in got if g["mode"] == 5 or ".m5." in g["text"]]
    old = str(tmp_path / "cg_choice_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(REPO, "tests", "native", "cg_choice_check.cpp"), "-o", old])
    np.savetxt(str(tmp_path / "r41.txt"), np.asarray([r[:41] for r in R_]), fmt="%d")
    p = subprocess.run([old, "zip", str(tmp_path / "r41.txt"), str(tmp_path / "settings.txt")], capture_output=True, text=True, check=True)
    want = [ln.split(" | ", 1)[1] if not ln.endswith(" | ") else "" for ln in p.stdout.split("\n")[:-1]]
    assert [g["text"] for g in got] == want
