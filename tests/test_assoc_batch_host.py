"""The batched association forward without a GPU: tests/assoc_batch_ref.py (the float64 restatement tests/test_assoc_batch_gpu.py holds the
kernels to) against the reference Associator's float64 run on ragged batches (tests/golden/assoc_batch.npz, made by
tests/golden/make_golden_assoc_batch.py); the power of the GPU test's bounds against two planted padding mistakes;
odam_amd.associator.collate against the reference collater's recorded output; and the argument contract of odam_assoc_ot_batch,
odam_assoc_reserve_batch and odam_assoc_forward_batch -- every refusal happens before the library touches the device (dummy non-null
pointers are never dereferenced, the handle comes from odam_assoc_create, which touches no device either)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import assoc_batch_ref  # noqa: E402
from make_golden_assoc_batch import BATCHES, THRESHOLD, samples_of  # noqa: E402
from make_golden_assoc_f64 import desc_rows  # noqa: E402

LAYERS = ["self", "cross"] * 4
FIX = np.load(os.path.join(HERE, "golden", "assoc_batch.npz"))
DIV = FIX["div_term"]        # the frame-index table of the fixture's reference run (assoc_ref.div_term)
FACTOR = 4.0                 # tests/test_assoc_batch_gpu.py: the kernels may leave float64 by 4 x the reference's own fp32 error
NAMES = list(BATCHES)


def batch_inputs(k):
    """batch k of the fixture as the restatement takes it: (tracks [sum T, 79, 100], detections [B, 79, 30], valid_list, gt pair lists)"""
    samples = samples_of(k, NAMES[k])
    det = -np.ones((len(samples), 79, 30), np.float32)
    for i, (T, n, seed, tr, de, gt) in enumerate(samples):
        det[i, :, :n] = de
        assert np.array_equal(gt, FIX[f"b{k}s{i}_gt"])
    return np.concatenate([s[3] for s in samples]), det, [(s[0], s[1]) for s in samples], [s[5] for s in samples]


@pytest.fixture(scope="module")
def state_dict():
    from odam_amd import weights
    return weights.make_associator_state_dict(2, 8, seed=0)


@pytest.fixture(scope="module")
def plain_forward(state_dict):
    """the unmutated float64 forward per batch, computed once (read only) -- on the frame-index table of the fixture's reference run"""
    cache = {}

    def get(k):
        if k not in cache:
            tr, de, valid, gt = batch_inputs(k)
            cache[k] = assoc_batch_ref.forward(state_dict, tr, de, valid, LAYERS, gt_matches=gt, div=DIV, threshold=THRESHOLD)
        return cache[k]
    return get


def test_fixture_holds_the_batches_of_the_generator():
    rows = [tuple(r) for r in FIX["batches"]]
    assert [(r[0], r[2], r[3]) for r in rows] == [(k, T, n) for k, name in enumerate(NAMES) for T, n in BATCHES[name]]
    assert all(seed == 1000 + 37 * k + i for k, i, _, _, seed in rows)
    assert sum(int(FIX[f"b{k}s{i}_robust"]) for k, i, *_ in rows) >= 12


@pytest.mark.parametrize("k", range(len(NAMES)), ids=NAMES)
def test_restatement_equals_the_reference_float64_run(plain_forward, k):
    """Z, the score blocks, the stored descriptor rows and the matches of assoc_batch_ref.forward equal the reference's float64 run of the
    batch: 1e-9 absolute (the bound of tests/test_assoc_ref_host.py: two float64 evaluations in another order), matches identical, the
    loss terms within 1e-9 per pair."""
    r = plain_forward(k)
    valid = BATCHES[NAMES[k]]
    tmax = max(T for T, _ in valid)
    assert r["t_max"] == tmax and r["desc"].shape == r["padded"].shape == (len(valid) * (tmax + 30), 256) and len(r["x_after"]) == 8
    for i, (T, n) in enumerate(valid):
        s = f"b{k}s{i}"
        assert r["Z"][i].shape == FIX[f"{s}_Z64"].shape == (T + 1, n + 1)
        assert np.abs(r["Z"][i] - FIX[f"{s}_Z64"]).max() <= 1e-9
        assert np.abs(r["scores"][i] - FIX[f"{s}_scores64"]).max() <= 1e-9
        desc = np.concatenate([r["desc"][i * tmax:(i + 1) * tmax], r["desc"][len(valid) * tmax + 30 * i:len(valid) * tmax + 30 * (i + 1)]])
        assert np.abs(desc[desc_rows(tmax + 30)] - FIX[f"{s}_desc64"]).max() <= 1e-9
        assert np.array_equal(r["matches"][i], FIX[f"{s}_matches"][1])
        assert abs(r["loss_terms"][i] - FIX[f"{s}_loss"][1]) <= 1e-9 * len(FIX[f"{s}_gt"])
        # the padding rows of the block are -1 in every column, the others are not
        pad = r["padded"][i * tmax + T:(i + 1) * tmax]
        assert np.all(pad == -1.0) and not np.any(np.all(r["padded"][i * tmax:i * tmax + T] == -1.0, axis=1))
    assert abs(r["loss_terms"].sum() - FIX[f"b{k}_loss"][1]) <= 1e-9 * sum(len(FIX[f"b{k}s{i}_gt"]) for i in range(len(valid)))


@pytest.mark.parametrize("mutate", ["no_padding", "zero_padding"])
@pytest.mark.parametrize("k", [0, 1, 4], ids=["A", "B", "E"])
def test_bounds_see_the_planted_padding_mistakes(state_dict, plain_forward, k, mutate):
    """The power of the GPU test on every batch that has padding rows: each sample run alone (a Python loop over the single-frame forward),
    or a padding of 0 instead of -1, moves some sample's Z (where Z64 > -6) by more than 100 x the bound the GPU test holds that sample's Z
    to (4 x the reference's own fp32 error of the sample, from the fixture).  A condition on the inputs, not a tolerance.  A sample that
    already has the batch's largest track count has no padding rows of its own batch row: "no_padding" leaves it where it was."""
    r = plain_forward(k)
    tr, de, valid, gt = batch_inputs(k)
    m = assoc_batch_ref.forward(state_dict, tr, de, valid, LAYERS, gt_matches=gt, div=DIV, mutate=mutate, threshold=THRESHOLD)
    tmax = max(T for T, _ in valid)
    ratios = []
    for i, (T, n) in enumerate(valid):
        big = FIX[f"b{k}s{i}_Z64"] > -6
        moved = float(np.abs(m["Z"][i] - r["Z"][i])[big].max())
        ratios.append(moved / (FACTOR * float(FIX[f"b{k}s{i}_err32"][3])))
        print(f"batch {NAMES[k]} sample {i} ({T}, {n}) {mutate}: Z moved {moved:.3e}, {ratios[-1]:.0f} x the GPU bound")
        if mutate == "no_padding" and T == tmax:
            assert moved <= 1e-9
    assert max(ratios) > 100.0, ratios


def test_collate_equals_the_reference_collater_on_batch_a():
    from odam_amd import associator
    samples = samples_of(0, "A")
    data = [{"tracks": torch.from_numpy(tr), "detections": torch.from_numpy(de), "match": torch.from_numpy(gt).long(), "img_path": f"A{i}",
             "pose": np.eye(4)} for i, (T, n, seed, tr, de, gt) in enumerate(samples)]
    out = associator.collate(data)
    assert sorted(out.keys()) == list(FIX["collate_keys"])
    assert out["detections"].dtype == torch.float32 and np.array_equal(out["detections"].numpy(), FIX["collate_detections"])
    assert [tuple(v) for v in out["valid_list"]] == [tuple(v) for v in FIX["collate_valid_list"]]
    assert list(out["track_batch_split"]) == list(FIX["collate_track_batch_split"])
    assert list(out["detection_batch_split"]) == list(FIX["collate_detection_batch_split"])
    assert tuple(out["tracks"].shape) == tuple(FIX["collate_tracks_shape"]) and torch.equal(out["tracks"], torch.cat([d["tracks"] for d in data]))
    assert tuple(out["gt_masks"].shape) == tuple(FIX["collate_gt_masks_shape"]) and float(out["gt_masks"].sum()) == float(FIX["collate_gt_masks_sum"])
    assert out["gt_masks"].dtype == torch.float32 and float(out["gt_masks"][:3, :5].min()) == 1.0 and float(out["gt_masks"][:3, 5:].max()) == 0.0
    assert all(torch.equal(a, d["match"]) for a, d in zip(out["gt_matches"], data))
    assert out["img_names"] == [f"A{i}" for i in range(4)] and len(out["poses"]) == 4


def test_gt_track_of_detections():
    from odam_amd import associator
    got = associator.gt_track_of_detections([(2, 0), (-1, 1), (5, 2), (1, -1), (0, 4), (3, 5)], n_tracks=5, n_det=5)
    assert got.tolist() == [2.0, -1.0, -1.0, -1.0, 0.0]      # track 5 of 5 is the dustbin; detection 3 has no pair; (3, 5) is a dustbin pair


# ---- the argument contract ----------------------------------------------------------------------------------------------------
P = ctypes.c_void_p(16)      # a pointer that only has to be non-null
N = None


@pytest.fixture(scope="module")
def L():
    from odam_amd import _lib
    return _lib.lib()


def _arr(values, dtype):
    return np.ascontiguousarray(values, dtype)


def ot(scores=P, off=P, lds=P, m=P, n=P, B=4, max_m=40, alpha=1.0, iters=100, gt=P, gt_off=P, Z=P, Z_off=P, terms=P, status=P):
    return (scores, off, lds, m, n, B, max_m, alpha, iters, gt, gt_off, Z, Z_off, terms, status, N)


OT_CASES = [(ot(**{k: N}), 1, ["null pointer"]) for k in ("scores", "off", "lds", "m", "n", "Z", "Z_off", "terms", "status")] + [
    (ot(gt=N), 1, ["gt and gt_off go together"]), (ot(gt_off=N), 1, ["gt and gt_off go together"]),
    (ot(iters=-1), 1, ["iters", "at least 0"]),
    (ot(B=0), 3, ["1 <= B <= 64"]), (ot(B=65), 3, ["1 <= B <= 64"]),
    (ot(max_m=0), 3, ["1 <= max_m <= 1024"]), (ot(max_m=1025), 3, ["1 <= max_m <= 1024"])]


@pytest.mark.parametrize("args,code,fragments", OT_CASES, ids=[str(i) for i in range(len(OT_CASES))])
def test_ot_batch_argument_contract(L, args, code, fragments):
    assert L.odam_assoc_ot_batch(*args) == code
    err = L.odam_last_error().decode()
    assert err.startswith("odam_assoc_ot_batch:"), err
    for f in fragments:
        assert f in err, err


@pytest.fixture()
def bare_handle(L):
    """odam_assoc_create alone: a handle that was never finalised owns nothing on the device"""
    made = []

    def make(max_tracks=1024):
        h = ctypes.c_void_p()
        cross = (ctypes.c_int * 2)(0, 1)
        assert L.odam_assoc_create(max_tracks, 2, cross, 2, 100, ctypes.byref(h)) == 0
        made.append(h)
        return h
    yield make
    for h in made:
        L.odam_assoc_destroy(h)


# (what changes from a valid call, handle's max_tracks, return code, fragments of odam_last_error())
FB_CASES = [
    (dict(T=[0, 3]), 1024, 3, ["sample 0", "T = 0", "T >= 1"]),
    (dict(n=[5, 0]), 1024, 3, ["sample 1", "n_det = 0", "1 <= n_det <= 30"]),
    (dict(n=[31, 5]), 1024, 3, ["sample 0", "n_det = 31"]),
    (dict(T=[600, 425]), 1024, 3, ["1025 tracks in the batch", "limit is 1024"]),
    (dict(T=[5, 4]), 8, 3, ["9 tracks in the batch", "max_tracks 8"]),
    (dict(B=0), 1024, 3, ["1 <= B <= 64"]),
    (dict(B=65), 1024, 3, ["1 <= B <= 64"]),
    (dict(gt=[(0, 0), (5, 1), (0, 0)]), 1024, 1, ["pair 1 of sample 0", "(5, 1)", "[-1, 4] x [-1, 5]"]),      # T_b itself is the dustbin, T_b + 1 is outside
    (dict(gt=[(0, 0), (-2, 1), (0, 0)]), 1024, 1, ["pair 1 of sample 0", "(-2, 1)"]),
    (dict(gt=[(0, 0), (0, 0), (1, 7)]), 1024, 1, ["pair 0 of sample 1", "(1, 7)", "[-1, 3] x [-1, 6]"]),
    (dict(gt=[(0, 0), (0, 0), (1, -2)]), 1024, 1, ["pair 0 of sample 1", "(1, -2)"]),
    (dict(gt_off=[1, 2, 3]), 1024, 1, ["gt_off must start at 0"]),
    (dict(gt_off=[0, 2, 1]), 1024, 1, ["gt_off must not decrease"]),
    (dict(gt_off=[0, 2, 5000]), 1024, 3, ["more than 4096 ground-truth pairs"]),
    # everything in order, dustbin indices written both ways: refused only for the block that was never reserved
    (dict(gt=[(4, 5), (-1, -1), (3, 6)]), 1024, 3, ["padded block of 68 rows", "larger than the reservation of 0"]),
]


@pytest.mark.parametrize("change,max_tracks,code,fragments", FB_CASES, ids=[str(i) for i in range(len(FB_CASES))])
def test_forward_batch_argument_contract(L, bare_handle, change, max_tracks, code, fragments):
    a = dict(T=[4, 3], n=[5, 6], B=2, gt=[(0, 0), (-1, 1), (2, -1)], gt_off=[0, 2, 3])
    a.update(change)
    T, n, gt, gt_off, z_off = _arr(a["T"], np.int32), _arr(a["n"], np.int32), _arr(a["gt"], np.int32), _arr(a["gt_off"], np.int32), _arr([0, 30], np.int64)
    rc = L.odam_assoc_forward_batch(bare_handle(max_tracks), P, T.ctypes.data, P, n.ctypes.data, a["B"], gt.ctypes.data, gt_off.ctypes.data, P,
                                    z_off.ctypes.data, P, P, N)
    err = L.odam_last_error().decode()
    assert rc == code, err
    assert err.startswith("odam_assoc_forward_batch:"), err
    for f in fragments:
        assert f in err, err


def test_forward_batch_null_pointers_and_unpaired_gt(L, bare_handle):
    T, n, z_off = _arr([4, 3], np.int32), _arr([5, 6], np.int32), _arr([0, 30], np.int64)
    gt, gt_off = _arr([(0, 0)], np.int32), _arr([0, 1, 1], np.int32)
    good = [bare_handle(), P, T.ctypes.data, P, n.ctypes.data, 2, gt.ctypes.data, gt_off.ctypes.data, P, z_off.ctypes.data, P, P, N]
    for i in (0, 1, 2, 3, 4, 8, 9, 10, 11):
        args = list(good)
        args[i] = N
        assert L.odam_assoc_forward_batch(*args) == 1 and "null pointer" in L.odam_last_error().decode(), i
    for i in (6, 7):
        args = list(good)
        args[i] = N
        assert L.odam_assoc_forward_batch(*args) == 1 and "gt and gt_off go together" in L.odam_last_error().decode(), i


@pytest.mark.parametrize("max_batch,max_t", [(0, 8), (65, 8), (4, 0), (4, 1025), (-1, -1)])
def test_reserve_batch_refuses(L, bare_handle, max_batch, max_t):
    assert L.odam_assoc_reserve_batch(bare_handle(), max_batch, max_t) == 3
    err = L.odam_last_error().decode()
    assert err.startswith("odam_assoc_reserve_batch:") and "1 <= max_batch <= 64" in err and "1 <= max_tracks_per_sample <= 1024" in err


def test_reserve_batch_needs_a_finalised_handle(L, bare_handle):
    assert L.odam_assoc_reserve_batch(N, 4, 8) == 1 and "null handle" in L.odam_last_error().decode()
    assert L.odam_assoc_reserve_batch(bare_handle(), 4, 8) == 1 and "odam_assoc_finalize first" in L.odam_last_error().decode()
