"""The device cut of the validation samples (odam_samples_cut, odam_amd.assoc_samples.SceneTable.cut) on a synthetic scene of 70 objects x
301 frames (tests/assoc_samples_ref.py: make_table) and on the reference-run fixture (tests/golden/assoc_samples.npz).

cut() against cut_host() -- the same plan through numpy, in the kernel's operation order: equal BITS on every channel but 12 and 13 (copies,
correctly rounded float64 products, sums and quotients, one rounding to float32), and 1 float32 ulp on channels 12 and 13 (sin / cos of the
same float64 angle by the device's library and by libm agree to a few float64 ulp, so their float32 roundings are equal or neighbours).
How many of those elements differ at all is recorded (conftest.measured: assoc_samples/...; a run is kept in
profiles/assoc_samples_test_measured.json).  A whole file runs in a few seconds: one scene, built once."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import assoc_samples_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_OBJ, N_FRAMES, IMG_SIZE = 70, 301, (1296, 968)
F_CAP, F_30 = 250, 251           # frames given 31 unmatched rows (past the cap) and exactly 30 detections
LAYERS = {"GNN_layers": ["self", "cross"] * 4, "self_GNN_layers": ["self", "self"], "sinkhorn_iterations": 100}
THRESHOLD = 0.1


def make_scene_arrays():
    table, _ = ref.make_table(np.random.RandomState(11), N_OBJ, N_FRAMES, p_obs=0.06, last_birth=200)
    n30 = 30 - int((table[:, F_30, 0] != -1).sum())      # (the table's draws come before the unmatched rows': the same table again below)
    rs = np.random.RandomState(11)
    table, unmatched = ref.make_table(rs, N_OBJ, N_FRAMES, p_obs=0.06, last_birth=200, forced_unmatched={F_CAP: 31, F_30: n30})
    return table, unmatched, ref.make_poses(rs, N_FRAMES)


@pytest.fixture(scope="module")
def scene():
    from odam_amd import assoc_samples
    table, unmatched, poses = make_scene_arrays()
    s = assoc_samples.SceneTable(table, unmatched, poses, IMG_SIZE, device=DEV)
    yield s
    s.close()


def compare(measured, scene, frames, n_times=100, use_gt_det=False, name=None):
    """cut == cut_host: bits on every channel but 12 and 13, 1 ulp there; returns the device batch"""
    got = scene.cut(frames, use_gt_det=use_gt_det, n_times=n_times)
    want = scene.cut_host(frames, use_gt_det=use_gt_det, n_times=n_times)
    assert got["tracks"].is_cuda and got["detections"].is_cuda
    assert got["valid_list"] == want["valid_list"] and all(np.array_equal(a, b) for a, b in zip(got["gt_matches"], want["gt_matches"]))
    sum_t = sum(t for t, _ in got["valid_list"])
    assert tuple(got["tracks"].shape) == (sum_t, 79, n_times) and tuple(got["detections"].shape) == (len(frames), 79, 30)
    differing = 0
    for key in ("tracks", "detections"):
        g, w = got[key].cpu().numpy(), want[key].numpy()
        exact = [c for c in range(79) if c not in (12, 13)]
        assert np.array_equal(g[:, exact].view(np.uint32), w[:, exact].view(np.uint32)), key
        u = ref.ulps(g[:, 12:14], w[:, 12:14])
        assert u.max() <= 1, (key, int(u.max()))
        differing += int((u > 0).sum())
        n_real = int((w[:, 12:14] != -1).sum())
        print(f"{name or frames}: {key} channels 12-13 differ in {int((u > 0).sum())} of {n_real} computed elements")
    if name:
        measured(f"assoc_samples/sincos_differing/{name}", differing)
    return got


def early_frames(scene, specials, count=64):
    """`specials` filled up with the earliest frames that have a track, to `count` frames in ascending order"""
    rest = [f for f in scene.usable_frames() if f not in specials]
    return sorted(specials + rest[:count - len(specials)])


def test_the_scene_holds_the_cases(scene):
    ix = scene.ix
    assert ix.n_tracks([300])[0] > 64 and N_FRAMES % 64 != 0
    f = np.array([1, 99, 100, 101, 260])
    assert ix.cum[0, f].tolist() == [1, 99, 100, 101, 260]                      # object 0 is seen in every frame
    births = np.argmax(ix.valid, axis=1)
    assert (ix.cum[np.arange(N_OBJ), births] == 0).all() and len(set(births.tolist())) > 30      # count 0: an object in its birth frame
    assert ix.n_detections([2])[0] == 1 and ix.n_detections([F_30])[0] == 30 and ix.n_detections([F_CAP])[0] > 30


def test_cut_equals_cut_host_batch_of_one(measured, scene):
    n_det = {f: compare(measured, scene, [f], name=f"B1_f{f}")["valid_list"][0][1] for f in (2, 100, F_30, F_CAP, 300)}
    assert (n_det[2], n_det[F_30], n_det[F_CAP]) == (1, 30, 30)
    assert compare(measured, scene, [F_CAP], use_gt_det=True, name="B1_gt")["valid_list"][0][1] < 30


def test_cut_equals_cut_host_batch_of_64(measured, scene):
    births = np.argmax(scene.ix.valid, axis=1)
    frames = early_frames(scene, [2, 99, 100, 101, 260, F_CAP, F_30, int(births[20]), int(births[20]) + 1])
    assert len(frames) == 64 and scene.ix.n_tracks(frames).sum() <= 1024
    counts = set(scene.ix.cum[:, frames].reshape(-1).tolist())
    assert {0, 1, 99, 100, 101, 260} <= counts
    compare(measured, scene, frames, name="B64")


def test_cut_equals_cut_host_at_the_track_limit(measured, scene):
    n_t = scene.ix.n_tracks(np.arange(N_FRAMES))
    full = [int(f) for f in np.flatnonzero(n_t == N_OBJ)][:13]                   # 13 x 70 = 910 tracks; two more frames bring 114
    pair = next((a, b) for a in range(5, 250) for b in range(a + 1, 250) if n_t[a] + n_t[b] == 1024 - 13 * N_OBJ)
    frames = sorted(full + list(pair))
    assert int(n_t[frames].sum()) == 1024
    compare(measured, scene, frames, name="sumT1024")
    with pytest.raises(Exception, match="1 <= sum_t <= 1024"):
        scene.cut(frames + [1])


@pytest.mark.parametrize("n_times", [7, 128])
def test_cut_equals_cut_host_other_windows(measured, scene, n_times):
    got = compare(measured, scene, [4, 50, 101, 129, 260, F_CAP], n_times=n_times, name=f"n_times{n_times}")
    first = got["tracks"][got["valid_list"][0][0] + got["valid_list"][1][0]].cpu().numpy()      # object 0 in the sample of frame 101
    k = min(n_times, 101)
    assert (first[0, :k] == np.arange(101 - k, 101)).all() and (first[:, k:] == -1).all()


def test_bits_do_not_depend_on_the_batch(scene):
    """the sample of frame 260 alone, first and last in a batch of 64, and in a second call"""
    others = [f for f in scene.usable_frames() if f != 260][:63]
    alone = scene.cut([260])
    T = alone["valid_list"][0][0]
    assert T == N_OBJ and scene.ix.n_tracks(others).sum() + T <= 1024
    a_t, a_d = alone["tracks"].cpu(), alone["detections"][0].cpu()
    first, last, again = scene.cut([260] + others), scene.cut(others + [260]), scene.cut([260])
    assert torch.equal(first["tracks"][:T].cpu(), a_t) and torch.equal(first["detections"][0].cpu(), a_d)
    assert torch.equal(last["tracks"][-T:].cpu(), a_t) and torch.equal(last["detections"][-1].cpu(), a_d)
    assert torch.equal(again["tracks"].cpu(), a_t) and torch.equal(again["detections"][0].cpu(), a_d)


def test_projected_box_of_minus_one_sets_the_status_of_its_sample_alone():
    from odam_amd import assoc_samples
    table, unmatched, poses = make_scene_arrays()
    table[3, 150, 79:83] = -1      # object 3 is a live track of frame 150 (born before frame 200)
    assert (table[3, :150, 0] != -1).any()
    s = assoc_samples.SceneTable(table, unmatched, poses, IMG_SIZE, device=DEV)
    try:
        tracks, dets, status = s.cut_raw(s.plan([149, 150, 151]))
        assert status.cpu().tolist() == [0, 1, 0]
        with pytest.raises(AssertionError, match="wrong projected bbox"):
            s.cut([149, 150, 151])
        assert s.cut([149, 151])["valid_list"][0][0] >= 1
    finally:
        s.close()


def test_fixture_through_the_device_cut(measured):
    """the reference's own run: the discrete outputs equal, the tensors within the bound of tests/test_assoc_samples_host.py"""
    from odam_amd import assoc_samples
    fix, frames, use_gt, img_size, unmatched = ref.load_fixture()
    s = assoc_samples.SceneTable(fix["table"], unmatched, fix["T_wcs"], img_size, device=DEV)
    try:
        differing = 0
        for gt in (False, True):
            idx = [i for i in range(len(frames)) if use_gt[i] == gt]
            out = s.cut([frames[i] for i in idx], use_gt_det=gt)
            tr, de = out["tracks"].cpu().numpy(), out["detections"].cpu().numpy()
            t0 = 0
            for b, i in enumerate(idx):
                T, n = out["valid_list"][b]
                assert (T, n) == tuple(fix["collate_valid_list"][i])
                assert np.array_equal(out["gt_matches"][b], fix[f"s{i}_match"]) and np.array_equal(out["scores"][b], fix[f"s{i}_scores"])
                assert out["global_track_ids"][b] == fix[f"s{i}_gids"].tolist()
                differing += sum(ref.check_against_fixture(fix, tr[t0:t0 + T], de[b, :, :n], i, "device cut"))
                assert (de[b, :, n:] == -1).all()
                t0 += T
        measured("assoc_samples/fixture_differing", differing)
    finally:
        s.close()


def test_validate_scene_equals_validate_on_the_downloaded_cut(scene):
    """same input bits, same kernels: loss terms, correct counts and detection counts equal exactly -- offsets, order and batching"""
    from odam_amd import associator, weights
    net = associator.Associator(LAYERS, max_tracks=256, device=DEV)
    net.load_state_dict(weights.make_associator_state_dict(2, 8, seed=0))
    frames = list(range(20, 60, 2)) + [F_CAP, 2]
    try:
        got = associator.validate_scene(net, scene, THRESHOLD, batch_size=8, frames=frames)
        samples = []
        for chunk in scene.batches(frames, 8):
            batch = scene.cut(chunk)
            tr, de = batch["tracks"].cpu(), batch["detections"].cpu()
            t0 = 0
            for b, (T, n) in enumerate(batch["valid_list"]):
                samples.append({"tracks": tr[t0:t0 + T], "detections": de[b, :, :n], "match": batch["gt_matches"][b]})
                t0 += T
        want = associator.validate(net, samples, THRESHOLD, 8)
    finally:
        net.close()
    assert got["frames"] == frames and len(got["loss_terms"]) == len(frames)
    assert got["loss_terms"] == want["loss_terms"] and got["correct"] == want["correct"] and got["n_det"] == want["n_det"]
    assert got["loss"] == want["loss"] and got["accuracy"] == want["accuracy"]
    assert all(np.isfinite(got["loss_terms"])) and got["n_det"][-2:] == [30, 1]
