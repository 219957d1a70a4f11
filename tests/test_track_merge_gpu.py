"""The track merge on the device (csrc/track_merge.hip, include/odam_merge.h): the clustering kernel against scipy and sklearn on the
device's own IoU block, the assembly against its numpy restatement (tests/merge_ref.py, which tests/test_track_merge_host.py holds
against merge._merge_cluster), and merge_process(on_device=True) / merge_scenes / merge_packed against the host path.  Everything is
discrete or a copied float64 word: every comparison is exact."""
import numpy as np
import pytest
import torch

import merge_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def fitter():
    from odam_amd import sq
    f = sq.SqFitter(DEV, 10)
    yield f
    f.close()


def _rotz(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def synth_boxes(seed, n, n_obj):
    """n fragments of n_obj objects: the boxes of one object overlap (jittered copies), objects mostly do not; classes per object"""
    from odam_amd.multi_view import get_3d_box
    rs = np.random.RandomState(seed)
    dims = rs.uniform(.5, 1.5, (n_obj, 3)); yaw = rs.uniform(-3, 3, n_obj); ctr = rs.uniform(-6, 6, (n_obj, 3)) * [1, 1, 0.2]
    cls_obj = rs.randint(0, 8, n_obj)
    obj = rs.randint(0, n_obj, n)
    boxes = np.asarray([get_3d_box(dims[o] * rs.uniform(.8, 1.2, 3), _rotz(yaw[o] + rs.uniform(-.2, .2)), ctr[o] + rs.uniform(-.25, .25, 3))
                        for o in obj]).reshape(n, 8, 3)
    return boxes, cls_obj[obj]


def synth_scene(seed, n, n_obj, n_img=60):
    """an optim_process-like dict: tracks whose class column follows the object (sofa / chair histories mixed), and their boxes"""
    tracks, _, _, img_names = R.synth_tracks(seed, n, n_img, 2)
    boxes, cls = synth_boxes(seed + 100, n, n_obj)
    rs = np.random.RandomState(seed + 200)
    for t, c in zip(tracks, cls):
        t[:, 1] = c
        if c in (4, 5) and len(t) > 2:
            t[: len(t) // 3, 1] = 9 - c      # a minority of the other label: the median stays
        t[:, 2:6] = rs.uniform(0, 640, (len(t), 4))
    return {"tracks": tracks, "bboxes_qc": list(boxes)}, img_names


def golden_scene(golden):
    z = golden("sq_merge.npz")
    tracks = [z[f"track{i}"].copy() for i in range(int(z["n_tracks"]))]
    return {"tracks": tracks, "bboxes_qc": list(z["bboxes_qc"])}, [int(x) for x in z["img_names"]], \
        [z[f"merged{i}"] for i in range(int(z["n_merged"]))]


def _classes(data):
    return np.array([int(np.median(t[:, 1])) for t in data["tracks"]], np.int32)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y)


# ---- 1. clustering ---------------------------------------------------------------------------------------------------------------------
def check_clustering(fitter, iou_blocks, a_off, pair_off, d_iou):
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform
    from sklearn.cluster import AgglomerativeClustering
    cl = fitter.merge_cluster(d_iou, a_off, pair_off)
    link, labels = cl["linkage"].cpu().numpy(), cl["labels"].cpu().numpy()
    assert cl["status"].cpu().tolist() == [0] * len(iou_blocks)
    for s, iou in enumerate(iou_blocks):
        n = len(iou)
        cost = R.cost_from_iou(iou)
        want = linkage(squareform(cost, checks=False), "average")
        got = link[a_off[s]:a_off[s] + n - 1]
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (s, n)
        sk = AgglomerativeClustering(n_clusters=None, distance_threshold=0.95, metric="precomputed", linkage="average").fit(cost)
        assert np.array_equal(labels[a_off[s]:a_off[s] + n], sk.labels_), (s, n)
        assert int(cl["n_cluster"][s]) == sk.n_clusters_
    return cl


def _device_iou(fitter, datas):
    from odam_amd import evaluate
    boxes = [np.asarray(d["bboxes_qc"], np.float64).reshape(-1, 8, 3) for d in datas]
    cls = [_classes(d) for d in datas]
    r = evaluate.iou_scenes(boxes, boxes, cls, cls, gate=2, fitter=fitter, want_bev=False)
    h = r["iou3d"].cpu().numpy()
    blocks = [h[r["pair_off"][s]:r["pair_off"][s + 1]].reshape(len(b), len(b)) for s, b in enumerate(boxes)]
    return r, blocks


def test_clustering_three_small_scenes_in_one_launch(fitter, golden):
    datas = [synth_scene(1, 2, 1)[0], synth_scene(2, 3, 2)[0], golden_scene(golden)[0]]
    r, blocks = _device_iou(fitter, datas)
    assert [len(b) for b in blocks] == [2, 3, 9]
    cl = check_clustering(fitter, blocks, r["a_off"], r["pair_off"], r["iou3d"])
    assert int(cl["n_cluster"][2]) == 5


@pytest.mark.parametrize("n", [64, 65, 257])
def test_clustering_equals_scipy_and_sklearn(fitter, n):
    r, blocks = _device_iou(fitter, [synth_scene(n, n, max(2, n // 4))[0]])
    off_diag = blocks[0][np.triu_indices(n, 1)]
    assert (off_diag > 0.05).sum() > n // 4 and (off_diag == 0).sum() > n      # merges below the threshold, and exact ties at cost 1
    check_clustering(fitter, blocks, r["a_off"], r["pair_off"], r["iou3d"])


def test_clustering_all_costs_equal(fitter):
    """every pair at the same distance: every decision is a tie; one scene below the threshold, one above"""
    blocks = [np.full((7, 7), 0.5), np.full((6, 6), 0.03125)]
    a_off = np.array([0, 7, 13]); pair_off = np.array([0, 49, 85])
    d_iou = torch.from_numpy(np.concatenate([b.reshape(-1) for b in blocks])).to(DEV)
    cl = check_clustering(fitter, blocks, a_off, pair_off, d_iou)
    assert cl["n_cluster"].cpu().tolist() == [1, 6]


def test_clustering_refuses_what_it_cannot_take(fitter):
    from odam_amd import _lib
    with pytest.raises(_lib.OdamError, match="ODAM_E_LIMIT|code 3"):
        fitter.merge_cluster(torch.zeros(1025 * 1025, device=DEV, dtype=torch.float64), [0, 1025], [0, 1025 * 1025])
    iou = np.full((3, 3), 0.5); iou[0, 2] = np.nan
    cl = fitter.merge_cluster(torch.from_numpy(iou.reshape(-1)).to(DEV), [0, 3], [0, 9])
    assert cl["status"].cpu().tolist() == [R.BAD_COST]


# ---- 2. assembly -----------------------------------------------------------------------------------------------------------------------
def run_assemble(fitter, scenes):
    """scenes: (tracks, labels, n_cluster, img_names) -> the device's outputs on the host, cut to what the head says was written"""
    a_off = np.concatenate([[0], np.cumsum([len(s[0]) for s in scenes])])
    cl = {"labels": torch.from_numpy(np.concatenate([s[1] for s in scenes]).astype(np.int32)).to(DEV),
          "n_cluster": torch.tensor([s[2] for s in scenes], device=DEV, dtype=torch.int32),
          "status": torch.zeros(len(scenes), device=DEV, dtype=torch.int32)}
    tracks = [t for s in scenes for t in s[0]]
    rows = np.concatenate([t[:, :14] for t in tracks])
    row_off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])])
    res = fitter.merge_assemble(cl, a_off, rows, row_off, [s[3] for s in scenes])
    head = res["head"].cpu().numpy()
    ns = len(scenes)
    n_total, r_total = int(head[2 * ns]), int(head[2 * ns + 1])
    return {"out_off": res["out_off"][:n_total + 1].cpu().numpy(), "out_src": res["out_src"][:r_total].cpu().numpy(),
            "out_cls": res["out_cls"][:n_total].cpu().numpy(), "n_out": head[:ns], "status": head[ns:2 * ns],
            "rows14": res["rows14"][:r_total].cpu().numpy()}, rows


def check_assemble(got, rows, ref):
    for k in ("n_out", "status", "out_off", "out_cls", "out_src"):
        assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    want = rows[ref["out_src"]].copy()
    want[:, 1] = np.repeat(ref["out_cls"], np.diff(ref["out_off"]))
    assert np.array_equal(got["rows14"].view(np.uint64), want.view(np.uint64))


def test_assembly_equals_the_restatement(fitter):
    """two scenes in one call; tracks of 1..40 rows; one cluster of 3 + 3 members whose 1200-odd candidates need a 2048-key sort; an
    equal-length pair; frames that name no image; a cluster without a row"""
    big = R.synth_tracks(5, 30, 500, 5, big=(3, 400))
    small = R.synth_tracks(6, 11, 25, 4)
    assert sum(len(t) for t, l in zip(big[0], big[1]) if l == 1) > 1024
    e = big[2]
    assert len(big[0][e]) == len(big[0][e + 1]) and big[1][e] == big[1][e + 1]
    scenes = [big, small]
    ref = R.assemble(scenes)
    assert ref["status"].tolist() == [0, 0] and ref["n_out"].tolist() == [4, 3]      # cluster 0 of either scene has no row
    got, rows = run_assemble(fitter, scenes)
    check_assemble(got, rows, ref)


def test_assembly_statuses_are_reported_per_scene(fitter):
    ok = R.synth_tracks(7, 12, 30, 4)
    bad_cls = R.synth_tracks(8, 12, 30, 4)
    bad_cls[0][5][0, 1] = 2.5
    rep = R.synth_tracks(9, 12, 30, 4)
    k = next(i for i in range(12) if rep[1][i] != 0 and len(rep[0][i]) > 1)
    rep[0][k][:2, 0] = rep[3][0]
    scenes = [bad_cls, ok, rep]
    ref = R.assemble(scenes)
    assert ref["status"].tolist() == [R.BAD_CLASS, 0, R.REPEATED_FRAME] and ref["n_out"][1] > 0
    got, rows = run_assemble(fitter, scenes)
    check_assemble(got, rows, ref)


def test_assembly_scan_carries_past_1024_cluster_slots(fitter):
    """three scenes of 500 + 400 + 200 tracks, every track its own cluster: 1100 cluster slots in one call, so the one-workgroup scan
    over the slots takes a second trip that starts from the first trip's carry; tracks of one or two rows, every seventh on frames
    that name no image (a slot that keeps nothing: the two scanned counts differ)"""
    scenes = []
    for s, n in enumerate((500, 400, 200)):
        rs = np.random.RandomState(40 + s)
        img_names = [int(v) for v in rs.permutation(np.arange(12) * 3 + 7)]
        tracks = []
        for t in range(n):
            k = int(rs.randint(1, 3))
            tr = rs.uniform(-1, 1, (k, 14))
            tr[:, 0] = rs.choice(img_names, k, replace=False) + (1 if t % 7 == 3 else 0)      # + 1: between the images' ids
            tr[:, 1] = rs.randint(0, 8)
            tracks.append(tr)
        scenes.append((tracks, np.arange(n, dtype=np.int32), n, img_names))
    ref = R.assemble(scenes)
    assert ref["status"].tolist() == [0, 0, 0] and ref["n_out"].tolist() == [500 - 71, 400 - 57, 200 - 29]
    assert sum(len(s[0]) for s in scenes) > 1024
    got, rows = run_assemble(fitter, scenes)
    check_assemble(got, rows, ref)


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------------
def test_merge_process_on_device_returns_the_reference_tracks(fitter, golden):
    from odam_amd import merge
    data, img_names, ref = golden_scene(golden)
    before = [t.copy() for t in data["tracks"]]
    out = merge.merge_process(data, img_names, fitter=fitter, on_device=True)
    assert len(ref) == 5
    _same(out, ref)
    _same(data["tracks"], before)      # the input tracks are untouched


def test_odam_process_merge_process_takes_the_option(fitter, golden):
    """OdamProcess.merge_process(data, on_device=True) on a stand-in that has what the method reads: the sequence's frames, the
    fitter, the refine state it drops"""
    import logging
    import types
    from odam_amd import processor
    data, img_names, ref = golden_scene(golden)
    proc = types.SimpleNamespace(logger=logging.getLogger("test"), _refine_state={"track_ids": [0]}, usable_frames=img_names,
                                 _fitter=lambda: fitter)
    _same(processor.OdamProcess.merge_process(proc, data, on_device=True), ref)
    assert proc._refine_state is None
    _same(processor.OdamProcess.merge_process(proc, data), ref)


def test_merge_scenes_equals_merge_process_scene_by_scene(fitter, golden):
    from odam_amd import merge
    g = golden_scene(golden)
    s1, s2 = synth_scene(11, 20, 6), synth_scene(12, 33, 9)
    datas, names = [s1[0], g[0], s2[0]], [s1[1], g[1], s2[1]]
    before = [[t.copy() for t in d["tracks"]] for d in datas]
    got = merge.merge_scenes(datas, names, fitter)
    for k in range(3):
        want = merge.merge_process(datas[k], names[k], fitter=fitter)
        assert 1 < len(want) < len(datas[k]["tracks"])      # something merged, something did not
        _same(got[k], want)
        _same(datas[k]["tracks"], before[k])


def test_every_fallback_yields_the_host_result(fitter, monkeypatch):
    from odam_amd import merge
    data, names = synth_scene(13, 14, 4)
    host = lambda d, nm: merge.merge_process(d, nm, fitter=fitter)
    # the kernels did run for the unchanged scene ...
    calls = []
    real = fitter.merge_assemble
    monkeypatch.setattr(fitter, "merge_assemble", lambda *a, **k: calls.append(1) or real(*a, **k))
    _same(merge.merge_process(data, names, fitter=fitter, on_device=True), host(data, names))
    assert calls == [1]
    # ... and not for a scene of one track (returned untouched), repeated image names or a float32 track
    one = {"tracks": data["tracks"][:1], "bboxes_qc": data["bboxes_qc"][:1]}
    out = merge.merge_process(one, names, fitter=fitter, on_device=True)
    assert len(out) == 1 and out[0] is one["tracks"][0]
    rep_names = list(names) + [names[0]]
    _same(merge.merge_process(data, rep_names, fitter=fitter, on_device=True), host(data, rep_names))
    f32 = {"tracks": [t.astype(np.float32) if i == 3 else t for i, t in enumerate(data["tracks"])], "bboxes_qc": data["bboxes_qc"]}
    _same(merge.merge_process(f32, names, fitter=fitter, on_device=True), host(f32, names))
    assert calls == [1]
    # a status from the device: a class of 2.5, a frame id twice in one track
    c25 = {"tracks": [t.copy() for t in data["tracks"]], "bboxes_qc": data["bboxes_qc"]}
    c25["tracks"][2][0, 1] = 2.5
    _same(merge.merge_process(c25, names, fitter=fitter, on_device=True), host(c25, names))
    twice = {"tracks": [t.copy() for t in data["tracks"]], "bboxes_qc": data["bboxes_qc"]}
    k = next(i for i, t in enumerate(twice["tracks"]) if len(t) > 1)
    twice["tracks"][k][1, 0] = twice["tracks"][k][0, 0] = names[0]
    _same(merge.merge_process(twice, names, fitter=fitter, on_device=True), host(twice, names))
    assert calls == [1, 1, 1]
    assert merge.merge_packed(c25, names, fitter) is None and merge.merge_packed(one, names, fitter) is None


def test_prepare_on_the_packed_block_equals_prepare_on_the_merged_tracks(fitter):
    from odam_amd import merge
    data, names = synth_scene(14, 25, 7)
    merged = merge.merge_process(data, names, fitter=fitter)
    blk = merge.merge_packed(data, names, fitter)
    rows = np.concatenate([t[:, :14] for t in merged])
    offs = np.concatenate([[0], np.cumsum([len(t) for t in merged])])
    assert np.array_equal(blk["row_offsets"].cpu().numpy(), offs)
    assert np.array_equal(blk["rows14"].cpu().numpy().view(np.uint64), rows.view(np.uint64))
    assert np.array_equal(np.concatenate(data["tracks"])[blk["src"].cpu().numpy()][:, 2:], np.concatenate(merged)[:, 2:])
    assert blk["cls"].cpu().tolist() == [int(t[0, 1]) for t in merged]
    rs = np.random.RandomState(0)
    P_cws = rs.uniform(-1, 1, (len(names), 3, 4))
    a = fitter.prepare(blk["rows14"], blk["row_offsets"], names, P_cws, 480, 640)
    b = fitter.prepare(rows, offs, names, P_cws, 480, 640)
    for k in ("cls", "n_obs", "n_valid", "status"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["n_valid"] > 0).any()
    done = a["status"] == 0
    for k in ("init", "pose", "bboxes_dl"):
        x, y = a[k].cpu().numpy()[done], b[k].cpu().numpy()[done]
        assert np.array_equal(x.view(np.uint32 if x.dtype == np.float32 else np.uint64), y.view(np.uint32 if x.dtype == np.float32 else np.uint64)), k
    views = np.concatenate([np.arange(offs[o], offs[o] + a["n_obs"][o]) for o in range(len(merged))])
    for k in ("view_img", "view_row", "valid", "tgt", "mask", "P"):
        assert np.array_equal(a[k].cpu().numpy()[views], b[k].cpu().numpy()[views]), k
