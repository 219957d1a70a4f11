"""The reference's own ScanNetTrack.get_by_sequence and ScanNetTrack.collater (src/datasets/scan_net_track.py:285-341, :34-97) run on a
synthetic scene table: tests/golden/assoc_samples.npz.  Build container only (imports the reference through refenv).
Run: python tests/golden/make_golden_assoc_samples.py

The dataset object is made with ScanNetTrack.__new__ (its __init__ opens a pickle of the real dataset) and given `files`, the three path
patterns and max_objs; the three files get_by_sequence reads per frame -- the pose .txt, the scene's meta file with its axisAlignment line and
a JPEG whose only use is its size -- are written into a temporary directory.  The scene is tests/assoc_samples_ref.py's
make_table(RandomState(SEED), 8, 140, ...) with 31 unmatched detections forced into frame CAP_FRAME.

Stored: table [8, 140, 83]; unm_frames [U] / unm_rows [U, 79] (the `unmatched` dict, keyed by str(frame)); T_wcs [140, 4, 4], the axis-aligned
camera-to-world poses exactly as get_by_sequence forms them (axis_align @ inv(read_extrinsic(file))); img_size; frames [6], use_gt_det [6];
per sample s<i>: _tracks [T, 79, 100] float32, _detections [79, n] float32, _match [pairs, 2], _scores [T, n], _gids; and the collater's
detections [6, 79, 30], valid_list and gt_scores on the six samples.
The six samples: a frame where object 0 has more than 100 earlier observations; the birth frame of an object (a [-1, j] pair); frames with
unmatched detections; CAP_FRAME (more than 30 detections after concatenation: 30 detections and 30 pairs come back); one use_gt_det=True
sample; an early frame."""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

from assoc_samples_ref import make_poses, make_table  # noqa: E402

SEED, N_OBJ, N_FRAMES, CAP_FRAME, IMG_SIZE = 5, 8, 140, 131, (1296, 968)


def scene():
    rs = np.random.RandomState(SEED)
    table, unmatched = make_table(rs, N_OBJ, N_FRAMES, p_obs=0.12, dense=(0,), quiet=4, last_birth=125, forced_unmatched={CAP_FRAME: 31},
                                  img_size=IMG_SIZE)
    return table, unmatched, make_poses(rs, N_FRAMES), np.linalg.inv(make_poses(rs, 1)[0])      # ..., file poses, axis alignment


def sampled_frames(table):
    """(frame, use_gt_det) of the six samples"""
    valid = table[:, :, 0] != -1
    births = [int(np.argmax(valid[o])) for o in range(N_OBJ)]
    born = max(b for b in births if 20 < b < 125)      # an object first seen in the sampled frame, with tracks before it
    return [(6, False), (born, False), (104, False), (120, True), (CAP_FRAME, False), (139, False)]


def main():
    import refenv
    refenv.setup()
    import torch
    from src.datasets.scan_net_track import ScanNetTrack
    from src.datasets import scannet_utils
    table, unmatched, poses, axis = scene()
    keep = table.copy()
    frames = sampled_frames(table)
    out = {"table": table, "img_size": np.asarray(IMG_SIZE), "frames": np.asarray([f for f, _ in frames]),
           "use_gt_det": np.asarray([int(g) for _, g in frames]),
           "unm_frames": np.asarray([int(k) for k, rows in unmatched.items() for _ in rows]),
           "unm_rows": np.asarray([r for rows in unmatched.values() for r in rows])}
    with tempfile.TemporaryDirectory() as tmp:
        from PIL import Image
        os.makedirs(os.path.join(tmp, "pose"))
        os.makedirs(os.path.join(tmp, "color"))
        with open(os.path.join(tmp, "meta.txt"), "w") as fh:
            fh.write("sceneType = synthetic\naxisAlignment = " + " ".join(repr(float(x)) for x in axis.reshape(-1)) + "\n")
        for f in range(N_FRAMES):
            np.savetxt(os.path.join(tmp, "pose", f"{f}.txt"), poses[f], fmt="%.17g")
        for f, _ in frames:
            Image.new("RGB", IMG_SIZE).save(os.path.join(tmp, "color", f"{f}.jpg"))
        ds = ScanNetTrack.__new__(ScanNetTrack)
        ds.files = {"scene": {"tracks": table, "unmatched": unmatched}}
        ds.img_path = os.path.join(tmp, "color", "{1}.jpg")
        ds.pose_path = os.path.join(tmp, "pose", "{1}.txt")
        ds.meta_path = os.path.join(tmp, "meta.txt")
        ds.max_objs = 30
        align = scannet_utils.read_meta_file(ds.meta_path.format("scene"))
        out["T_wcs"] = np.stack([align @ np.linalg.inv(scannet_utils.read_extrinsic(ds.pose_path.format("scene", f))) for f in range(N_FRAMES)])
        samples = []
        for i, (f, gt) in enumerate(frames):
            s = ds.get_by_sequence("scene", f, f, use_gt_det=gt)
            samples.append(s)
            out[f"s{i}_tracks"] = s["tracks"].numpy().copy()
            out[f"s{i}_detections"] = s["detections"].numpy().copy()
            out[f"s{i}_match"] = np.asarray(s["match"], np.int64)
            out[f"s{i}_scores"] = s["scores"].numpy()
            out[f"s{i}_gids"] = np.asarray(s["global_track_ids"], np.int64)
            print(f"sample {i}: frame {f}, use_gt_det {gt}: tracks {tuple(s['tracks'].shape)}, detections {tuple(s['detections'].shape)}, "
                  f"{len(s['match'])} pairs, rows per track {[int((t[0] != -1).sum()) for t in s['tracks']]}")
        col = ScanNetTrack.collater(samples)
        out["collate_detections"] = col["detections"].numpy()
        out["collate_valid_list"] = np.asarray(col["valid_list"], np.int64)
        out["collate_gt_scores"] = col["gt_scores"].numpy()
        assert torch.equal(col["tracks"], torch.cat([s["tracks"] for s in samples]))
    assert np.array_equal(keep, table), "the reference changed the table"
    # the conditions the tests rely on
    i_cap = [f for f, _ in frames].index(CAP_FRAME)
    assert out[f"s{i_cap}_detections"].shape[1] == 30 and len(out[f"s{i_cap}_match"]) == 30
    assert any((out[f"s{i}_match"][:, 0] == -1).any() and (out[f"s{i}_match"][(out[f"s{i}_match"][:, 0] == -1), 1] < (table[:, f, 0] != -1).sum()).any()
               for i, (f, _) in enumerate(frames)), "no object first seen in a sampled frame"
    assert any((out[f"s{i}_tracks"][:, 0, -1] != -1).any() for i in range(len(frames))), "no track with 100 kept rows"
    path = os.path.join(HERE, "assoc_samples.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
