"""The reference Associator (src/models/associator.py:202-268) run on ragged BATCHES with eval_only=False, in float32 and in float64, and
its collater on one of them: tests/golden/assoc_batch.npz.  Build container only (imports the reference through refenv).
Run: python tests/golden/make_golden_assoc_batch.py

Weights make_associator_state_dict(2, 8, seed=0); the inputs of sample i of batch k are make_inputs(T, n_det, 1000 + 37 k + i) of
make_golden_assoc.py, the ground-truth pairs gt_pairs(T, n_det, seed) below -- deterministic, so the tests regenerate the tensors and the
fixture stores the seeds and the (small) pair lists.  The float64 run is the one of make_golden_assoc_f64.py: model.double() with the
frame-index product position * div_term kept in float32.

div_term [128] float32: the encoding's table as this run computed it (see make_golden_assoc_f64.py).
batches [n_samples, 5] int32: batch, index in the batch, T, n_det, seed.
Per sample s = b<k>s<i>:
  <s>_gt         [k, 2] int32     (track, detection) pairs, -1 = dustbin
  <s>_Z64        [(T + 1), (n_det + 1)]
  <s>_scores64   [T, 30]
  <s>_desc64     rows desc_rows(Tmax + 30) of the sample's descriptors [Tmax + 30, 256] (its Tmax track rows, padding included, then its 30
                 detection slots)
  <s>_err32      [4] the float32 run's largest deviation from the float64 run at the sample's descriptors (all Tmax + 30 rows), scores,
                 exp(Z), and Z where Z64 > -6
  <s>_gt_err32   sum over the pairs of |Z32 - Z64|
  <s>_loss       [2] the sample's loss term sum_pairs -Z[track, detection] from the float32 and from the float64 run
  <s>_matches    [2, n_det] hungarian_matching at threshold 0.1 of the float32 and of the float64 run
  <s>_robust     1 when hungarian_matching(exp(Z64 + delta)) equals the unperturbed float64 matches for 32 seeded draws of delta uniform in
                 +-4 x the sample's Z error (err32[3])
b<k>_loss [2]: the reference's "loss" of the whole batch, float32 and float64.
collate_*: the reference's collater (src/scripts/run_association.py:68-123) on batch A: the padded detections, valid_list, the two
split lists, the shapes of tracks and gt_masks and gt_masks' sum."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_golden_assoc import CFG, make_inputs  # noqa: E402
from make_golden_assoc_f64 import desc_rows  # noqa: E402

BATCHES = {"A": [(3, 5), (17, 30), (1, 1), (9, 2)],           # ragged, a 1 x 1 sample
           "B": [(65, 30), (2, 7), (64, 30)],                 # 63 padding rows; 65 keys: one 64-key chunk plus one key
           "C": [(40, 12)],                                   # batch of one
           "D": [(8, 8)] * 3,                                 # no padding
           "E": [(129, 17), (127, 17), (5, 30)]}              # both sides of the single-frame Sinkhorn kernel switch at 128 rows
THRESHOLD = 0.1
MIN_ROBUST = 12


def seed_of(k, i):
    return 1000 + 37 * k + i


def gt_pairs(T, n_det, seed):
    """one pair per detection -- about 30 % on the track dustbin (written -1), the others on a random track -- and up to two pairs that
    send a track to the detection dustbin"""
    rs = np.random.RandomState(seed + 500000)
    pairs = [(-1 if rs.uniform() < 0.3 else int(rs.randint(0, T)), d) for d in range(n_det)]
    pairs += [(int(rs.randint(0, T)), -1) for _ in range(min(2, T - 1))]
    return np.asarray(pairs, np.int32).reshape(-1, 2)


def samples_of(k, name):
    """[(T, n_det, seed, tracks [T, 79, 100], detections [79, n_det], gt [k, 2])] of batch `name` (the k-th)"""
    out = []
    for i, (T, n) in enumerate(BATCHES[name]):
        tr, de = make_inputs(T, n, seed_of(k, i))
        out.append((T, n, seed_of(k, i), tr, de[0][:, :n], gt_pairs(T, n, seed_of(k, i))))
    return out


def _hungarian(P, thr):
    from scipy.optimize import linear_sum_assignment
    match = np.zeros(P.shape[1]) - 1
    for r, c in zip(*linear_sum_assignment(1 - P)):
        if P[r, c] > thr:
            match[c] = r
    return match


def main():
    import refenv
    refenv.setup()
    orig_to = torch.Tensor.to
    torch.Tensor.to = lambda self, *a, **k: self if (a and a[0] == "cuda") else orig_to(self, *a, **k)
    from src.models.associator import Associator
    import types
    sys.modules.setdefault("src.main_track", types.SimpleNamespace(get_args_parser=None))      # run_association.py imports it; the tree lacks the file
    from src.scripts.run_association import collater
    from odam_amd import weights
    sd = weights.make_associator_state_dict(2, 8, seed=0)
    models, caps = {}, {}
    for tag in ("32", "64"):
        m = Associator(CFG)
        m.load_state_dict(sd, strict=True)
        m.eval()
        caps[tag] = []
        m.final_proj.register_forward_hook(lambda mod, i, o, store=caps[tag]: store.append(o.detach()))
        models[tag] = m
    m64 = models["64"].double()
    div32 = models["32"].positional_encoding.div_term

    def encoding64(position):
        a = (position.float().unsqueeze(-1) * div32).double()       # the float32 product
        pe = torch.zeros(position.shape[0], position.shape[1], 256, dtype=torch.float64)
        pe[:, :, 0::2] = torch.sin(a)
        pe[:, :, 1::2] = torch.cos(a)
        return pe.transpose(1, 2)
    m64.positional_encoding.forward = encoding64
    data = {"div_term": div32.numpy().copy()}
    table, n_robust = [], 0
    for k, name in enumerate(BATCHES):
        samples = samples_of(k, name)
        batch = collater([{"tracks": torch.from_numpy(tr), "detections": torch.from_numpy(de), "match": torch.from_numpy(gt).long(),
                           "img_path": f"{name}{i}", "pose": np.eye(4)} for i, (T, n, seed, tr, de, gt) in enumerate(samples)])
        if name == "A":
            data["collate_detections"] = batch["detections"].numpy()
            data["collate_valid_list"] = np.asarray(batch["valid_list"], np.int32)
            data["collate_track_batch_split"] = np.asarray(batch["track_batch_split"], np.int32)
            data["collate_detection_batch_split"] = np.asarray(batch["detection_batch_split"], np.int32)
            data["collate_tracks_shape"] = np.asarray(batch["tracks"].shape, np.int32)
            data["collate_gt_masks_shape"] = np.asarray(batch["gt_masks"].shape, np.int32)
            data["collate_gt_masks_sum"] = np.float64(batch["gt_masks"].sum().item())
            data["collate_keys"] = np.asarray(sorted(batch.keys()))
        tmax = max(T for T, *_ in samples)
        got = {}
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            caps[tag].clear()
            with torch.no_grad():
                out = models[tag]({"tracks": batch["tracks"].to(dt), "detections": batch["detections"].to(dt), "valid_list": batch["valid_list"],
                                   "gt_matches": batch["gt_matches"]}, THRESHOLD, eval_only=False, device="cpu")
                d0, d1 = caps[tag]                                     # [B, 256, Tmax], [B, 256, 30]
                scores = torch.einsum("bdn,bdm->bnm", d0, d1) / CFG["descriptor_dim"] ** .5
            got[tag] = {"Z": [p[0].double().numpy() for p in out["pred"]], "scores": scores.double().numpy(),
                        "desc": torch.cat([d0.transpose(1, 2), d1.transpose(1, 2)], 1).double().numpy(),      # [B, Tmax + 30, 256]
                        "loss": float(out["loss"]), "matches": [np.asarray(m) for m in out["matches"]]}
        data[f"b{k}_loss"] = np.array([got["32"]["loss"], got["64"]["loss"]])
        for i, (T, n, seed, tr, de, gt) in enumerate(samples):
            s = f"b{k}s{i}"
            Z32, Z64 = got["32"]["Z"][i], got["64"]["Z"][i]
            big = Z64 > -6
            err = np.array([np.abs(got["32"]["desc"][i] - got["64"]["desc"][i]).max(),
                            np.abs(got["32"]["scores"][i, :T] - got["64"]["scores"][i, :T]).max(),
                            np.abs(np.exp(Z32) - np.exp(Z64)).max(), np.abs(Z32[big] - Z64[big]).max()])
            at = lambda Z: np.array([Z[t, d] for t, d in gt])      # (numpy's negative index: -1 is the dustbin)
            m64_ = _hungarian(np.exp(Z64[:-1, :-1]), THRESHOLD)
            assert np.array_equal(m64_, got["64"]["matches"][i])
            rs = np.random.RandomState(seed + 900000)
            robust = all(np.array_equal(_hungarian(np.exp(Z64[:-1, :-1] + rs.uniform(-4 * err[3], 4 * err[3], (T, n))), THRESHOLD), m64_)
                         for _ in range(32))
            n_robust += int(robust)
            data[f"{s}_gt"] = gt
            data[f"{s}_Z64"] = Z64
            data[f"{s}_scores64"] = got["64"]["scores"][i, :T]
            data[f"{s}_desc64"] = got["64"]["desc"][i][desc_rows(tmax + 30)]
            data[f"{s}_err32"] = err
            data[f"{s}_gt_err32"] = np.float64(np.abs(at(Z32) - at(Z64)).sum())
            data[f"{s}_loss"] = np.array([-at(Z32).astype(np.float64).sum(), -at(Z64).sum()])
            data[f"{s}_matches"] = np.stack([got["32"]["matches"][i], got["64"]["matches"][i]])
            data[f"{s}_robust"] = np.int32(robust)
            table.append((k, i, T, n, seed))
            print(name, i, "T", T, "n_det", n, "fp32 vs float64: desc %.2e scores %.2e exp(Z) %.2e Z %.2e" % tuple(err),
                  "gt %.2e" % data[f"{s}_gt_err32"], "loss32 %.6f loss64 %.6f" % tuple(data[f"{s}_loss"]), "robust", robust,
                  "matches equal", np.array_equal(got["32"]["matches"][i], got["64"]["matches"][i]))
        assert abs(sum(data[f"b{k}s{i}_loss"][1] for i in range(len(samples))) - got["64"]["loss"]) < 1e-9
    assert n_robust >= MIN_ROBUST, n_robust
    data["batches"] = np.asarray(table, np.int32)
    torch.Tensor.to = orig_to
    np.savez_compressed(os.path.join(HERE, "assoc_batch.npz"), **data)
    print("robust", n_robust, "of", len(table), "| bytes", os.path.getsize(os.path.join(HERE, "assoc_batch.npz")))


if __name__ == "__main__":
    main()
