"""Host restatement of the association network's BATCHED forward with the validation loss (odam_amd/csrc/assoc_batch.hip, include/odam_assoc.h:
odam_assoc_forward_batch; the reference's Associator.forward with eval_only=False, src/models/associator.py:202-268) in float64, torch on
the CPU, built on the functions of tests/assoc_ref.py: the tracks of all samples through the encoder and the fuser, the time means padded
with -1 to the batch's largest track count, the matching layers over [B, Tmax + 30] rows -- the padding rows are keys and queries like any
other --, the final projection, the per-sample score blocks, the optimal transport, the loss terms sum_pairs -Z[track, detection] and the
Hungarian matches.

mutate= plants one of two mistakes: "no_padding" runs every sample alone (a Python loop over the single-frame forward: no padding rows at
all), "zero_padding" pads with 0 instead of -1.  tests/test_assoc_batch_host.py shows that the GPU test's bounds see both."""
import math

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from assoc_ref import D, ND, _Weights, _attend, _propagate, frame_encoding, sinkhorn

MUTATIONS = (None, "no_padding", "zero_padding")


def hungarian_matching(P, threshold):
    """associator.py:19-35 on a float64 score matrix [T, n]: per detection the matched track where its score exceeds threshold, else -1"""
    match = np.zeros(P.shape[1]) - 1
    for r, c in zip(*linear_sum_assignment(1 - P)):
        if P[r, c] > threshold:
            match[c] = r
    return match


def loss_term(Z, pairs):
    """sum over the (track, detection) pairs, in order, of -Z[track, detection]; -1 (like the counts themselves) is the dustbin"""
    m, n = Z.shape[0] - 1, Z.shape[1] - 1
    s = 0.0
    for t, d in np.asarray(pairs).reshape(-1, 2).astype(np.int64):
        s += -float(Z[m if t < 0 else t, n if d < 0 else d])
    return s


def forward(sd, tracks, detections, valid_list, layers, gt_matches=None, iters=100, mutate=None, div=None, threshold=0.1):
    """sd: state dict; tracks [sum T, 79, 100], detections [B, 79, 30] (float32 values), valid_list [(T_b, n_b)] * B, gt_matches [[k_b, 2]] * B
    or None; layers: the matching layers' names; div: the frame-index table (default assoc_ref.div_term()).
    -> dict: padded [B Tmax + 30 B, 256] (the B Tmax track rows, then the 30 B detection rows: the library's row order), x_after (list of
    the same, one per matching layer), desc (the same after the final projection), scores [[T_b, 30]] * B, Z [[(T_b + 1), (n_b + 1)]] * B,
    loss_terms [B], matches [[n_b]] * B.  With mutate="no_padding" every sample has its own largest track count, so the three row blocks
    are lists of per-sample blocks [T_b + 30, 256] instead."""
    if mutate not in MUTATIONS:
        raise ValueError(mutate)
    W = _Weights(sd)
    tr = torch.as_tensor(np.asarray(tracks, np.float32))
    de = torch.as_tensor(np.asarray(detections, np.float32)).reshape(-1, 79, ND)
    valid = [(int(t), int(n)) for t, n in valid_list]
    B = len(valid)
    assert tr.shape[0] == sum(t for t, _ in valid) and de.shape[0] == B
    n_self = len({k.split(".")[2] for k in sd if k.startswith("fuser.layers.")})
    pad_value = 0.0 if mutate == "zero_padding" else -1.0
    with torch.no_grad():
        def encode(x):      # [..., 79, L] -> [..., L, 256]
            f = x[..., 1:, :].transpose(-1, -2).double()
            return W.lin("encoder.2", torch.relu(W.lin("encoder.0", f))) + frame_encoding(x[..., 0, :], div)
        xt = encode(tr)                                                     # [sum T, 100, 256]
        xd = encode(de)                                                     # [B, 30, 256]
        for i in range(n_self):
            xt = xt + _propagate(W, f"fuser.layers.{i}.", xt, lambda q, k, v, m: _attend(q, k, v))
        fused = xt.mean(dim=1)                                              # [sum T, 256]
        starts = np.r_[0, np.cumsum([t for t, _ in valid])]

        def run(group):
            """the samples of `group` as one padded batch -> (padded, x_after, desc) as [len(group), Tmax + 30, 256] tensors"""
            tmax = max(valid[b][0] for b in group)
            xp = torch.full((len(group), tmax, D), pad_value, dtype=torch.float64)
            for i, b in enumerate(group):
                xp[i, :valid[b][0]] = fused[starts[b]:starts[b + 1]]
            x = torch.cat([xp, xd[list(group)]], 1)
            padded, after = x.clone(), []
            for i, name in enumerate(layers):
                if name not in ("self", "cross"):
                    raise ValueError(name)

                def src_of(q, k, v, m, cross=name == "cross"):
                    kt, vt, kd, vd = k[:, :tmax], v[:, :tmax], k[:, tmax:], v[:, tmax:]
                    a_t = _attend(q[:, :tmax], kd, vd) if cross else _attend(q[:, :tmax], kt, vt)
                    a_d = _attend(q[:, tmax:], kt, vt) if cross else _attend(q[:, tmax:], kd, vd)
                    return torch.cat([a_t, a_d], 1)
                x = x + _propagate(W, f"gnn.layers.{i}.", x, src_of)
                after.append(x.clone())
            return tmax, padded, after, W.lin("final_proj", x)

        groups = [[b] for b in range(B)] if mutate == "no_padding" else [list(range(B))]
        runs = [run(g) for g in groups]
        out = {"scores": [], "Z": [], "loss_terms": [], "matches": []}
        for b, (T, n) in enumerate(valid):
            tmax, _, _, desc = runs[b] if mutate == "no_padding" else runs[0]
            d = desc[0 if mutate == "no_padding" else b]
            scores = d[:T] @ d[tmax:].T / math.sqrt(D)
            Z = sinkhorn(scores[:, :n], float(sd["bin_score"]), iters).numpy()
            out["scores"].append(scores.numpy())
            out["Z"].append(Z)
            out["loss_terms"].append(loss_term(Z, gt_matches[b]) if gt_matches is not None else 0.0)
            out["matches"].append(hungarian_matching(np.exp(Z[:-1, :-1]), threshold))
        out["loss_terms"] = np.asarray(out["loss_terms"])

        def rows(t):      # [B, Tmax + 30, 256] -> the library's row order
            tmax = t.shape[1] - ND
            return torch.cat([t[:, :tmax].reshape(-1, D), t[:, tmax:].reshape(-1, D)], 0).numpy().copy()
        if mutate == "no_padding":
            out.update(padded=[r[1][0].numpy() for r in runs], x_after=[[a[0].numpy() for a in r[2]] for r in runs], desc=[r[3][0].numpy() for r in runs])
        else:
            _, padded, after, desc = runs[0]
            out.update(padded=rows(padded), x_after=[rows(a) for a in after], desc=rows(desc), t_max=runs[0][0])
    return out
