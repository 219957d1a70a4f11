"""Track merging between the two super-quadric passes -- SURVEY.md section 8(f) rank 4.

`merge_process` keeps the behaviour of the reference's (likojack/ODAM src/scripts/run_merge.py:79-130): cost
= 1 - 3D IoU of the fitted boxes for mergeable class pairs, sklearn AgglomerativeClustering on the precomputed
cost (average linkage, threshold 0.95), per image the observation of the longest member track,
scipy.stats.mode for the merged class.

The pair cost is not the reference's per-pair Python polygon clipper + qhull (box_utils.py:24-120) but a closed
form for two convex quadrilaterals evaluated for all mergeable pairs at once: the intersection's boundary is
made of the pieces of either polygon's edges that lie inside the other polygon; each edge is cut against the
other polygon's four half-planes parametrically and the area is the boundary integral of (x dy - y dx) / 2.
Config-5 sizes (500 objects, 125 k pairs) take milliseconds.  Values agree with the reference's box3d_iou to
rounding (tests/golden/box_iou.npz), clusters are identical (tests/golden/sq_merge.npz).

`AgglomerativeClustering(affinity=...)` of the reference is spelled `metric=` in scikit-learn >= 1.2.
"""
import numpy as np
import scipy.stats
from sklearn.cluster import AgglomerativeClustering


def _boundary_inside(P, Q, closed):
    """Green's-theorem contribution of the parts of P's edges that lie inside the convex quadrilateral Q.

    P, Q: [n, 4, 2] counter-clockwise vertex lists.  Each edge p -> q of P is cut against the four half-planes of Q
    parametrically (enter = largest t at which the edge crosses into a half-plane, leave = smallest t at which it
    crosses out); the surviving piece [enter, leave] contributes cross(p(enter), p(leave)) / 2.  `closed` says whether
    an edge lying exactly on Q's boundary counts as inside (it must count for one of the two polygons only)."""
    p = P                                            # [n, 4, 2]
    d = np.roll(P, -1, axis=1) - P                   # edge vectors
    a = Q[:, None, :, :]                             # [n, 1, 4, 2] half-plane anchors
    e = (np.roll(Q, -1, axis=1) - Q)[:, None, :, :]  # half-plane directions; inside = left of a -> a + e
    pp = p[:, :, None, :]; dd = d[:, :, None, :]
    dist = e[..., 0] * (pp[..., 1] - a[..., 1]) - e[..., 1] * (pp[..., 0] - a[..., 0])   # [n, 4 edges, 4 planes]
    rate = e[..., 0] * dd[..., 1] - e[..., 1] * dd[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -dist / rate
    par = rate == 0
    out_par = par & ((dist < 0) if closed else (dist <= 0))       # parallel and on the wrong side: nothing survives
    enter = np.where((rate > 0) & ~par, t, -np.inf).max(axis=2)
    leave = np.where((rate < 0) & ~par, t, np.inf).min(axis=2)
    t0 = np.clip(enter, 0.0, 1.0); t1 = np.clip(leave, 0.0, 1.0)
    ok = (t1 > t0) & ~out_par.any(axis=2)
    s = p + t0[..., None] * d; q = p + t1[..., None] * d
    return np.where(ok, s[..., 0] * q[..., 1] - s[..., 1] * q[..., 0], 0.0).sum(axis=1) * 0.5


def _signed_area(R):
    x, y = R[..., 0], R[..., 1]
    return 0.5 * (x * np.roll(y, -1, axis=-1) - y * np.roll(x, -1, axis=-1)).sum(axis=-1)


def rect_intersection_area(R1, R2):
    """Area of the intersection of convex quadrilaterals R1[i] and R2[i] ([n, 4, 2], any winding), all pairs at
    once: the boundary of the intersection is {edges of R1 inside R2} + {edges of R2 inside R1}, and the area is
    the line integral of (x dy - y dx) / 2 along it."""
    s1 = _signed_area(R1); s2 = _signed_area(R2)
    A = np.where((s1 < 0)[:, None, None], R1[:, ::-1], R1)
    B = np.where((s2 < 0)[:, None, None], R2[:, ::-1], R2)
    return np.maximum(_boundary_inside(A, B, True) + _boundary_inside(B, A, False), 0.0)


def box3d_iou_pairs(C1, C2):
    """3D IoU and bird's-eye IoU of box pairs (C1[i], C2[i]), [n, 8, 3] corner arrays in the layout of
    `compute_oriented_bbox` / `get_3d_box` (top face 0-3, bottom face 4-7) -- the quantity of the reference's
    box3d_iou (src/utils/box_utils.py:98-120), evaluated for all pairs at once.  The reference clips rectangle 1
    (corners 3,2,1,0) by rectangle 2 with a clipper that assumes rectangle 2 is counter-clockwise in that order
    and returns nothing otherwise; that case (a box whose top face winds the other way) keeps its IoU of 0."""
    C1 = np.asarray(C1, np.float64); C2 = np.asarray(C2, np.float64)
    R1 = C1[:, 3::-1, :2]; R2 = C2[:, 3::-1, :2]
    a1 = np.abs(_signed_area(R1)); a2 = np.abs(_signed_area(R2))
    inter = np.where(_signed_area(R2) > 0, rect_intersection_area(R1, R2), 0.0)
    iou_bev = inter / (a1 + a2 - inter)
    dz = np.maximum(0.0, np.minimum(C1[:, 0, 2], C2[:, 0, 2]) - np.maximum(C1[:, 4, 2], C2[:, 4, 2]))

    def vol(c):
        return (np.linalg.norm(c[:, 0] - c[:, 1], axis=1) * np.linalg.norm(c[:, 1] - c[:, 2], axis=1)
                * np.linalg.norm(c[:, 0] - c[:, 4], axis=1))
    iv = inter * dz
    return iv / (vol(C1) + vol(C2) - iv), iou_bev


def box3d_iou(c1, c2):
    """one pair: (iou_3d, iou_bev)"""
    a, b = box3d_iou_pairs(np.asarray(c1)[None], np.asarray(c2)[None])
    return float(a[0]), float(b[0])


def cost_matrix(tracks, bboxes_qc, fitter=None):
    """run_merge.py:92-118: 1 - 3D IoU for mergeable class pairs, 1 otherwise; symmetric, zero diagonal.
    All mergeable pairs (i < j) go through one vectorised IoU evaluation -- on the host, or with an sq.SqFitter in ONE launch
    over the n x n block (evaluate.box3d_iou_matrix, gate 2 = this class rule).  iou(b_i, b_j) and iou(b_j, b_i) need not be
    equal (the clipper is not symmetric in winding), so the device path too reads the upper triangle i < j and mirrors it."""
    n = len(tracks)
    cls = np.array([int(np.median(t[:, 1])) for t in tracks])
    boxes = np.asarray([np.asarray(b, np.float64) for b in bboxes_qc]).reshape(n, 8, 3)
    if fitter is not None:
        from . import evaluate
        iou = evaluate.box3d_iou_matrix(boxes, boxes, cls, cls, gate=2, fitter=fitter)["iou3d"].cpu().numpy()
        cost = np.triu(1 - iou, 1)
        return cost + cost.T
    sofa_chair = (cls == 4) | (cls == 5)             # run_merge.py:105-108
    ok = (cls[:, None] == cls[None, :]) | (sofa_chair[:, None] & sofa_chair[None, :])
    i, j = np.nonzero(np.triu(ok, 1))
    cost = np.triu(np.ones((n, n)), 1)
    if len(i):
        cost[i, j] = 1 - box3d_iou_pairs(boxes[i], boxes[j])[0]
    return cost + cost.T


def _merge_cluster(tracks, mask, img_names):
    """run_merge.py:24-58: per image keep the observation of the longest member track; class = mode"""
    members = [i for i in range(len(tracks)) if mask[i]]
    dom = np.concatenate([tracks[i][:, 1] for i in members], axis=0)
    dom = int(scipy.stats.mode(dom).mode)
    by_frame = {}
    for i in members:
        for row in tracks[i]:
            by_frame.setdefault(row[0], []).append((i, row))
    out = []
    for name in img_names:
        cands = by_frame.get(name)
        if not cands:
            continue
        # np.argmax over track lengths in member order: first longest wins
        best = max(range(len(cands)), key=lambda k: (len(tracks[cands[k][0]]), -k))
        row = cands[best][1].copy()   # the reference selects rows with a boolean mask (a copy, run_merge.py:36):
        row[1] = dom                  # the merged class goes into the copy, the input tracks stay as they were
        out.append(row)
    return np.asarray(out)


def _device_scene(data, img_names):
    """what the device merge needs of one scene -- (tracks, rows14 of all tracks, boxes, classes) -- or None when the scene is one the
    kernels do not restate and the host path has to take it: a single track (returned untouched by the reference: no image
    filtering, no class change), more tracks than the clustering kernel holds, image names that are not all different integers
    inside int32, a track that is not a float64 array of at least 14 columns, an empty track, tracks of different widths"""
    from . import sq
    tracks = data["tracks"]
    n = len(tracks)
    if n < 2 or n > sq.MERGE_MAX_TRACKS:
        return None
    try:
        if sq.unique_frame_ids(img_names) is None or any(int(f) != f for f in img_names):
            return None
    except (TypeError, ValueError):
        return None
    for t in tracks:
        if not isinstance(t, np.ndarray) or t.dtype != np.float64 or t.ndim != 2 or t.shape[1] < 14 or t.shape[1] != tracks[0].shape[1] \
                or len(t) == 0:
            return None
    cls = np.array([int(np.median(t[:, 1])) for t in tracks], np.int32)
    boxes = np.asarray([np.asarray(b, np.float64) for b in data["bboxes_qc"]]).reshape(n, 8, 3)
    return tracks, [t[:, :14] for t in tracks], boxes, cls


def _device_merge(datas, img_names_list, fitter, want_rows14, rows=None):
    """the three device steps for the scenes _device_scene accepts: ONE IoU launch, ONE clustering launch, ONE assembly pass, ONE small
    copy back.  Returns (scenes, picked, res, head): scenes[k] = _device_scene's answer or None, picked = indices of the scenes that
    went to the device (in launch order), res = SqFitter.merge_assemble's dict, head = its "head" on the host.
    rows: for ONE scene, a packed block of its tracks' rows that is on the device already (track_store.TrackRows.packed(): the rows
    pass 1 was fitted from), used instead of the concatenate and the upload."""
    from . import evaluate
    fitter = evaluate._default_fitter(fitter)
    scenes = [_device_scene(d, names) for d, names in zip(datas, img_names_list)]
    picked = [k for k, s in enumerate(scenes) if s is not None]
    if not picked:
        return scenes, picked, None, None
    if rows is not None:
        if len(datas) != 1:
            raise ValueError("merge: a packed block of rows stands for the tracks of ONE scene")
        off = np.asarray(rows["row_offsets"], np.int64)
        if not np.array_equal(np.diff(off), [len(t) for t in scenes[0][0]]):
            raise ValueError("merge: the packed block of rows does not hold the tracks of this scene (rows per track differ)")
    r = evaluate._iou_launch([scenes[k][2] for k in picked], [scenes[k][2] for k in picked], [scenes[k][3] for k in picked],
                             [scenes[k][3] for k in picked], 2, fitter, False)
    cl = fitter.merge_cluster(r["iou3d"], r["a_off"], r["pair_off"])
    if rows is not None:
        rows14, row_off = rows["rows14"], off
    else:
        rows14 = np.concatenate([t for k in picked for t in scenes[k][1]])
        row_off = np.concatenate([[0], np.cumsum([len(t) for k in picked for t in scenes[k][1]])])
    res = fitter.merge_assemble(cl, r["a_off"], rows14, row_off, [img_names_list[k] for k in picked], want_rows14=want_rows14)
    return scenes, picked, res, res["head"].cpu().numpy()


def _gather_merged(tracks, off, src, cls, base=0):
    """the merged [n, 82] tracks of one scene on the host: merged track i holds the rows src[off[i] .. off[i + 1] - 1] - base of
    np.concatenate(tracks), with column 1 = cls[i]"""
    allrows = np.concatenate(tracks)
    merged = []
    for i in range(len(cls)):
        t = allrows[src[off[i]:off[i + 1]] - base]      # (fancy indexing: a copy, the caller's tracks stay as they were)
        t[:, 1] = cls[i]
        merged.append(t)
    return merged


def tracks_from_packed(block, data):
    """The merged [n, 82] tracks merge_scenes returns for the scene, gathered on the host from merge_packed's block ("src",
    "row_offsets", "cls": ONE small copy back) and the caller's tracks data["tracks"].  A caller that goes on from the block on the
    device (SqFitter.prepare, track_store.TrackRows.adopt) calls this after it has enqueued that work."""
    import torch
    n, r = int(block["cls"].shape[0]), int(block["src"].shape[0])
    h = torch.cat([block["row_offsets"].to(torch.int32), block["src"].to(torch.int32), block["cls"].to(torch.int32)]).cpu().numpy()
    return _gather_merged(data["tracks"], h[:n + 1], h[n + 1:n + 1 + r], h[n + 1 + r:])


def merge_scenes(datas, img_names_list, fitter=None):
    """merge_process for many scenes at once on the device: the IoU of all pairs of all scenes in one launch, the clustering of all
    scenes in one launch (SqFitter.merge_cluster), the assembly of all merged tracks in one pass (SqFitter.merge_assemble).
    datas: one optim_process dict per scene; img_names_list: one list of frame ids per scene.  Returns, per scene, the list of
    merged [n, 82] tracks merge_process returns, decision for decision.  Only offsets, source-row indices and classes come back from
    the device; the merged rows are gathered on the host from the caller's tracks.  A scene the kernels do not restate
    (_device_scene), or one that comes back with a status (a class that is not an integer in 0..63, a frame id twice in one track,
    more than 16384 rows in one cluster), goes down the host path for this call."""
    if len(datas) != len(img_names_list):
        raise ValueError("one list of image names per scene")
    scenes, picked, res, head = _device_merge(datas, img_names_list, fitter, False)
    out = [None] * len(datas)
    if picked:
        ns = len(picked)
        n_out, status, n_total, r_total = head[:ns], head[ns:2 * ns], int(head[2 * ns]), int(head[2 * ns + 1])
        off = res["out_off"][:n_total + 1].cpu().numpy()
        src = res["out_src"][:r_total].cpu().numpy()
        cls = res["out_cls"][:n_total].cpu().numpy()
        o = base = 0
        for q, k in enumerate(picked):
            tracks = scenes[k][0]
            if status[q] == 0:
                out[k] = _gather_merged(tracks, off[o:o + int(n_out[q]) + 1], src, cls[o:o + int(n_out[q])], base)
            o += int(n_out[q])
            base += sum(len(t) for t in tracks)
    for k, m in enumerate(out):
        if m is None:
            out[k] = merge_process(datas[k], img_names_list[k], fitter)
    return out


def merge_packed(data, img_names, fitter=None, rows=None):
    """One scene merged on the device and left there, for callers that go straight into SqFitter.prepare: {"rows14" [R_out, 14]
    float64 (column 1 = the merged class), "row_offsets" [n_out + 1] int32, "cls" [n_out] int32, "src" [R_out] int32 (indices into
    np.concatenate(data["tracks"]))}, all device tensors; or None when the scene has to go down the host path (merge_scenes).
    rows: the packed block pass 1 was fitted from (_device_merge), in place of the concatenate and the upload of the tracks' rows;
    tracks_from_packed gives the host tracks of the block."""
    scenes, picked, res, head = _device_merge([data], [img_names], fitter, True, rows=rows)
    if not picked or head[1] != 0:
        return None
    n_out, r_out = int(head[2]), int(head[3])
    return {"rows14": res["rows14"][:r_out], "row_offsets": res["out_off"][:n_out + 1], "cls": res["out_cls"][:n_out],
            "src": res["out_src"][:r_out]}


def merge_packed_scenes(datas, img_names_list, fitter=None, rows=None):
    """merge_packed for MANY scenes whose rows are on the device already: _device_merge's three steps in the launches of one scene --
    ONE IoU launch, ONE merge_cluster, ONE merge_assemble(want_rows14=True), ONE small copy back (the head).
    rows: the combined packed block of the scenes' tracks (track_store.pack_scenes: "rows14", "row_offsets", "trk_off"), one scene
    per entry of datas.  Returns (block, scenes):
      block   {"rows14" [R_out, 14], "row_offsets" [n_total + 1] int32, "cls" [n_total] int32, "src" [R_out] int32} on the device: the
              merged tracks of all scenes that went to the device, one scene after the other in the order of datas, and on the host
              "n_out" [S] (merged tracks per scene; 0 for a scene that did not go), "status" [S] (-1 for a scene _device_scene refuses),
              "row_base" [S] (what "src" of the scene's rows counts from: its first row among the rows that went).  None where no scene went.
      scenes  per scene None -- _device_scene refuses it, or it came back with a status: the caller's host path -- or the scene's own
              merge_packed dict, sliced out of the block LAZILY: a callable without arguments (the slices cost two small launches a
              scene, which a caller that adopts the whole block -- track_store.adopt_scenes, tracks_from_packed_scenes -- never pays)."""
    import torch
    from . import evaluate
    if rows is None:
        raise ValueError("merge_packed_scenes: rows= the combined packed block of the scenes (track_store.pack_scenes)")
    if len(datas) != len(img_names_list):
        raise ValueError("one list of image names per scene")
    trk = np.asarray(rows["trk_off"], np.int64)
    off = np.asarray(rows["row_offsets"], np.int64)
    S = len(datas)
    if len(trk) != S + 1:
        raise ValueError(f"merge: the packed block of rows holds {len(trk) - 1} scenes, {S} were given")
    fitter = evaluate._default_fitter(fitter)
    scenes = [_device_scene(d, names) for d, names in zip(datas, img_names_list)]
    picked = [k for k, s in enumerate(scenes) if s is not None]
    for k in picked:
        if not np.array_equal(np.diff(off[trk[k]:trk[k + 1] + 1]), [len(t) for t in scenes[k][0]]):
            raise ValueError(f"merge: the packed block of rows does not hold the tracks of scene {k} (rows per track differ)")
    if not picked:
        return None, [None] * S
    r = evaluate._iou_launch([scenes[k][2] for k in picked], [scenes[k][2] for k in picked], [scenes[k][3] for k in picked],
                             [scenes[k][3] for k in picked], 2, fitter, False)
    cl = fitter.merge_cluster(r["iou3d"], r["a_off"], r["pair_off"])
    if len(picked) == S:
        rows14, row_off = rows["rows14"], off
    else:      # the scenes that went, device to device
        rows14 = torch.cat([rows["rows14"][int(off[trk[k]]):int(off[trk[k + 1]])] for k in picked])
        row_off = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(off[trk[k]:trk[k + 1] + 1]) for k in picked]))])
    res = fitter.merge_assemble(cl, r["a_off"], rows14, row_off, [img_names_list[k] for k in picked], want_rows14=True)
    head = res["head"].cpu().numpy()
    ns = len(picked)
    n_total, r_total = int(head[2 * ns]), int(head[2 * ns + 1])
    n_out, status, row_base = np.zeros(S, np.int64), np.full(S, -1, np.int64), np.zeros(S, np.int64)
    base = 0
    for q, k in enumerate(picked):
        n_out[k], status[k], row_base[k] = int(head[q]), int(head[ns + q]), base
        base += int(off[trk[k + 1]] - off[trk[k]])
    block = {"rows14": res["rows14"][:r_total], "row_offsets": res["out_off"][:n_total + 1], "cls": res["out_cls"][:n_total],
             "src": res["out_src"][:r_total], "n_out": n_out, "status": status, "row_base": row_base}
    first = np.concatenate([[0], np.cumsum(n_out)])

    def one(k):
        def cut():      # merge_packed's dict for scene k; the two row bounds are the only words read back
            o = block["row_offsets"][int(first[k]):int(first[k + 1]) + 1]
            a, b = (int(x) for x in o[[0, -1]].cpu().numpy())
            return {"rows14": block["rows14"][a:b], "row_offsets": o - a, "cls": block["cls"][int(first[k]):int(first[k + 1])],
                    "src": block["src"][a:b] - int(row_base[k])}
        return cut
    return block, [one(k) if status[k] == 0 else None for k in range(S)]


def tracks_from_packed_scenes(block, datas):
    """tracks_from_packed for every scene of merge_packed_scenes' block with ONE small copy back: per scene the merged [n, 82] host
    tracks gathered from datas[k]["tracks"], or None for a scene that did not come back merged (status != 0)."""
    import torch
    n, r = int(block["cls"].shape[0]), int(block["src"].shape[0])
    h = torch.cat([block["row_offsets"].to(torch.int32), block["src"].to(torch.int32), block["cls"].to(torch.int32)]).cpu().numpy()
    off, src, cls = h[:n + 1], h[n + 1:n + 1 + r], h[n + 1 + r:]
    out, o = [], 0
    for k, data in enumerate(datas):
        k_out = int(block["n_out"][k])
        if block["status"][k] == 0:
            out.append(_gather_merged(data["tracks"], off[o:o + k_out + 1], src, cls[o:o + k_out], int(block["row_base"][k])))
        else:
            out.append(None)
        o += k_out
    return out


def merge_process(data, img_names, fitter=None, on_device=False):
    """run_merge.py:79-130: data = optim_process output dict; returns the list of merged [n,82] tracks.  With a fitter the pair
    costs come from the device (cost_matrix); with on_device the clustering and the assembly too (merge_scenes: the same tracks,
    decision for decision)."""
    if on_device:
        return merge_scenes([data], [img_names], fitter)[0]
    tracks = data["tracks"]
    n = len(tracks)
    if n == 1:
        merged = tracks
    else:
        cost = cost_matrix(tracks, data["bboxes_qc"], fitter)
        labels = AgglomerativeClustering(n_clusters=None, distance_threshold=0.95, metric="precomputed",
                                         linkage="average").fit(cost).labels_
        merged = [_merge_cluster(tracks, labels == c, img_names) for c in np.unique(labels)]
    return [t for t in merged if len(t) > 0]
