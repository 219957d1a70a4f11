"""numpy restatement of the two kernels of csrc/track_merge.hip (include/odam_merge.h), decision for decision.

`linkage_average` is scipy's nearest-neighbour chain for method="average" followed by its stable sort and union-find relabelling;
`labels_from_linkage` is sklearn's _hc_cut (heapq on negated node ids).  `assemble` is merge.py::_merge_cluster for every cluster
of every scene the way the device does it: members ranked by (rows descending, track ascending), keys (image << 32 | candidate),
one sort, the first key of each image.  The tests hold these against scipy, sklearn and merge._merge_cluster themselves."""
import heapq

import numpy as np

MAX_TRACKS = 1024
MAX_CAND = 16384
BAD_OFFSETS, BAD_COST, NOT_CLUSTERED, BAD_CLASS, REPEATED_FRAME, TOO_MANY_ROWS = 1, 2, 3, 4, 5, 6
N_CLASS = 64


def cost_from_iou(iou):
    """merge.cost_matrix: 1 - iou of the upper triangle i < j, mirrored, zero diagonal"""
    c = np.triu(1 - np.asarray(iou, np.float64), 1)
    return c + c.T


def linkage_average(C):
    """scipy.cluster.hierarchy.linkage(squareform(C), "average"), bit for bit"""
    n = len(C)
    D = np.array(C, np.float64)
    size = np.ones(n, np.int64)
    Z = np.zeros((n - 1, 4))
    chain = []
    low = 0
    for k in range(n - 1):
        if not chain:                                  # 1. the chain restarts at the lowest live index
            while size[low] == 0:
                low += 1
            chain = [low]
        while True:
            x = chain[-1]
            live = np.flatnonzero(size > 0)
            live = live[live != x]
            i = live[np.argmin(D[x, live])]            # 2. the lowest index with the strictly smallest distance ...
            cur = D[x, i]
            y = int(i)
            if len(chain) > 1 and not cur < D[x, chain[-2]]:
                y = chain[-2]                          #    ... the previous chain element wins an exact tie
            if len(chain) > 1 and y == chain[-2]:
                break
            chain.append(y)
        chain = chain[:-2]
        if x > y:
            x, y = y, x
        nx, ny = int(size[x]), int(size[y])
        Z[k] = (x, y, cur, nx + ny)                    # 3. merge (x, y), x < y; the cluster stays at y
        size[x] = 0
        size[y] = nx + ny
        for i in np.flatnonzero(size > 0):
            if i != y:
                D[i, y] = D[y, i] = (float(nx) * D[i, x] + float(ny) * D[i, y]) / float(nx + ny)
    Z = Z[np.argsort(Z[:, 2], kind="stable")]          # 4. stable by distance, then scipy's label()
    parent = list(range(2 * n - 1))
    usize = [1] * (2 * n - 1)

    def find(a):
        p = a
        while parent[a] != a:
            a = parent[a]
        while parent[p] != a:
            p, parent[p] = parent[p], a
        return a
    for r in range(n - 1):
        a, b = find(int(Z[r, 0])), find(int(Z[r, 1]))
        Z[r, 0], Z[r, 1] = min(a, b), max(a, b)
        parent[a] = parent[b] = n + r
        usize[n + r] = usize[a] + usize[b]
        Z[r, 3] = usize[n + r]
    return Z


def labels_from_linkage(Z, n, threshold):
    """sklearn's labels_ for distance_threshold=threshold: (labels [n], n_clusters)"""
    children = Z[:, :2].astype(np.int64)
    n_cl = int((Z[:, 2] >= threshold).sum()) + 1       # 5.
    nodes = [-(int(max(children[-1])) + 1)]
    for _ in range(n_cl - 1):                          # 6. the label of a cluster is its position in the heap array
        ch = children[-nodes[0] - n]
        heapq.heappush(nodes, -int(ch[0]))
        heapq.heappushpop(nodes, -int(ch[1]))
    node_label = np.full(2 * n - 1, -1, np.int64)
    for i, nd in enumerate(nodes):
        node_label[-nd] = i
    for v in range(2 * n - 2, n - 1, -1):
        if node_label[v] >= 0:
            node_label[children[v - n]] = node_label[v]
    return node_label[:n].astype(np.int32), n_cl


def cluster(iou, threshold=0.95):
    """one scene: {"linkage" [n-1, 4], "labels" [n], "n_cluster"} from the n x n IoU block"""
    n = len(iou)
    if n == 1:
        return {"linkage": np.zeros((0, 4)), "labels": np.zeros(1, np.int32), "n_cluster": 1}
    Z = linkage_average(cost_from_iou(iou))
    labels, n_cl = labels_from_linkage(Z, n, threshold)
    return {"linkage": Z, "labels": labels, "n_cluster": n_cl}


def assemble_scene(tracks, labels, n_cluster, img_names, cap=MAX_CAND):
    """one scene: tracks = list of [k, >= 2] float64 arrays (columns 0 and 1 are read), labels [n], img_names all different.
    Returns (status, [(cls, src), ...]) with src = indices into np.concatenate(tracks), one entry per cluster that has a row."""
    names = np.asarray([int(f) for f in img_names], np.int64)
    order = np.argsort(names, kind="stable")
    ids = names[order].astype(np.float64)
    row0 = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    out, status = [], 0
    for c in range(n_cluster):
        members = [t for t in range(len(tracks)) if labels[t] == c]
        ranked = sorted(members, key=lambda t: (-len(tracks[t]), t))
        n_cand = sum(len(tracks[t]) for t in ranked)
        if n_cand > cap:
            status = max(status, TOO_MANY_ROWS)
            continue
        if n_cand == 0:
            continue
        keys, owner, src, hist = [], [], [], np.zeros(N_CLASS, np.int64)
        for t in ranked:
            for i, row in enumerate(tracks[t]):
                j = len(owner)
                owner.append(t)
                src.append(int(row0[t]) + i)
                f = row[0]
                lo = int(np.searchsorted(ids, f, side="left")) if f == f else len(ids)
                if lo < len(ids) and ids[lo] == f:
                    keys.append((int(order[lo]) << 32) | j)
                cl = row[1]
                if 0 <= cl <= N_CLASS - 1 and cl == np.floor(cl):
                    hist[int(cl)] += 1
                else:
                    status = max(status, BAD_CLASS)
        keys.sort()
        chosen = []
        for a, key in enumerate(keys):
            if a == 0 or (keys[a - 1] >> 32) != (key >> 32):
                chosen.append(src[key & 0xffffffff])
            elif owner[keys[a - 1] & 0xffffffff] == owner[key & 0xffffffff]:
                status = max(status, REPEATED_FRAME)
        if chosen:
            out.append((int(np.argmax(hist)), np.asarray(chosen, np.int64)))
    return status, out


def assemble(scenes, cap=MAX_CAND):
    """scenes: list of (tracks, labels, n_cluster, img_names).  Returns the device's outputs for the whole call: "out_off", "out_src",
    "out_cls", "n_out" [n_scene], "status" [n_scene]; source rows are numbered across scenes; a scene with a status has no track."""
    off, src, cls, n_out, status = [0], [], [], [], []
    base = 0
    for tracks, labels, n_cluster, img_names in scenes:
        st, out = assemble_scene(tracks, labels, n_cluster, img_names, cap)
        if st:
            out = []
        for c, rows in out:
            cls.append(c)
            src.append(rows + base)
            off.append(off[-1] + len(rows))
        n_out.append(len(out))
        status.append(st)
        base += sum(len(t) for t in tracks)
    return {"out_off": np.asarray(off, np.int32), "out_src": np.concatenate(src).astype(np.int32) if src else np.zeros(0, np.int32),
            "out_cls": np.asarray(cls, np.int32), "n_out": np.asarray(n_out, np.int32), "status": np.asarray(status, np.int32)}


def synth_tracks(seed, n_tracks, n_img, n_cluster, max_rows=40, width=82, big=None):
    """A seeded scene for the assembly: tracks of 1..max_rows rows over n_img images whose frame ids are shuffled and not contiguous,
    some rows on frames that name no image, sofa / chair labels mixed inside tracks, cluster 0 holding only frames outside img_names
    (a cluster with no row), tracks 1 and 2 of equal length in one cluster.  big = (members, rows): cluster 1 gets that many extra
    tracks of that many rows.  Returns (tracks, labels int32 [n], n_cluster, img_names)."""
    rs = np.random.RandomState(seed)
    img_names = [int(v) for v in rs.permutation(np.arange(n_img) * 3 + 7)]
    outside = np.arange(n_img) * 3 + 8                 # ids between the images' ids: they name no image
    labels = rs.randint(1, n_cluster, n_tracks).astype(np.int32)
    labels[:n_cluster] = np.arange(n_cluster)          # every label occurs
    lengths = rs.randint(1, max_rows + 1, n_tracks)
    if n_tracks >= n_cluster + 3:
        e = n_cluster
        labels[e] = labels[e + 1] = labels[e + 2] = 1
        lengths[e] = lengths[e + 1] = min(max_rows, n_img)   # equal-length members, the longest: the first in track order wins
    lengths = np.minimum(lengths, n_img)
    tracks = []
    for t in range(n_tracks):
        k = int(lengths[t])
        tr = rs.uniform(-1, 1, (k, width))
        if labels[t] == 0:
            tr[:, 0] = rs.choice(outside, k, replace=False)
        else:
            tr[:, 0] = rs.choice(img_names, k, replace=False)
            out = rs.uniform(size=k) < 0.15
            tr[out, 0] = rs.choice(outside, k, replace=False)[out]
        tr[:, 1] = rs.choice([4, 5], k) if t % 2 else rs.randint(0, 8)
        tracks.append(tr)
    if big is not None:
        for _ in range(big[0]):
            tr = rs.uniform(-1, 1, (big[1], width))
            tr[:, 0] = rs.choice(img_names, big[1], replace=False)
            tr[:, 1] = rs.choice([4, 5], big[1])
            tracks.append(tr)
        labels = np.concatenate([labels, np.full(big[0], 1, np.int32)])
    return tracks, labels, n_cluster, img_names
