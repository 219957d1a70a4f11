"""The device track merge without a device: tests/merge_ref.py (the numpy restatement of csrc/track_merge.hip) against scipy, sklearn
and odam_amd.merge._merge_cluster themselves, and the two entry points' argument checks and ctypes signatures.  CPU only."""
import ctypes
import os
import re

import numpy as np
import pytest

import merge_ref as R
from conftest import REPO


def _seeded_cost(rs, n, frac_one, quarters):
    c = rs.uniform(0.3, 1.0, (n, n))
    c[rs.uniform(size=(n, n)) < frac_one] = 1.0
    if quarters:
        c = np.round(c * 4) / 4      # ties below the threshold too
    c = np.triu(c, 1)
    return c + c.T


def _cases():
    rs = np.random.RandomState(0)
    k = 0
    for n in range(2, 61):
        for frac in (0.3, 0.7, 0.95):
            yield n, _seeded_cost(rs, n, frac, k % 4 == 0)
            k += 1


def test_linkage_equals_scipy_bit_for_bit():
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform
    n_cases = 0
    for n, c in _cases():
        want = linkage(squareform(c, checks=False), "average")
        got = R.linkage_average(c)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), n
        n_cases += 1
    assert n_cases == 59 * 3


def test_labels_equal_sklearn():
    from sklearn.cluster import AgglomerativeClustering
    seen_clusters = set()
    for n, c in _cases():
        want = AgglomerativeClustering(n_clusters=None, distance_threshold=0.95, metric="precomputed", linkage="average").fit(c).labels_
        got, n_cl = R.labels_from_linkage(R.linkage_average(c), n, 0.95)
        assert np.array_equal(got, want), n
        assert n_cl == want.max() + 1
        seen_clusters.add(n_cl)
    assert 1 in seen_clusters and max(seen_clusters) > 20


def test_cost_from_iou_reads_the_upper_triangle_only():
    from odam_amd import merge
    rs = np.random.RandomState(1)
    iou = rs.uniform(0, 1, (7, 7))      # not symmetric
    c = R.cost_from_iou(iou)
    assert np.array_equal(c, c.T) and (np.diag(c) == 0).all() and np.array_equal(np.triu(c, 1), np.triu(1 - iou, 1))
    assert merge.cost_matrix.__doc__ and "upper triangle" in merge.cost_matrix.__doc__


def _host_merge(tracks, labels, img_names):
    from odam_amd import merge
    out = [merge._merge_cluster(tracks, labels == c, img_names) for c in np.unique(labels)]
    return [t for t in out if len(t) > 0]


def _ref_merge(tracks, labels, n_cluster, img_names):
    st, out = R.assemble_scene(tracks, labels, n_cluster, img_names)
    assert st == 0
    allrows = np.concatenate(tracks)
    merged = []
    for cls, src in out:
        t = allrows[src]
        t[:, 1] = cls
        merged.append(t)
    return merged


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x, y)


def test_assembly_equals_merge_cluster_on_the_golden(golden):
    from sklearn.cluster import AgglomerativeClustering
    from odam_amd import merge
    z = golden("sq_merge.npz")
    tracks = [z[f"track{i}"].copy() for i in range(int(z["n_tracks"]))]
    img_names = [int(x) for x in z["img_names"]]
    cost = merge.cost_matrix(tracks, list(z["bboxes_qc"]))
    labels = AgglomerativeClustering(n_clusters=None, distance_threshold=0.95, metric="precomputed", linkage="average").fit(cost).labels_
    got_labels, n_cl = R.labels_from_linkage(R.linkage_average(cost), len(tracks), 0.95)
    assert np.array_equal(got_labels, labels)
    got = _ref_merge(tracks, got_labels, n_cl, img_names)
    _same(got, _host_merge(tracks, labels, img_names))
    _same(got, [z[f"merged{i}"] for i in range(int(z["n_merged"]))])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_assembly_equals_merge_cluster_on_seeded_tracks(seed):
    """mixed sofa / chair labels, equal-length members, frames outside img_names, a cluster with no row"""
    tracks, labels, n_cl, img_names = R.synth_tracks(seed, 24, 50, 6)
    e = n_cl
    assert len(tracks[e]) == len(tracks[e + 1]) and labels[e] == labels[e + 1]
    host = _host_merge(tracks, labels, img_names)
    assert len(host) < len(np.unique(labels))      # the cluster whose frames name no image is gone
    assert any(len(np.unique(t[:, 1])) > 1 for t in tracks)
    _same(_ref_merge(tracks, labels, n_cl, img_names), host)


def test_assembly_statuses():
    tracks, labels, n_cl, img_names = R.synth_tracks(3, 12, 30, 4)
    assert R.assemble_scene(tracks, labels, n_cl, img_names)[0] == 0
    t = [x.copy() for x in tracks]
    t[5][0, 1] = 2.5
    assert R.assemble_scene(t, labels, n_cl, img_names)[0] == R.BAD_CLASS
    t = [x.copy() for x in tracks]
    k = next(i for i in range(len(t)) if labels[i] != 0 and len(t[i]) > 1)
    t[k][:2, 0] = img_names[0]
    assert R.assemble_scene(t, labels, n_cl, img_names)[0] == R.REPEATED_FRAME
    assert R.assemble_scene(tracks, labels, n_cl, img_names, cap=8)[0] == R.TOO_MANY_ROWS
    # a frame id that is no integer names no image (the host dict's behaviour, not a truncation)
    t = [x.copy() for x in tracks]
    k = max((i for i in range(len(t)) if labels[i] != 0), key=lambda i: (len(t[i]), -i))      # the longest: its rows win
    t[k][:, 0] += 0.5
    r0 = sum(len(x) for x in t[:k])
    own = lambda out: sum(int(((s >= r0) & (s < r0 + len(t[k]))).sum()) for _, s in out)
    assert own(R.assemble_scene(tracks, labels, n_cl, img_names)[1]) > 0 and own(R.assemble_scene(t, labels, n_cl, img_names)[1]) == 0
    _same(_ref_merge(t, labels, n_cl, img_names), _host_merge(t, labels, img_names))


C_TO_CTYPES = {"int": ctypes.c_int, "double": ctypes.c_double, "long long": ctypes.c_longlong}


def _header_args(txt, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, f"{name} is not declared in include/odam_merge.h"
    names, want = [], []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        names.append(arg.split()[-1].lstrip("*"))
        want.append(ctypes.c_void_p if "*" in arg else C_TO_CTYPES[arg.replace("const ", "").rsplit(" ", 1)[0]])
    return names, want


def test_entry_points_signatures_and_argument_checks():
    """the argument lists odam_amd.sq gives ctypes are the header's; the symbols are exported; null pointers, more than 1024 tracks
    in a scene and a negative scene count are refused before any device work (no GPU here)"""
    from odam_amd import _lib, sq
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "odam_merge.h")).read(), flags=re.S)
    for name in ("odam_merge_cluster", "odam_merge_assemble"):
        names, want = _header_args(txt, name)
        assert sq.MERGE_ARGTYPES[name] == want, name
        assert hasattr(_lib.lib(), name)
        f = sq._merge_entry(name)
        assert list(f.argtypes) == want and f.restype is ctypes.c_int
    for name, value in (("ODAM_MERGE_MAX_TRACKS", sq.MERGE_MAX_TRACKS), ("ODAM_MERGE_BAD_OFFSETS", R.BAD_OFFSETS),
                        ("ODAM_MERGE_BAD_COST", R.BAD_COST), ("ODAM_MERGE_NOT_CLUSTERED", R.NOT_CLUSTERED),
                        ("ODAM_MERGE_BAD_CLASS", R.BAD_CLASS), ("ODAM_MERGE_REPEATED_FRAME", R.REPEATED_FRAME),
                        ("ODAM_MERGE_TOO_MANY_ROWS", R.TOO_MANY_ROWS)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, txt).group(1)) == value, name
    assert R.MAX_TRACKS == sq.MERGE_MAX_TRACKS and R.MAX_CAND == sq.PREPARE_MAX_ROWS
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    L = _lib.lib()
    fc = sq._merge_entry("odam_merge_cluster")
    okc = lambda **kw: [kw.get("ctx", p), kw.get("n_scene", 1), kw.get("a_off", p), p, 2, 4, kw.get("max_tracks", 2), p, 0.95,
                        kw.get("scratch", p), p, p, p, p, None]
    assert fc(*okc(ctx=None)) == 1 and b"odam_merge_cluster" in L.odam_last_error()      # ODAM_E_INVALID
    assert fc(*okc(a_off=None)) == 1 and fc(*okc(scratch=None)) == 1
    assert fc(*okc(n_scene=-1)) == 1
    assert fc(*okc(max_tracks=1025)) == 3 and b"1024" in L.odam_last_error()              # ODAM_E_LIMIT
    assert fc(*okc(n_scene=0)) == 0                                                       # the empty call launches nothing
    fa = sq._merge_entry("odam_merge_assemble")
    oka = lambda **kw: [kw.get("ctx", p), kw.get("n_scene", 1), p, 2, kw.get("labels", p), p, p, p, p, 4, 4, p, p, p, 3, p,
                        kw.get("out_off", p), p, p, None, p, p, p, None]
    assert fa(*oka(ctx=None)) == 1 and b"odam_merge_assemble" in L.odam_last_error()
    assert fa(*oka(labels=None)) == 1 and fa(*oka(out_off=None)) == 1 and fa(*oka(n_scene=-1)) == 1
    assert fa(*oka(n_scene=0)) == 0
