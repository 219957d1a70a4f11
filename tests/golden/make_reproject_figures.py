#!/usr/bin/env python3
"""The CPU figures of tests/golden/reproject.md: the numpy restatement of the reprojection kernels (tests/reproject_ref.py) against
the reference-run fixtures that already exist (sq_steps.npz, quadric_svd.npz, dq_fits.npz).  No new fixture, no GPU.
   python tests/golden/make_reproject_figures.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import quadric_svd_ref as S      # noqa: E402
import reproject_ref as R        # noqa: E402

STEPS = (0, 100, 199)


def sq_steps_rows(z):
    """(case, step, restated loss_2d, the reference's logged loss_2d, fewest valid points in a view)"""
    for c in range(int(z["n_cases"])):
        P, tgt, mask = z[f"c{c}_P"], z[f"c{c}_tgt"], z[f"c{c}_mask"]
        for k in STEPS:
            r = R.reproject(z[f"c{c}_pts{k}"][None], [len(P)], P)
            s = R.reprojection_score(r["ext"], r["n_valid"] == 0, [len(P)], tgt, mask, 1e9, 1e9)
            yield c, k, s["loss_2d"][0], z[f"c{c}_l2d"][k], int(r["n_valid"].min())


def main():
    g = lambda n: np.load(os.path.join(HERE, n))
    z = g("sq_steps.npz")
    worst = 0.0
    for c, k, ours, ref, nv in sq_steps_rows(z):
        rel = abs(float(ours) - float(ref)) / abs(float(ref))
        worst = max(worst, rel)
        print("sq_steps case %d step %3d: loss_2d %.9g  reference %.9g  rel %.3e (%.2f float32 ulp)  fewest valid points %d"
              % (c, k, ours, ref, rel, rel / 2.0 ** -24 / 2, nv))
    print("1. sq_steps: worst relative deviation of the restated loss_2d %.3e" % worst)
    z = g("quadric_svd.npz")
    kind = z["kind"].astype(int)
    w_exact, w_bbox = 0.0, 0.0
    for i in range(int(z["n_obj"])):
        P, edges = R.svd_track_views(z, i)
        ext, st = R.reproject_dq_one(z["gt_Q"][i], P)
        dev = np.abs(ext - edges).max(axis=0).max()
        w_bbox = max(w_bbox, np.abs(ext - R.get_bbox_rows(z["gt_Q"][i], P)).max())
        if np.isfinite(z["ref_Q"][i]).all():
            e2, s2 = R.reproject_dq_one(z["ref_Q"][i], P)
            ok = s2 == 0
            w_bbox = max(w_bbox, np.abs(e2[ok] - R.get_bbox_rows(z["ref_Q"][i], P[ok])).max()) if ok.any() else w_bbox
        if kind[i] in (S.KIND_EXACT, S.KIND_TWO_VIEWS):
            assert (st == 0).all()
            w_exact = max(w_exact, dev)
        print("quadric_svd object %2d kind %d, %3d views: box of gt_Q vs the track's edges %.3e px" % (i, kind[i], len(P), dev))
    print("2. quadric_svd: exact objects (kind 0 and 3) worst %.3e px" % w_exact)
    d = g("dq_fits.npz")
    for c in range(int(d["n_cases"])):
        Q, P = d[f"c{c}_Q"], d[f"c{c}_P"]
        ext, st = R.reproject_dq_one(Q, P)
        assert (st == 0).all()
        w_bbox = max(w_bbox, np.abs(ext - R.get_bbox_rows(Q, P)).max())
    print("3. restatement vs sq.DualQuadric.get_bbox over dq_fits (float32 Q cast up) and quadric_svd (float64 Q): worst %.3e px" % w_bbox)


if __name__ == "__main__":
    main()
