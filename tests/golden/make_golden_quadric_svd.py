"""Golden vectors of the reference's closed-form dual quadric: compute_quadric_svd (likojack/ODAM src/super_quadric/sq_libs.py:30-36)
over the plane vectors of load_pred_object (src/utils/tracking_gt_utils.py:198-205), unpacked by quadric_2mat
(src/super_quadric/quadric_helper.py:16-36) -- IMPORTED here at generation time only (refenv.py; nothing of it is copied).

quadric_svd.npz (float64 arrays only):
  K [3, 3], T_wcs [300, 4, 4], P_cws [300, 3, 4] (= K @ inv(T_wc)[:3]), img_names [300], img_hw [2]   one ring of cameras at ~2.5 m
  n_obj, track<i> [n_obs, 82]     one track per object in the 82-column layout (columns 2..5: the box x_min, y_min, x_max, y_max)
  views, noise_px, kind [n_obj]   kind: 0 exact edges, 1 the same object with 1 px Gaussian noise on every edge, 2 exact with some
                                  edges inside the 20 px border band, 3 two views only, 4 noisy and not an ellipsoid (seed searched)
  gt_Q [n_obj, 4, 4]              the ellipsoid the boxes were drawn from, normalised (Q[3,3] = -1)
  ref_vec [n_obj, 10]             the reference's compute_quadric_svd(plane_vecs of load_pred_object)
  ref_Q [n_obj, 4, 4]             its quadric_2mat, normalised Q <- -Q / Q[3,3]
  ref_is_ellipsoid [n_obj]        DualQuadric(ref_Q).get_srt()[3] of the reference
  status1_seed                    the seed the kind-4 search stopped at
and writes quadric_svd.md: per problem the restatement's (tests/quadric_svd_ref.py) deviation from the reference's result in units
of u = 2^-52 lambda_10 / (lambda_2 - lambda_1), whose worst value is the RATIO the tests' tolerance is built from.
Run: python tests/golden/make_golden_quadric_svd.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402

N_CAM = 300
IMG_H, IMG_W = 480, 640
VIEWS = (3, 4, 10, 64, 65, 129, 300)
EXACT, NOISY, MASKED, TWO_VIEWS, NOT_ELLIPSOID = range(5)


def cameras():
    from odam_amd import synth
    rs = np.random.RandomState(2024)
    T = []
    for i in range(N_CAM):
        ang = 2 * np.pi * i / N_CAM
        eye = np.array([2.5 * np.cos(ang), 2.5 * np.sin(ang), 1.3 + 0.2 * np.sin(2 * ang)])
        T.append(synth.look_at(eye, np.array([0.0, 0.0, 0.5]) + rs.normal(0, 0.03, 3)))
    return np.asarray(T), synth.K_SCANNET.copy()


def ellipsoid(rs, semi=(0.4, 0.25, 0.5)):
    a = np.asarray(semi) * rs.uniform(0.8, 1.2, 3)
    yaw = rs.uniform(-np.pi, np.pi)
    t = np.array([rs.uniform(-0.2, 0.2), rs.uniform(-0.2, 0.2), 0.5 + rs.uniform(-0.1, 0.1)])
    c, s = np.cos(yaw), np.sin(yaw)
    T = np.eye(4)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:3, 3] = t
    return T @ np.diag([a[0] ** 2, a[1] ** 2, a[2] ** 2, -1.0]) @ T.T, a, yaw, t


def exact_box(Q, P):
    """tangent lines of the conic C = P Q P^T: x_min, y_min, x_max, y_max"""
    C = P @ Q @ P.T
    bx = np.sqrt(C[0, 2] ** 2 - C[0, 0] * C[2, 2])
    by = np.sqrt(C[1, 2] ** 2 - C[1, 1] * C[2, 2])
    xs = sorted([(C[0, 2] + bx) / C[2, 2], (C[0, 2] - bx) / C[2, 2]])
    ys = sorted([(C[1, 2] + by) / C[2, 2], (C[1, 2] - by) / C[2, 2]])
    return np.array([xs[0], ys[0], xs[1], ys[1]])


def make_track(Q, a, yaw, t, frames, img_names, P_cws, noise, rs, clip=False):
    rows = []
    for i in frames:
        bb = exact_box(Q, P_cws[i])
        if noise:
            bb = bb + rs.normal(0, noise, 4)
        if clip:
            bb = np.clip(bb, [0, 0, 0, 0], [IMG_W, IMG_H, IMG_W, IMG_H])
        row = -np.ones(82)
        row[0] = img_names[i]
        row[1] = 5
        row[2:6] = bb
        row[6:9] = 2 * a * rs.uniform(0.9, 1.1, 3)
        row[9:12] = t + rs.normal(0, 0.05, 3)
        row[12] = yaw + rs.normal(0, 0.08)
        row[13] = rs.uniform(0.8, 1.0)
        row[78:82] = bb
        rows.append(row)
    return np.asarray(rows)


def spread(F, start):
    return sorted({(start + (j * N_CAM) // F) % N_CAM for j in range(F)})


def reference(track, img_names, T_wcs, K):
    import refenv
    refenv.setup()
    import src.super_quadric.quadric_helper as helper
    import src.super_quadric.sq_libs as L
    import src.utils.tracking_gt_utils as tg
    _, _, plane_vecs, _, _, _, _ = tg.load_pred_object(track, img_names, list(T_wcs), IMG_H, IMG_W, K)
    vec = L.compute_quadric_svd([np.asarray(pv) for pv in plane_vecs if len(pv) > 0])
    vec = np.real(np.asarray(vec)).astype(np.float64)
    Q = helper.quadric_2mat(vec)
    Q = -Q / Q[3, 3]
    return vec, Q, bool(L.DualQuadric(Q).get_srt()[3])


def main():
    import quadric_svd_ref as R
    T_wcs, K = cameras()
    P_cws = np.stack([K @ np.linalg.inv(T)[:3, :] for T in T_wcs])
    img_names = [3 * i + 1 for i in range(N_CAM)]
    tracks, views, noise_px, kind, gt = [], [], [], [], []

    def add(track, Q, k, noise):
        tracks.append(track); views.append(len(track)); noise_px.append(noise); kind.append(k); gt.append(-Q / Q[3, 3])

    for n, F in enumerate(VIEWS):
        rs = np.random.RandomState(100 + n)
        Q, a, yaw, t = ellipsoid(rs)
        frames = spread(F, int(rs.randint(0, N_CAM)))
        add(make_track(Q, a, yaw, t, frames, img_names, P_cws, 0.0, rs), Q, EXACT, 0.0)
        add(make_track(Q, a, yaw, t, frames, img_names, P_cws, 1.0, rs), Q, NOISY, 1.0)
    # a tall object: its top and bottom edges fall inside the border band in some views
    rs = np.random.RandomState(300)
    Q, a, yaw, t = ellipsoid(rs, semi=(0.45, 0.3, 0.93))
    add(make_track(Q, a, yaw, t, spread(12, 7), img_names, P_cws, 0.0, rs, clip=True), Q, MASKED, 0.0)
    vals = tracks[-1][:, [2, 4, 3, 5]]
    m = (vals > 20) & (vals < np.array([IMG_W, IMG_W, IMG_H, IMG_H]) - 20)
    assert 0 < (~m).sum() < m.size and m.any(axis=1).all() and m.sum() >= 9, m
    print("masked object: %d of %d edges masked" % ((~m).sum(), m.size))
    rs = np.random.RandomState(301)
    Q, a, yaw, t = ellipsoid(rs)
    add(make_track(Q, a, yaw, t, [40, 140], img_names, P_cws, 0.0, rs), Q, TWO_VIEWS, 0.0)
    # three nearby views with 1 px noise: search the seed at which the reference's own result is not an ellipsoid
    seed = 1000
    while True:
        rs = np.random.RandomState(seed)
        Q, a, yaw, t = ellipsoid(rs)
        tr = make_track(Q, a, yaw, t, [10, 22, 34], img_names, P_cws, 1.0, rs)
        if not reference(tr, img_names, T_wcs, K)[2]:
            break
        seed += 1
    print("status-1 case: seed", seed)
    add(tr, Q, NOT_ELLIPSOID, 1.0)

    refs = [reference(tr, img_names, T_wcs, K) for tr in tracks]
    data = dict(K=K, T_wcs=T_wcs, P_cws=P_cws, img_names=np.asarray(img_names, np.float64), img_hw=np.array([IMG_H, IMG_W], np.float64),
                n_obj=np.float64(len(tracks)), views=np.asarray(views, np.float64), noise_px=np.asarray(noise_px),
                kind=np.asarray(kind, np.float64), gt_Q=np.stack(gt), ref_vec=np.stack([r[0] for r in refs]),
                ref_Q=np.stack([r[1] for r in refs]), ref_is_ellipsoid=np.asarray([float(r[2]) for r in refs]),
                status1_seed=np.float64(seed))
    for i, tr in enumerate(tracks):
        data[f"track{i}"] = tr
    out = os.path.join(HERE, "quadric_svd.npz")
    np.savez_compressed(out, **data)
    print("quadric_svd.npz: %d objects, %d bytes" % (len(tracks), os.path.getsize(out)))

    # the tolerance table
    z = np.load(out)
    lines, worst = [], 0.0
    for i in range(len(tracks)):
        P, e, msk = R.track_rows(z, i)
        Qr, eig, st, _ = R.solve_one(P, e, msk)
        if st == 2:
            lines.append("| %2d | %d | %3d | %.0f | 2 | - | - | - | - | - |" % (i, kind[i], views[i], noise_px[i]))
            continue
        u = R.scale_u(eig)
        err = R.q_err(Qr, refs[i][1])
        egt = R.q_err(Qr, gt[i])
        worst = max(worst, err / u)
        lines.append("| %2d | %d | %3d | %.0f | %d | %.3e | %.3e | %.3e | %.3f | %.3e |" % (
            i, kind[i], views[i], noise_px[i], st, (eig[1] - eig[0]) / eig[2], u, err, err / u, egt))
        assert (st == 0) == refs[i][2], i
    md = MD % dict(table="\n".join(lines), worst=worst, seed=seed)
    with open(os.path.join(HERE, "quadric_svd.md"), "w") as f:
        f.write(md)
    print(md)


MD = """# quadric_svd.npz: the closed-form dual quadric, restatement against the reference

Written by `make_golden_quadric_svd.py` together with the fixture.  Per problem: the restatement `tests/quadric_svd_ref.py`
(rows and Gram matrix in the kernel's order, `numpy.linalg.eigh`) against the reference's stored result (`Sigma.T @ Sigma` by the
host BLAS, `numpy.linalg.eig`), as `err = max|Q_a - Q_b| / max|Q_b|` on the normalised matrices, in units of the problem's
natural scale `u = 2^-52 * lambda_10 / (lambda_2 - lambda_1)`.  `err vs truth` is the restatement against the ellipsoid the
boxes were drawn from (meaningful for exact edges: kinds 0 and 2).

kind: 0 exact edges, 1 the same with 1 px noise, 2 exact with masked edges, 3 two views (status 2), 4 noisy, not an ellipsoid
(seed %(seed)d).

| object | kind | views | noise px | status | (l2 - l1) / l10 | u | err vs reference | err / u | err vs truth |
|---|---|---|---|---|---|---|---|---|---|
%(table)s

Worst err / u over the fixture: **%(worst).3f**.  This is `RATIO` in `tests/quadric_svd_ref.py`; the tests allow
`8 * RATIO * u` per problem for device against restatement, device against reference and, on the exact-edge problems, against
the ground truth (the margin covers a third backward-stable algorithm, the device's Jacobi, and nothing else).
"""


if __name__ == "__main__":
    main()
