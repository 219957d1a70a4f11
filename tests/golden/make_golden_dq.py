"""Golden vectors of the reference's dual-quadric model: QuadricOptimizer / DualQuadric (likojack/ODAM
src/super_quadric/sq_libs.py:39-348), IMPORTED here at generation time only (refenv.py; nothing of it is copied).

dq_fits.npz, per problem c<i>_ (12 synthetic problems of 10 ... 300 views, edges near the image border masked by the
generator of the problems and a few more dropped at random):
  init5, half_dims, P, tgt, mask     the inputs in the layout of odam_dq_fit_batch
  p_after [6, 5]                     the reference's parameters after steps 1, 2, 5, 20, 100, 500 (STEPS)
  loss [500]                         its loss_2d log
  tf_p, tf_m, tf_v, tf_g [2, 5]      before steps 1 and 100: parameters, Adam moments, autograd gradient (teacher forcing)
  Q [4, 4], points [2500, 3], bbox_qc [8, 3], srt_scale / srt_R / srt_t, is_ellipsoid, bbox2d [F', 4]
                                     final DualQuadric: matrix, compute_ellipsoid_points, compute_oriented_bbox, get_srt,
                                     get_bbox(P, False, False) of the first views
  n_final [8, 5], n_Q, n_bbox_qc     the same fit re-run with its initial state moved by 1 - 2 float32 ulps (NUDGES)
and one optim_process-level case op_* on the scene of sq_optim.npz: the driver of src/scripts/run_multi_view.py:44-69 with
QuadricOptimizer in the place of SuperQuadricOptimizer (500 steps, n_views = 10): Q per object, fitted flags, bboxes_qc,
bboxes_dl, final parameters; op_n_final / op_n_bboxes_qc: the same with every fit's initial state moved by NUDGES[k].
Also prints the reference's objects per second (one CPU thread per fit), which DESIGN quotes.
Run: python tests/golden/make_golden_dq.py
"""
import os
import sys
import time
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

CASES = [(10, 500), (12, 501), (16, 502), (24, 503), (40, 504), (64, 505), (65, 506), (100, 507), (128, 508), (200, 509),
         (256, 510), (300, 511)]
STEPS = (1, 2, 5, 20, 100, 500)
TF_STEPS = (1, 100)
# (which, ulps): which = 0..2 a translate component, 3 = all three translate components, 4 = yaw
NUDGES = [(0, 1), (0, -1), (1, 1), (2, -1), (3, 2), (3, -2), (4, 1), (4, -1)]


def _ulps(x, n):
    x = np.float32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, np.float32(np.inf if n > 0 else -np.inf))
    return x


def problem(F, seed):
    """synthetic problem + a few more dropped edges -> translate, angle (float32), dims, bbox_lines, P"""
    from odam_amd import synth
    prob = synth.make_sq_problem(F, seed)
    rs = np.random.RandomState(seed + 7)
    for d in prob["bbox_lines"]:
        for name in list(d):
            if len(d) > 1 and rs.uniform() < 0.08:
                del d[name]
    return prob


def _ref():
    import torch
    torch.set_num_threads(1)
    import refenv
    refenv.setup()
    import src.super_quadric.sq_libs as L
    import src.utils.box_utils as bu
    L.print = lambda *a, **k: None          # run() prints the loss every step
    return L, bu


def _params(opt):
    return np.concatenate([opt.translate.detach().numpy(), [opt.quat.item()], [opt.scale_factor.item()]]).astype(np.float32)


def _one(job):
    ci, F, seed, k = job
    L, bu = _ref()
    prob = problem(F, seed)
    t = np.asarray(prob["translate"], np.float32).copy()
    ang = np.float32(prob["angle"])
    if k >= 0:
        which, n = NUDGES[k]
        if which < 3:
            t[which] = _ulps(t[which], n)
        elif which == 3:
            t = np.array([_ulps(v, n) for v in t], np.float32)
        else:
            ang = _ulps(ang, n)
    opt = L.QuadricOptimizer(t, ang, prob["dims"])
    rec = dict(p_after=[], tf_p=[], tf_m=[], tf_v=[], tf_g=[])
    tensors = [opt.translate, opt.quat, opt.scale_factor]
    real_step = opt.optimizer.step
    count = [0]

    def step():
        count[0] += 1
        if k < 0 and count[0] in TF_STEPS:
            st = opt.optimizer.state
            flat = lambda xs: np.concatenate([np.asarray(x, np.float32).reshape(-1) for x in xs])
            rec["tf_p"].append(_params(opt))
            rec["tf_g"].append(flat([x.grad.numpy() for x in tensors]))
            rec["tf_m"].append(flat([st[x]["exp_avg"].numpy() if x in st and "exp_avg" in st[x] else np.zeros(x.numel()) for x in tensors]))
            rec["tf_v"].append(flat([st[x]["exp_avg_sq"].numpy() if x in st and "exp_avg_sq" in st[x] else np.zeros(x.numel()) for x in tensors]))
        real_step()
        if count[0] in STEPS:
            rec["p_after"].append(_params(opt))
    opt.optimizer.step = step
    t0 = time.time()
    Qw = opt.run(prob["bbox_lines"], prob["P"])
    dt = time.time() - t0
    pts, is_ell = Qw.compute_ellipsoid_points()
    out = dict(final=_params(opt), Q=np.asarray(Qw.Q, np.float32), bbox_qc=np.asarray(bu.compute_oriented_bbox(pts), np.float64), seconds=dt)
    if k < 0:
        scale, R, t_wo, _ = Qw.get_srt()
        nb = min(F, 8)
        out.update(points=pts, is_ellipsoid=bool(is_ell), srt_scale=np.asarray(scale), srt_R=np.asarray(R), srt_t=np.asarray(t_wo),
                   bbox2d=np.stack([Qw.get_bbox(prob["P"][f], False, False) for f in range(nb)]),
                   loss=np.asarray([float(l[0]) for l in opt.loss_log], np.float32),
                   **{kk: np.asarray(v, np.float32) for kk, v in rec.items()})
    return ci, k, out


def _scene_case(k):
    """run_multi_view.py:44-69 with QuadricOptimizer; k >= 0: the initial state of every fit moved by NUDGES[k]"""
    L, bu = _ref()
    from scipy.spatial.transform import Rotation
    import src.utils.tracking_gt_utils as tg
    from make_golden import SCENE
    from odam_amd import synth
    sc = synth.make_scene(**SCENE)
    Qs, fitted, qc, dl, finals = [], [], [], [], []
    for track in sc["tracks"]:
        _, bboxes_lines, _, _, T_wos, scales, _ = tg.load_pred_object(track, sc["img_names"], sc["T_wcs"], sc["img_h"], sc["img_w"], sc["K"])
        T_wo = tg.averaging_T_wos(T_wos)
        scales = np.mean(np.asarray([s for s in scales if len(s) > 0]), axis=0)
        bbox_pred = bu.get_3d_box(scales, T_wo[:3, :3], T_wo[:3, 3])
        dl.append(bbox_pred)
        valid = [i for i, _ in enumerate(sc["img_names"]) if len(bboxes_lines[i]) > 0]
        lines = [b for b in bboxes_lines if len(b) > 0]
        t = np.asarray(T_wo[:3, 3], np.float32)
        ang = np.float32(Rotation.from_matrix(T_wo[:3, :3]).as_euler("zxy")[0])
        if k >= 0:
            which, n = NUDGES[k]
            if which < 3:
                t[which] = _ulps(t[which], n)
            elif which == 3:
                t = np.array([_ulps(v, n) for v in t], np.float32)
            else:
                ang = _ulps(ang, n)
        opt = L.QuadricOptimizer(t, ang, scales)      # (the float32 rounding above is what its torch.tensor(..., float32) does)
        if len(valid) < 10:
            Qs.append(np.asarray(opt.Q_init.Q, np.float32)); qc.append(bbox_pred); fitted.append(False)
        else:
            Qw = opt.run(lines, np.asarray(sc["P_cws"])[valid])
            pts, _ = Qw.compute_ellipsoid_points(use_numpy=True)
            Qs.append(np.asarray(Qw.Q, np.float32)); qc.append(bu.compute_oriented_bbox(pts)); fitted.append(True)
        finals.append(_params(opt))
    if k >= 0:
        return k, np.stack(finals), np.asarray(qc, np.float64)
    return dict(op_Q=np.stack(Qs), op_fitted=np.asarray(fitted), op_bboxes_qc=np.asarray(qc, np.float64),
                op_bboxes_dl=np.asarray(dl, np.float64), op_final=np.stack(finals))


def main():
    from odam_amd import sq
    import refenv
    refenv.setup()          # builds the reference's sampler binding once, before the workers look for it
    jobs = [(ci, F, seed, k) for ci, (F, seed) in enumerate(CASES) for k in range(-1, len(NUDGES))]
    jobs.sort(key=lambda j: -j[1])
    with Pool(7) as pool:
        scene = pool.map_async(_scene_case, list(range(-1, len(NUDGES))), chunksize=1)
        res = pool.map(_one, jobs, chunksize=1)
        sres = scene.get()
    data = sres[0]
    data["op_n_final"] = np.stack([r[1] for r in sorted(sres[1:], key=lambda r: r[0])])
    data["op_n_bboxes_qc"] = np.stack([r[2] for r in sorted(sres[1:], key=lambda r: r[0])])
    n = len(CASES)
    data.update(n_cases=np.int32(n), views=np.asarray([c[0] for c in CASES], np.int32), steps=np.asarray(STEPS, np.int32),
                tf_steps=np.asarray(TF_STEPS, np.int32), nudges=np.asarray(NUDGES, np.int32))
    secs = []
    for ci, (F, seed) in enumerate(CASES):
        prob = problem(F, seed)
        tgt, mask = sq.lines_to_targets(prob["bbox_lines"])
        pre = f"c{ci}_"
        data[pre + "init5"] = np.concatenate([np.asarray(prob["translate"], np.float32), [np.float32(prob["angle"])], [np.float32(1)]]).astype(np.float32)
        data[pre + "half_dims"] = (np.asarray(prob["dims"], np.float64) / 2).astype(np.float32)      # sq_libs.py:56-58
        data[pre + "P"] = prob["P"].astype(np.float32).reshape(-1, 12)
        data[pre + "tgt"] = tgt
        data[pre + "mask"] = mask
        data[pre + "n_final"] = np.zeros((len(NUDGES), 5), np.float32)
        data[pre + "n_Q"] = np.zeros((len(NUDGES), 4, 4), np.float32)
        data[pre + "n_bbox_qc"] = np.zeros((len(NUDGES), 8, 3))
    for ci, k, out in res:
        pre = f"c{ci}_"
        secs.append(out.pop("seconds"))
        if k < 0:
            for kk, v in out.items():
                data[pre + kk] = v
        else:
            data[pre + "n_final"][k] = out["final"]
            data[pre + "n_Q"][k] = out["Q"]
            data[pre + "n_bbox_qc"][k] = out["bbox_qc"]
    np.savez_compressed(os.path.join(HERE, "dq_fits.npz"), **data)
    print("dq_fits.npz: %d problems, %d fits of 500 steps; reference %.2f s per object (median, one thread) = %.2f objects/s" % (
        n, len(res), float(np.median(secs)), 1.0 / float(np.median(secs))))
    print("masked edges per problem:", [int((data[f"c{ci}_mask"] == 0).sum()) for ci in range(n)])


if __name__ == "__main__":
    main()
