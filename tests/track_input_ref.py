"""High-precision restatement of the projected extent of a track's surface (OdamProcess._prepare_tracks, odam_amd/processor.py:385-391;
reference src/processor.py:181-207): what odam_sq_project_extents computes on the device and what becomes channels 2..5 of every
track row the association network sees.

    cam = [x y z 1] @ T_cw[:3].T        q = cam @ K.T        (u, v) = (q_0, q_1) / q_2        extent = min / max over the 1000 points

extents() evaluates it in numpy.longdouble (64-bit mantissa on x86) from the float32 surface points and returns, with the four
extents, every point's (u, v) and a bound on what a float64 evaluation of the same formula may differ from it by:

    S_k = |x T_k0| + |y T_k1| + |z T_k2| + |T_k3|          (the size of the terms of cam_k)
    A_j = sum_k |K_jk| S_k                                  (the size of the terms of q_j)
    B_u = 16 eps (A_0 + |u| A_2) / |q_2|     B_v = 16 eps (A_1 + |v| A_2) / |q_2|     eps = 2^-53

First order: cam_k carries at most 4 eps S_k (three products, three additions, in any order, fused or not), q_j at most
3 eps A_j of its own plus 4 eps A_j inherited: |dq_j| <= 7 eps A_j; u = q_0 / q_2 moves by (|dq_0| + |u| |dq_2|) / |q_2| and by
eps |u| <= eps |u| A_2 / |q_2| for the division: 8 eps (A_0 + |u| A_2) / |q_2|, doubled for the second-order terms.  The
constant is this derivation, not a measurement.

extents_f64() is the float64 numpy code of the processor's host path, operation for operation."""
import numpy as np

EPS = 2.0 ** -53
LD = np.longdouble


def extents(points_f32, T_cw, K):
    """points_f32 [n, P, 3] float32; T_cw [4, 4] or [3, 4]; K [3, 3] -> dict of
    ext [n, 4] longdouble (u_min, v_min, u_max, v_max), arg [n, 4] int (the point that attains each), uv [n, P, 2] longdouble,
    bound [n, P, 2] float64 (B_u, B_v per point), depth [n, P] float64 (q_2)"""
    p = np.asarray(points_f32)
    assert p.dtype == np.float32 and p.ndim == 3 and p.shape[2] == 3
    p = p.astype(LD)
    T = np.asarray(T_cw, np.float64)[:3].astype(LD)
    Kl = np.asarray(K, np.float64)[:3, :3].astype(LD)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    cam = [x * T[k, 0] + y * T[k, 1] + z * T[k, 2] + T[k, 3] for k in range(3)]
    S = [np.abs(x * T[k, 0]) + np.abs(y * T[k, 1]) + np.abs(z * T[k, 2]) + np.abs(T[k, 3]) for k in range(3)]
    q = [cam[0] * Kl[j, 0] + cam[1] * Kl[j, 1] + cam[2] * Kl[j, 2] for j in range(3)]
    A = [S[0] * np.abs(Kl[j, 0]) + S[1] * np.abs(Kl[j, 1]) + S[2] * np.abs(Kl[j, 2]) for j in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = q[0] / q[2], q[1] / q[2]
        Bu = 16 * EPS * (A[0] + np.abs(u) * A[2]) / np.abs(q[2])
        Bv = 16 * EPS * (A[1] + np.abs(v) * A[2]) / np.abs(q[2])
    uv = np.stack([u, v], axis=-1)
    arg = np.stack([u.argmin(1), v.argmin(1), u.argmax(1), v.argmax(1)], axis=1)
    ext = np.stack([u.min(1), v.min(1), u.max(1), v.max(1)], axis=1)
    return {"ext": ext, "arg": arg, "uv": uv, "bound": np.stack([Bu, Bv], axis=-1).astype(np.float64), "depth": q[2].astype(np.float64)}


def extents_f64(points_f32, T_cw, K):
    """the host path of OdamProcess._prepare_tracks (odam_amd/processor.py:385-391) on points [n, P, 3]: float64 numpy -> [n, 4]"""
    pts_all = np.asarray(points_f32)
    T_cw = np.asarray(T_cw, np.float64)
    cam = (np.concatenate([pts_all, np.ones_like(pts_all[..., 2:])], axis=2) @ T_cw.T)[..., :3]
    pix = cam @ np.asarray(K, np.float64).T
    with np.errstate(divide="ignore", invalid="ignore"):
        pix = np.ascontiguousarray((pix / pix[..., -1:]).transpose(0, 2, 1))
    lo, hi = pix.min(axis=2), pix.max(axis=2)
    return np.concatenate([lo[:, :2], hi[:, :2]], axis=1)
