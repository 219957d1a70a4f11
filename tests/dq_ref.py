"""Host restatement of the dual-quadric fit (odam_amd/csrc/dq_core.h, dq_fit.hip) -- two forms.

  * fit32 / grad32: numpy float32 with the kernel's operation order, operation by operation: every fmaf of the kernel is
    fma32 here (exact product in binary64, sum rounded to odd, one rounding to binary32 = the fused result), cosf / sinf are
    the host libm's (which odam_amd/csrc/sq_math.h equals bit for bit, tests/test_sq_math.py), the per-view sums follow the
    kernel's lane partials and butterfly.  tests/test_dq_gpu.py asks the device for these bits.
  * loss64: the same loss written from the reference's formulas (likojack/ODAM src/super_quadric/sq_libs.py:68-78, :123-168)
    in torch float64, differentiated by autograd -- what the closed-form gradient is judged against.
"""
import ctypes
import ctypes.util

import numpy as np

f32 = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("cosf", "sinf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float]


def cosf(x):
    return f32(_libm.cosf(ctypes.c_float(float(x))))


def sinf(x):
    return f32(_libm.sinf(ctypes.c_float(float(x))))


def fma32(a, b, c):
    """fmaf(a, b, c) for float32 operands: a * b is exact in binary64; the sum is rounded to odd there (TwoSum gives the
    error's sign), so the final rounding to binary32 is the correctly rounded fused result."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    shape = a.shape
    a, b, c = a.reshape(-1), b.reshape(-1), c.reshape(-1)
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (s.view(np.int64) & 1) == 0
        fix = (err != 0) & even & np.isfinite(s) & np.isfinite(err)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        out = s.astype(np.float32).reshape(shape)
    return out[()] if out.ndim == 0 else out


def adam_table(n_iters):
    """-(lr / bias_correction1), sqrt(bias_correction2) per step: Python floats, cast at use (torch _single_tensor_adam)."""
    tab = np.zeros((n_iters, 2), np.float32)
    for t in range(1, n_iters + 1):
        bc1 = 1.0 - 0.9 ** float(t)
        bc2 = 1.0 - 0.999 ** float(t)
        tab[t - 1] = (f32(-(0.01 / bc1)), f32(bc2 ** 0.5))
    return tab


def adam_step(p, m, v, g, neg_step, bc2_sqrt):
    """sq_core.h adam_scalar on float32 vectors; returns the new (p, m, v)."""
    w1, w2, b2, eps = f32(1.0 - 0.9), f32(1.0 - 0.999), f32(0.999), f32(1e-8)
    with np.errstate(all="ignore"):
        m = fma32(w1, g - m, m)
        v = v * b2
        v = fma32(w2 * g, g, v)
        denom = np.sqrt(v) / f32(bc2_sqrt) + eps
        p = p + (f32(neg_step) * m) / denom
    return p.astype(np.float32), m, v


def make_obj(p, h):
    p = np.asarray(p, np.float32)
    h = np.asarray(h, np.float32)
    c, s = cosf(p[3]), sinf(p[3])
    sc = p[4] * h
    a = sc * sc
    tx, ty, tz = p[0], p[1], p[2]
    t00, t01, t10, t11 = c * a[0], (-s) * a[1], s * a[0], c * a[1]
    Q = np.zeros(16, np.float32)
    Q[0] = fma32(-tx, tx, fma32(t01, -s, t00 * c))
    Q[1] = fma32(-tx, ty, fma32(t01, c, t00 * s))
    Q[2] = (-tx) * tz
    Q[3] = -tx
    Q[4] = fma32(-ty, tx, fma32(t11, -s, t10 * c))
    Q[5] = fma32(-ty, ty, fma32(t11, c, t10 * s))
    Q[6] = (-ty) * tz
    Q[7] = -ty
    Q[8] = (-tz) * tx
    Q[9] = (-tz) * ty
    Q[10] = fma32(-tz, tz, a[2])
    Q[11] = -tz
    Q[12], Q[13], Q[14], Q[15] = -tx, -ty, -tz, f32(-1.0)
    return dict(c=c, s=s, sc=sc, a=a, Q=Q)


def _dot4(a, b):
    return fma32(a[3], b[3], fma32(a[2], b[2], fma32(a[1], b[1], a[0] * b[0])))


def _sgn(x):
    return np.where(x > 0, f32(1), np.where(x < 0, f32(-1), f32(0))).astype(np.float32)


def _axis(cii, ci2, c22, t_lo, t_hi, m_lo, m_hi, invF, g22):
    z = np.zeros_like(cii)
    D = f32(4) * (ci2 * ci2) - (f32(4) * cii) * c22
    bad = ~(D >= 0)
    b = np.sqrt(np.where(bad, f32(0), D))
    r = f32(0.5) / c22
    s2 = f32(2) * ci2
    u0, u1 = s2 + b, s2 - b
    x0, x1 = r * u0, r * u1
    min0, max0 = ~(x1 < x0), ~(x1 > x0)
    lo, hi = np.where(min0, x0, x1), np.where(max0, x0, x1)
    d_lo, d_hi = lo - t_lo, hi - t_hi
    a_lo, a_hi = np.abs(d_lo), np.abs(d_hi)
    g_lo, g_hi = (_sgn(d_lo) * m_lo) * invF, (_sgn(d_hi) * m_hi) * invF
    n_lo, n_hi = np.isnan(d_lo), np.isnan(d_hi)
    a_lo, g_lo = np.where(n_lo, z, a_lo), np.where(n_lo, z, g_lo)
    a_hi, g_hi = np.where(n_hi, z, a_hi), np.where(n_hi, z, g_hi)
    l_lo, l_hi = np.where(bad, z, a_lo * m_lo), np.where(bad, z, a_hi * m_hi)
    skip = bad | ((g_lo == 0) & (g_hi == 0))
    gx0 = np.where(min0, g_lo, z) + np.where(max0, g_hi, z)
    gx1 = np.where(min0, z, g_lo) + np.where(max0, z, g_hi)
    g_r = gx0 * u0 + gx1 * u1
    g_b = r * (gx0 - gx1)
    g_D = (f32(0.5) * g_b) / b
    gi2 = np.where(skip, z, (f32(2) * r) * (gx0 + gx1) + g_D * (f32(8) * ci2))
    gii = np.where(skip, z, -((f32(4) * c22) * g_D))
    g22 = np.where(skip, g22, g22 + (-(g_r * (r / c22)) - (f32(4) * cii) * g_D))
    return bad, l_lo.astype(np.float32), l_hi.astype(np.float32), gii.astype(np.float32), gi2.astype(np.float32), g22.astype(np.float32)


def view_terms(o, p, h, P, tgt, mask, invF):
    """dq_core.h view_terms for all views at once: l [4][F], g [5][F], bad [F]."""
    M = [np.ascontiguousarray(P[:, k], np.float32) for k in range(12)]
    Q = o["Q"]
    with np.errstate(all="ignore"):
        MQ = [[_dot4(M[4 * i:4 * i + 4], [Q[k], Q[4 + k], Q[8 + k], Q[12 + k]]) for k in range(4)] for i in range(3)]
        c00, c02 = _dot4(MQ[0], M[0:4]), _dot4(MQ[0], M[8:12])
        c11, c12 = _dot4(MQ[1], M[4:8]), _dot4(MQ[1], M[8:12])
        c22 = _dot4(MQ[2], M[8:12])
        t = [np.ascontiguousarray(tgt[:, k], np.float32) for k in range(4)]
        m = [np.ascontiguousarray(mask[:, k], np.float32) for k in range(4)]
        g22 = np.zeros_like(c22)
        badx, l0, l1, g00, g02, g22 = _axis(c00, c02, c22, t[0], t[1], m[0], m[1], invF, g22)
        bady, l2, l3, g11, g12, g22 = _axis(c11, c12, c22, t[2], t[3], m[2], m[3], invF, g22)
        c, s = o["c"], o["s"]
        z, q = [], []
        for i in range(3):
            r = M[4 * i:4 * i + 4]
            z.append(fma32(r[2], p[2], fma32(r[1], p[1], r[0] * p[0])) + r[3])
            q.append([fma32(r[1], s, r[0] * c), fma32(r[1], c, r[0] * (-s)), r[2]])
        two = f32(2)
        e0 = (two * g00) * z[0] + g02 * z[2]
        e1 = (two * g11) * z[1] + g12 * z[2]
        e2 = (g02 * z[0] + g12 * z[1]) + (two * g22) * z[2]
        g = [-((M[k] * e0 + M[4 + k] * e1) + M[8 + k] * e2) for k in range(3)]
        S = [(((g00 * q[0][k]) * q[0][k] + (g02 * q[0][k]) * q[2][k]) + (g22 * q[2][k]) * q[2][k]) +
             ((g11 * q[1][k]) * q[1][k] + (g12 * q[1][k]) * q[2][k]) for k in range(3)]
        X = ((((two * g00) * (q[0][0] * q[0][1]) + g02 * (q[0][0] * q[2][1] + q[0][1] * q[2][0])) +
              (two * g22) * (q[2][0] * q[2][1])) +
             ((two * g11) * (q[1][0] * q[1][1]) + g12 * (q[1][0] * q[2][1] + q[1][1] * q[2][0])))
        a, sc = o["a"], o["sc"]
        g.append((a[0] - a[1]) * X)
        g.append((((two * sc[0]) * h[0]) * S[0] + ((two * sc[1]) * h[1]) * S[1]) + ((two * sc[2]) * h[2]) * S[2])
    return np.stack([l0, l1, l2, l3]).astype(np.float32), np.stack(g).astype(np.float32), badx | bady


def wave_sums(rows):
    """rows [n][F] float32 -> [n]: lane l adds views l, l + 64, ... in order (from +0); butterfly over XOR 32, 16, ..., 1."""
    n, F = rows.shape
    J = (F + 63) // 64
    pad = np.zeros((n, J * 64), np.float32)
    pad[:, :F] = rows
    pad = pad.reshape(n, J, 64)
    part = np.zeros((n, 64), np.float32)
    idx = np.arange(64)
    with np.errstate(all="ignore"):
        for j in range(J):
            part = part + pad[:, j]
        for off in (32, 16, 8, 4, 2, 1):
            part = part + part[:, idx ^ off]
    return part[:, 0]


def grad32(p, h, P, tgt, mask):
    """loss and the five gradient components at state p, as the kernel computes them; third value: a discriminant was negative."""
    p = np.asarray(p, np.float32)
    h = np.asarray(h, np.float32)
    F = len(P)
    Ff = f32(F)
    invF = f32(1.0) / Ff
    o = make_obj(p, h)
    l, g, bad = view_terms(o, p, h, np.asarray(P, np.float32).reshape(F, 12), tgt, mask, invF)
    s = wave_sums(np.concatenate([l, g]))
    with np.errstate(all="ignore"):
        loss = ((s[0] / Ff + s[1] / Ff) + s[2] / Ff) + s[3] / Ff
    return f32(loss), s[4:9].astype(np.float32), bool(bad.any())


def fit32(init5, h, P, tgt, mask, n_iters):
    """odam_dq_fit_batch for one object: dict(out5, Q, loss [n_iters], traj [n_iters, 5], status (code, step))."""
    p = np.asarray(init5, np.float32).copy()
    h = np.asarray(h, np.float32)
    m = np.zeros(5, np.float32)
    v = np.zeros(5, np.float32)
    tab = adam_table(n_iters)
    loss = np.full(n_iters, np.nan, np.float32)
    traj = np.zeros((n_iters, 5), np.float32)
    code, first = 0, -1
    for it in range(n_iters):
        l, g, bad = grad32(p, h, P, tgt, mask)
        if bad:
            code, first = 1, it
            traj[it:] = p
            break
        p, m, v = adam_step(p, m, v, g, tab[it, 0], tab[it, 1])
        loss[it] = l
        traj[it] = p
    return dict(out5=p, Q=make_obj(p, h)["Q"].reshape(4, 4), loss=loss, traj=traj, status=(code, first))


def loss64(p, h, P, tgt, mask):
    """The reference's loss_2d in torch float64 from its formulas; p: torch float64 tensor [5] (requires_grad as the caller likes)."""
    import torch
    h = torch.as_tensor(np.asarray(h, np.float64))
    Ms = torch.as_tensor(np.asarray(P, np.float64).reshape(-1, 3, 4))
    tgt = torch.as_tensor(np.asarray(tgt, np.float64))
    mask = torch.as_tensor(np.asarray(mask, np.float64))
    scale = (p[4] * h) ** 2                                                   # sq_libs.py:229
    c, s = torch.cos(p[3]), torch.sin(p[3])
    zero, one = torch.zeros((), dtype=torch.float64), torch.ones((), dtype=torch.float64)
    R = torch.stack([c, -s, zero, s, c, zero, zero, zero, one]).reshape(3, 3)  # :102-121
    T = torch.cat([torch.cat([R, p[:3, None]], 1), torch.tensor([[0., 0., 0., 1.]], dtype=torch.float64)], 0)
    Q = T @ torch.diag(torch.cat([scale, torch.tensor([-1.], dtype=torch.float64)])) @ T.T      # :68-78
    C = Ms @ Q @ Ms.permute(0, 2, 1)                                          # :156
    loss = 0
    for i, (k_lo, k_hi) in ((0, (0, 1)), (1, (2, 3))):                         # :128-140
        b = torch.sqrt(4 * C[:, i, 2] ** 2 - 4 * C[:, i, i] * C[:, 2, 2])
        x0 = 0.5 / C[:, 2, 2] * (2 * C[:, i, 2] + b)
        x1 = 0.5 / C[:, 2, 2] * (2 * C[:, i, 2] - b)
        st = torch.stack([x0, x1], 0)
        lo, hi = torch.min(st, 0).values, torch.max(st, 0).values
        for pred, k in ((-lo, k_lo), (-hi, k_hi)):                            # :161-167 (gt = -pixel)
            l = (pred - (-tgt[:, k])).abs()
            l = torch.where(torch.isnan(l), torch.zeros_like(l), l) * mask[:, k]
            loss = loss + l.mean()
    return loss


def grad64(p, h, P, tgt, mask):
    import torch
    x = torch.tensor(np.asarray(p, np.float64), requires_grad=True)
    l = loss64(x, h, P, tgt, mask)
    l.backward()
    return float(l.detach()), x.grad.numpy().copy()


# ---- fixture helpers shared by tests/test_dq_host.py and tests/test_dq_gpu.py ----------------------------------------------------
STEPS = (1, 2, 5, 20, 100, 500)


def case(z, ci):
    pre = f"c{ci}_"
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


def rel(a, b, floor=1e-3):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


def fitted_box(Q):
    """run_multi_view.py:66-67 for a dual quadric: oriented box of its 2500 ellipsoid points"""
    from odam_amd import multi_view, sq
    pts, _ = sq.DualQuadric(np.asarray(Q, np.float32).reshape(4, 4)).compute_ellipsoid_points(use_numpy=True)
    return multi_view.compute_oriented_bbox(pts)


def survey_row(d, out5, Q):
    """One problem of the free-running table: our deviation e from the un-nudged reference, the reference's own spread s over
    its eight nudged runs (both: max relative difference of the five parameters, floor 1e-3), 3-D IoU of the fitted boxes."""
    from odam_amd import merge
    ref = d["p_after"][-1]
    e = rel(out5, ref)
    s = max(rel(x, ref) for x in d["n_final"])
    iou = merge.box3d_iou_pairs(fitted_box(Q)[None], d["bbox_qc"][None])[0][0]
    siou = merge.box3d_iou_pairs(d["n_bbox_qc"], np.repeat(d["bbox_qc"][None], len(d["n_bbox_qc"]), 0))[0].min()
    return dict(views=len(d["P"]), e=e, s=s, iou=float(iou), siou=float(siou))


def check_survey_row(r):
    """DESIGN 2.2's hard bound, per problem"""
    assert r["e"] <= max(1e-4, 3 * r["s"]), r
    if r["s"] <= 1e-4:
        assert r["e"] <= 1e-4, r
    assert r["iou"] >= min(0.99, 1 - 3 * (1 - r["siou"])), r


def format_table(rows):
    lines = ["# free-running 500-step dual-quadric fits (tests/dq_ref.py fit32 == odam_dq_fit_batch bit for bit) against the reference",
             "# e: max relative deviation of the five final parameters from the un-nudged reference fit (floor 1e-3)",
             "# s: the same for the reference's own eight re-runs with the initial state moved by 1-2 float32 ulps",
             "# iou: 3-D IoU of our fitted box with the reference's; siou: the smallest among the reference's nudged runs",
             "problem views        e        s     iou    siou"]
    for i, r in enumerate(rows):
        lines.append("%7d %5d %8.2e %8.2e %7.4f %7.4f" % (i, r["views"], r["e"], r["s"], r["iou"], r["siou"]))
    n = len(rows)
    lines.append("# reference reproducible at 1e-4 under its own nudges (s <= 1e-4): %d of %d; ours within 1e-4 of the reference: %d of %d"
                 % (sum(r["s"] <= 1e-4 for r in rows), n, sum(r["e"] <= 1e-4 for r in rows), n))
    return "\n".join(lines) + "\n"


def discriminant_problem(d, view=3, inside=True):
    """The inputs of fixture problem d with one camera moved INTO the initial ellipsoid (its centre): every tangent plane
    through that camera is imaginary, C_02^2 - C_00 C_22 < 0 by Cauchy-Schwarz, the reference's assert fires at step 0."""
    P = d["P"].copy().reshape(-1, 3, 4).astype(np.float64)
    M = P[view]
    c = d["init5"][:3].astype(np.float64)
    M[:, 3] = -(M[:, :3] @ c)          # same rotation and intrinsics, optical centre at the object's centre
    P[view] = M
    return P.astype(np.float32).reshape(-1, 12)


class RefFitter:
    """test double with SqFitter.fit_dual's interface over fit32 (tests only: optim_process's host logic without a GPU)"""

    def fit_dual(self, init5, half_dims, view_counts, P, tgt, mask, n_iters=500, **kw):
        import torch
        outs, Qs, st, off = [], [], [], 0
        for i, F in enumerate(view_counts):
            r = fit32(init5[i], half_dims[i], P[off:off + F], tgt[off:off + F], mask[off:off + F], n_iters)
            outs.append(r["out5"]); Qs.append(r["Q"]); st.append(r["status"]); off += F
        st = np.asarray(st, np.int32).reshape(-1, 2)
        assert (st[:, 0] == 0).all()
        return {"params": torch.from_numpy(np.stack(outs)), "Q": torch.from_numpy(np.stack(Qs)), "status": st, "loss": None, "traj": None}


def check_optim_process(out, z, tracks):
    """optim_process(representation="dual_quadric") against the op_* case of dq_fits.npz: unfitted objects exact, bboxes_dl exact,
    fitted objects inside the free-running bounds (check_survey_row) with the reference's own spread over its nudged runs."""
    from odam_amd import merge, sq
    n = len(tracks)
    assert len(out["quadrics"]) == n and all(isinstance(q, sq.DualQuadric) for q in out["quadrics"])
    assert np.allclose(np.asarray(out["bboxes_dl"]), z["op_bboxes_dl"], rtol=0, atol=1e-12)
    assert np.array_equal(out["fitted"], z["op_fitted"]) and out["fitted"].sum() >= 3 and (~out["fitted"]).sum() >= 1
    rows = []
    for i in range(n):
        ref = z["op_final"][i]
        if not out["fitted"][i]:
            assert np.array_equal(out["params"][i], ref)
            assert np.array_equal(np.asarray(out["quadrics"][i].Q, np.float32), z["op_Q"][i])
            assert np.allclose(out["bboxes_qc"][i], z["op_bboxes_dl"][i], rtol=0, atol=1e-12)
            continue
        e = rel(out["params"][i], ref)
        s = max(rel(p[i], ref) for p in z["op_n_final"])
        iou = merge.box3d_iou_pairs(np.asarray(out["bboxes_qc"][i])[None], z["op_bboxes_qc"][i][None])[0][0]
        siou = merge.box3d_iou_pairs(z["op_n_bboxes_qc"][:, i], np.repeat(z["op_bboxes_qc"][i][None], len(z["op_n_bboxes_qc"]), 0))[0].min()
        row = dict(views=len(tracks[i]), e=e, s=s, iou=float(iou), siou=float(siou))
        print("object %d: %s" % (i, row))
        rows.append(row)
    for row in rows:
        check_survey_row(row)
    return rows
