"""Dual-quadric fit, host side: the float32 restatement of the kernel (tests/dq_ref.py) against float64 autograd and against
the reference's stored QuadricOptimizer runs (tests/golden/dq_fits.npz, make_golden_dq.py), and odam_amd.sq.DualQuadric against the
reference's DualQuadric outputs.  tests/test_dq_gpu.py asks the device for the restatement's bits."""
import os

import numpy as np
import pytest

import dq_ref

# Gradient bounds: 4 x the worst deviation measured over the fixture (24 states: before steps 1 and 100 of the 12 problems),
# relative to max|g| -- 8.6e-6 against float64 autograd, 1.34e-5 against the reference's own float32 gradient.  Both are above
# the super-quadric path's 1e-5: the conic entries C = M Q M^T are differences of terms ~1e6 (z_0^2 z_2^2 in the discriminant
# cancels), evaluated in float32 by the reference and by the kernel alike -- the reference's own float32 gradient is 1.5e-5 from
# float64 at those states (DESIGN, dual-quadric section).
G_BOUND_F64 = 4 * 8.6e-6
G_BOUND_REF = 4 * 1.34e-5


@pytest.fixture(scope="module")
def fits(golden):
    return golden("dq_fits.npz")


@pytest.fixture(scope="module")
def free_runs(fits):
    out = []
    for ci in range(int(fits["n_cases"])):
        d = dq_ref.case(fits, ci)
        out.append((d, dq_ref.fit32(d["init5"], d["half_dims"], d["P"], d["tgt"], d["mask"], 500)))
    return out


def test_fma32_is_the_fused_result():
    """the emulation against cases where rounding the binary64 sum first would round twice"""
    f = np.float32
    a, b = f(1 + 2.0 ** -12), f(1 + 2.0 ** -12)          # a * b = 1 + 2^-11 + 2^-24: a tie of float32 after the sum with c below
    for c, want in ((f(2.0 ** -60), 1 + 2.0 ** -11 + 2.0 ** -23), (f(-2.0 ** -60), 1 + 2.0 ** -11), (f(0), 1 + 2.0 ** -11)):
        assert float(dq_ref.fma32(a, b, c)) == want
    rs = np.random.RandomState(0)
    x, y, z = (rs.standard_normal(100000).astype(np.float32) for _ in range(3))
    exact = (x.astype(np.longdouble) * y.astype(np.longdouble) + z.astype(np.longdouble)).astype(np.float32)
    assert np.array_equal(dq_ref.fma32(x, y, z), exact)      # (x87 extended: 64-bit significand holds the 48-bit product + z to round-to-nearest once in nearly all draws)


def test_gradient_vs_float64_autograd_and_reference(fits):
    worst64 = worst_ref = 0.0
    for ci in range(int(fits["n_cases"])):
        d = dq_ref.case(fits, ci)
        for j in range(len(d["tf_p"])):
            loss, g, bad = dq_ref.grad32(d["tf_p"][j], d["half_dims"], d["P"], d["tgt"], d["mask"])
            l64, g64 = dq_ref.grad64(d["tf_p"][j], d["half_dims"], d["P"], d["tgt"], d["mask"])
            gr = d["tf_g"][j]
            e64 = np.abs(g - g64).max() / np.abs(g64).max()
            eref = np.abs(g - gr).max() / np.abs(gr).max()
            print("problem %d before step %d: vs float64 %.2e  vs reference float32 %.2e  (reference vs float64 %.2e)" % (
                ci, int(fits["tf_steps"][j]), e64, eref, np.abs(gr - g64).max() / np.abs(g64).max()))
            worst64, worst_ref = max(worst64, e64), max(worst_ref, eref)
            assert not bad
            assert abs(float(loss) - l64) <= 1e-5 * abs(l64)
            assert abs(float(loss) - float(d["loss"][int(fits["tf_steps"][j]) - 1])) <= 1e-5 * abs(l64)
    print("worst: vs float64 %.3e, vs reference %.3e" % (worst64, worst_ref))
    assert worst64 <= G_BOUND_F64 and worst_ref <= G_BOUND_REF


def _ulps(a, b):
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


def test_teacher_forced_adam_step(fits):
    """From the reference's stored state (parameters, moments) and its stored gradient the step lands within 1 ulp of the
    reference's next parameters, per parameter (the bound of DESIGN 2.1, tests/test_sq_oracle.py); with the restatement's OWN
    gradient at that state every parameter is within 1 ulp OR within that test's 1.2e-7 (one ulp at unit magnitude: a parameter
    near zero -- a translate component of 0.02 -- has ulps of 2e-9, smaller than the gradient's 1e-5 share of the 0.01 step)."""
    tab = dq_ref.adam_table(500)
    idx = {int(s): i for i, s in enumerate(fits["steps"])}
    for ci in range(int(fits["n_cases"])):
        d = dq_ref.case(fits, ci)
        for j, st in enumerate(int(s) for s in fits["tf_steps"]):
            want = d["p_after"][idx[st]]
            p1, _, _ = dq_ref.adam_step(d["tf_p"][j], d["tf_m"][j], d["tf_v"][j], d["tf_g"][j], tab[st - 1, 0], tab[st - 1, 1])
            assert _ulps(p1, want).max() <= 1, (ci, st, p1, want)
            _, g, _ = dq_ref.grad32(d["tf_p"][j], d["half_dims"], d["P"], d["tgt"], d["mask"])
            p2, _, _ = dq_ref.adam_step(d["tf_p"][j], d["tf_m"][j], d["tf_v"][j], g, tab[st - 1, 0], tab[st - 1, 1])
            assert ((_ulps(p2, want) <= 1) | (np.abs(p2 - want) <= 1.2e-7)).all(), (ci, st, p2, want)


def test_free_running_fit_vs_reference_spread(fits, free_runs):
    """500 free-running steps per problem: deviation from the un-nudged reference against the reference's own spread.
    The table is committed as tests/golden/dq_fits_table.txt and must be what this run computes."""
    rows = []
    for d, r in free_runs:
        assert r["status"] == (0, -1)
        row = dq_ref.survey_row(d, r["out5"], r["Q"])
        rows.append(row)
        # the early trajectory tracks the reference closely (before the first L1 sign decision differs)
        assert dq_ref.rel(r["traj"][0], d["p_after"][0]) <= 1e-6 and dq_ref.rel(r["traj"][4], d["p_after"][2]) <= 1e-5
        assert abs(float(r["loss"][0]) - float(d["loss"][0])) <= 1e-5 * abs(float(d["loss"][0]))
    table = dq_ref.format_table(rows)
    print(table)
    for row in rows:
        dq_ref.check_survey_row(row)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dq_fits_table.txt")) as f:
        assert f.read() == table


def test_negative_discriminant_gives_status_1(fits):
    d = dq_ref.case(fits, 3)
    P = dq_ref.discriminant_problem(d)
    r = dq_ref.fit32(d["init5"], d["half_dims"], P, d["tgt"], d["mask"], 20)
    assert r["status"] == (1, 0)
    assert np.array_equal(r["out5"], d["init5"]) and np.isnan(r["loss"]).all() and np.array_equal(r["traj"], np.tile(d["init5"], (20, 1)))
    # the float64 form of the reference's formulas has a NaN sqrt there too (what its assert tests)
    import torch
    with np.errstate(all="ignore"):
        M = torch.as_tensor(P.reshape(-1, 3, 4)[3].astype(np.float64))
        Q = torch.as_tensor(dq_ref.make_obj(d["init5"], d["half_dims"])["Q"].reshape(4, 4).astype(np.float64))
        C = M @ Q @ M.T
        assert float(4 * C[0, 2] ** 2 - 4 * C[0, 0] * C[2, 2]) < 0
    # and the untouched problem runs through
    assert dq_ref.fit32(d["init5"], d["half_dims"], d["P"], d["tgt"], d["mask"], 20)["status"] == (0, -1)


def _canon(scale, R):
    """eigen-pairs in a fixed order (ascending scale) and sign (largest component of each vector positive)"""
    o = np.argsort(scale)
    R = np.real(np.asarray(R))[:, o].copy()
    for k in range(3):
        if R[np.argmax(np.abs(R[:, k])), k] < 0:
            R[:, k] *= -1
    return np.asarray(scale)[o], R


def test_dual_quadric_class_vs_reference(fits):
    """get_srt / compute_ellipsoid_points / get_bbox on the reference's final Q against its stored outputs.
    Bounds: the stored values are float32 (points, scale) or float64 computed from a float32 Q.  Same LAPACK routine on the same
    matrix: srt and bbox2d to 1e-12 relative; points are float32 roundings of |x| <= ~3 (scene coordinates, metres): one ulp =
    2.4e-7, so 5e-7 absolute covers the rounding of two evaluations that may differ in the last bit of a float64 cos / sin."""
    from odam_amd import sq
    for ci in range(int(fits["n_cases"])):
        d = dq_ref.case(fits, ci)
        q = sq.DualQuadric(d["Q"])
        scale, R, t, ok = q.get_srt()
        assert ok == bool(d["is_ellipsoid"]) and scale.dtype == np.float32
        s0, R0 = _canon(scale, R)
        s1, R1 = _canon(d["srt_scale"], d["srt_R"])
        assert np.allclose(s0, s1, rtol=1e-6, atol=0) and np.allclose(R0, R1, rtol=0, atol=1e-12)
        assert np.allclose(t, d["srt_t"], rtol=0, atol=0)
        pts, ok2 = q.compute_ellipsoid_points(use_numpy=True)
        assert pts.shape == (2500, 3) and pts.dtype == np.float32 and ok2 == ok
        assert np.abs(d["points"]).max() < 4.0
        # the point SET is invariant under eigenvector order / sign only up to a re-parametrisation of the grid, so compare the
        # surface: every stored point satisfies our ellipsoid's equation and vice versa, to float32 rounding of the coordinates
        for P_, (sc_, R_, t_) in ((d["points"], (s0, R0, np.asarray(t).reshape(3))), (pts, (s1, R1, d["srt_t"].reshape(3)))):
            y = (P_.astype(np.float64) - t_) @ R_
            lvl = (y * y / sc_.astype(np.float64)).sum(1)
            # d lvl / d x = 2 y / scale <= 2 / sqrt(min scale): a 5e-7 move of a coordinate
            assert np.abs(lvl - 1).max() <= 3 * 5e-7 * 2 / np.sqrt(sc_.min()) + 1e-6, ci
        if np.allclose(np.real(R), d["srt_R"], atol=1e-12):      # same LAPACK order and sign (this machine): the grid itself
            assert np.abs(pts - d["points"]).max() <= 5e-7
        Pm = d["P"].reshape(-1, 3, 4).astype(np.float32).astype(np.float64)
        for f in range(len(d["bbox2d"])):
            got = q.get_bbox(Pm[f], False, False)
            lines = q.get_bbox(Pm[f], False, True)
            # stored from the float64 P of the generator; here from its float32 rounding: pixels ~ 640 x 6e-8 relative x the
            # conditioning of the conic (~1e2) -> 5e-3 px
            assert np.abs(got - d["bbox2d"][f]).max() <= 5e-3
            assert [float(-l[2]) for l in lines] == [float(v) for v in got]


def test_representations_table():
    from odam_amd import sq
    assert sq.REPRESENTATIONS["dual_quadric"] == 3
    assert {k: sq.REPRESENTATIONS[k] for k in ("super_quadric", "cube", "quadric")} == {"super_quadric": 0, "cube": 1, "quadric": 2}
    i5, h = sq.init_dual([1.0, 2.0, 3.0], 0.5, [0.4, 0.6, 0.8])
    assert i5.dtype == np.float32 and np.array_equal(i5, np.array([1, 2, 3, 0.5, 1], np.float32))
    assert np.array_equal(h, (np.array([0.4, 0.6, 0.8]) / 2).astype(np.float32))


def test_optim_process_dual_quadric_host_path(fits, golden):
    """optim_process(representation="dual_quadric") with the restatement standing in for the GPU fitter, against the reference's
    driver (run_multi_view.py:44-69 over QuadricOptimizer) on the scene of sq_optim.npz"""
    from odam_amd.multi_view import optim_process
    z = golden("sq_optim.npz")
    tracks = [z[f"track{i}"] for i in range(int(z["n_tracks"]))]
    out = optim_process(tracks, [int(x) for x in z["img_names"]], z["T_wcs"], z["P_cws"], 480, 640, z["K"], "dual_quadric", True, 500, 10,
                        fitter=dq_ref.RefFitter(), return_params=True)
    assert set(out) >= {"tracks", "bboxes_qc", "bboxes_dl", "quadrics"}
    dq_ref.check_optim_process(out, fits, tracks)
    pts, ok = out["quadrics"][int(np.flatnonzero(out["fitted"])[0])].compute_ellipsoid_points(use_numpy=True)
    assert pts.shape == (2500, 3) and pts.dtype == np.float32 and ok
