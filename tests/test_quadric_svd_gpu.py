"""gfx950 closed-form dual quadric (odam_dq_svd_batch through odam_amd.sq.SqFitter.quadric_svd) against its host restatement
tests/quadric_svd_ref.py, the reference's stored results and the ground truth (tests/golden/quadric_svd.npz): bit-identical
results however the objects are dealt to launches and workgroups, and Q / eig / status within the tolerance of
tests/golden/quadric_svd.md -- err = max|Q_a - Q_b| / max|Q_b| <= 8 * RATIO * u per problem, u = 2^-52 l10 / (l2 - l1).

Eigenvalues: both solvers are backward stable, |d lambda| <= p(n) 2^-52 ||A||_2 each with p(n) of the order of n = 10 (Weyl), so
the device's and LAPACK's eigenvalues are held to 2 n 2^-52 lambda_10 of each other."""
import numpy as np
import pytest

import quadric_svd_ref as R

pytestmark = pytest.mark.gpu

EIG_BOUND = 2 * 10 * 2.0 ** -52


@pytest.fixture(scope="module")
def fitter():
    from odam_amd import sq
    f = sq.SqFitter("cuda:0", 10)
    yield f
    f.close()


@pytest.fixture(scope="module")
def fx(golden):
    return golden("quadric_svd.npz")


@pytest.fixture(scope="module")
def rows(fx):
    return [R.track_rows(fx, i) for i in range(int(fx["n_obj"]))]


@pytest.fixture(scope="module")
def restated(rows):
    return [R.solve_one(*r)[:3] for r in rows]


def _call(fitter, probs):
    out = fitter.quadric_svd([len(p[2]) for p in probs], np.concatenate([p[0] for p in probs]), np.concatenate([p[1] for p in probs]),
                             np.concatenate([p[2] for p in probs]))
    assert out["Q"].dtype.is_floating_point and out["Q"].element_size() == 8 and out["status"].dtype == np.int32
    return {"Q": out["Q"].cpu().numpy(), "eig": out["eig"].cpu().numpy(), "status": out["status"]}


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _same_bits(a, j, b, k):
    assert np.array_equal(_bits(a["Q"][j]), _bits(b["Q"][k])) and np.array_equal(_bits(a["eig"][j]), _bits(b["eig"][k]))
    assert a["status"][j] == b["status"][k]


def _check(out, j, want, tag):
    """object j of a device result against a restatement (Q, eig, status)"""
    Q, eig, st = want
    assert out["status"][j] == st, (tag, out["status"][j], st)
    if st == 2:
        assert np.isnan(out["Q"][j]).all() and np.isnan(out["eig"][j]).all()
        return
    err = R.q_err(out["Q"][j], Q)
    de = np.abs(out["eig"][j] - eig).max() / eig[2]
    print("%s: Q err %.3e = %.3f u (bound %.2f u), eig %.2f x 2^-52 l10" % (tag, err, err / R.scale_u(eig), R.MARGIN * R.RATIO, de * 2.0 ** 52))
    assert err <= R.bound(eig), (tag, err, R.bound(eig))
    assert de <= EIG_BOUND, (tag, de)
    assert out["Q"][j][3, 3] == -1.0 and np.array_equal(out["Q"][j], out["Q"][j].T)


@pytest.fixture(scope="module")
def alone(fitter, rows):
    """every fixture object in a launch of its own, at the default group size"""
    return [_call(fitter, [r]) for r in rows]


def test_fixture_vs_restatement_reference_and_truth(fx, alone, restated, measured):
    for i, want in enumerate(restated):
        _check(alone[i], 0, want, "object %d" % i)
        if want[2] == 2:
            continue
        eig = want[1]
        err_ref = R.q_err(alone[i]["Q"][0], fx["ref_Q"][i])
        measured("quadric_svd_vs_reference_in_u", err_ref / R.scale_u(eig))
        measured("quadric_svd_vs_restatement_in_u", R.q_err(alone[i]["Q"][0], want[0]) / R.scale_u(eig))
        assert err_ref <= R.bound(eig), (i, err_ref, R.bound(eig))
        assert alone[i]["status"][0] == (0 if fx["ref_is_ellipsoid"][i] else 1)
        if int(fx["kind"][i]) in (R.KIND_EXACT, R.KIND_MASKED):
            err_gt = R.q_err(alone[i]["Q"][0], fx["gt_Q"][i])
            print("object %d vs truth: %.3e (bound %.3e)" % (i, err_gt, R.bound(eig)))
            assert err_gt <= R.bound(eig), (i, err_gt, R.bound(eig))


def test_one_launch_equals_each_alone_and_repeats(fitter, rows, alone):
    both = [_call(fitter, rows), _call(fitter, rows)]
    for out in both:
        for i in range(len(rows)):
            _same_bits(out, i, alone[i], 0)


# 5 objects: a good one, the two-view object (status 2), 300 views, the not-an-ellipsoid object (status 1), a good one -- so the
# bad ones sit between good ones and, with 2, 4 or 8 objects per workgroup, the last workgroup is partly filled
MIXED = (0, 15, 12, 16, 7)


@pytest.mark.parametrize("waves", [1, 2, 4, 8])
def test_group_sizes_bit_identical(fitter, fx, rows, alone, waves):
    assert [int(fx["kind"][i]) for i in MIXED[1::2]] == [R.KIND_TWO_VIEWS, R.KIND_NOT_ELLIPSOID]
    try:
        fitter.set_dual_group_waves(waves)
        one = _call(fitter, [rows[6]])
        _same_bits(one, 0, alone[6], 0)
        five = _call(fitter, [rows[i] for i in MIXED])
        assert five["status"].tolist() == [0, 2, 0, 1, 0]
        for j, i in enumerate(MIXED):
            _same_bits(five, j, alone[i], 0)
        allofthem = _call(fitter, rows)
        for i in range(len(rows)):
            _same_bits(allofthem, i, alone[i], 0)
    finally:
        fitter.set_dual_group_waves(4)


@pytest.mark.parametrize("views", [3, 63, 64, 65, 129, 300])
def test_view_counts_at_the_lane_stride(fitter, fx, views):
    P, e, m, gt = R.exact_problem(fx["P_cws"], views, 900 + views)
    assert len(P) == views
    out = _call(fitter, [(P, e, m)])
    want = R.solve_one(P, e, m)[:3]
    _check(out, 0, want, "%d views" % views)
    assert out["status"][0] == 0 and R.q_err(out["Q"][0], gt) <= R.bound(want[1])


def test_all_masked_view_in_the_middle(fitter, fx):
    """a view without any constraint inside an object (lane 3's first view) adds nothing: the result is that of the restatement
    with the same mask and its edge values are never read (NaN here)"""
    P, e, m, gt = R.exact_problem(fx["P_cws"], 70, 77)
    m = m.copy(); e = e.copy()
    m[3] = 0; e[3] = np.nan
    m[66, 1] = 0; e[66, 1] = np.nan
    out = _call(fitter, [(P, e, m)])
    want = R.solve_one(P, e, m)[:3]
    _check(out, 0, want, "masked view")
    assert out["status"][0] == 0 and R.q_err(out["Q"][0], gt) <= R.bound(want[1])
    # and it is the same problem as the one with that view removed, up to the summation order
    keep = np.arange(70) != 3
    less = _call(fitter, [(P[keep], e[keep], m[keep])])
    assert R.q_err(less["Q"][0], out["Q"][0]) <= R.bound(want[1])


def test_statuses_inputs_and_limits(fitter, rows, alone):
    import torch
    from odam_amd import _lib
    # fewer than 9 unmasked edges in three views; a view count of 0 between good objects
    P, e, m = rows[4]
    m8 = np.zeros_like(m[:3]); m8[0] = 1; m8[1] = 1
    out = _call(fitter, [rows[2], (P[:3], e[:3], m8), (P[:0], e[:0], m[:0]), rows[4]])
    assert out["status"].tolist() == [0, 2, 2, 0]
    assert np.isnan(out["Q"][1:3]).all() and np.isnan(out["eig"][1:3]).all()
    _same_bits(out, 0, alone[2], 0)
    _same_bits(out, 3, alone[4], 0)
    # nine edges are enough to be computed (whatever the shape turns out to be)
    m9 = m8.copy(); m9[2, 0] = 1
    assert _call(fitter, [(P[:3], e[:3], m9)])["status"][0] in (0, 1)
    # torch inputs on the device, float32 mask as a bool tensor: the same bits
    dev = fitter.quadric_svd([len(m)], torch.from_numpy(P).cuda(), torch.from_numpy(e).cuda(), torch.from_numpy(m != 0).cuda())
    assert np.array_equal(_bits(dev["Q"].cpu().numpy()[0]), _bits(alone[4]["Q"][0]))
    # empty call; a negative count is refused on the host
    assert fitter.quadric_svd([], np.zeros((0, 12)), np.zeros((0, 4)), np.zeros((0, 4)))["Q"].shape == (0, 4, 4)
    with pytest.raises(_lib.OdamError):
        fitter.quadric_svd([-1], np.zeros((0, 12)), np.zeros((0, 4)), np.zeros((0, 4)))


def test_odam_process_closed_form_quadrics(fitter, fx):
    """OdamProcess.closed_form_quadrics on a short sequence (the fixture's tracks of at most 10 views, and the two bad ones) against
    multi_view.closed_form_quadrics over the restatement; it reads the tracks and leaves everything else alone"""
    from odam_amd import multi_view
    from odam_amd.processor import OdamProcess
    ids = [i for i in range(int(fx["n_obj"])) if fx["views"][i] <= 10]
    tracks = [fx[f"track{i}"].copy() for i in ids]
    names = [int(x) for x in fx["img_names"]]
    proc = OdamProcess(None, None, None, None, fitter=fitter)
    proc.init_sequence(fx["K"], R.IMG_H, R.IMG_W)
    proc.usable_frames, proc.T_wcs, proc.P_cws = names, list(fx["T_wcs"]), list(fx["P_cws"])
    proc.tracks = [t.copy() for t in tracks]
    out = proc.closed_form_quadrics()
    ref = multi_view.closed_form_quadrics(tracks, names, fx["T_wcs"], fx["P_cws"], R.IMG_H, R.IMG_W, fx["K"], fitter=R.RefFitter())
    assert set(out) == set(ref) and out["status"].tolist() == ref["status"].tolist()
    assert sorted(set(out["status"].tolist())) == [0, 1, 2]
    assert np.array_equal(np.asarray(out["bboxes_dl"]), np.asarray(ref["bboxes_dl"]))
    for j in range(len(ids)):
        if ref["status"][j] == 0:
            assert R.q_err(out["quadrics"][j].Q, ref["quadrics"][j].Q) <= R.bound(ref["eig"][j])
            pts = out["quadrics"][j].compute_ellipsoid_points(use_numpy=True)[0]
            assert np.array_equal(out["bboxes_qc"][j], multi_view.compute_oriented_bboxes(pts[None])[0][0])
        else:
            assert out["quadrics"][j] is None and np.array_equal(out["bboxes_qc"][j], out["bboxes_dl"][j])
    assert proc._refine_state is None and all(np.array_equal(a, b) for a, b in zip(proc.tracks, tracks))
    out3 = proc.closed_form_quadrics(n_views=4)      # the three-view tracks drop out
    assert [q is None for q in out3["quadrics"]] == [fx["views"][i] < 4 or ref["status"][j] != 0 for j, i in enumerate(ids)]
