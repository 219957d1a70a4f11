"""Closed-form dual quadric, host side: the numpy restatement (tests/quadric_svd_ref.py) against the reference's stored results and
the ground truth (tests/golden/quadric_svd.npz, make_golden_quadric_svd.py), multi_view.closed_form_quadrics behind a stub fitter,
and the C declaration against what odam_amd.sq gives ctypes.  tests/test_quadric_svd_gpu.py asks the device for the same.

Tolerance (tests/golden/quadric_svd.md): err = max|Q_a - Q_b| / max|Q_b| on normalised Q is bounded per problem by
8 * RATIO * u, u = 2^-52 lambda_10 / (lambda_2 - lambda_1), RATIO = 0.395 = the worst restatement-vs-reference err / u measured
over the fixture when it was generated."""
import ctypes
import os
import re

import numpy as np
import pytest

import quadric_svd_ref as R
from conftest import REPO


@pytest.fixture(scope="module")
def fx(golden):
    return golden("quadric_svd.npz")


@pytest.fixture(scope="module")
def restated(fx):
    """solve_one of every fixture object (computed once): (Q, eig, status)"""
    out = []
    for i in range(int(fx["n_obj"])):
        P, e, m = R.track_rows(fx, i)
        out.append(R.solve_one(P, e, m)[:3])
    return out


def test_fixture_is_what_the_generator_describes(fx):
    kind, views = fx["kind"].astype(int), fx["views"].astype(int)
    for k in (R.KIND_EXACT, R.KIND_NOISY):
        assert sorted(views[kind == k]) == [3, 4, 10, 64, 65, 129, 300]
    assert [int((kind == k).sum()) for k in (R.KIND_MASKED, R.KIND_TWO_VIEWS, R.KIND_NOT_ELLIPSOID)] == [1, 1, 1]
    assert all(a.dtype == np.float64 for a in fx.values())
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "quadric_svd.npz")) < 400 * 1024
    i = int(np.flatnonzero(kind == R.KIND_MASKED)[0])
    m = R.track_rows(fx, i)[2]
    assert 0 < (m == 0).sum() < m.size and (m != 0).sum() >= 9
    i = int(np.flatnonzero(kind == R.KIND_NOT_ELLIPSOID)[0])
    assert fx["ref_is_ellipsoid"][i] == 0 and fx["ref_is_ellipsoid"].sum() == len(kind) - 2


def test_restatement_vs_reference(fx, restated):
    worst = 0.0
    for i, (Q, eig, st) in enumerate(restated):
        if int(fx["kind"][i]) == R.KIND_TWO_VIEWS:
            assert st == 2 and np.isnan(Q).all() and np.isnan(eig).all()
            continue
        err, u = R.q_err(Q, fx["ref_Q"][i]), R.scale_u(eig)
        worst = max(worst, err / u)
        print("object %2d: err %.3e = %.3f u (u %.3e, bound %.3e)" % (i, err, err / u, u, R.bound(eig)))
        assert st == (0 if fx["ref_is_ellipsoid"][i] else 1), i
        assert Q[3, 3] == -1.0 and np.array_equal(Q, Q.T)
        assert err <= R.bound(eig), (i, err, R.bound(eig))
        # the reference's vector itself, up to sign and scale: the same direction
        v = fx["ref_vec"][i]
        assert R.q_err(R.normalise(R.quadric_2mat(v)), fx["ref_Q"][i]) == 0.0
    print("worst restatement-vs-reference err / u = %.3f (RATIO = %.3f)" % (worst, R.RATIO))


def test_exact_edges_vs_ground_truth(fx, restated):
    """exact tangent lines: the null vector of A is the ellipsoid itself, to the same bound"""
    n = 0
    for i, (Q, eig, st) in enumerate(restated):
        if int(fx["kind"][i]) not in (R.KIND_EXACT, R.KIND_MASKED):
            continue
        n += 1
        err = R.q_err(Q, fx["gt_Q"][i])
        print("object %2d (%3d views): vs truth %.3e, bound %.3e" % (i, int(fx["views"][i]), err, R.bound(eig)))
        assert st == 0 and err <= R.bound(eig), (i, err, R.bound(eig))
        assert abs(eig[0]) <= 64 * 2.0 ** -52 * eig[2]      # lambda_1 = 0 up to the rounding of a 10 x 10 Gram matrix's entries
    assert n == 8


def test_gram_order_is_the_kernels():
    """the lane partials and the butterfly, written out naively for one object with masked edges and 130 views"""
    rs = np.random.RandomState(3)
    F = 130
    P = rs.standard_normal((F, 12))
    e = rs.uniform(30, 400, (F, 4))
    m = (rs.uniform(size=(F, 4)) > 0.2).astype(np.float32)
    m[64] = 0
    s = R.plane_rows(P, e)
    part = [np.zeros((10, 10)) for _ in range(64)]
    for lane in range(64):
        for v in range(lane, F, 64):
            for k in range(4):
                if m[v, k]:
                    part[lane] = part[lane] + np.outer(s[v, k], s[v, k])
    for off in (32, 16, 8, 4, 2, 1):
        part = [part[l] + part[l ^ off] for l in range(64)]
    A, n = R.gram(P, e, m)
    assert n == int(m.sum()) and np.array_equal(A, part[0]) and np.array_equal(A, A.T)
    assert np.allclose(A, sum(np.outer(s[v, k], s[v, k]) for v in range(F) for k in range(4) if m[v, k]), rtol=1e-13, atol=0)


def _args(fx):
    return (R.fixture_tracks(fx), [int(x) for x in fx["img_names"]], fx["T_wcs"], fx["P_cws"], R.IMG_H, R.IMG_W, fx["K"])


def test_closed_form_quadrics_with_stub_fitter(fx, restated):
    from odam_amd import multi_view, sq
    args = _args(fx)
    n = len(args[0])
    kind = fx["kind"].astype(int)
    out = multi_view.closed_form_quadrics(*args, n_views=3, fitter=R.RefFitter())
    assert set(out) == {"quadrics", "bboxes_qc", "bboxes_dl", "status", "eig"}
    assert out["status"].dtype == np.int32 and out["eig"].shape == (n, 3)
    want = [2 if k == R.KIND_TWO_VIEWS else 1 if k == R.KIND_NOT_ELLIPSOID else 0 for k in kind]
    assert out["status"].tolist() == want
    # bboxes_dl is optim_process's (no track reaches its fit with this n_views, so its fitter is never called)
    op = multi_view.optim_process(*args, "super_quadric", True, 200, 10 ** 9, fitter=object())
    assert np.array_equal(np.asarray(out["bboxes_dl"]), np.asarray(op["bboxes_dl"]))
    for i in range(n):
        Q, eig, st = restated[i]
        if want[i] == 0:
            q = out["quadrics"][i]
            assert isinstance(q, sq.DualQuadric) and q.Q.dtype == np.float64 and np.array_equal(q.Q, Q)
            assert np.array_equal(out["eig"][i], eig)
            pts, ok = q.compute_ellipsoid_points(use_numpy=True)
            assert ok and pts.shape == (2500, 3)
            box = np.asarray(out["bboxes_qc"][i])
            assert box.shape == (8, 3) and np.array_equal(box, multi_view.compute_oriented_bboxes(pts[None])[0][0])
            assert not np.array_equal(box, out["bboxes_dl"][i])
        else:
            assert out["quadrics"][i] is None and np.array_equal(out["bboxes_qc"][i], out["bboxes_dl"][i])
    two = int(np.flatnonzero(kind == R.KIND_TWO_VIEWS)[0])
    assert np.isnan(out["eig"][two]).all()          # not sent: fewer than n_views valid views
    # the n_views rule: with 2 the two-view track IS sent and comes back with status 2; with 11 the short tracks are not sent
    out2 = multi_view.closed_form_quadrics(*args, n_views=2, fitter=R.RefFitter())
    assert out2["status"].tolist() == want and out2["quadrics"][two] is None
    sent = []

    class Spy:
        @staticmethod
        def quadric_svd(view_counts, P, edges, mask):
            sent.append(list(view_counts))
            return R.quadric_svd(view_counts, P, edges, mask)
    out11 = multi_view.closed_form_quadrics(*args, n_views=11, fitter=Spy())
    views = fx["views"].astype(int)
    assert sent == [[int(v) for v in views if v >= 11]]
    for i in range(n):
        if views[i] < 11:
            assert out11["quadrics"][i] is None and out11["status"][i] == 2 and np.array_equal(out11["bboxes_qc"][i], out11["bboxes_dl"][i])
        else:
            assert np.array_equal(out11["quadrics"][i].Q, out["quadrics"][i].Q)
    # no track at all
    empty = multi_view.closed_form_quadrics([], *args[1:], fitter=R.RefFitter())
    assert empty["quadrics"] == [] and empty["status"].shape == (0,) and empty["eig"].shape == (0, 3)


def test_edge_values_are_the_float64_track_columns(fx):
    """not the fit's float32 targets: a track whose edges differ below float32 resolution gives a different Q"""
    from odam_amd import multi_view
    args = list(_args(fx))
    tr = args[0][4].copy()
    seen = []

    class Spy:
        @staticmethod
        def quadric_svd(view_counts, P, edges, mask):
            seen.append((np.asarray(P), np.asarray(edges), np.asarray(mask)))
            return R.quadric_svd(view_counts, P, edges, mask)
    multi_view.closed_form_quadrics([tr], *args[1:], fitter=Spy())
    P, e, m = seen[0]
    assert P.dtype == np.float64 and e.dtype == np.float64
    assert np.array_equal(e, tr[:, [2, 4, 3, 5]]) and not np.array_equal(e, e.astype(np.float32))
    wantP, wante, wantm = R.track_rows(fx, 4)
    assert np.array_equal(P, wantP) and np.array_equal(e, wante) and np.array_equal(m, wantm)


C_TO_CTYPES = {"int": ctypes.c_int}


def test_dq_svd_ctypes_signature_matches_the_header():
    """the argument list odam_amd.sq gives ctypes for odam_dq_svd_batch is the header's, argument by argument; the symbol is
    exported; argument checks come before any device work, with the neighbour's codes"""
    from odam_amd import _lib, sq
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "odam_sq.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+odam_dq_svd_batch\s*\(([^)]*)\)\s*;", txt)
    assert m, "odam_dq_svd_batch is not declared in include/odam_sq.h"
    names, want = [], []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        names.append(arg.split()[-1].lstrip("*"))
        want.append(ctypes.c_void_p if "*" in arg else C_TO_CTYPES[arg.replace("const ", "").rsplit(" ", 1)[0]])
    assert names == ["ctx", "n_obj", "view_offsets", "P", "edges", "mask", "max_views", "out_Q", "out_eig", "status", "stream"]
    assert sq.DQ_SVD_ARGTYPES == want
    assert hasattr(_lib.lib(), "odam_dq_svd_batch")
    f = sq._dq_svd_entry()
    assert list(f.argtypes) == want and f.restype is ctypes.c_int
    assert f(None, 1, None, None, None, None, 4, None, None, None, None) == 1          # ODAM_E_INVALID
    assert b"odam_dq_svd_batch" in _lib.lib().odam_last_error()
    # with every pointer given (never dereferenced on these paths): a negative count, the view limit, the empty call
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert f(p, -1, p, p, p, p, 4, p, p, p, None) == 1
    assert f(p, 1, p, p, p, p, 0, p, p, p, None) == 3 and f(p, 1, p, p, p, p, 16 * 1024 + 1, p, p, p, None) == 3      # ODAM_E_LIMIT
    assert b"max_views" in _lib.lib().odam_last_error()
    assert f(p, 0, p, p, p, p, 4, p, p, p, None) == 0
