"""gfx950 dual-quadric fit (odam_dq_fit_batch through odam_amd.sq.SqFitter.fit_dual) against its host restatement
tests/dq_ref.py: BIT FOR BIT -- parameters after every step, the loss log, Q, the status -- on the reference fixture
(tests/golden/dq_fits.npz), at 1 ... 3000 views, for 1, 30 and 500 objects per call and however the objects are dealt to
workgroups; the discriminant rule; optim_process(representation="dual_quadric") against the reference's driver."""
import numpy as np
import pytest

import dq_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fitter():
    from odam_amd import sq
    f = sq.SqFitter("cuda:0", 200)      # (fit_dual's step count is not bounded by the context's max_iters)
    yield f
    f.close()


@pytest.fixture(scope="module")
def fits(golden):
    return golden("dq_fits.npz")


@pytest.fixture(scope="module")
def restated(fits):
    """fit32 of every fixture problem, 500 steps (computed once)"""
    out = []
    for ci in range(int(fits["n_cases"])):
        d = dq_ref.case(fits, ci)
        out.append((d, dq_ref.fit32(d["init5"], d["half_dims"], d["P"], d["tgt"], d["mask"], 500)))
    return out


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _call(fitter, ds, n_iters, **kw):
    return fitter.fit_dual(np.stack([d["init5"] for d in ds]), np.stack([d["half_dims"] for d in ds]), [len(d["P"]) for d in ds],
                           np.concatenate([d["P"] for d in ds]), np.concatenate([d["tgt"] for d in ds]),
                           np.concatenate([d["mask"] for d in ds]), n_iters=n_iters, want_loss=True, want_traj=True, **kw)


def _same(out, j, r):
    """object j of a fit_dual result == one fit32 result, in every bit"""
    assert tuple(int(x) for x in out["status"][j]) == tuple(r["status"]), (j, out["status"][j], r["status"])
    assert np.array_equal(_bits(out["traj"][j].cpu().numpy()), _bits(r["traj"])), j
    assert np.array_equal(_bits(out["loss"][j].cpu().numpy()), _bits(r["loss"])), j
    assert np.array_equal(_bits(out["params"][j].cpu().numpy()), _bits(r["out5"])), j
    assert np.array_equal(_bits(out["Q"][j].cpu().numpy()), _bits(r["Q"])), j


def test_fixture_problems_bit_exact_and_vs_reference(fitter, restated):
    """every fixture problem, alone and all twelve in one call; the device's free-running table is the committed one"""
    rows = []
    for d, r in restated:
        out = _call(fitter, [d], 500)
        _same(out, 0, r)
        rows.append(dq_ref.survey_row(d, out["params"][0].cpu().numpy(), out["Q"][0].cpu().numpy()))
    for row in rows:
        dq_ref.check_survey_row(row)
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dq_fits_table.txt")) as f:
        assert f.read() == dq_ref.format_table(rows)
    out = _call(fitter, [d for d, _ in restated], 500)
    for j, (_, r) in enumerate(restated):
        _same(out, j, r)


@pytest.mark.parametrize("views", [1, 2, 63, 64, 65, 128, 129, 256, 257, 1000, 3000])
def test_view_counts_bit_exact(fitter, views):
    """1 ... 3000 views: one, two and four views per lane in registers, then the per-step loop"""
    from odam_amd import sq, synth
    prob = synth.make_sq_problem(views, 700 + views)
    tgt, mask = sq.lines_to_targets(prob["bbox_lines"])
    i5, h = sq.init_dual(prob["translate"], prob["angle"], prob["dims"])
    d = dict(init5=i5, half_dims=h, P=prob["P"].astype(np.float32).reshape(-1, 12), tgt=tgt, mask=mask)
    n_iters = 60
    r = dq_ref.fit32(i5, h, d["P"], tgt, mask, n_iters)
    out = _call(fitter, [d], n_iters, check=False)
    _same(out, 0, r)


@pytest.mark.parametrize("n_obj", [30, 500])
def test_many_objects_any_workgroup_shape(fitter, restated, n_obj):
    """30 and 500 objects in one call (the fixture problems in turn, so 10 ... 300 views side by side), with 1, 2, 4 and 8
    objects per workgroup: every object equals its restatement"""
    ds = [restated[j % len(restated)][0] for j in range(n_obj)]
    try:
        for waves in (1, 2, 4, 8):
            fitter.set_dual_group_waves(waves)
            out = _call(fitter, ds, 500)
            tr, ls, pp, qq = (out[k].cpu().numpy() for k in ("traj", "loss", "params", "Q"))
            for j in range(n_obj):
                r = restated[j % len(restated)][1]
                assert np.array_equal(_bits(tr[j]), _bits(r["traj"])) and np.array_equal(_bits(ls[j]), _bits(r["loss"])), (waves, j)
                assert np.array_equal(_bits(pp[j]), _bits(r["out5"])) and np.array_equal(_bits(qq[j]), _bits(r["Q"])), (waves, j)
            assert (out["status"] == np.array([0, -1])).all()
    finally:
        fitter.set_dual_group_waves(4)


def test_negative_discriminant_status(fitter, restated):
    """one object of the call has a camera inside its ellipsoid: status 1 at step 0 for it alone, the others bit-equal to a call
    without it; the Python layer raises AssertionError as the reference does (sq_libs.py:129,136)"""
    ds = [restated[j][0] for j in (0, 3, 5, 9)]
    bad = dict(restated[3][0])
    bad["P"] = dq_ref.discriminant_problem(restated[3][0])
    with_bad = _call(fitter, [ds[0], bad, ds[2], ds[3]], 500, check=False)
    clean = _call(fitter, ds, 500)
    assert with_bad["status"].tolist() == [[0, -1], [1, 0], [0, -1], [0, -1]]
    for j in (0, 2, 3):
        for k in ("traj", "loss", "params", "Q"):
            assert np.array_equal(_bits(with_bad[k][j].cpu().numpy()), _bits(clean[k][j].cpu().numpy())), (j, k)
    _same(with_bad, 1, dq_ref.fit32(bad["init5"], bad["half_dims"], bad["P"], bad["tgt"], bad["mask"], 500))
    assert np.array_equal(with_bad["params"][1].cpu().numpy(), bad["init5"]) and np.isnan(with_bad["loss"][1].cpu().numpy()).all()
    with pytest.raises(AssertionError):
        _call(fitter, [ds[0], bad], 20)


def test_limits(fitter, restated):
    from odam_amd import _lib
    d = restated[0][0]
    with pytest.raises(_lib.OdamError):
        fitter.fit_dual(d["init5"][None], d["half_dims"][None], [16 * 1024 + 1], np.zeros((16 * 1024 + 1, 12), np.float32),
                        np.zeros((16 * 1024 + 1, 4), np.float32), np.zeros((16 * 1024 + 1, 4), np.float32), n_iters=1)


def test_optim_process_dual_quadric(fitter, fits, golden):
    from odam_amd.multi_view import optim_process
    from odam_amd.processor import OdamProcess
    z = golden("sq_optim.npz")
    tracks = [z[f"track{i}"] for i in range(int(z["n_tracks"]))]
    args = (tracks, [int(x) for x in z["img_names"]], z["T_wcs"], z["P_cws"], 480, 640, z["K"])
    out = optim_process(*args, "dual_quadric", True, 500, 10, fitter=fitter, return_params=True)
    dq_ref.check_optim_process(out, fits, tracks)
    # the device path == the restatement behind the same host logic, bit for bit
    ref = optim_process(*args, "dual_quadric", True, 500, 10, fitter=dq_ref.RefFitter(), return_params=True)
    assert np.array_equal(_bits(out["params"]), _bits(ref["params"]))
    assert all(np.array_equal(_bits(a.Q), _bits(b.Q)) for a, b in zip(out["quadrics"], ref["quadrics"]))
    assert np.array_equal(np.asarray(out["bboxes_qc"]), np.asarray(ref["bboxes_qc"]))
    # n_iters is honoured
    short = optim_process(*args, "dual_quadric", True, 20, 10, fitter=fitter, return_params=True)
    assert not np.array_equal(short["params"][out["fitted"]], out["params"][out["fitted"]])
    # OdamProcess(representation="dual_quadric") reaches it, with the reference's 500 steps
    proc = OdamProcess(None, None, None, None, representation="dual_quadric", fitter=fitter)
    proc.init_sequence(z["K"], 480, 640)
    proc.usable_frames, proc.T_wcs, proc.P_cws = args[1], list(z["T_wcs"]), list(z["P_cws"])
    via = proc.optim_process(tracks, return_params=True)
    assert np.array_equal(_bits(via["params"]), _bits(out["params"]))


def test_super_quadric_on_the_same_tracks_is_unchanged(fitter, oracle, golden):
    """representation="super_quadric" on the tracks of the case above: the values of the existing goldens (sq_optim.npz with
    sq_optim_spread.npz, the bounds of tests/test_sq_gpu.py) and, bit for bit, the CPU oracle's fit behind the same host logic --
    which is what this path returned before "dual_quadric" existed (tests/test_sq_gpu.py pins GPU == oracle)"""
    from odam_amd.multi_view import optim_process
    from test_multi_view_host import OracleFitter
    from test_sq_gpu import check_against_spread
    z = golden("sq_optim.npz")
    tracks = [z[f"track{i}"] for i in range(int(z["n_tracks"]))]
    args = (tracks, [int(x) for x in z["img_names"]], z["T_wcs"], z["P_cws"], 480, 640, z["K"], "super_quadric", True, 200, 10)
    out = optim_process(*args, fitter=fitter, return_params=True)
    assert np.allclose(np.asarray(out["bboxes_dl"]), z["bboxes_dl"], rtol=0, atol=1e-12)
    check_against_spread(out, z["params"], z["bboxes_qc"], golden("sq_optim_spread.npz"))
    ref = optim_process(*args, fitter=OracleFitter(oracle), return_params=True)
    assert np.array_equal(_bits(out["params"]), _bits(ref["params"]))
    assert np.array_equal(np.asarray(out["bboxes_qc"]), np.asarray(ref["bboxes_qc"]))
