"""Resumable super-quadric fits without a GPU: the step-loop restatement (tests/sq_resume_ref.py) held to the CPU oracle, the
bookkeeping of optim_process(resume=...) / OdamProcess.refine with a stub fitter, and the ctypes signature of odam_sq_fit_resume."""
import ctypes
import logging
import os
import re

import numpy as np
import pytest
import torch

import sq_resume_ref as ref
from conftest import REPO


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _golden_cases(golden):
    z = golden("sq_steps.npz")
    for c in range(int(z["n_cases"])):
        yield c, {k[len(f"c{c}_"):]: z[k] for k in z.files if k.startswith(f"c{c}_")}


@pytest.fixture(scope="module")
def table():
    return ref.adam_table(200)


# ---- the restatement is the oracle's fit -------------------------------------------------------------------------------------------
def test_restatement_equals_oracle_fit_on_the_golden_problems(oracle, golden, table):
    """the reference-generated problems of sq_steps.npz, 200 uninterrupted steps, as the goldens were made (super_quadric, prior):
    parameters after every step, loss_2d of every step and the end state, bit for bit"""
    for c, d in _golden_cases(golden):
        cls = int(d["cls"])
        op, otraj, oloss = oracle.fit(d["p0"], d["P"], d["tgt"], d["mask"], cls, n_iters=200, want_traj=True, want_loss=True)
        f = ref.Fit(d["p0"])
        traj, loss = ref.run(oracle, f, d["P"], d["tgt"], d["mask"], cls, 200, table)
        assert np.array_equal(_bits(traj), _bits(otraj)), c
        assert np.array_equal(_bits(loss), _bits(oloss)), c
        assert np.array_equal(_bits(f.p), _bits(op)) and f.t == 200
        assert np.array_equal(_bits(f.s0), _bits(d["p0"][4:7]))


@pytest.mark.parametrize("rep", ["super_quadric", "cube", "quadric"])
@pytest.mark.parametrize("prior", [True, False])
def test_restatement_equals_oracle_fit_in_every_representation(oracle, golden, table, rep, prior):
    """the same problems in all three representations (cube starts from shape logits -10000, sq_libs.py:362-371), with and without
    the scale prior, 60 steps"""
    for c, d in _golden_cases(golden):
        p0 = d["p0"].copy()
        if rep == "cube":
            p0[7:] = -10000.0
        cls = int(d["cls"]) if prior else -1
        op, otraj, oloss = oracle.fit(p0, d["P"], d["tgt"], d["mask"], cls, n_iters=60, representation=ref.REP[rep], want_traj=True,
                                      want_loss=True)
        f = ref.Fit(p0, rep)
        traj, loss = ref.run(oracle, f, d["P"], d["tgt"], d["mask"], cls, 60, table)
        assert np.array_equal(_bits(traj), _bits(otraj)), c
        assert np.array_equal(_bits(loss), _bits(oloss)), c
        assert np.array_equal(_bits(f.p), _bits(op))
        if rep != "super_quadric":
            assert np.array_equal(_bits(traj[:, 7:]), _bits(np.repeat(p0[None, 7:], 60, 0)))


@pytest.mark.parametrize("k", [1, 37, 199])
def test_split_and_continue_inside_the_restatement_equals_uninterrupted(oracle, golden, table, k):
    """k steps, the state through its 32-float row and back, 200 - k more steps == 200 steps"""
    _, d = next(_golden_cases(golden))
    cls = int(d["cls"])
    whole = ref.Fit(d["p0"])
    wt, wl = ref.run(oracle, whole, d["P"], d["tgt"], d["mask"], cls, 200, table)
    a = ref.Fit(d["p0"])
    t1, l1 = ref.run(oracle, a, d["P"], d["tgt"], d["mask"], cls, k, table)
    row = a.row()
    assert row[30] == k and row[31] == 0 and np.array_equal(_bits(row[27:30]), _bits(d["p0"][4:7]))
    b = ref.Fit.from_row(row)
    t2, l2 = ref.run(oracle, b, d["P"], d["tgt"], d["mask"], cls, 200 - k, table)
    assert np.array_equal(_bits(np.concatenate([t1, t2])), _bits(wt))
    assert np.array_equal(_bits(np.concatenate([l1, l2])), _bits(wl))
    assert np.array_equal(_bits(b.row()), _bits(whole.row()))
    with pytest.raises(ValueError):
        ref.run(oracle, b, d["P"], d["tgt"], d["mask"], cls, 1, table)      # step 201 of a 200-row table


# ---- bookkeeping of optim_process(resume=...) and OdamProcess.refine ---------------------------------------------------------------
class StubFitter:
    """SqFitter's interface without a fit: parameters stay where they start, the state counts the steps, every call is recorded"""

    def __init__(self, oracle):
        self.o = oracle
        self.calls = []

    def fit(self, params0, class_ids, view_counts, P, tgt, mask, n_iters=200, representation="super_quadric", prior=True,
            want_points=True, state=None, want_state=False, **kw):
        from odam_amd import sq
        n = len(view_counts)
        st = sq.cold_state(params0, representation) if state is None else np.array(torch.as_tensor(state).cpu().numpy(), np.float32)
        assert st.shape == (n, 32)
        self.calls.append(dict(n=n, view_counts=list(view_counts), t0=st[:, 30].astype(int).tolist(), had_state=state is not None,
                               want_state=want_state, n_iters=n_iters, params0=np.array(params0, np.float32)))
        out_st = st.copy()
        out_st[:, 30] += n_iters
        out = {"params": torch.from_numpy(out_st[:, :9].copy()),
               "points": torch.from_numpy(np.stack([self.o.points(p) for p in out_st[:, :9]]))}
        if want_state:
            out["state"] = torch.from_numpy(out_st)
        return out

    def points(self, params):
        return torch.from_numpy(np.stack([self.o.points(p) for p in np.asarray(params).reshape(-1, 9)]))


@pytest.fixture(scope="module")
def scene(golden):
    z = golden("sq_optim.npz")
    tracks = [z[f"track{i}"] for i in range(int(z["n_tracks"]))]
    return dict(tracks=tracks, img_names=[int(x) for x in z["img_names"]], T_wcs=z["T_wcs"], P_cws=z["P_cws"], K=z["K"], img_h=480, img_w=640)


def _optim(sc, tracks, fitter, representation="super_quadric", n_iters=40, **kw):
    from odam_amd.multi_view import optim_process
    return optim_process(tracks, sc["img_names"], sc["T_wcs"], sc["P_cws"], sc["img_h"], sc["img_w"], sc["K"], representation, True,
                         n_iters, 10, fitter=fitter, return_params=True, **kw)


def _grown(sc):
    """the scene's tracks cut to their first rows so that at least one fitted track of the full scene is still below 10 views"""
    full = sc["tracks"]
    early = [t[:max(1, len(t) // 3)] if i % 2 else t for i, t in enumerate(full)]
    return early, full


def test_optim_process_resumes_known_tracks_and_starts_the_others_cold(scene, oracle):
    early, full = _grown(scene)
    fit = StubFitter(oracle)
    plain = _optim(scene, early, fit)
    assert "state" not in plain and not fit.calls[-1]["had_state"] and not fit.calls[-1]["want_state"]      # the call it always was
    o1 = _optim(scene, early, fit, return_state=True)
    s1 = o1["state"]
    ids1 = s1["track_ids"].tolist()
    assert ids1 == np.flatnonzero(o1["fitted"]).tolist() and s1["representation"] == "super_quadric"
    assert fit.calls[-1]["t0"] == [0] * len(ids1) and fit.calls[-1]["want_state"]
    assert torch.as_tensor(s1["state"])[:, 30].tolist() == [40.0] * len(ids1)
    o2 = _optim(scene, full, fit, n_iters=25, resume=s1, return_state=True)
    ids2 = o2["state"]["track_ids"].tolist()
    new = [i for i in ids2 if i not in ids1]
    assert set(ids1) < set(ids2) and new, (ids1, ids2)      # tracks that were below n_views the first time are fitted now
    assert fit.calls[-1]["t0"] == [40 if i in ids1 else 0 for i in ids2]
    assert torch.as_tensor(o2["state"]["state"])[:, 30].tolist() == [65.0 if i in ids1 else 25.0 for i in ids2]
    # a cold track inside a resumed call gets the row of a fit that has not begun: its own initial parameters
    cold = _optim(scene, full, fit, return_state=True)
    assert np.array_equal(_bits(fit.calls[-2]["params0"]), _bits(fit.calls[-1]["params0"]))
    # view counts follow the CURRENT tracks, for resumed tracks too
    assert fit.calls[-2]["view_counts"] == fit.calls[-1]["view_counts"]
    # resume without return_state: continues, returns no state
    o3 = _optim(scene, full, fit, n_iters=5, resume=o2["state"])
    assert "state" not in o3 and fit.calls[-1]["t0"] == [65 if i in ids1 else 25 for i in ids2]
    # a resume that names none of the fitted tracks: all cold
    none = {"state": np.zeros((0, 32), np.float32), "track_ids": np.zeros(0, np.int64), "representation": "super_quadric"}
    _optim(scene, full, fit, resume=none)
    assert fit.calls[-1]["t0"] == [0] * len(ids2)


def test_optim_process_refuses_what_it_cannot_resume(scene, oracle):
    early, full = _grown(scene)
    fit = StubFitter(oracle)
    s1 = _optim(scene, full, fit, return_state=True)["state"]
    n_calls = len(fit.calls)
    with pytest.raises(ValueError, match="super_quadric.*cube"):
        _optim(scene, full, fit, representation="cube", resume=s1)
    beyond = dict(s1, track_ids=np.concatenate([s1["track_ids"][:-1], [len(full)]]))
    with pytest.raises(ValueError, match=f"track {len(full)}.*{len(full)} tracks"):
        _optim(scene, full, fit, resume=beyond)
    with pytest.raises(ValueError, match="dual_quadric"):
        _optim(scene, full, fit, representation="dual_quadric", resume=s1)
    with pytest.raises(ValueError, match="dual_quadric"):
        _optim(scene, full, fit, representation="dual_quadric", return_state=True)
    assert len(fit.calls) == n_calls      # refused before any fit


def _process(scene, oracle, tracks):
    from odam_amd.processor import OdamProcess
    proc = OdamProcess(None, None, None, None)
    proc.init_sequence(scene["K"], scene["img_h"], scene["img_w"])
    proc.tracks = [t.copy() for t in tracks]
    proc.usable_frames, proc.T_wcs, proc.P_cws = scene["img_names"], scene["T_wcs"], scene["P_cws"]
    proc.fitter = StubFitter(oracle)
    proc.refine_fitter = StubFitter(oracle)
    return proc


def test_refine_keeps_its_state_in_the_process_and_optim_process_never_reads_it(scene, oracle, monkeypatch, caplog):
    early, full = _grown(scene)
    proc = _process(scene, oracle, early)
    r1 = proc.refine(n_iters=40)
    assert set(r1) == {"tracks", "bboxes_qc", "bboxes_dl", "quadrics"}
    ids1 = proc._refine_state["track_ids"].tolist()
    assert proc.refine_fitter.calls[-1]["t0"] == [0] * len(ids1)
    proc.tracks = [t.copy() for t in full]      # the scan goes on: longer tracks, same indices
    proc.refine(n_iters=40)
    ids2 = proc._refine_state["track_ids"].tolist()
    assert proc.refine_fitter.calls[-1]["t0"] == [40 if i in ids1 else 0 for i in ids2] and set(ids1) < set(ids2)
    # the offline call: its own fitter, 200 steps from the detector's guess, no state in or out
    out = proc.optim_process(proc.tracks)
    c = proc.fitter.calls[-1]
    assert not c["had_state"] and not c["want_state"] and c["n_iters"] == 200 and "state" not in out
    assert len(proc.refine_fitter.calls) == 2 and proc._refine_state["track_ids"].tolist() == ids2
    # merge_process drops the state, with a log line
    from odam_amd import merge
    monkeypatch.setattr(merge, "merge_process", lambda data, frames: ["merged"])
    with caplog.at_level(logging.INFO, logger="OdamProcess"):
        assert proc.merge_process(out) == ["merged"]
    assert proc._refine_state is None
    assert any("Dropping the fit state" in r.getMessage() for r in caplog.records)
    proc.refine(n_iters=40)
    assert proc.refine_fitter.calls[-1]["t0"] == [0] * len(ids2)      # cold again
    # init_sequence clears it
    assert proc._refine_state is not None
    proc.init_sequence(scene["K"], scene["img_h"], scene["img_w"])
    assert proc._refine_state is None
    # the dual quadric is out of scope
    proc.representation = "dual_quadric"
    with pytest.raises(ValueError, match="dual_quadric"):
        proc.refine()


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
C_TO_CTYPES = {"int": ctypes.c_int, "float": ctypes.c_float}


def _declared(name, txt):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, f"{name} is not declared in include/odam_sq.h"
    want, names = [], []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        names.append(arg.split()[-1].lstrip("*"))
        want.append(ctypes.c_void_p if "*" in arg else C_TO_CTYPES[arg.replace("const ", "").rsplit(" ", 1)[0]])
    return names, want


def test_fit_resume_ctypes_signature_matches_the_header():
    """the argument list sq.py gives ctypes for odam_sq_fit_resume is the header's, argument by argument: odam_sq_fit_batch's arguments
    in their order, then state_in, t0, state_out before the stream -- and odam_sq_fit_batch's own declaration has not moved"""
    from odam_amd import _lib, sq
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "odam_sq.h")).read(), flags=re.S)
    batch_names, _ = _declared("odam_sq_fit_batch", txt)
    assert batch_names == ["ctx", "n_obj", "init_params", "class_id", "view_offsets", "P", "tgt", "mask", "prior_icov", "n_iters",
                           "representation", "max_views", "out_params", "out_points", "loss_log", "traj", "stream"]
    names, want = _declared("odam_sq_fit_resume", txt)
    assert names == batch_names[:-1] + ["state_in", "t0", "state_out", "stream"]
    assert sq.FIT_RESUME_ARGTYPES == want
    assert re.search(r"#define\s+ODAM_SQ_STATE_FLOATS\s+32\b", txt) and sq.STATE_FLOATS == 32
    f = sq._fit_resume_entry()
    assert list(f.argtypes) == want and f.restype is ctypes.c_int
    # argument checks come before any device work: a null context is code 1 with a message
    assert f(None, 1, None, None, None, None, None, None, None, 10, 0, 4, None, None, None, None, None, None, None, None) == 1
    assert b"odam_sq_fit_resume" in _lib.lib().odam_last_error()


def test_cold_state_rows():
    from odam_amd import sq
    p0 = np.arange(18, dtype=np.float32).reshape(2, 9)
    st = sq.cold_state(p0, "quadric")
    assert st.shape == (2, 32) and st.dtype == np.float32
    assert np.array_equal(st[:, :9], p0) and not st[:, 9:27].any() and np.array_equal(st[:, 27:30], p0[:, 4:7])
    assert st[:, 30].tolist() == [0, 0] and st[:, 31].tolist() == [2, 2]
