"""Resumable super-quadric fits on the GPU (odam_sq_fit_resume through SqFitter.fit(state=, want_state=)): a fit of n steps equals a
fit of k steps followed by a resumed fit of n - k steps on the same views, bit for bit, on every output -- on every launch shape --
and where the views change between launches the result is the step-loop restatement's (tests/sq_resume_ref.py, held to the CPU
oracle in tests/test_sq_resume_host.py)."""
import ctypes

import numpy as np
import pytest
import torch

import sq_resume_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("params", "points", "loss", "traj", "state")


@pytest.fixture(scope="module")
def fitter():
    from odam_amd import sq
    f = sq.SqFitter(DEV, 200)
    yield f
    f.close()


@pytest.fixture(scope="module")
def table():
    return ref.adam_table(200)


def _pack(probs, rep="super_quadric"):
    from odam_amd import sq
    p0 = np.stack([sq.init_params(p["translate"], p["angle"], p["dims"], rep) for p in probs])
    tm = [sq.lines_to_targets(p["bbox_lines"]) for p in probs]
    P = np.concatenate([p["P"].astype(np.float32).reshape(-1, 12) for p in probs])
    tgt = np.concatenate([t for t, _ in tm]); mask = np.concatenate([m for _, m in tm])
    return p0, [p["class_id"] for p in probs], [len(p["P"]) for p in probs], P, tgt, mask


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _chain(fitter, pack, steps, **kw):
    """the fit in len(steps) launches, each resumed from the one before: outputs of the last launch, loss / traj concatenated"""
    outs, st = [], None
    for n in steps:
        o = fitter.fit(*pack, n_iters=n, want_loss=True, want_traj=True, want_state=True, state=st, **kw)
        st = o["state"]
        outs.append(o)
    last = dict(outs[-1])
    last["loss"] = torch.cat([o["loss"] for o in outs], 1)
    last["traj"] = torch.cat([o["traj"] for o in outs], 1)
    return last


def _same(a, b):
    for k in KEYS:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


VIEWS = [1, 3, 10, 64, 65, 300, 300, 17]
CONFIGS = {"super_quadric with prior": ("super_quadric", True), "cube without prior": ("cube", False), "quadric with prior": ("quadric", True)}
_whole = {}


def _eight(fitter, name):
    """the 8-object problem of a configuration and its uninterrupted 200-step fit (computed once, never modified)"""
    from odam_amd import synth
    rep, prior = CONFIGS[name]
    pack = _pack([synth.make_sq_problem(F, 300 + 7 * i + F) for i, F in enumerate(VIEWS)], rep)
    if name not in _whole:
        _whole[name] = _chain(fitter, pack, [200], representation=rep, prior=prior)
    return pack, dict(representation=rep, prior=prior), _whole[name]


@pytest.mark.parametrize("k", [1, 37, 199])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_split_equals_whole(fitter, config, k):
    pack, kw, whole = _eight(fitter, config)
    assert whole["state"].shape == (8, 32)
    assert whole["state"][:, 30].tolist() == [200.0] * 8 and whole["state"][:, 31].tolist() == [float(ref.REP[kw["representation"]])] * 8
    assert torch.equal(whole["state"][:, :9], whole["params"])
    assert torch.equal(whole["state"][:, 27:30], torch.from_numpy(pack[0][:, 4:7]).to(DEV))      # scales_init: the first launch's
    _same(_chain(fitter, pack, [k, 200 - k], **kw), whole)


def test_the_resumable_entry_with_null_state_is_the_cold_fit(fitter):
    """want_state alone goes through odam_sq_fit_resume with a null state_in; fit() without the new arguments through
    odam_sq_fit_batch: the same bits, and no "state" key in the call that did not ask"""
    pack, kw, whole = _eight(fitter, "super_quadric with prior")
    plain = fitter.fit(*pack, n_iters=200, want_loss=True, want_traj=True, **kw)
    assert "state" not in plain
    for k in KEYS[:-1]:
        assert torch.equal(plain[k], whole[k]), k


def test_three_way_chain(fitter):
    pack, kw, whole = _eight(fitter, "super_quadric with prior")
    _same(_chain(fitter, pack, [60, 60, 80], **kw), whole)


def test_state_is_accepted_from_the_host(fitter):
    pack, kw, whole = _eight(fitter, "super_quadric with prior")
    a = fitter.fit(*pack, n_iters=60, want_state=True, **kw)
    b = fitter.fit(*pack, n_iters=140, want_state=True, state=a["state"].cpu().numpy(), **kw)
    assert torch.equal(b["state"], whole["state"]) and torch.equal(b["points"], whole["points"])


def test_several_workgroups_per_object(fitter):
    """2 objects x 300 views: the launch takes the view split (every workgroup loads the state, one stores it)"""
    from odam_amd import synth
    pack = _pack([synth.make_sq_problem(300, 41), synth.make_sq_problem(300, 42)])
    whole = _chain(fitter, pack, [120])
    assert fitter.last_launch()["split"] > 1, fitter.last_launch()
    parts = _chain(fitter, pack, [50, 70])
    assert fitter.last_launch()["split"] > 1      # the resumed launch is shaped as the cold one
    _same(parts, whole)


@pytest.mark.parametrize("n,views,shape", [(200, "unequal", dict(threads=1024, split=1, ordered=False)),
                                           (300, "unequal", dict(threads=1024, split=1, ordered=True)),
                                           (300, "equal", dict(threads=512, split=1, ordered=False))],
                         ids=["200 objects, one workgroup each", "300 objects, longest first", "300 objects, two workgroups per CU"])
def test_mixed_launch_shapes(fitter, n, views, shape):
    """a state made by a launch of 2 objects (view split) continues inside a launch of n objects that start cold around it: one
    workgroup per object; with more objects than CUs dealt longest first (unequal views) or two workgroups per CU (equal views)"""
    from odam_amd import sq, synth
    two = [synth.make_sq_problem(96, 51), synth.make_sq_problem(96, 52)]
    pack2 = _pack(two)
    whole = _chain(fitter, pack2, [100])
    first = fitter.fit(*pack2, n_iters=40, want_state=True)
    assert fitter.last_launch()["split"] > 1
    at = (5, n - 50)
    cache = {F: synth.make_sq_problem(F, 600 + F) for F in sorted({96 if views == "equal" else 10 + (i * 7) % 61 for i in range(n)})}
    probs = [cache[96 if views == "equal" else 10 + (i * 7) % 61] for i in range(n)]
    for j, i in enumerate(at):
        probs[i] = two[j]
    pack = _pack(probs)
    st = torch.from_numpy(sq.cold_state(pack[0], "super_quadric")).to(DEV)
    st[list(at)] = first["state"]
    o = fitter.fit(*pack, n_iters=60, want_state=True, want_traj=True, state=st)
    got = fitter.last_launch()
    assert got["grid"] == n and {k: got[k] for k in shape} == shape, got
    idx = torch.tensor(at, device=DEV)
    for k in ("params", "points", "state"):
        assert torch.equal(o[k][idx], whole[k]), k
    assert torch.equal(o["traj"][idx], whole["traj"][:, 40:])
    # the objects around them: 60 steps from cold, as in a launch of their own
    assert o["state"][:, 30].tolist() == [100.0 if i in at else 60.0 for i in range(n)]
    cold = fitter.fit(*pack, n_iters=60)
    others = torch.tensor([i for i in range(n) if i not in at], device=DEV)
    assert torch.equal(o["params"][others], cold["params"][others])


def test_grouped_path(fitter):
    """one object of 1100 views (more than one workgroup's 1024 rows: _fit_grouped), beside a small one"""
    from odam_amd import synth
    pack = _pack([synth.make_sq_problem(1100, 61), synth.make_sq_problem(12, 62)])
    whole = _chain(fitter, pack, [80])
    _same(_chain(fitter, pack, [40, 40]), whole)


def _one(seed, F):
    from odam_amd import synth
    pr = synth.make_sq_problem(F, seed)
    return pr, _pack([pr])


def test_grown_view_set(fitter, oracle, table):
    """100 steps on the first 12 views of a 30-view object, then 100 on all 30: the restatement's bits; and not the cold fit's"""
    pr, (p0, cls, vc, P, tgt, mask) = _one(71, 30)
    a = fitter.fit(p0, cls, [12], P[:12], tgt[:12], mask[:12], n_iters=100, want_loss=True, want_state=True)
    b = fitter.fit(p0, cls, [30], P, tgt, mask, n_iters=100, want_loss=True, want_state=True, state=a["state"])
    f = ref.Fit(p0[0])
    _, l1 = ref.run(oracle, f, P[:12], tgt[:12], mask[:12], cls[0], 100, table)
    assert np.array_equal(_bits(a["state"].cpu().numpy()[0]), _bits(f.row()))
    _, l2 = ref.run(oracle, f, P, tgt, mask, cls[0], 100, table)
    assert np.array_equal(_bits(b["params"].cpu().numpy()[0]), _bits(f.p))
    assert np.array_equal(_bits(a["loss"].cpu().numpy()[0]), _bits(l1)) and np.array_equal(_bits(b["loss"].cpu().numpy()[0]), _bits(l2))
    assert np.array_equal(_bits(b["state"].cpu().numpy()[0]), _bits(f.row()))
    cold = fitter.fit(p0, cls, [30], P, tgt, mask, n_iters=200)
    assert np.abs(cold["params"].cpu().numpy()[0] - b["params"].cpu().numpy()[0]).max() > 0      # the state was used


def test_scales_init_is_carried(fitter, oracle, table):
    """the prior is measured from words 27..29, not from the parameters a resumed launch starts at"""
    moved = None
    for seed in range(80, 100):      # an object whose scales move by more than 1e-3 in its first 50 steps (found with the restatement)
        pr, pack = _one(seed, 14)
        f = ref.Fit(pack[0][0])
        ref.run(oracle, f, pack[3], pack[4], pack[5], pack[1][0], 50, table)
        if np.abs(f.p[4:7] - f.s0).max() > 1e-3:
            moved = (pack, f)
            break
    assert moved is not None
    (p0, cls, vc, P, tgt, mask), f = moved
    a = fitter.fit(p0, cls, vc, P, tgt, mask, n_iters=50, want_state=True)
    assert np.array_equal(_bits(a["state"].cpu().numpy()[0]), _bits(f.row()))
    true = fitter.fit(p0, cls, vc, P, tgt, mask, n_iters=50, want_state=True, state=a["state"])
    wrong_state = a["state"].clone()
    wrong_state[:, 27:30] = wrong_state[:, 4:7]      # "the prior restarts at the current scales"
    wrong = fitter.fit(p0, cls, vc, P, tgt, mask, n_iters=50, want_state=True, state=wrong_state)
    ref.run(oracle, f, P, tgt, mask, cls[0], 50, table)
    assert np.array_equal(_bits(true["state"].cpu().numpy()[0]), _bits(f.row()))
    assert not torch.equal(true["params"], wrong["params"])
    # without prior the words are carried and change nothing
    n1 = fitter.fit(p0, cls, vc, P, tgt, mask, n_iters=50, prior=False, want_state=True)
    ws = n1["state"].clone()
    ws[:, 27:30] = ws[:, 4:7]
    assert torch.equal(fitter.fit(p0, cls, vc, P, tgt, mask, n_iters=50, prior=False, state=n1["state"])["params"],
                       fitter.fit(p0, cls, vc, P, tgt, mask, n_iters=50, prior=False, state=ws)["params"])


def test_limits(fitter):
    """t0 + n_iters > max_iters: ODAM_E_LIMIT, both numbers named, nothing launched"""
    from odam_amd import _lib, sq
    pr, (p0, cls, vc, P, tgt, mask) = _one(91, 6)
    a = fitter.fit(p0, cls, vc, P, tgt, mask, n_iters=150, want_state=True)
    with pytest.raises(_lib.OdamError, match=r"150 steps.*51 more.*201.*max_iters 200"):
        fitter.fit(p0, cls, vc, P, tgt, mask, n_iters=51, state=a["state"])
    fitter.fit(p0, cls, vc, P, tgt, mask, n_iters=50, state=a["state"])      # exactly the table's length is allowed
    with pytest.raises(ValueError, match="'super_quadric'.*'cube'"):
        fitter.fit(p0, cls, vc, P, tgt, mask, n_iters=10, representation="cube", state=a["state"])
    # the entry point itself: the check is made on the host array before anything is enqueued
    dev = lambda x, dt: torch.as_tensor(x).to(device=DEV, dtype=dt).contiguous()
    d = [dev(p0, torch.float32), dev(np.asarray(cls, np.int32), torch.int32), dev(np.array([0, vc[0]], np.int32), torch.int32),
         dev(P, torch.float32), dev(tgt, torch.float32), dev(mask, torch.float32), fitter._prior_dev()]
    sentinel = torch.full((1, 9), -12345.0, device=DEV)
    st_out = torch.full((1, 32), -12345.0, device=DEV)
    t0 = np.array([150], np.int32)
    rc = sq._fit_resume_entry()(fitter._h, 1, *[_lib.ptr(x) for x in d], 51, 0, vc[0], _lib.ptr(sentinel), None, None, None,
                                _lib.ptr(a["state"]), t0.ctypes.data_as(ctypes.c_void_p), _lib.ptr(st_out),
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 3
    msg = _lib.lib().odam_last_error().decode()
    assert "201" in msg and "200" in msg, msg
    torch.cuda.synchronize()
    assert (sentinel == -12345.0).all() and (st_out == -12345.0).all()


def test_online_chain(oracle):
    """the 40-frame whole-chain sequence in chunks of 10 frames with OdamProcess.refine(50) after each chunk: association is untouched,
    the state after four refines is the restatement's on the same four view sets, and the offline optim_process at the end returns
    what it returns in a run that never refined"""
    import os, sys
    from conftest import REPO
    from odam_amd import associator, detector, sq, synth, transforms, weights
    from odam_amd.processor import OdamProcess
    from test_e2e import SEQ
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import scene_weights
    seq = synth.make_sequence(**SEQ)
    det = detector.Detector(max_batch=8, device=DEV, n_streams=1)
    det.load_state_dict(weights.make_state_dict(seed=0, scene=True))
    net = associator.Associator({"GNN_layers": ["self", "cross"] * 4, "self_GNN_layers": ["self", "self"], "sinkhorn_iterations": 100},
                                max_tracks=64, device=DEV)
    net.load_state_dict(scene_weights.make_scene_associator_state_dict(2, 8, seed=0))
    from PIL import Image
    names, T = list(seq["img_names"]), list(seq["T_wcs"])

    def run(refine):
        proc = OdamProcess(det, net, transforms.Transforms(size=SEQ["h"]), None)
        proc.init_sequence(seq["K"], SEQ["h"], SEQ["w"])
        dets = [np.asarray(r, np.float64).reshape(-1, 79) for r in proc.detect_frames([Image.fromarray(f) for f in seq["frames"]], names)]
        calls = []
        for c in range(0, 40, 10):
            proc.process_frames(names[c:c + 10], T[c:c + 10], dets[c:c + 10])
            if refine:
                if proc.refine_fitter is None:      # record what every refine hands the fitter
                    proc.refine_fitter = sq.SqFitter(DEV, 200)
                    fit = proc.refine_fitter.fit
                    proc.refine_fitter.fit = lambda *a, **kw: calls.append((a, kw)) or fit(*a, **kw)
                proc.refine(n_iters=50)
                calls[-1] = calls[-1] + (proc._refine_state["track_ids"].copy(),)
        return proc, calls

    plain, _ = run(False)
    proc, calls = run(True)
    assert len(proc.tracks) == len(plain.tracks) and len(calls) == 4
    for a, b in zip(proc.tracks, plain.tracks):
        assert a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    # the restatement, driven with the four view sets the fitter was given
    table = ref.adam_table(200)
    fits = {}
    for (a, kw, ids) in calls:
        p0, cls, vc, P, tgt, mask = a
        off = 0
        for j, t in enumerate(ids.tolist()):
            F = vc[j]
            if t not in fits:
                fits[t] = ref.Fit(p0[j])
            ref.run(oracle, fits[t], P[off:off + F], tgt[off:off + F], mask[off:off + F], int(cls[j]), 50, table)
            off += F
    st = proc._refine_state
    ids = st["track_ids"].tolist()
    assert len(ids) >= 8 and {fits[t].t for t in ids} >= {200} and len(calls[0][2]) < len(ids)      # tracks joined on the way
    got = st["state"].cpu().numpy()
    for j, t in enumerate(ids):
        assert np.array_equal(_bits(got[j]), _bits(fits[t].row())), t
    # the offline chain's fit: untouched by the refines
    o1, o2 = proc.optim_process(proc.tracks, return_params=True), plain.optim_process(plain.tracks, return_params=True)
    assert np.array_equal(_bits(o1["params"]), _bits(o2["params"])) and np.array_equal(o1["fitted"], o2["fitted"])
    assert np.array_equal(np.asarray(o1["bboxes_qc"]), np.asarray(o2["bboxes_qc"]))
    proc.refine_fitter.close(); net.close(); det.close()
