"""The association network's kernels (odam_amd/csrc/assoc.hip) against the float64 restatement of the forward (tests/assoc_ref.py, tied to
the reference Associator's float64 run by tests/test_assoc_ref_host.py) past 64 tracks, stage by stage: the sizes at which stage_attn's
online softmax runs over several 64-key chunks, stage_gemm's last 16-row block is ragged, gnn_rowpart_kernel deals short or empty row
shares to the XCDs, the launch sequence calls launch_attention_d64 with Lq = Lk = T, and the Sinkhorn step changes kernels.

Stages without an entry point of their own: a handle built with the first K names of GNN_layers, and the same weights, computes exactly
the first K matching layers; after its forward the row block X (odam_assoc_debug_read, which = 0) holds x_after[K - 1] in its columns
0 .. 255 (K = 0: the fused tracks and encoded detections).  K = 0, 1 (a self layer), 2 (self, then cross) and 8 (everything).

Bounds.  The reference's own fp32 run leaves its float64 run by c<i>_err32 of tests/golden/assoc_f64.npz at the descriptors, the scores,
exp(Z) and Z (where Z64 > -6); the kernels are another fp32 evaluation of the same graph in another summation order (a four-way K split,
MFMA blocks, an online softmax), so twice that is what to expect and FACTOR = 4 leaves another factor of two of headroom.  The stages
before the descriptors have no fp32 reference run: they are held to 4 x the descriptor error of the case, scaled by
max |stage| / max |desc| of the float64 values.  tests/test_assoc_ref_host.py shows that a one-key mistake in the matching attention past
100 keys moves the descriptors by 140 - 330 x that bound.  Every measured error and its ratio to the reference's fp32 error is recorded
(conftest.measured: assoc_f64/<stage>/<path>/T<T>, assoc_f64_ratio/...).

Measured on an MI355X (profiles/assoc_f64_test_measured.json), largest ratio to the reference's fp32 error over all cases and paths:
fused 1.96, x_after0 1.64, x_after1 1.66, x_after7 1.33, desc 1.49, scores 1.94, exp(Z) 2.34 (2.7e-5 at most,
where entries of the dustbin row reach n_det = 30), Z 1.16 -- no stage needs more than the factor 4.  With the last key dropped
in stage_attn past 100 tracks (an experiment, profiles/assoc_f64_planted_mistake.txt) the same test fails from x_after0 on with ratios of
200 - 1700.

The float64 values are computed on this host with the frame-index table this host's torch computes (assoc_ref.div_term), which is
the table odam_amd.associator hands the library here; the fixture's float64 arrays belong to the table of the host that made them and
are not used.

T = 1024 (the native limit): final outputs only.  The fixture holds the reference's fp32 error for it but no arrays (they would double
the file); the float64 values come from the restatement, as at every other size."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYERS = ["self", "cross"] * 4
FACTOR = 4.0
# (T, n_det): why
CASES = [(3, 30),                                  # 33 rows, R = 5: XCD 6 holds 3 rows and XCD 7 none
         (63, 30), (64, 30), (65, 30),             # one key chunk not full; exactly full; one chunk plus a single key
         (98, 5),                                  # 128 rows: a multiple of both 16 and 8
         (99, 30),                                 # 129 rows: a last 16-row block with a single row
         (127, 17), (128, 17), (129, 17),          # the Sinkhorn kernel switch (128 rows with the dustbin); two chunks full; two chunks plus one key
         (300, 30),                                # five chunks; the sixteen-wave Sinkhorn kernel
         (1024, 30)]                               # the native limit
MERGE0_CASES = [(65, 30), (129, 17), (300, 30)]
PARAMS = [(T, n, 1) for T, n in CASES] + [(T, n, 0) for T, n in MERGE0_CASES]


@pytest.fixture(scope="module", autouse=True)
def _torch_threads():
    """the float64 restatement runs on the host: as many threads as the environment grants, not as many as the machine has cores"""
    old = torch.get_num_threads()
    env = os.environ.get("OMP_NUM_THREADS", "")
    torch.set_num_threads(int(env) if env.isdigit() and int(env) > 0 else min(16, len(os.sched_getaffinity(0))))
    yield
    torch.set_num_threads(old)


@pytest.fixture(scope="module")
def state_dict():
    from odam_amd import weights
    return weights.make_associator_state_dict(2, 8, seed=0)


@pytest.fixture(scope="module")
def float64_forward(state_dict):
    """inputs and the float64 forward per case, computed once and shared by the folded and the unfolded run of a case (read only)"""
    import assoc_ref
    from make_golden_assoc import make_inputs
    cache = {}

    def get(T, n_det):
        if (T, n_det) not in cache:
            tr, de = make_inputs(T, n_det, 100 + T)
            cache[(T, n_det)] = (tr, de, assoc_ref.forward(state_dict, tr, de, n_det, LAYERS))
        return cache[(T, n_det)]
    return get


def _dump(h, which, rows, cols):
    from odam_amd import _lib
    buf = np.empty((rows, cols), np.float32)
    _lib.check(_lib.lib().odam_assoc_debug_read(h, which, buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_longlong(buf.size)), "odam_assoc_debug_read")
    return buf


def _decisive(P64):
    """the margin rule of test_process_sequence_with_network: no entry within 1e-3 of a threshold, no two candidates of a detection or of
    a track within 1e-3 of each other"""
    core = P64[:-1, :-1]
    m = min(np.abs(core - 0.1).min(), np.abs(core - 0.2).min())
    for mat in (core, core.T):
        if mat.shape[0] > 1:
            srt = np.sort(mat, axis=0)
            m = min(m, (srt[-1] - srt[-2]).min())
    return m > 1e-3


@pytest.mark.parametrize("T,n_det,merge", PARAMS, ids=[f"T{T}-n{n}-merge{m}" for T, n, m in PARAMS])
def test_forward_vs_float64_stage_by_stage(golden, measured, state_dict, float64_forward, T, n_det, merge):
    """Every path of the forward against float64 at every stage: odam_config assoc.persist = 2 (rows dealt to the XCDs, the default) and
    the launch sequence (what assoc.persist = 0 makes of every forward: odam_assoc_forward_sequence on the same handle); assoc.persist = 1
    (device-wide barriers) must equal 2 bit for bit at every stage, as it does at the sizes of tests/test_assoc_gpu.py.  merge = 1: the
    attention's merge projection folded into the MLP (default); 0: as its own layer.  Also: Z finite, of the right shape, and the
    Hungarian matches from our Z equal to those from the float64 Z wherever the float64 decision does not hang on a tie."""
    from odam_amd import _lib, associator
    z = golden("assoc_f64.npz")
    ci = [i for i, c in enumerate(z["cases"]) if tuple(c) == (T, n_det)][0]
    e_desc, e_scores, e_P, e_Z = (float(v) for v in z[f"c{ci}_err32"])
    tr, de, ref = float64_forward(T, n_det)
    tr_d, de_d = torch.from_numpy(tr).to(DEV), torch.from_numpy(de).to(DEV)
    L = _lib.lib()
    old = (_lib.get_config("assoc.merge"), _lib.get_config("assoc.persist"))
    tag = "" if merge else "_unfolded"
    failures = []

    def compare(stage, path, got, want, ref_err, where=None):
        d = np.abs(got.astype(np.float64) - want)
        err = float(d[where].max() if where is not None else d.max())
        measured(f"assoc_f64/{stage}/{path}{tag}/T{T}", err)
        measured(f"assoc_f64_ratio/{stage}/{path}{tag}/T{T}", err / ref_err)
        print(f"T {T} n_det {n_det} merge {merge} {stage:10s} {path:8s} err {err:.3e}  reference fp32 {ref_err:.3e}  ratio {err / ref_err:.2f}")
        if not err <= FACTOR * ref_err:
            failures.append((stage, path, err, ref_err, err / ref_err))

    try:
        for K in ((8,) if T == 1024 else (0, 1, 2, 8)):
            _lib.set_config("assoc.merge", merge); _lib.set_config("assoc.persist", 2)
            net = associator.Associator({"GNN_layers": LAYERS[:K], "self_GNN_layers": ["self", "self"], "sinkhorn_iterations": 100},
                                        max_tracks=T, device=DEV)
            net.load_state_dict(state_dict)      # the weights of the first K matching layers are read from the one 8-layer state dict
            try:
                h = net._handle()
                on = ctypes.c_int()
                _lib.check(L.odam_assoc_info(h, ctypes.byref(on), None, None), "odam_assoc_info")
                assert on.value == 1, "the persistent matching kernel is not in use on this device"
                out = {}
                for path, persist, sequence in (("persist2", 2, False), ("persist1", 1, False), ("sequence", 2, True)):
                    _lib.set_config("assoc.persist", persist)      # which persistent kernel: read at every launch
                    Z = net.assignment(tr_d, de_d, T, n_det, sequence=sequence)
                    X = _dump(h, 0, T + 30, 512)[:, :256]           # (synchronises the device)
                    out[path] = {"Z": Z.cpu().numpy(), "X": X, "desc": _dump(h, 1, T + 30, 256), "scores": _dump(h, 2, T, 32)[:, :30]}
                lost = ctypes.c_uint()
                _lib.check(L.odam_assoc_lost_launches(h, ctypes.byref(lost)), "odam_assoc_lost_launches")
                assert lost.value == 0
            finally:
                net.close()
            for k in ("Z", "X", "desc", "scores"):
                assert np.array_equal(out["persist1"][k].view(np.uint32), out["persist2"][k].view(np.uint32)), (K, k)
            stage, want = ("fused", ref["fused"]) if K == 0 else (f"x_after{K - 1}", ref["x_after"][K - 1])
            e_stage = e_desc * np.abs(want).max() / np.abs(ref["desc"]).max()
            for path in ("persist2", "sequence"):
                o = out[path]
                assert np.isfinite(o["X"]).all()
                compare(stage, path, o["X"], want, e_stage)
                if K < 8:
                    continue
                Zg = o["Z"].astype(np.float64)
                assert Zg.shape == (T + 1, n_det + 1) and np.isfinite(Zg).all()
                compare("desc", path, o["desc"], ref["desc"], e_desc)
                compare("scores", path, o["scores"], ref["scores"], e_scores)
                compare("expZ", path, np.exp(Zg), np.exp(ref["Z"]), e_P)
                compare("Z", path, Zg, ref["Z"], e_Z, where=ref["Z"] > -6)
                if _decisive(np.exp(ref["Z"])):
                    ours = associator.hungarian_matching(torch.from_numpy(np.exp(Zg[:-1, :-1])), 0.1)
                    theirs = associator.hungarian_matching(torch.from_numpy(np.exp(ref["Z"][:-1, :-1])), 0.1)
                    assert np.array_equal(ours, theirs), path
    finally:
        _lib.set_config("assoc.merge", old[0]); _lib.set_config("assoc.persist", old[1])
    assert not failures, failures
