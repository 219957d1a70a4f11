"""The batched association forward on the GPU (odam_amd/csrc/assoc_batch.hip, include/odam_assoc.h).

odam_assoc_ot_batch against the float64 iteration (assoc_ref.sinkhorn) within the tolerance of tests/test_assoc_gpu.py --
2e-5 max(1, |ref|max) on Z, twice that on exp(Z) / max(exp(ref), 1) -- on one ragged batch that holds every size at which something
changes: 1 x 1, a few rows, 31 / 32 rows (a sweep of 16-lane rows ends), 127 / 128 rows (with the dustbin: one 64-row column pass more),
300 and 1024 rows (the limit, 140 KB of LDS); the 256-thread form of the kernel is taken when every sample of a launch has at most 127
rows, so dropping the large samples changes the kernel under the small ones -- their bits must not move.

odam_assoc_forward_batch on the batches of tests/golden/assoc_batch.npz against tests/assoc_batch_ref.py (tied to the reference's float64
run by tests/test_assoc_batch_host.py) computed on THIS host's frame-index table, which is the one the library is handed here.  Bounds: the
rule and the factor of tests/test_assoc_f64_gpu.py -- FACTOR = 4 x the reference's own fp32 error of that sample, from the fixture (the
kernels are another fp32 evaluation of the same graph in another summation order); the loss term 4 x the fixture's sum |Z32 - Z64| over
the sample's pairs.  tests/test_assoc_batch_host.py shows that running every sample alone, or padding with 0, moves some sample's Z by
8,000 - 25,000 x that bound.  Every measured error and its ratio to the reference's fp32 error is recorded (conftest.measured:
assoc_batch/...)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import assoc_batch_ref  # noqa: E402
import assoc_ref  # noqa: E402
from make_golden_assoc_batch import BATCHES, THRESHOLD, samples_of  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYERS = ["self", "cross"] * 4
CFG = {"GNN_layers": LAYERS, "self_GNN_layers": ["self", "self"], "sinkhorn_iterations": 100}
FACTOR = 4.0
NAMES = list(BATCHES)
FIX = np.load(os.path.join(HERE, "golden", "assoc_batch.npz"))


@pytest.fixture(scope="module", autouse=True)
def _torch_threads():
    """the float64 restatement runs on the host: as many threads as the environment grants, not as many as the machine has cores"""
    old = torch.get_num_threads()
    env = os.environ.get("OMP_NUM_THREADS", "")
    torch.set_num_threads(int(env) if env.isdigit() and int(env) > 0 else min(16, len(os.sched_getaffinity(0))))
    yield
    torch.set_num_threads(old)


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


# ---- odam_assoc_ot_batch ---------------------------------------------------------------------------------------------------------
OT_SHAPES = [(1, 1), (3, 5), (31, 30), (32, 30), (127, 17), (128, 17), (300, 30), (1024, 30)]
OT_PAD = 3      # the row stride is n + 3; the columns in between hold NaN


def _ot_samples(scale, seed=0):
    """[(m, n, scores [m, n + 3] float32 with NaN behind column n, gt [k, 2])]: k = 0 for the first sample, dustbins written -1, m and n"""
    out = []
    for i, (m, n) in enumerate(OT_SHAPES):
        rng = np.random.default_rng(seed + 1000 * m + n)
        sc = np.full((m, n + OT_PAD), np.nan, np.float32)
        sc[:, :n] = (rng.standard_normal((m, n)) * scale).astype(np.float32)
        k = 0 if i == 0 else int(rng.integers(1, 40))
        gt = np.stack([rng.integers(-1, m + 1, k), rng.integers(-1, n + 1, k)], 1).astype(np.int32).reshape(-1, 2)
        out.append((m, n, sc, gt))
    return out


def _ot_batch(samples, alpha, iters, max_m=None):
    """one launch over `samples` -> ([Z_b float32], loss_terms float64 [B], status int32 [B])"""
    from odam_amd import _lib
    B = len(samples)
    score_off = np.r_[0, np.cumsum([s[2].size for s in samples])].astype(np.int64)
    z_off = np.r_[0, np.cumsum([(m + 1) * (n + 1) for m, n, _, _ in samples])].astype(np.int64)
    gt_off = np.r_[0, np.cumsum([len(s[3]) for s in samples])].astype(np.int32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    scores = dev(np.concatenate([s[2].reshape(-1) for s in samples]))
    gt = dev(np.concatenate([s[3] for s in samples] + [np.zeros((1, 2), np.int32)]))
    d_off, d_zoff, d_gtoff = dev(score_off[:-1]), dev(z_off[:-1]), dev(gt_off)
    d_lds = dev(np.asarray([s[2].shape[1] for s in samples], np.int32))
    d_m, d_n = dev(np.asarray([s[0] for s in samples], np.int32)), dev(np.asarray([s[1] for s in samples], np.int32))
    Z = torch.full((int(z_off[-1]),), 7.0, device=DEV)
    terms = torch.full((B,), 7.0, device=DEV, dtype=torch.float64)
    status = torch.full((B,), 7, device=DEV, dtype=torch.int32)
    _lib.check(_lib.lib().odam_assoc_ot_batch(scores.data_ptr(), d_off.data_ptr(), d_lds.data_ptr(), d_m.data_ptr(), d_n.data_ptr(), B,
                                              max(s[0] for s in samples) if max_m is None else max_m, alpha, iters, gt.data_ptr(),
                                              d_gtoff.data_ptr(), Z.data_ptr(), d_zoff.data_ptr(), terms.data_ptr(), status.data_ptr(), _stream()),
               "odam_assoc_ot_batch")
    Zh = Z.cpu().numpy()
    return [Zh[z_off[b]:z_off[b + 1]].reshape(samples[b][0] + 1, samples[b][1] + 1) for b in range(B)], terms.cpu().numpy(), status.cpu().numpy()


def _pair_order_sum(Z, gt):
    s = 0.0
    for t, d in gt:
        s += -float(Z[Z.shape[0] - 1 if t < 0 else t, Z.shape[1] - 1 if d < 0 else d])
    return s


@pytest.mark.parametrize("iters", [0, 1, 100])
@pytest.mark.parametrize("alpha", [1.0, -0.5])
@pytest.mark.parametrize("scale", [1.0, 8.0])
def test_ot_batch_vs_float64_iteration(measured, scale, alpha, iters):
    samples = _ot_samples(scale)
    Zs, terms, status = _ot_batch(samples, alpha, iters)
    assert status.tolist() == [0] * len(samples)
    worst = 0.0
    for (m, n, sc, gt), Z, term in zip(samples, Zs, terms):
        ref = assoc_ref.sinkhorn(torch.from_numpy(sc[:, :n].astype(np.float64)), alpha, iters).numpy()
        tol = 2e-5 * max(1.0, float(np.abs(ref).max()))
        Zd = Z.astype(np.float64)
        assert np.isfinite(Zd).all()
        err = float(np.abs(Zd - ref).max())
        errp = float((np.abs(np.exp(Zd) - np.exp(ref)) / np.maximum(np.exp(ref), 1.0)).max())
        print(f"scale {scale} alpha {alpha} iters {iters} {m}x{n}: Z err {err:.3e} ({err / tol:.3f} of the bound), exp(Z) err {errp:.3e} ({errp / (2 * tol):.3f})")
        worst = max(worst, err / tol, errp / (2 * tol))
        assert err <= tol, (m, n, err, tol)
        assert errp <= 2 * tol, (m, n, errp, 2 * tol)
        assert term == _pair_order_sum(Z, gt), (m, n)      # exactly: the binary64 sum of the kernel's own Z in pair order
    measured(f"assoc_batch/ot_share_of_bound/s{scale:g}_a{alpha:g}_it{iters}", worst)


def test_ot_batch_bits_do_not_depend_on_the_batch():
    """permuting the batch, dropping samples (which also moves the small samples from the 1024-thread to the 256-thread kernel), a larger
    max_m and a second call leave every Z and loss term bit-identical; a sample whose scores hold a NaN gets status 1 and a zero loss term
    and moves nobody else; a sample outside the launch's limits gets status 2 and nothing else written"""
    samples = _ot_samples(8.0)
    Zs, terms, status = _ot_batch(samples, 1.0, 100)
    same = lambda a, b: a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    Z2, t2, _ = _ot_batch(samples, 1.0, 100)
    assert all(same(a, b) for a, b in zip(Zs, Z2)) and np.array_equal(terms, t2)
    perm = [5, 0, 7, 2, 4, 1, 6, 3]
    Zp, tp, sp = _ot_batch([samples[i] for i in perm], 1.0, 100)
    for j, i in enumerate(perm):
        assert same(Zp[j], Zs[i]) and tp[j] == terms[i] and sp[j] == 0, i
    for keep in ([0, 1, 2, 3, 4], [4, 2], [7], [3, 6], [5, 4]):      # at most 127 rows: the 256-thread kernel; 128 rows and more: 1024 threads
        Zk, tk, _ = _ot_batch([samples[i] for i in keep], 1.0, 100)
        for j, i in enumerate(keep):
            assert same(Zk[j], Zs[i]) and tk[j] == terms[i], (keep, i)
    Zm, tm, _ = _ot_batch([samples[i] for i in (1, 2)], 1.0, 100, max_m=1024)
    assert same(Zm[0], Zs[1]) and same(Zm[1], Zs[2]) and tm[0] == terms[1] and tm[1] == terms[2]
    # NaN status
    m, n, sc, gt = samples[3]
    bad = sc.copy(); bad[7, 3] = np.nan
    Zn, tn, sn = _ot_batch([samples[2], (m, n, bad, gt), samples[4]], 1.0, 100)
    assert sn.tolist() == [0, 1, 0] and tn[1] == 0.0 and np.isnan(Zn[1]).any()
    assert same(Zn[0], Zs[2]) and same(Zn[2], Zs[4]) and tn[0] == terms[2] and tn[2] == terms[4]
    # a sample larger than the launch's max_m is refused by the kernel: status 2, Z left alone (the fill value of _ot_batch)
    Zl, tl, sl = _ot_batch([samples[1], samples[4]], 1.0, 100, max_m=100)
    assert sl.tolist() == [0, 2] and tl[1] == 0.0 and np.all(Zl[1] == 7.0) and same(Zl[0], Zs[1])
    # a pair outside the sample is left out and flagged
    m, n, sc, gt = samples[1]
    Zo, to, so = _ot_batch([(m, n, sc, np.concatenate([gt, [[m + 1, 0]], [[0, -2]]]).astype(np.int32))], 1.0, 100)
    assert so.tolist() == [4] and to[0] == terms[1] and same(Zo[0], Zs[1])


# ---- odam_assoc_forward_batch -------------------------------------------------------------------------------------------------------
def batch_inputs(k):
    samples = samples_of(k, NAMES[k])
    det = -np.ones((len(samples), 79, 30), np.float32)
    for i, s in enumerate(samples):
        det[i, :, :s[1]] = s[4]
    return np.concatenate([s[3] for s in samples]), det, [(s[0], s[1]) for s in samples], [s[5] for s in samples]


@pytest.fixture(scope="module")
def state_dict():
    from odam_amd import weights
    return weights.make_associator_state_dict(2, 8, seed=0)


@pytest.fixture(scope="module")
def float64_forward(state_dict):
    """inputs and the float64 forward per batch on this host's frame-index table, computed once and shared (read only)"""
    cache = {}

    def get(k):
        if k not in cache:
            tr, de, valid, gt = batch_inputs(k)
            cache[k] = (tr, de, valid, gt, assoc_batch_ref.forward(state_dict, tr, de, valid, LAYERS, gt_matches=gt, threshold=THRESHOLD))
        return cache[k]
    return get


def _dump(h, which, rows, cols):
    from odam_amd import _lib
    buf = np.empty((rows, cols), np.float32)
    _lib.check(_lib.lib().odam_assoc_debug_read(h, which, buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_longlong(buf.size)), "odam_assoc_debug_read")
    return buf


def _net(state_dict, max_tracks):
    from odam_amd import associator
    net = associator.Associator(CFG, max_tracks=max_tracks, device=DEV)
    net.load_state_dict(state_dict)
    return net


PARAMS = [(k, merge) for k in range(len(NAMES)) for merge in (1, 0)]


@pytest.mark.parametrize("k,merge", PARAMS, ids=[f"{NAMES[k]}-merge{m}" for k, m in PARAMS])
def test_forward_batch_vs_float64(measured, state_dict, float64_forward, k, merge):
    from odam_amd import _lib, associator
    tr, de, valid, gt, ref = float64_forward(k)
    B, tmax, RT = len(valid), max(T for T, _ in valid), len(valid) * max(T for T, _ in valid)
    R = RT + 30 * B
    old = _lib.get_config("assoc.merge")
    _lib.set_config("assoc.merge", merge)
    tag = "" if merge else "_unfolded"
    failures = []
    try:
        net = _net(state_dict, sum(T for T, _ in valid))
        try:
            Z, z_off, terms, status = net.forward_batch(torch.from_numpy(tr), torch.from_numpy(de), valid, gt)
            h = net._handle()
            padded, desc = _dump(h, 3, R, 256), _dump(h, 4, R, 256)      # (synchronises the device)
            scores = _dump(h, 5, sum(T for T, _ in valid), 32)
            Zh, terms, status = Z.cpu().numpy(), terms.cpu().numpy(), status.cpu().numpy()
        finally:
            net.close()
    finally:
        _lib.set_config("assoc.merge", old)
    assert status.tolist() == [0] * B
    starts = np.r_[0, np.cumsum([T for T, _ in valid])]

    def compare(stage, i, got, want, ref_err, where=None):
        d = np.abs(got.astype(np.float64) - want)
        err = float(d[where].max() if where is not None else d.max())
        name = f"{stage}/{NAMES[k]}{i}{tag}"
        measured(f"assoc_batch/{name}", err)
        measured(f"assoc_batch_ratio/{name}", err / ref_err)
        print(f"batch {NAMES[k]} sample {i} {valid[i]} merge {merge} {stage:7s} err {err:.3e}  reference fp32 {ref_err:.3e}  ratio {err / ref_err:.2f}")
        if not err <= FACTOR * ref_err:
            failures.append((stage, i, err, ref_err, err / ref_err))

    for i, (T, n) in enumerate(valid):
        s = f"b{k}s{i}"
        e_desc, e_scores, e_P, e_Z = (float(v) for v in FIX[f"{s}_err32"])
        # the block as assembled: padding rows exactly -1, the others the time means / encoded detections
        assert np.all(padded[i * tmax + T:(i + 1) * tmax] == -1.0)
        rows = np.r_[i * tmax:(i + 1) * tmax, RT + 30 * i:RT + 30 * (i + 1)]
        compare("padded", i, padded[rows], ref["padded"][rows], e_desc * np.abs(ref["padded"]).max() / np.abs(ref["desc"]).max())
        compare("desc", i, desc[rows], ref["desc"][rows], e_desc)
        compare("scores", i, scores[starts[i]:starts[i + 1], :30], ref["scores"][i], e_scores)
        Zg = Zh[z_off[i]:z_off[i + 1]].reshape(T + 1, n + 1).astype(np.float64)
        assert np.isfinite(Zg).all()
        compare("expZ", i, np.exp(Zg), np.exp(ref["Z"][i]), e_P)
        compare("Z", i, Zg, ref["Z"][i], e_Z, where=ref["Z"][i] > -6)
        compare("loss", i, np.asarray(terms[i]), ref["loss_terms"][i], float(FIX[f"{s}_gt_err32"]))
        assert terms[i] == _pair_order_sum(Zh[z_off[i]:z_off[i + 1]].reshape(T + 1, n + 1), gt[i])
        if int(FIX[f"{s}_robust"]):
            ours = associator.hungarian_matching(torch.from_numpy(Zh[z_off[i]:z_off[i + 1]].reshape(T + 1, n + 1)[:-1, :-1]).exp(), THRESHOLD)
            assert np.array_equal(ours, FIX[f"{s}_matches"][1]) and np.array_equal(ours, FIX[f"{s}_matches"][0]), (i, ours)
    assert not failures, failures


def test_batch_of_one_has_the_launch_sequence_descriptors(state_dict, float64_forward):
    """batch C: one sample, no padding -- the same launches on the same rows as odam_assoc_forward_sequence, so the descriptors are its bits"""
    tr, de, valid, gt, ref = float64_forward(NAMES.index("C"))
    (T, n), = valid
    net = _net(state_dict, T)
    try:
        h = net._handle()
        Zs = net.assignment(torch.from_numpy(tr).to(DEV), torch.from_numpy(de[0]).to(DEV), T, n, sequence=True).cpu().numpy()
        seq = _dump(h, 1, T + 30, 256)
        Z, z_off, _, _ = net.forward_batch(torch.from_numpy(tr), torch.from_numpy(de), valid, gt)
        bat = _dump(h, 4, T + 30, 256)
        Zb = Z.cpu().numpy().reshape(T + 1, n + 1)
    finally:
        net.close()
    assert np.array_equal(seq.view(np.uint32), bat.view(np.uint32))
    e_Z = float(FIX["b2s0_err32"][3])
    big = ref["Z"][0] > -6
    assert np.abs(Zb.astype(np.float64) - ref["Z"][0])[big].max() <= FACTOR * e_Z
    assert np.abs(Zs.astype(np.float64) - ref["Z"][0])[big].max() <= FACTOR * e_Z


def _batch_dict(k, with_gt=True):
    tr, de, valid, gt = batch_inputs(k)
    d = {"tracks": torch.from_numpy(tr), "detections": torch.from_numpy(de), "valid_list": valid}
    if with_gt:
        d["gt_matches"] = [torch.from_numpy(g).long() for g in gt]
    return d


@pytest.mark.parametrize("k", [0, 1, 4], ids=["A", "B", "E"])
def test_matches_equal_scipy_on_the_kernels_own_Z_under_both_settings(state_dict, k):
    """assoc.hungarian = 1 solves the samples inside 32 x 128 on the device behind the transport (batch E's 129 and 127 x 17 are solved by
    scipy on the host either way), 0 solves all of them on the host: every sample's matches equal hungarian_matching on the downloaded Z"""
    from odam_amd import _lib, associator
    old = _lib.get_config("assoc.hungarian")
    net = _net(state_dict, 256)
    try:
        for setting in (0, 1):
            _lib.set_config("assoc.hungarian", setting)
            out = net(_batch_dict(k, with_gt=False), THRESHOLD, eval_only=True)
            for b, (Zb, match) in enumerate(zip(out["pred"], out["matches"])):
                assert np.array_equal(np.asarray(match, np.float64), associator.hungarian_matching(Zb[0][:-1, :-1].exp(), THRESHOLD)), (setting, b)
    finally:
        _lib.set_config("assoc.hungarian", old)
        net.close()


def test_associator_call_on_batch_a(state_dict):
    net = _net(state_dict, 64)
    try:
        d = _batch_dict(0)
        out = net(d, THRESHOLD, eval_only=False)
        assert set(out) == {"pred", "loss", "matches", "loss_terms"}
        assert len(out["pred"]) == len(out["matches"]) == 4 and tuple(out["loss_terms"].shape) == (4,) and out["loss_terms"].dtype == torch.float64
        for (T, n), Zb, match in zip(d["valid_list"], out["pred"], out["matches"]):
            assert tuple(Zb.shape) == (1, T + 1, n + 1) and Zb.dtype == torch.float32 and np.asarray(match).shape == (n,)
        assert torch.is_tensor(out["loss"]) and out["loss"].dim() == 0 and out["loss"].dtype == torch.float64
        assert float(out["loss"]) == sum(out["loss_terms"].tolist()) and float(out["loss"]) > 0
        for i in range(4):
            assert abs(float(out["loss_terms"][i]) - float(FIX[f"b0s{i}_loss"][1])) <= FACTOR * float(FIX[f"b0s{i}_gt_err32"])
        ev = net(_batch_dict(0, with_gt=False), THRESHOLD, eval_only=True)
        assert float(ev["loss"]) == 0.0 and ev["loss_terms"].tolist() == [0.0] * 4
        assert all(torch.equal(a, b) for a, b in zip(ev["pred"], out["pred"]))
        assert all(np.array_equal(a, b) for a, b in zip(ev["matches"], out["matches"]))
        with pytest.raises(KeyError):
            net(_batch_dict(0, with_gt=False), THRESHOLD, eval_only=False)
        # a NaN frame index in one sample's detections (a NaN feature would be dropped by the encoder's fmax-relu): that sample's Z is NaN --
        # the call raises where scipy raises in the reference, naming the sample
        bad = _batch_dict(0)
        bad["detections"][2, 0, 0] = float("nan")
        with pytest.raises(ValueError, match="sample 2"):
            net(bad, THRESHOLD, eval_only=False)
    finally:
        net.close()


def test_validate_in_batches_of_four(state_dict):
    """associator.validate over the 14 samples of the fixture's batches, regrouped four at a time, against the restatement run on the same
    groups: every loss term within 4 x the fixture's sum |Z32 - Z64| of that sample, the correct-detection count equal on every sample whose
    float64 matches survive the fixture's perturbation rule in its new batch, the mean loss and the share accordingly"""
    from odam_amd import associator
    samples, keys = [], []
    for k, name in enumerate(NAMES):
        for i, (T, n, seed, tr, de, gt) in enumerate(samples_of(k, name)):
            samples.append({"tracks": torch.from_numpy(tr), "detections": torch.from_numpy(de), "match": torch.from_numpy(gt).long(),
                            "img_path": f"{name}{i}", "pose": None})
            keys.append(f"b{k}s{i}")
    net = _net(state_dict, 256)
    try:
        got = associator.validate(net, samples, THRESHOLD, 4)
    finally:
        net.close()
    assert len(got["loss_terms"]) == 14
    want_terms, want_correct, robust = [], [], []
    for i0 in range(0, 14, 4):
        batch = associator.collate(samples[i0:i0 + 4])
        ref = assoc_batch_ref.forward(state_dict, batch["tracks"].numpy(), batch["detections"].numpy(), batch["valid_list"], LAYERS,
                                      gt_matches=[g.numpy() for g in batch["gt_matches"]], threshold=THRESHOLD)
        for j, (T, n) in enumerate(batch["valid_list"]):
            want_terms.append(ref["loss_terms"][j])
            want_correct.append(int((ref["matches"][j] == associator.gt_track_of_detections(batch["gt_matches"][j], T, n)).sum()))
            e = 4 * float(FIX[f"{keys[i0 + j]}_err32"][3])
            rs = np.random.RandomState(i0 + j)
            core = ref["Z"][j][:-1, :-1]
            robust.append(all(np.array_equal(assoc_batch_ref.hungarian_matching(np.exp(core + rs.uniform(-e, e, core.shape)), THRESHOLD), ref["matches"][j])
                              for _ in range(8)))
    bound = 0.0
    for i, key in enumerate(keys):
        b = FACTOR * float(FIX[f"{key}_gt_err32"])
        print(f"{key}: loss term {got['loss_terms'][i]:.6f}, float64 {want_terms[i]:.6f}, |diff| {abs(got['loss_terms'][i] - want_terms[i]):.2e}, bound {b:.2e}, robust {robust[i]}")
        assert abs(got["loss_terms"][i] - want_terms[i]) <= b, key
        bound += b
        if robust[i]:
            assert got["correct"][i] == want_correct[i], key
    assert abs(got["loss"] - np.mean(want_terms)) <= bound / 14
    assert got["n_det"] == [n for name in NAMES for _, n in BATCHES[name]]
    if all(robust):
        assert got["accuracy"] == sum(want_correct) / sum(got["n_det"])
