"""tests/assoc_ref.py (the float64 restatement of the association forward that tests/test_assoc_f64_gpu.py holds the kernels to) against
the reference Associator's float64 run (tests/golden/assoc_f64.npz, made by tests/golden/make_golden_assoc_f64.py), and the power of
the GPU test's descriptor bound against a one-key mistake in the matching attention.  CPU only."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import assoc_ref  # noqa: E402
from make_golden_assoc import make_inputs  # noqa: E402
from make_golden_assoc_f64 import desc_rows  # noqa: E402

LAYERS = ["self", "cross"] * 4
DIV = np.load(os.path.join(HERE, "golden", "assoc_f64.npz"))["div_term"]      # the frame-index table of the fixture's reference run (assoc_ref.div_term)
DESC_FACTOR = 4.0        # tests/test_assoc_f64_gpu.py: the kernels' descriptors may leave float64 by 4 x the reference's own fp32 error


@pytest.fixture(scope="module")
def state_dict():
    from odam_amd import weights
    return weights.make_associator_state_dict(2, 8, seed=0)


@pytest.fixture(scope="module")
def plain_forward(state_dict):
    """the unmutated float64 forward per case, computed once -- on the frame-index table of the fixture's reference run"""
    cache = {}

    def get(T, n_det):
        if (T, n_det) not in cache:
            tr, de = make_inputs(T, n_det, 100 + T)
            cache[(T, n_det)] = (tr, de, assoc_ref.forward(state_dict, tr, de, n_det, LAYERS, div=DIV))
        return cache[(T, n_det)]
    return get


def _cases():
    z = np.load(os.path.join(HERE, "golden", "assoc_f64.npz"))
    return [(i, int(T), int(n)) for i, (T, n) in enumerate(z["cases"])]


@pytest.mark.parametrize("ci,T,n_det", [c for c in _cases() if c[1] <= 300], ids=lambda v: str(v))
def test_restatement_equals_the_reference_float64_run(golden, plain_forward, ci, T, n_det):
    """Z, the score matrix and the stored descriptor rows of assoc_ref.forward equal the reference's float64 run to 1e-9 (absolute; the
    values reach 11.6 at the descriptors and 116 at the scores, so this is 1e-10 relative and better: two float64 evaluations in another
    order).  Every case of the fixture that stores arrays; T = 1024 stores the reference's fp32 error only (its arrays would double the
    file), and the restatement has no path of its own for it."""
    z = golden("assoc_f64.npz")
    _, _, r = plain_forward(T, n_det)
    assert r["Z"].shape == z[f"c{ci}_Z64"].shape == (T + 1, n_det + 1)
    assert r["scores"].shape == z[f"c{ci}_scores64"].shape == (T, 30)
    assert r["desc"].shape == (T + 30, 256) and len(r["x_after"]) == 8 and r["fused"].shape == (T + 30, 256)
    assert np.abs(r["desc"][desc_rows(T + 30)] - z[f"c{ci}_desc64"]).max() <= 1e-9
    assert np.abs(r["scores"] - z[f"c{ci}_scores64"]).max() <= 1e-9
    assert np.abs(r["Z"] - z[f"c{ci}_Z64"]).max() <= 1e-9
    # what the fixture says about the reference's fp32 run is about these values
    assert np.isclose(np.abs(r["desc"]).max(), z[f"c{ci}_max"][0], rtol=1e-9) and np.isclose(np.abs(r["scores"]).max(), z[f"c{ci}_max"][1], rtol=1e-9)


@pytest.mark.parametrize("mutate", ["drop_last_key", "dup_last_key"])
@pytest.mark.parametrize("T,n_det", [(129, 17), (300, 30)])
def test_descriptor_bound_sees_a_one_key_mistake(golden, state_dict, plain_forward, T, n_det, mutate):
    """The power of the GPU test: one key of the matching attention dropped, or counted twice, wherever it has more than 100 keys (the tail
    of the online softmax's last 64-key chunk) moves the final descriptors by at least 50 x the bound the GPU test holds the kernels'
    descriptors to at that case (4 x the reference's own fp32 error, from the fixture).  A condition on the test's inputs, not a
    tolerance: if it fails, the inputs are too bland to show the mistake and have to change, not the factor."""
    z = golden("assoc_f64.npz")
    ci = [c for c, t, n in _cases() if (t, n) == (T, n_det)][0]
    bound = DESC_FACTOR * float(z[f"c{ci}_err32"][0])
    tr, de, r = plain_forward(T, n_det)
    m = assoc_ref.forward(state_dict, tr, de, n_det, LAYERS, mutate=mutate, div=DIV)
    moved = float(np.abs(m["desc"] - r["desc"]).max())
    print(f"T {T} {mutate}: desc moved {moved:.3e}, GPU bound {bound:.3e}, ratio {moved / bound:.0f}; "
          f"exp(Z) moved {np.abs(np.exp(m['Z']) - np.exp(r['Z'])).max():.3e}")
    assert moved >= 50.0 * bound, (moved, bound)
    # the mutation touches nothing before the first matching layer with more than 100 keys, and no layer at or below 100 keys
    assert np.array_equal(m["fused"], r["fused"])
    small = assoc_ref.forward(state_dict, tr[:99], de, n_det, LAYERS[:2], mutate=mutate, div=DIV)
    plain = assoc_ref.forward(state_dict, tr[:99], de, n_det, LAYERS[:2], div=DIV)
    assert np.array_equal(small["desc"], plain["desc"])


def test_prefix_of_the_layer_list_is_the_network_cut_there(state_dict, plain_forward):
    """what the GPU test's stage comparison rests on: with the first K names of the layer list the restatement computes x_after[K - 1] of
    the full forward as its last row block (K = 0: fused), bit for bit, and applies the final projection to it"""
    tr, de, full = plain_forward(65, 30)
    for K in (0, 1, 2):
        cut = assoc_ref.forward(state_dict, tr, de, 30, LAYERS[:K], div=DIV)
        assert len(cut["x_after"]) == K
        last = cut["x_after"][-1] if K else cut["fused"]
        assert np.array_equal(last, full["x_after"][K - 1] if K else full["fused"])


def test_frame_encoding_takes_the_float32_product():
    """position * div_term is a float32 product (the operation's definition); its sine and cosine are float64"""
    pos = np.array([[5000.0, -1.0, 390.0, 0.0]], np.float32)
    e = assoc_ref.frame_encoding(pos).numpy()
    a32 = (torch.from_numpy(pos).unsqueeze(-1) * assoc_ref.div_term()).numpy()
    assert a32.dtype == np.float32 and e.dtype == np.float64 and e.shape == (1, 4, 256)
    assert np.abs(e[..., 0::2] - np.sin(a32.astype(np.float64))).max() <= 1e-15
    assert np.abs(e[..., 1::2] - np.cos(a32.astype(np.float64))).max() <= 1e-15
    # ... which is NOT the float64 product: at frame 5000 the two differ by far more than the 1e-9 the restatement is tied with
    a64 = pos.astype(np.float64)[..., None] * assoc_ref.div_term().double().numpy()
    assert np.abs(np.sin(a64) - e[..., 0::2]).max() > 1e-5
