"""Host restatement of the association network's forward (odam_amd/csrc/assoc.hip, include/odam_assoc.h: odam_assoc_forward) in
float64, torch on the CPU: frame-index encoding, encoder, the per-track fuser layers, the mean over time, the matching layers on the
[T + 30] row block, the final projection, the score matrix and the optimal transport in log space.  Token-major rows, as the library
keeps them; the weights are the state dict's, under the reference's key names (Conv1d weights [N, K, 1]), unpermuted: head h of
the attention is made of the projected channels h, 4 + h, 8 + h, ...

What belongs to the operation and is therefore NOT done in float64: the product position * div_term of the frame-index encoding is
formed in float32 (prepare_kernel does, and so does the network this one was trained as), from the float32 div_term table the library
is handed (odam_amd/associator.py); sine and cosine of that float32 number are then taken in float64.

All 30 detection slots, the -1 padding included, are rows of the matching layers (keys and queries); only the score matrix is cut to
n_det columns before the optimal transport.

forward() returns every stage by name, so that a test can say WHERE a kernel leaves the float64 values.  mutate= plants one of two
mistakes in the matching layers' attention wherever it has more than 100 keys -- the last key dropped ("drop_last_key") or counted
twice ("dup_last_key"): what a wrong chunk tail in an online softmax does -- for the host test that shows the GPU test's bounds would
see it (tests/test_assoc_ref_host.py)."""
import math

import numpy as np
import torch

D, HEADS, ND = 256, 4, 30
MUTATIONS = (None, "drop_last_key", "dup_last_key")


def div_term():
    """the float32 table odam_amd.associator hands the library as "pe_div_term": torch's float32 exp on THIS host.  Its last bit is the
    host's (vector math libraries differ between CPUs), and at frame index 5000 one ulp of a table entry is 3e-4 in the angle: a forward is
    comparable only with one that was given the same table.  The library on this host gets this one; the reference run of
    tests/golden/assoc_f64.npz stored its own, and the host test hands that to forward()."""
    return torch.exp(torch.arange(0, D, 2).float() * (-math.log(10000.0) / D))


def frame_encoding(position, div=None):
    """position [...] float32 frame indices -> [..., 256] float64: sin in the even channels, cos in the odd ones, of the FLOAT32 product
    with the float32 table div [128] (default: div_term())"""
    div = div_term() if div is None else torch.as_tensor(np.asarray(div, np.float32))
    a = (torch.as_tensor(position, dtype=torch.float32).unsqueeze(-1) * div).double()
    out = torch.empty(a.shape[:-1] + (D,), dtype=torch.float64)
    out[..., 0::2] = torch.sin(a)
    out[..., 1::2] = torch.cos(a)
    return out


class _Weights:
    def __init__(self, sd):
        self.sd = sd

    def lin(self, name, x):
        w = self.sd[name + ".weight"].double()
        return x @ w.reshape(w.shape[0], w.shape[1]).T + self.sd[name + ".bias"].double()


def _attend(q, k, v, mutate=None):
    """q [..., n, 256], k, v [..., m, 256] -> [..., n, 256]: four heads of 64, channel c = 4 d + h, softmax(q k / 8) v"""
    if mutate is not None and k.shape[-2] > 100:
        if mutate == "drop_last_key":
            k, v = k[..., :-1, :], v[..., :-1, :]
        elif mutate == "dup_last_key":
            k, v = torch.cat([k, k[..., -1:, :]], -2), torch.cat([v, v[..., -1:, :]], -2)
        else:
            raise ValueError(mutate)
    split = lambda t: t.reshape(t.shape[:-1] + (D // HEADS, HEADS))
    qh, kh, vh = split(q), split(k), split(v)
    s = torch.einsum("...ndh,...mdh->...hnm", qh, kh) / math.sqrt(D // HEADS)
    p = torch.softmax(s, dim=-1)
    return torch.einsum("...hnm,...mdh->...ndh", p, vh).reshape(q.shape)


def _propagate(W, pre, x, src_of, mutate=None):
    """one attentional propagation layer (weights under `pre`): delta = mlp([x | merge(attention(q(x), k(src), v(src)))]); src_of maps the
    projected keys / values of ALL rows to those a query set sees -- every delta comes from the layer's inputs"""
    q, k, v = (W.lin(pre + f"attn.proj.{i}", x) for i in range(3))
    msg = W.lin(pre + "attn.merge", src_of(q, k, v, mutate))
    h = torch.relu(W.lin(pre + "mlp.0", torch.cat([x, msg], -1)))
    return W.lin(pre + "mlp.2", h)


def sinkhorn(scores, alpha, iters):
    """scores [m, n] float64 -> log assignment [(m + 1), (n + 1)] with the dustbin row and column at score alpha, times (m + n)"""
    m, n = scores.shape
    Z = torch.full((m + 1, n + 1), float(alpha), dtype=torch.float64)
    Z[:m, :n] = scores
    norm = -math.log(m + n)
    log_mu = torch.full((m + 1,), norm, dtype=torch.float64); log_mu[-1] = math.log(n) + norm
    log_nu = torch.full((n + 1,), norm, dtype=torch.float64); log_nu[-1] = math.log(m) + norm
    u, v = torch.zeros(m + 1, dtype=torch.float64), torch.zeros(n + 1, dtype=torch.float64)
    for _ in range(iters):
        u = log_mu - torch.logsumexp(Z + v[None, :], dim=1)
        v = log_nu - torch.logsumexp(Z + u[:, None], dim=0)
    return Z + u[:, None] + v[None, :] - norm


def forward(sd, tracks, detections, n_det, layers, iters=100, mutate=None, div=None):
    """sd: state dict (torch tensors); tracks [T, 79, 100], detections [79, 30] or [1, 79, 30] (float32 values, channel 0 = frame index,
    -1 padding); layers: the matching layers' names ("self" / "cross"), as many as are to be run -- the weights gnn.layers.0 .. are taken
    in order, so a prefix of the list is the network cut after that many layers.  div: the frame-index encoding's float32 table [128]
    (default: div_term(), what the library is handed on this host).
    -> dict of float64 numpy arrays: fused [T + 30, 256] (time means of the fuser output, then the encoded detections), x_after (list, one
    [T + 30, 256] per matching layer), desc [T + 30, 256], scores [T, 30] (with the 1 / 16), Z [(T + 1), (n_det + 1)]."""
    if mutate not in MUTATIONS:
        raise ValueError(mutate)
    W = _Weights(sd)
    tr = torch.as_tensor(np.asarray(tracks, np.float32))
    de = torch.as_tensor(np.asarray(detections, np.float32)).reshape(79, ND)
    T = tr.shape[0]
    n_self = len({k.split(".")[2] for k in sd if k.startswith("fuser.layers.")})
    with torch.no_grad():
        def encode(x):      # [..., 79, L] -> [..., L, 256]
            f = x[..., 1:, :].transpose(-1, -2).double()
            h = torch.relu(W.lin("encoder.0", f))
            return W.lin("encoder.2", h) + frame_encoding(x[..., 0, :], div)
        xt = encode(tr)                                                     # [T, 100, 256]
        xd = encode(de)                                                     # [30, 256]
        for i in range(n_self):
            xt = xt + _propagate(W, f"fuser.layers.{i}.", xt, lambda q, k, v, m: _attend(q, k, v))      # over a track's own time steps
        x = torch.cat([xt.mean(dim=1), xd], 0)                              # the [T + 30] row block
        out = {"fused": x.numpy().copy(), "x_after": []}
        for i, name in enumerate(layers):
            if name not in ("self", "cross"):
                raise ValueError(name)
            cross = name == "cross"

            def src_of(q, k, v, m, cross=cross):
                kt, vt, kd, vd = k[:T], v[:T], k[T:], v[T:]
                a_t = _attend(q[:T], kd, vd, m) if cross else _attend(q[:T], kt, vt, m)
                a_d = _attend(q[T:], kt, vt, m) if cross else _attend(q[T:], kd, vd, m)
                return torch.cat([a_t, a_d], 0)
            x = x + _propagate(W, f"gnn.layers.{i}.", x, src_of, mutate)
            out["x_after"].append(x.numpy().copy())
        desc = W.lin("final_proj", x)
        scores = desc[:T] @ desc[T:].T / math.sqrt(D)
        Z = sinkhorn(scores[:, :n_det], float(sd["bin_score"]), iters)
    out.update(desc=desc.numpy(), scores=scores.numpy(), Z=Z.numpy())
    return out
