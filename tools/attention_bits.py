#!/usr/bin/env python3
"""Digests of the attention output (odam_op_attention_hd, the detector's launcher and kernel choice) on fixed inputs, to compare two
builds of the library bit for bit (ODAM_AMD_LIB picks the build):

   python tools/attention_bits.py

One line per case with the SHA-256 of the output buffer: head dim {32, 64} x {fp32, bf16} x {no mask, mask} x four shapes that reach
a single key, a tile boundary (64 / 65), a ragged last tile of the 64-key and the 32-key tiling (850), a query block boundary (129)
and, with the mask, a leading 32-key block that is all padding.  Inputs come from numpy's default_rng and are rounded to bf16 here,
so the bytes do not depend on the torch build; the output rows are 8 elements wider than E and one row longer than B Lq, prefilled
with a sentinel and hashed whole.  The config switches stay at their defaults."""
import ctypes
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1, 4, 1, 1), (2, 4, 33, 64), (1, 8, 100, 65), (2, 4, 129, 850)]      # B, H, Lq, Lk


def key_mask(B, Lk):
    """non-zero = padded: the ragged tail (3 + 5 b keys of batch b), keys 40 and 45, and the whole of keys 0 .. 31 -- where that
    leaves a key (Lk = 1: nothing is padded, the kernel still takes its mask path)"""
    m = np.zeros((B, Lk), np.uint8)
    if Lk >= 64:
        m[:, :32] = 1
        m[:, [40, 45]] = 1
        for b in range(B):
            m[b, Lk - (3 + 5 * b):] = 1
    return m


def to_bf16_bits(x):
    u = x.view(np.uint32)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)      # round to nearest even (finite inputs)


def main():
    import torch
    from odam_amd import _lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    for D in (32, 64):
        for dt in ("fp32", "bf16"):
            for masked in (0, 1):
                for case, (B, H, Lq, Lk) in enumerate(SHAPES):
                    E = H * D
                    rng = np.random.default_rng(1000 * D + 100 * (dt == "bf16") + 10 * masked + case)
                    host = [rng.standard_normal((B * n, E), dtype=np.float32) for n in (Lq, Lk, Lk)]
                    if dt == "bf16":
                        dev = [torch.from_numpy(to_bf16_bits(x).view(np.int16)).view(torch.bfloat16).to("cuda:0") for x in host]
                    else:
                        dev = [torch.from_numpy(x).to("cuda:0") for x in host]
                    q, k, v = dev
                    ldo = E + 8
                    o = torch.full((B * Lq + 1, ldo), -12345.0, dtype=q.dtype, device="cuda:0")
                    m = torch.from_numpy(key_mask(B, Lk)).to("cuda:0") if masked else None
                    _lib.check(_lib.lib().odam_op_attention_hd(p(q), E, p(k), E, p(v), E, p(o), ldo, B, H, Lq, Lk, D, int(dt == "bf16"),
                                                               p(m), st), "attention_hd")
                    torch.cuda.synchronize()
                    raw = o.cpu().view(torch.int16 if dt == "bf16" else torch.int32).numpy().tobytes()
                    print(f"d={D} {dt} mask={masked} B={B} H={H} Lq={Lq} Lk={Lk} sha256={hashlib.sha256(raw).hexdigest()}", flush=True)


if __name__ == "__main__":
    main()
