"""Golden for the sampler's C ABI: the reference's own sampling.cpp, compiled as it lies by `make -C oracle ref` into
oracle/_ref/libodam_ref_sampler.so, called through `sample_on_batch`.  Stores inputs + outputs of
  abi_c<k>_*   -- the seven (B, M, N, buffer_size, seed) cases of tests/test_abi.py (full etas / omegas),
  pipe_*       -- 300 (a, e) pairs through the pipeline's call (B = M = 1, N = 1000, buffer 201, seed 0) for
                  tests/test_sq_oracle.py; per pair the sha256 of etas || omegas (float32 bytes), which pins every bit
                  in 32 bytes instead of 8000.
Run: make -C oracle ref && python tests/golden/make_golden_ref_sampler.py"""
import ctypes
import hashlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
ABI_CASES = ((1, 1, 1000, 201, 0), (2, 3, 257, 201, 0), (3, 2, 1000, 101, 7), (1, 5, 64, 513, 123456),
             (4, 1, 1, 2, 1), (1, 2, 2048, 3, 99), (2, 2, 100, 1001, 2 ** 31 - 1))


def sample_on_batch(L, shapes, eps, N, buffer_size, seed):
    fp = ctypes.POINTER(ctypes.c_float)
    B, M = shapes.shape[:2]
    et = np.full((B, M, N), np.nan, np.float32); om = np.full((B, M, N), np.nan, np.float32)
    L.sample_on_batch.restype = None
    L.sample_on_batch.argtypes = [fp, fp, fp, fp] + [ctypes.c_int] * 5
    L.sample_on_batch(shapes.ctypes.data_as(fp), eps.ctypes.data_as(fp), et.ctypes.data_as(fp), om.ctypes.data_as(fp),
                      B, M, N, buffer_size, seed)
    return et, om


def digest(et, om):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(et, np.float32).tobytes() +
                                        np.ascontiguousarray(om, np.float32).tobytes()).digest(), np.uint8)


def main():
    L = ctypes.CDLL(os.path.join(REPO, "oracle", "_ref", "libodam_ref_sampler.so"))
    out = {"abi_cases": np.array(ABI_CASES, np.int64)}
    rs = np.random.RandomState(5)
    for k, (B, M, N, nbuf, seed) in enumerate(ABI_CASES):
        shapes = rs.uniform(0.02, 1.6, (B, M, 3)).astype(np.float32)
        eps = rs.uniform(0.2, 1.6, (B, M, 2)).astype(np.float32)
        et, om = sample_on_batch(L, shapes.copy(), eps.copy(), N, nbuf, seed)
        out.update({f"abi_c{k}_shapes": shapes, f"abi_c{k}_eps": eps, f"abi_c{k}_etas": et, f"abi_c{k}_omegas": om})
    rs = np.random.RandomState(5)
    a_, e_, d_ = [], [], []
    for _ in range(300):
        a = rs.uniform(0.02, 1.6, 3).astype(np.float32); e = rs.uniform(0.2, 1.6, 2).astype(np.float32)
        et, om = sample_on_batch(L, a[None, None].copy(), e[None, None].copy(), 1000, 201, 0)
        a_.append(a); e_.append(e); d_.append(digest(et[0, 0], om[0, 0]))
    out.update(pipe_a=np.stack(a_), pipe_e=np.stack(e_), pipe_sha256=np.stack(d_))
    np.savez_compressed(os.path.join(HERE, "ref_sampler.npz"), **out)


if __name__ == "__main__":
    main()
