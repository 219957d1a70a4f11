"""The argument contract of the association's stand-alone C entry points (include/odam_assoc.h): odam_assoc_sinkhorn,
odam_assoc_hungarian and the creation of a track-window store.  Every call here is refused before the library touches the
device (dummy non-null pointers are never dereferenced), so the file runs without a GPU.  What the same entries compute
when they accept is in tests/test_assoc_gpu.py and tests/test_track_input_gpu.py."""
import ctypes

import pytest

P = ctypes.c_void_p(16)      # a pointer that only has to be non-null
N = None                     # a null pointer
F = ctypes.c_float
D = ctypes.c_double
LDS_LIMIT = 150 * 1024       # bytes of dynamic LDS the library enables for the two LDS-resident Sinkhorn kernels


@pytest.fixture(scope="module")
def L():
    from odam_amd import _lib
    return _lib.lib()


def sk(scores=P, lds=None, m=5, n=7, alpha=1.0, iters=100, out=P):
    return (scores, n if lds is None else lds, m, n, F(alpha), iters, out, N)


def hg(T, n, Z=P, ldz=None, out=P, status=P):
    return (Z, T, n, n if ldz is None else ldz, D(0.1), 0, out, status, N)


def general_need(m, n):
    """bytes of LDS of the general kernel: the (m+1) x (n+1) couplings, u and v in float32 (csrc/assoc_sinkhorn.hip)"""
    return 4 * ((m + 1) * (n + 1) + (m + 1) + (n + 1))


# (entry, arguments, return code, fragments of odam_last_error())
CASES = [
    ("odam_assoc_sinkhorn", sk(scores=N), 1, ["bad argument"]),
    ("odam_assoc_sinkhorn", sk(out=N), 1, ["bad argument"]),
    ("odam_assoc_sinkhorn", sk(m=0), 1, ["bad argument"]),
    ("odam_assoc_sinkhorn", sk(n=0, lds=4), 1, ["bad argument"]),
    ("odam_assoc_sinkhorn", sk(m=5, n=7, lds=6), 1, ["lds", "at least n"]),
    ("odam_assoc_sinkhorn", sk(m=5, n=7, lds=-1), 1, ["lds", "at least n"]),
    ("odam_assoc_sinkhorn", sk(iters=-1), 1, ["iters", "at least 0"]),
    # (m+1)(n+1) = 36000 exactly, which the entry admitted before it counted u and v: 216 KB against the 150 KB enabled
    ("odam_assoc_sinkhorn", sk(m=1, n=17999), 1, ["%d bytes of LDS" % general_need(1, 17999), "limit is %d" % LDS_LIMIT]),
    ("odam_assoc_sinkhorn", sk(m=2, n=11999), 1, ["%d bytes of LDS" % general_need(2, 11999), "limit is %d" % LDS_LIMIT]),
    ("odam_assoc_sinkhorn", sk(m=17999, n=1), 1, ["%d bytes of LDS" % general_need(17999, 1), "limit is %d" % LDS_LIMIT]),
    # one row past the largest 33-column problem that fits: 1129 x 33 + 1129 + 33 floats
    ("odam_assoc_sinkhorn", sk(m=1128, n=32), 1, ["%d bytes of LDS" % general_need(1128, 32), "limit is %d" % LDS_LIMIT]),
    ("odam_assoc_sinkhorn", sk(m=2 ** 31 - 1, n=2 ** 31 - 1, lds=2 ** 31 - 1), 1, ["bytes of LDS", "limit is %d" % LDS_LIMIT]),
    ("odam_assoc_hungarian", hg(33, 128), 3, ["more than 32 x 128"]),
    ("odam_assoc_hungarian", hg(32, 129), 3, ["more than 32 x 128"]),
    ("odam_assoc_hungarian", hg(128, 33), 3, ["more than 32 x 128"]),
    ("odam_assoc_hungarian", hg(129, 32), 3, ["more than 32 x 128"]),
    ("odam_assoc_hungarian", hg(40, 33), 3, ["more than 32 x 128"]),
    ("odam_assoc_hungarian", hg(4, 3, Z=N), 1, ["bad argument"]),
    ("odam_assoc_hungarian", hg(4, 3, out=N), 1, ["bad argument"]),
    ("odam_assoc_hungarian", hg(4, 3, status=N), 1, ["bad argument"]),
    ("odam_assoc_hungarian", hg(4, 3, ldz=2), 1, ["bad argument"]),
    ("odam_assoc_hungarian", hg(-1, 3), 1, ["bad argument"]),
    ("odam_trackwin_append", (N, 1, P, P, N), 1, ["bad argument"]),
]


@pytest.mark.parametrize("entry,args,code,fragments", CASES, ids=["%s-%d" % (c[0], i) for i, c in enumerate(CASES)])
def test_assoc_entry_argument_contract(L, entry, args, code, fragments):
    assert getattr(L, entry)(*args) == code
    err = L.odam_last_error().decode()
    assert err.startswith(entry + ":"), err
    for f in fragments:
        assert f in err, err


def test_the_oversized_case_is_one_the_old_check_admitted():
    """the first LDS cases above sit at (m+1)(n+1) = 36000, the bound the entry used to test: they are refused for the LDS alone"""
    for m, n in ((1, 17999), (2, 11999), (17999, 1)):
        assert (m + 1) * (n + 1) <= 36000 and general_need(m, n) > LDS_LIMIT
    assert general_need(1127, 32) <= LDS_LIMIT < general_need(1128, 32)      # tests/test_assoc_gpu.py runs 1127 x 32


@pytest.mark.parametrize("max_tracks,window", [(0, 100), (4097, 100), (8, 0), (8, 129), (8, -1)])
def test_trackwin_create_refuses(L, max_tracks, window):
    h = ctypes.c_void_p(0)
    assert L.odam_trackwin_create(max_tracks, window, ctypes.byref(h)) == 1
    assert L.odam_last_error().decode().startswith("odam_trackwin_create:")
    assert not h.value
