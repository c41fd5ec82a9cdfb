"""CPU checks of the plane segmentation's interface (lio_segment_plane, lio_plane_sample_triples): declared in the
header, exported by the library, listed in the binding; the host-only sampler equal to its restatement in Python
integers; the compute entry failing loudly (LIO_ERR_NODEV) without a device — there is no CPU path behind it —
and mirrored in Python with the reference's defaults (post_process/clustering.py:21-28)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from lio_gpu import _capi
from lio_gpu import filters as FL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = 2**64 - 1


def test_header_declares_both_entries_and_the_contract():
    src = open(os.path.join(ROOT, "include", "lio_gpu.h")).read()
    decl = re.search(r"int\s+lio_segment_plane\s*\(([^)]*)\)\s*;", src)
    assert decl, "lio_segment_plane is not declared"
    args = " ".join(decl.group(1).split())
    for piece in ("lio_filter* f", "const float* pts", "int64_t n", "int stride", "float distance_threshold",
                  "int ransac_n", "int64_t num_iterations", "uint64_t seed", "const int32_t* triples_opt",
                  "float* plane4_out", "int64_t* best_iteration", "int32_t* inliers_out", "int64_t* n_inliers",
                  "uint8_t* mask_opt", "int64_t* counts_opt", "uint64_t* sq_opt", "uint8_t* degenerate_opt",
                  "double* refit4_opt"):
        assert piece in args, piece
    decl = re.search(r"int\s+lio_plane_sample_triples\s*\(([^)]*)\)\s*;", src)
    assert decl, "lio_plane_sample_triples is not declared"
    args = " ".join(decl.group(1).split())
    for piece in ("uint64_t seed", "int64_t n", "int64_t num_iterations", "int32_t* out"):
        assert piece in args, piece
    # the tie-break between equal scores and the departures from Open3D are stated as the library's contract
    assert re.search(r"lowest hypothesis index", src, flags=re.I)
    assert re.search(r"all K hypotheses are always evaluated", src)
    assert re.search(r"inliers are\s+\*?\s*those of the winning hypothesis plane", src)


def test_symbols_are_exported_and_bound():
    L = _capi.lib()
    for name, nargs in (("lio_segment_plane", 18), ("lio_plane_sample_triples", 4)):
        assert name in _capi.EXPORTS
        assert hasattr(L, name)
        fn = getattr(L, name)
        assert fn.argtypes and len(fn.argtypes) == nargs and fn.restype is C.c_int


# ------------------------------------------------------------------ the sampler
def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def ref_triples(seed, n, k):
    def r(c):
        return _mix((seed + (c + 1) * 0x9E3779B97F4A7C15) & M64)

    out = np.zeros((k, 3), np.int64)
    for t in range(k):
        i0 = r(3 * t) % n
        i1 = r(3 * t + 1) % (n - 1)
        if i1 >= i0:
            i1 += 1
        i2 = r(3 * t + 2) % (n - 2)
        lo, hi = min(i0, i1), max(i0, i1)
        if i2 >= lo:
            i2 += 1
        if i2 >= hi:
            i2 += 1
        out[t] = (i0, i1, i2)
    return out


def lib_triples(seed, n, k):
    out = np.full((k, 3), -7, np.int32)
    rc = _capi.lib().lio_plane_sample_triples(seed, n, k, out.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, _capi.lib().lio_last_error()
    return out


@pytest.mark.parametrize("seed", [0, 7, M64])
@pytest.mark.parametrize("n,ks", [(3, (1, 257, 1000)), (4, (1, 257, 1000)), (5, (1, 257, 1000)), (64, (1, 257, 1000)),
                                  (4097, (1, 257, 1000)), (2**31 - 1, (64,))])
def test_sampler_equals_its_restatement(seed, n, ks):
    for k in ks:
        got = lib_triples(seed, n, k)
        ref = ref_triples(seed, n, k)
        np.testing.assert_array_equal(got.astype(np.int64), ref, err_msg=f"seed={seed} n={n} K={k}")
        assert (got >= 0).all() and (got.astype(np.int64) < n).all()
        assert (got[:, 0] != got[:, 1]).all() and (got[:, 0] != got[:, 2]).all() and (got[:, 1] != got[:, 2]).all()
        if n == 3:  # every triple is a permutation of (0, 1, 2)
            np.testing.assert_array_equal(np.sort(got, 1), np.tile([0, 1, 2], (k, 1)))
    if n == 64:  # a prefix of a longer run: hypothesis t depends on (seed, t) alone
        np.testing.assert_array_equal(lib_triples(seed, n, 1000)[:257], lib_triples(seed, n, 257))


def test_sampler_arguments():
    L = _capi.lib()
    out = np.full((4, 3), -7, np.int32)
    p = out.ctypes.data_as(C.POINTER(C.c_int32))
    for n in (0, 1, 2):  # legal: no hypothesis, nothing written
        assert L.lio_plane_sample_triples(1, n, 4, p) == 0
        assert (out == -7).all()
    assert L.lio_plane_sample_triples(1, 10, 0, None) == 0
    for n, k, q in ((-1, 4, p), (2**31, 4, p), (10, -1, p), (10, 2**20 + 1, p), (10, 4, None)):
        assert L.lio_plane_sample_triples(1, n, k, q) == _capi.LIO_ERR_ARG
        assert b"lio_plane_sample_triples" in L.lio_last_error()
    np.testing.assert_array_equal(FL.sample_triples(7, 64, 5).astype(np.int64), ref_triples(7, 64, 5))
    assert FL.sample_triples(7, 2, 5).shape == (0, 3)


# ------------------------------------------------------------------ the mirrors
def test_python_mirror_has_the_reference_defaults():
    assert issubclass(FL.PlaneSegmentation, FL._Handle)
    sig = inspect.signature(FL.PlaneSegmentation.segment_plane)
    assert sig.parameters["distance_threshold"].default == 0.2
    assert sig.parameters["ransac_n"].default == 3
    assert sig.parameters["num_iterations"].default == 1000
    assert sig.parameters["seed"].default == 0 and sig.parameters["triples"].default is None
    sig = inspect.signature(FL.cluster_objects)
    want = dict(nb_neighbors=20, std_ratio=2.0, distance_threshold=0.2, num_iterations=1000, seed=0, tolerance=0.5,
                min_size=10, max_size=10000)
    for k, v in want.items():
        assert sig.parameters[k].default == v, k


def test_cpp_mirror_is_declared():
    src = open(os.path.join(ROOT, "include", "lio_gpu.hpp")).read()
    body = src[src.index("class PlaneSegmentation"):]
    for m in ("setInputCloud", "setDistanceThreshold", "setMaxIterations", "setSeed",
              "segment(PointIndices& inliers, std::array<float, 4>& coefficients)"):
        assert m in body, m


def test_entry_fails_loudly_without_device():
    L = _capi.lib()
    if L.lio_device_count() > 0:
        pytest.skip("a device is visible; covered by the gpu tests")
    pts = np.zeros((8, 4), np.float32)
    plane = np.zeros(4, np.float32)
    inl = np.zeros(8, np.int32)
    best, m = C.c_int64(0), C.c_int64(0)
    rc = L.lio_segment_plane(None, pts.ctypes.data_as(C.POINTER(C.c_float)), 8, 4, 0.2, 3, 1000, 0, None,
                             plane.ctypes.data_as(C.POINTER(C.c_float)), C.byref(best),
                             inl.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(m), None, None, None, None, None)
    assert rc == _capi.LIO_ERR_NODEV
    assert b"no HIP device" in L.lio_last_error() or b"gfx950" in L.lio_last_error()
    with pytest.raises(_capi.LioError) as e:
        FL.PlaneSegmentation()
    assert e.value.code == _capi.LIO_ERR_NODEV
