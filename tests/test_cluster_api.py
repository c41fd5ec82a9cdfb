"""CPU checks of the Euclidean cluster extraction's interface (lio_euclidean_clusters): declared in the header,
exported by the library, listed in the binding, failing loudly (LIO_ERR_NODEV) without a device — there is no
CPU path behind it — and mirrored in Python with PCL's defaults."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lio_gpu import _capi
from lio_gpu import filters as FL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "lio_euclidean_clusters"


def test_header_declares_the_entry_and_its_contract():
    src = open(os.path.join(ROOT, "include", "lio_gpu.h")).read()
    decl = re.search(r"int\s+lio_euclidean_clusters\s*\(([^)]*)\)\s*;", src)
    assert decl, "lio_euclidean_clusters is not declared"
    args = " ".join(decl.group(1).split())
    for piece in ("lio_filter* f", "const float* pts", "int64_t n", "int stride", "float tolerance", "int64_t min_size",
                  "int64_t max_size", "int32_t* labels_out", "int64_t* n_clusters", "int64_t cap_clusters",
                  "int64_t* offsets_opt", "int32_t* indices_opt", "float* aabb6_opt", "int64_t* stats4_opt"):
        assert piece in args, piece
    # the tie-break between clusters of equal size is the library's contract and is stated as such
    assert re.search(r"lowest member index", src, flags=re.I)


def test_symbol_is_exported_and_bound():
    L = _capi.lib()
    assert NAME in _capi.EXPORTS
    assert hasattr(L, NAME)
    fn = getattr(L, NAME)
    assert fn.argtypes and len(fn.argtypes) == 14 and fn.restype is C.c_int


def test_python_mirror_has_pcl_defaults():
    assert issubclass(FL.EuclideanClusterExtraction, FL._Handle)
    for m in ("setClusterTolerance", "setMinClusterSize", "setMaxClusterSize", "extract"):
        assert hasattr(FL.EuclideanClusterExtraction, m)
    import inspect

    sig = inspect.signature(FL.EuclideanClusterExtraction.__init__)
    assert sig.parameters["tolerance"].default == 0.0
    assert sig.parameters["min_size"].default == 1
    assert sig.parameters["max_size"].default == 2**31 - 1  # INT_MAX


def test_cpp_mirror_is_declared():
    src = open(os.path.join(ROOT, "include", "lio_gpu.hpp")).read()
    assert re.search(r"struct\s+PointIndices\s*\{[^}]*std::vector<int>\s+indices;", src)
    body = src[src.index("class EuclideanClusterExtraction"):]
    for m in ("setInputCloud", "setClusterTolerance", "setMinClusterSize", "setMaxClusterSize", "extract", "labels()",
              "aabbs()"):
        assert m in body, m


def test_entry_fails_loudly_without_device():
    L = _capi.lib()
    if L.lio_device_count() > 0:
        pytest.skip("a device is visible; covered by the gpu tests")
    pts = np.zeros((8, 4), np.float32)
    labels = np.zeros(8, np.int32)
    m = C.c_int64(0)
    rc = L.lio_euclidean_clusters(None, pts.ctypes.data_as(C.POINTER(C.c_float)), 8, 4, 0.5, 10, 25000,
                                  labels.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(m), 0, None, None, None, None)
    assert rc == _capi.LIO_ERR_NODEV
    assert b"no HIP device" in L.lio_last_error() or b"gfx950" in L.lio_last_error()
    with pytest.raises(_capi.LioError) as e:
        FL.EuclideanClusterExtraction(0.5, 10, 25000)
    assert e.value.code == _capi.LIO_ERR_NODEV
