"""CPU checks of the DBSCAN interface (lio_dbscan): declared in the header with its contract in words, exported by
the library, listed in the binding, failing loudly (LIO_ERR_NODEV) without a device — there is no CPU path behind
it — and mirrored in Python with scikit-learn's defaults and in C++."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from lio_gpu import _capi
from lio_gpu import filters as FL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "lio_dbscan"


def test_header_declares_the_entry_and_its_contract():
    src = open(os.path.join(ROOT, "include", "lio_gpu.h")).read()
    decl = re.search(r"int\s+lio_dbscan\s*\(([^)]*)\)\s*;", src)
    assert decl, "lio_dbscan is not declared"
    args = " ".join(decl.group(1).split())
    pieces = ("lio_filter* f", "const float* pts", "int64_t n", "int stride", "float eps", "int64_t min_samples",
              "int32_t* labels_out", "uint8_t* core_opt", "int64_t* n_clusters", "int64_t cap_clusters",
              "int64_t* offsets_opt", "int32_t* indices_opt", "float* aabb6_opt", "int64_t* stats4_opt")
    assert len(args.split(",")) == 14
    for piece in pieces:
        assert piece in args, piece
    comment = " ".join(src[:decl.start()].rsplit("/*", 1)[1].replace("*", " ").split())
    # the inclusive test, in words, and set against the strict entries
    assert re.search(r"inclusive", comment, flags=re.I) and "<= e2" in comment and "strict" in comment
    # both tie rules, stated as the library's contract
    assert re.search(r"numbered by their lowest core index", comment, flags=re.I)
    assert re.search(r"lowest-numbered cluster among its core neighbours", comment, flags=re.I)
    assert comment.count("this library's contract") >= 2


def test_symbol_is_exported_and_bound():
    L = _capi.lib()
    assert NAME in _capi.EXPORTS
    assert hasattr(L, NAME)
    fn = getattr(L, NAME)
    assert fn.argtypes and len(fn.argtypes) == 14 and fn.restype is C.c_int


def test_python_mirror_has_scikit_learn_defaults():
    assert issubclass(FL.DBSCAN, FL._Handle) and hasattr(FL.DBSCAN, "fit")
    sig = inspect.signature(FL.DBSCAN.__init__)
    assert sig.parameters["eps"].default == 0.5
    assert sig.parameters["min_samples"].default == 5
    assert sig.parameters["device"].default == 0
    assert inspect.signature(FL.DBSCAN.fit).parameters["cap_clusters"].default is None
    sig = inspect.signature(FL.cluster_objects)
    assert sig.parameters["method"].default == "euclidean" and sig.parameters["min_samples"].default == 10
    with pytest.raises(ValueError):
        FL.cluster_objects(np.zeros((0, 4), np.float32), method="kmeans")


def test_cpp_mirror_is_declared():
    src = open(os.path.join(ROOT, "include", "lio_gpu.hpp")).read()
    body = src[src.index("class DBSCAN"):]
    body = body[:body.index("\n};")]
    for m in ("setInputCloud", "setEps", "setMinSamples", "extract(std::vector<PointIndices>&", "labels()", "core()",
              "aabbs()", "stats()", "lio_dbscan("):
        assert m in body, m


def test_entry_fails_loudly_without_device():
    L = _capi.lib()
    if L.lio_device_count() > 0:
        pytest.skip("a device is visible; covered by the gpu tests")
    pts = np.zeros((8, 4), np.float32)
    labels = np.zeros(8, np.int32)
    m = C.c_int64(0)
    rc = L.lio_dbscan(None, pts.ctypes.data_as(C.POINTER(C.c_float)), 8, 4, 0.5, 10,
                      labels.ctypes.data_as(C.POINTER(C.c_int32)), None, C.byref(m), 0, None, None, None, None)
    assert rc == _capi.LIO_ERR_NODEV
    assert b"no HIP device" in L.lio_last_error() or b"gfx950" in L.lio_last_error()
    with pytest.raises(_capi.LioError) as e:
        FL.DBSCAN(0.5, 10)
    assert e.value.code == _capi.LIO_ERR_NODEV
