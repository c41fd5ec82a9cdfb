"""CPU checks of the k-means interface (lio_kmeans): declared in the header with its contract, exported by the
library, listed in the binding; mirrored in Python and C++ with the reference call's defaults
(post_process/lidar_projection/src/lidar_projection.cpp:82-92: 5, (100, 0.1), 3); every argument error returned
before any device work — the arguments are judged before the handle, so this holds with or without a device —
and the entry failing loudly (LIO_ERR_NODEV) without one: there is no CPU path behind it."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from lio_gpu import _capi
from lio_gpu import filters as FL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
fp, i32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def test_header_declares_the_entry_and_the_contract():
    src = open(os.path.join(ROOT, "include", "lio_gpu.h")).read()
    decl = re.search(r"int\s+lio_kmeans\s*\(([^)]*)\)\s*;", src)
    assert decl, "lio_kmeans is not declared"
    args = " ".join(decl.group(1).split())
    pieces = ("lio_filter* f", "const float* pts", "int64_t n", "int stride", "int K", "int max_iter", "float eps",
              "int attempts", "uint64_t seed", "const float* init_centers_opt", "int32_t* labels_out",
              "float* centers_out", "double* compactness_out", "int64_t* counts_opt", "float* aabb6_opt",
              "int32_t* seeds_opt", "uint64_t* attempt_q_opt", "int32_t* attempt_iters_opt", "int64_t* stats6_opt")
    assert [p.strip() for p in args.split(",")] == list(pieces)
    doc = src[src.index("k-means with k-means++ seeding"):decl.start()]
    for said in (r"n = 0 included", r"LABELS ARE NOT REASSIGNED", r"LOWEST k WINS A TIE", r"LOWEST INDEX AMONG EQUALS",
                 r"identical bits", r"lio_alloc_count", r"subtract an origin", r"not bit parity"):
        assert re.search(said, doc), said


def test_symbol_is_exported_and_bound():
    L = _capi.lib()
    assert "lio_kmeans" in _capi.EXPORTS and hasattr(L, "lio_kmeans")
    assert len(L.lio_kmeans.argtypes) == 19 and L.lio_kmeans.restype is C.c_int


def test_python_mirror_has_the_reference_defaults():
    assert issubclass(FL.KMeans, FL._Handle)
    sig = inspect.signature(FL.KMeans.__init__)
    want = dict(n_clusters=5, max_iter=100, eps=0.1, attempts=3, seed=0, device=0)
    assert {k: v.default for k, v in sig.parameters.items() if k != "self"} == want
    assert inspect.signature(FL.KMeans.fit).parameters["init_centers"].default is None
    doc = FL.KMeans.__doc__
    for name in ("labels_", "cluster_centers_", "inertia_", "n_iter_", "best_attempt", "counts", "aabb", "seeds",
                 "attempt_q", "attempt_iters", "stats"):
        assert name in doc, name


def test_cpp_mirror_is_declared():
    src = open(os.path.join(ROOT, "include", "lio_gpu.hpp")).read()
    body = src[src.index("class KMeans"):]
    body = body[:body.index("\n};")]
    for m in ("setInputCloud", "setK(int k)", "setTermCriteria(int max_iter, double eps)", "setAttempts", "setSeed",
              "setInitialCenters", "double compute(std::vector<int>& labels, std::vector<std::array<float, 3>>& centers)",
              "counts()", "aabbs()", "seeds()", "stats()", "int k_ = 5;", "int max_iter_ = 100;", "double eps_ = 0.1;",
              "int attempts_ = 3;"):
        assert m in body, m


def _call(n=64, stride=4, K=5, max_iter=100, eps=0.1, attempts=3, init=None, pts=True, labels=True, centers=True,
          compactness=True, handle=None):
    """lio_kmeans on zeros with canaries in every output -> (status, outputs untouched)"""
    rows = min(max(n, 1), 128)  # a call that is refused reads none of them
    P = np.zeros((rows, 8), np.float32)
    lab = np.full(rows, -7, np.int32)
    cen = np.full((64, 3), -7, np.float32)
    comp = C.c_double(-7.0)
    rc = _capi.lib().lio_kmeans(handle, P.ctypes.data_as(fp) if pts else None, n, stride, K, max_iter, eps, attempts, 0,
                                init.ctypes.data_as(fp) if init is not None else None,
                                lab.ctypes.data_as(i32p) if labels else None, cen.ctypes.data_as(fp) if centers else None,
                                C.byref(comp) if compactness else None, None, None, None, None, None, None)
    return rc, bool((lab == -7).all() and (cen == -7).all() and comp.value == -7.0)


BAD = dict(
    n_negative=dict(n=-1), n_2_31=dict(n=2**31), n_zero=dict(n=0), n_below_k=dict(n=4),
    stride_2=dict(stride=2), stride_9=dict(stride=9), k_0=dict(K=0), k_65=dict(K=65, n=128),
    attempts_0=dict(attempts=0), attempts_17=dict(attempts=17), max_iter_0=dict(max_iter=0),
    max_iter_1001=dict(max_iter=1001), eps_negative=dict(eps=-0.1), eps_nan=dict(eps=float("nan")),
    eps_inf=dict(eps=float("inf")), no_pts=dict(pts=False), no_labels=dict(labels=False), no_centers=dict(centers=False),
    no_compactness=dict(compactness=False),
    init_nan=dict(init=np.array([0] * 44 + [np.nan], np.float32)), init_inf=dict(init=np.array([np.inf] + [0] * 44, np.float32)),
)


@pytest.mark.parametrize("case", sorted(BAD))
def test_argument_errors_come_before_any_device_work(case):
    # a NULL handle: were the arguments judged after it, the status would be the handle's (or LIO_ERR_NODEV)
    rc, untouched = _call(**BAD[case])
    assert rc == _capi.LIO_ERR_ARG and untouched, case
    assert b"lio_kmeans" in _capi.lib().lio_last_error()


def test_entry_fails_loudly_without_device():
    L = _capi.lib()
    rc, untouched = _call()
    assert untouched
    if L.lio_device_count() > 0:  # good arguments, no handle
        assert rc == _capi.LIO_ERR_ARG and b"handle is NULL" in L.lio_last_error()
        return
    assert rc == _capi.LIO_ERR_NODEV
    assert b"no HIP device" in L.lio_last_error() or b"gfx950" in L.lio_last_error()
    with pytest.raises(_capi.LioError) as e:
        FL.KMeans()
    assert e.value.code == _capi.LIO_ERR_NODEV


def test_cluster_palette_matches_the_ten_colours():
    bgr = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255), (128, 0, 0), (0, 128, 0),
           (0, 0, 128), (128, 128, 0)]
    labels = np.array(list(range(10)) + [10, 23, -1, 64], np.int32)
    out = FL.cluster_palette(labels)
    assert out.dtype == np.uint8 and out.shape == (14, 3)
    assert [tuple(int(v) for v in row) for row in out] == bgr + [bgr[0], bgr[3], (0, 0, 0), bgr[4]]
    assert FL.cluster_palette(np.zeros(0, np.int32)).shape == (0, 3)
    out[0] = 9  # a copy: the table is not the caller's to change
    assert tuple(FL.cluster_palette([0])[0]) == bgr[0]


def test_cluster_objects_has_no_kmeans_method():
    with pytest.raises(ValueError):
        FL.cluster_objects(np.zeros((16, 3), np.float32), method="kmeans")
