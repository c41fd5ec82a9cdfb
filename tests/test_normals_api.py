"""CPU checks of the normal estimation's interface (lio_estimate_normals): declared in the header with its
contract, exported by the library, listed in the binding; mirrored in Python and C++; every argument error returned
before any device work — the arguments are judged before the handle, so this holds with or without a device — and
the entry failing loudly (LIO_ERR_NODEV) without one: there is no CPU path behind it."""
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
    decl = re.search(r"int\s+lio_estimate_normals\s*\(([^)]*)\)\s*;", src)
    assert decl, "lio_estimate_normals is not declared"
    args = " ".join(decl.group(1).split())
    pieces = ("lio_filter* f", "const float* pts", "int64_t n", "int stride", "float radius", "int k",
              "const float* viewpoints_opt", "int vp_stride", "float* normals_out", "float* curvature_opt",
              "int32_t* counts_opt", "int64_t* stats6_opt")
    assert [p.strip() for p in args.split(",")] == list(pieces)
    doc = src[src.index("Surface normals and curvature per point"):decl.start()]
    for said in (r"THE TEST IS STRICT", r"THEN INDEX j", r"LOWEST INDEX AMONG EQUALS", r"rint", r"at most 10 sweeps",
                 r"DEGENERATE", r"a NaN s flips nothing", r"vp_stride 0", r"identical\s+bits", r"lio_alloc_count",
                 r"not bit parity", r"with or without a device"):
        assert re.search(said, doc), said


def test_symbol_is_exported_and_bound():
    L = _capi.lib()
    assert "lio_estimate_normals" in _capi.EXPORTS and hasattr(L, "lio_estimate_normals")
    assert len(L.lio_estimate_normals.argtypes) == 12 and L.lio_estimate_normals.restype is C.c_int


def test_python_mirror():
    assert issubclass(FL.NormalEstimation, FL._Handle)
    sig = inspect.signature(FL.NormalEstimation.__init__)
    assert {k: v.default for k, v in sig.parameters.items() if k != "self"} == dict(k=20, radius=0.0, device=0)
    assert inspect.signature(FL.NormalEstimation.compute).parameters["viewpoint"].default is None
    for name in ("curvature", "counts", "stats"):
        assert name in FL.NormalEstimation.__doc__, name


def test_with_normals_makes_point_xyzi_normal_rows():
    pts = np.arange(20, dtype=np.float32).reshape(4, 5)
    nrm = np.arange(12, dtype=np.float32).reshape(4, 3) + 100
    cur = np.arange(4, dtype=np.float32) + 200
    out = FL.with_normals(pts, nrm, cur)
    assert out.dtype == np.float32 and out.shape == (4, 8)
    assert np.array_equal(out[:, :4], pts[:, :4]) and np.array_equal(out[:, 4:7], nrm) and np.array_equal(out[:, 7], cur)
    out3 = FL.with_normals(pts[:, :3], nrm, cur)
    assert np.array_equal(out3[:, :3], pts[:, :3]) and (out3[:, 3] == 0).all() and np.array_equal(out3[:, 4:], out[:, 4:])
    assert FL.with_normals(np.zeros((0, 4), np.float32), np.zeros((0, 3)), np.zeros(0)).shape == (0, 8)
    with pytest.raises(ValueError):
        FL.with_normals(pts, nrm[:3], cur)


def test_with_normals_rows_are_saved_as_point_xyzi_normal(tmp_path):
    from lio_gpu import formats

    rows = FL.with_normals(np.arange(12, dtype=np.float32).reshape(3, 4), np.eye(3, dtype=np.float32), np.full(3, 0.5, np.float32))
    path = str(tmp_path / "map.pcd")
    formats.write_pcd_binary(path, rows, FL.POINT_XYZI_NORMAL_FIELDS)
    raw = open(path, "rb").read()
    head, body = raw[:raw.index(b"DATA binary\n")].decode(), raw[raw.index(b"DATA binary\n") + 12:]
    assert "FIELDS x y z intensity normal_x normal_y normal_z curvature" in head and "POINTS 3" in head
    assert np.array_equal(np.frombuffer(body, np.float32).reshape(3, 8), rows)


def test_cpp_mirror_is_declared():
    src = open(os.path.join(ROOT, "include", "lio_gpu.hpp")).read()
    body = src[src.index("class NormalEstimation"):]
    body = body[:body.index("\n};")]
    for m in ("setInputCloud", "setKSearch(int k)", "setRadiusSearch(double radius)",
              "setViewPoint(float vx, float vy, float vz)", "setViewPoints", "useNoViewPoint",
              "void compute(std::vector<Normal>& out)", "counts()", "stats()", "int k_ = 0;", "double radius_ = 0.0;"):
        assert m in body, m


def _call(n=64, stride=4, radius=0.0, k=16, vp=False, vp_stride=0, pts=True, normals=True, handle=None):
    """lio_estimate_normals on zeros with canaries in every output -> (status, outputs untouched)"""
    rows = min(max(n, 1), 128)  # a call that is refused reads none of them
    P = np.zeros((rows, 8), np.float32)
    V = np.zeros((rows, 8), np.float32)
    nrm = np.full((rows, 3), -7, np.float32)
    cur = np.full(rows, -7, np.float32)
    cnt = np.full(rows, -7, np.int32)
    st = np.full(6, -7, np.int64)
    rc = _capi.lib().lio_estimate_normals(handle, P.ctypes.data_as(fp) if pts else None, n, stride, radius, k,
                                          V.ctypes.data_as(fp) if vp else None, vp_stride,
                                          nrm.ctypes.data_as(fp) if normals else None, cur.ctypes.data_as(fp),
                                          cnt.ctypes.data_as(i32p), st.ctypes.data_as(i64p))
    return rc, bool((nrm == -7).all() and (cur == -7).all() and (cnt == -7).all() and (st == -7).all())


BAD = dict(
    n_negative=dict(n=-1), n_2_31=dict(n=2**31), stride_2=dict(stride=2), stride_9=dict(stride=9),
    neither=dict(k=0, radius=0.0), k_1=dict(k=1), k_2=dict(k=2), k_256=dict(k=256), k_negative=dict(k=-3),
    k_2_with_radius=dict(k=2, radius=0.5), radius_negative=dict(radius=-0.5), radius_nan=dict(radius=float("nan")),
    radius_inf=dict(radius=float("inf")), radius_nan_no_k=dict(radius=float("nan"), k=0),
    radius_square_underflows=dict(radius=1e-30), radius_square_overflows=dict(radius=1e30),
    vp_stride_1=dict(vp=True, vp_stride=1), vp_stride_2=dict(vp=True, vp_stride=2), vp_stride_9=dict(vp=True, vp_stride=9),
    vp_stride_negative=dict(vp=True, vp_stride=-3), no_pts=dict(pts=False), no_normals=dict(normals=False),
)


@pytest.mark.parametrize("case", sorted(BAD))
def test_argument_errors_come_before_any_device_work(case):
    # a NULL handle: were the arguments judged after it, the status would be the handle's (or LIO_ERR_NODEV)
    rc, untouched = _call(**BAD[case])
    assert rc == _capi.LIO_ERR_ARG and untouched, case
    assert b"lio_estimate_normals" in _capi.lib().lio_last_error()


@pytest.mark.parametrize("good", (dict(), dict(k=3), dict(k=255), dict(k=0, radius=0.5), dict(radius=0.5, k=30),
                                  dict(n=0), dict(vp=True), dict(vp=True, vp_stride=3), dict(vp=True, vp_stride=8),
                                  dict(stride=3), dict(stride=8)),
                         ids=lambda g: "-".join(f"{k}{v}" for k, v in g.items()) or "defaults")
def test_entry_fails_loudly_without_device(good):
    L = _capi.lib()
    rc, untouched = _call(**good)
    assert untouched
    if L.lio_device_count() > 0:  # good arguments, no handle
        assert rc == _capi.LIO_ERR_ARG and b"handle is NULL" in L.lio_last_error()
        return
    assert rc == _capi.LIO_ERR_NODEV
    assert b"no HIP device" in L.lio_last_error() or b"gfx950" in L.lio_last_error()
    with pytest.raises(_capi.LioError) as e:
        FL.NormalEstimation()
    assert e.value.code == _capi.LIO_ERR_NODEV
