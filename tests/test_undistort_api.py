"""CPU checks of the undistortion interface (lio_undistort_map, lio_undistorter_*): declared in the header with the
contract in words, exported and bound, no new struct, every argument error that needs no handle with the word that
names its bound (they are made before the handle is looked at, so they show without a device), lio_gpu.camera's host
helpers, and LIO_ERR_NODEV without a device — there is no CPU path behind any of it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lio_gpu import _capi
from lio_gpu import camera as CAM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"lio_undistort_map": 6, "lio_undistorter_create": 2, "lio_undistorter_destroy": 1, "lio_undistorter_set_camera": 5,
         "lio_undistorter_run": 5, "lio_undistorter_get_timing": 2}
u8p = C.POINTER(C.c_uint8)


def test_header_declares_the_entries_and_the_contract():
    src = open(os.path.join(ROOT, "include", "lio_gpu.h")).read()
    for name, nargs in NAMES.items():
        decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    text = " ".join(src.replace("*", " ").split())
    for words in ("xn = ((double)j - dst.cx) / dst.fx", "qu = rint(u 32.0)", "TIES TO EVEN", "THE TEST IS FALSE ON NaN",
                  "sx = qu >> 5", "ax = qu & 31", "NEVER LOADED", "out = (sum w p + 512) >> 10",
                  "AGREEMENT WITH cv2.undistort IS THIS READING OF ITS SOURCE AND IS UNVERIFIED", "1..32767"):
        assert words in text, words
    assert "typedef struct lio_undistorter lio_undistorter;" in src


def test_symbols_are_exported_and_bound():
    L = _capi.lib()
    for name, nargs in NAMES.items():
        assert name in _capi.EXPORTS
        fn = getattr(L, name)
        assert fn.argtypes and len(fn.argtypes) == nargs and fn.restype is C.c_int, name


def test_no_new_struct():
    L = _capi.lib()
    assert _capi._ABI_CAMERA_STRUCTS == ("Camera", "ColorizeParams")
    assert L.lio_abi_camera_struct_sizes(None, 0) == 2
    src = open(os.path.join(ROOT, "include", "lio_gpu.h")).read()
    part = src[src.index("image undistortion"):src.index("wire / disk formats")]
    assert "typedef struct lio_undistorter lio_undistorter;" in part and "{" not in part


def cam(**kw):
    a = dict(fx=32.0, fy=24.0, cx=32.0, cy=24.0, dist=(0.0,) * 8, r2_max=np.inf, width=64, height=48)
    a.update(kw)
    return _capi.Camera(a["fx"], a["fy"], a["cx"], a["cy"], (C.c_double * 8)(*a["dist"]), a["r2_max"], a["width"], a["height"])


def d8(k, v):
    d = [0.0] * 8
    d[k] = v
    return tuple(d)


# (src, dst or None, the word of the message)
BAD_CAMERAS = [
    (None, None, "src is NULL"),
    (cam(width=0), None, "1..32767"), (cam(height=0), None, "1..32767"), (cam(width=32768), None, "1..32767"),
    (cam(height=40000), None, "1..32767"), (cam(width=-5), None, "1..32767"),
    (cam(), cam(width=0), "1..32767"), (cam(), cam(height=32768), "1..32767"),
    (cam(fx=np.nan), None, "intrinsic"), (cam(cy=np.inf), None, "intrinsic"), (cam(), cam(cx=-np.inf), "intrinsic"),
    (cam(), cam(fy=np.nan), "intrinsic"),
    (cam(dist=d8(0, np.nan)), None, "distortion coefficient"), (cam(dist=d8(7, np.inf)), None, "distortion coefficient"),
    (cam(), cam(fx=0.0), "must not be 0"), (cam(), cam(fy=-0.0), "must not be 0"), (cam(fx=0.0), None, "must not be 0"),
    (cam(), cam(dist=d8(4, 1e-300)), "all zero"), (cam(), cam(dist=d8(0, np.nan)), "all zero"),
]


def expect_arg(rc, word):
    L = _capi.lib()
    assert rc == _capi.LIO_ERR_ARG, (rc, word, L.lio_last_error())
    assert word.encode() in L.lio_last_error(), (word, L.lio_last_error())


@pytest.mark.parametrize("k", range(len(BAD_CAMERAS)))
def test_camera_errors_name_their_bound_before_any_handle(k):
    """with a NULL handle: LIO_ERR_ARG comes before the handle (and the device) is looked at"""
    L = _capi.lib()
    src, dst, word = BAD_CAMERAS[k]
    ps = C.byref(src) if src is not None else None
    pd = C.byref(dst) if dst is not None else None
    expect_arg(L.lio_undistort_map(None, ps, pd, None, None, None), word)
    expect_arg(L.lio_undistorter_set_camera(None, ps, pd, 3, None), word)


def test_the_other_argument_errors():
    L = _capi.lib()
    c = cam()
    for channels in (0, 2, 4, -1):
        expect_arg(L.lio_undistorter_set_camera(None, C.byref(c), None, channels, None), "channels must be 1 or 3")
    buf = np.zeros(16, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    expect_arg(L.lio_undistorter_run(None, None, 16, p, 16), "image is NULL")
    expect_arg(L.lio_undistorter_run(None, p, 16, None, 16), "out is NULL")
    expect_arg(L.lio_undistorter_create(0, None), "out is NULL")
    # a zero dst dist and a dst that differs from src are fine as far as the arguments go: the handle is next
    rc = L.lio_undistort_map(None, C.byref(c), C.byref(cam(fx=16.0, width=67, height=5)), None, None, None)
    assert rc in (_capi.LIO_ERR_NODEV, _capi.LIO_ERR_ARG) and (rc == _capi.LIO_ERR_NODEV or b"handle is NULL" in L.lio_last_error())


def test_rectified_camera():
    c = CAM.CameraModel(1419.5, 1419.8, 2091.7, 1231.7, 4096, 2464, dist=(0.47, 0.02, 1e-7, -2e-7, 8e-5, 0.8, 0.11, 0.0017),
                        r2_max=4.0)
    r = c.rectified()
    assert r.dist == (0.0,) * 8 and (r.fx, r.fy, r.cx, r.cy, r.width, r.height) == (c.fx, c.fy, c.cx, c.cy, 4096, 2464)
    assert r.r2_max == 4.0 and c.dist[0] == 0.47  # the raw camera is unchanged
    s = c.rectified(fx=700.0, width=2048, height=1232)
    assert (s.fx, s.fy, s.width, s.height) == (700.0, c.fy, 2048, 1232) and s.dist == (0.0,) * 8
    with pytest.raises(ValueError):
        c.rectified(width=0)


def test_image_forms():
    buf = np.arange(4 * 40, dtype=np.uint8).reshape(4, 40)
    view3 = np.lib.stride_tricks.as_strided(buf, (4, 8, 3), (40, 3, 1))
    a, pitch, ch = CAM._plane(view3, 8, 4)
    assert (pitch, ch) == (40, 3) and a.ctypes.data == buf.ctypes.data  # a padded view goes up as it is
    view1 = buf[:, :8]
    a, pitch, ch = CAM._plane(view1, 8, 4)
    assert (pitch, ch) == (40, 1) and a.ctypes.data == buf.ctypes.data
    a, pitch, ch = CAM._plane(view1[:, :, None], 8, 4)                      # h x w x 1 is one channel
    assert (pitch, ch) == (40, 1) and a.ctypes.data == buf.ctypes.data
    a, pitch, ch = CAM._plane(np.zeros((4, 16), np.uint8)[:, ::2], 8, 4)    # anything else is copied
    assert (pitch, ch) == (8, 1) and a.flags.c_contiguous
    a, pitch, ch = CAM._plane(np.zeros((4, 16, 3), np.uint8)[:, ::2], 8, 4)
    assert (pitch, ch) == (24, 3) and a.flags.c_contiguous
    for bad in (np.zeros((4, 8, 3), np.float32), np.zeros((4, 8, 2), np.uint8), np.zeros((8, 4, 3), np.uint8),
                np.zeros((4, 8, 4), np.uint8), np.zeros(32, np.uint8)):
        with pytest.raises(ValueError):
            CAM._plane(bad, 8, 4)


def test_cpp_mirror_is_declared():
    src = open(os.path.join(ROOT, "include", "lio_gpu.hpp")).read()
    assert "inline void undistort_map(" in src and "lio_undistort_map(" in src and "struct UndistortMap" in src
    body = src[src.index("class Undistorter"):]
    body = body[:body.index("\n};")]
    for m in ("setCamera(", "undistort(", "timing()", "lio_undistorter_set_camera(", "lio_undistorter_run(",
              "lio_undistorter_get_timing("):
        assert m in body, m


def test_entries_fail_loudly_without_device():
    L = _capi.lib()
    if L.lio_device_count() > 0:
        pytest.skip("a device is visible; covered by the gpu tests")
    h = C.c_void_p()
    rc = L.lio_undistorter_create(0, C.byref(h))
    assert rc == _capi.LIO_ERR_NODEV and not h.value
    assert b"no HIP device" in L.lio_last_error() or b"gfx950" in L.lio_last_error()
    c = cam()
    buf = np.zeros(64 * 48 * 3, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    ms = np.zeros(3)
    assert L.lio_undistort_map(None, C.byref(c), None, None, None, None) == _capi.LIO_ERR_NODEV
    assert L.lio_undistorter_set_camera(None, C.byref(c), None, 3, None) == _capi.LIO_ERR_NODEV
    assert L.lio_undistorter_run(None, p, 192, p, 192) == _capi.LIO_ERR_NODEV
    assert L.lio_undistorter_get_timing(None, ms.ctypes.data_as(_capi.dp)) == _capi.LIO_ERR_NODEV
    assert L.lio_undistorter_destroy(None) == _capi.LIO_OK
    model = CAM.CameraModel(32, 24, 32, 24, 64, 48)
    with pytest.raises(_capi.LioError) as e:
        CAM.Undistorter()
    assert e.value.code == _capi.LIO_ERR_NODEV
    with pytest.raises(_capi.LioError) as e:
        CAM.undistort_map(model)
    assert e.value.code == _capi.LIO_ERR_NODEV
    with pytest.raises(_capi.LioError) as e:
        CAM.undistort_image(buf.reshape(48, 64, 3), model)
    assert e.value.code == _capi.LIO_ERR_NODEV
