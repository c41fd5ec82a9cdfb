"""CPU checks of the overlay interface (lio_overlay_*): declared in the header with the contract in words, exported
and bound, the new struct under a third ABI list, lio_gpu.camera's own argument checks (made before the device is
touched), the C++ mirror, and LIO_ERR_NODEV without a device — there is no CPU path behind any of it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lio_gpu import _capi
from lio_gpu import camera as CAM
from lio_gpu import filters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"lio_abi_overlay_struct_sizes": 2, "lio_overlay_create": 3, "lio_overlay_destroy": 1, "lio_overlay_set_cloud": 4,
         "lio_overlay_set_labels": 3, "lio_overlay_set_colors": 3, "lio_overlay_set_palette": 3, "lio_overlay_draw": 9,
         "lio_overlay_draw_undistorted": 10, "lio_overlay_get_timing": 2}


def test_header_declares_the_entries_and_the_contract():
    src = open(os.path.join(ROOT, "include", "lio_gpu.h")).read()
    for name, nargs in NAMES.items():
        decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    text = " ".join(src.replace("*", " ").split())
    for words in ("TIES TO EVEN, which is what cv::circle does", "THE CENTRE IS ROUNDED ONLY AFTER THE VALIDITY TEST",
                  "THE DISC IS CLIPPED TO THE IMAGE, NEVER WRAPPED", "ONE HALF-WIDTH PER |ROW OFFSET|", "3: {3, 2, 2, 0} (29)",
                  "key_i = (hi << 32) | (0xFFFFFFFF - i)", "THE MINIMUM STAYS", "ON EQUAL FLOAT DEPTH THE HIGHER INDEX WINS",
                  "NO SWIZZLE", "A POINT WITH label < 0 IS NOT DRAWN AT ALL AND OWNS NOTHING", "palette[label % P]",
                  "EVERY OTHER PIXEL BYTE FOR BYTE THE INPUT'S", "ONE UPLOAD AND ONE DOWNLOAD",
                  "AGREEMENT WITH cv2.circle IS OUR READING OF ITS SOURCE AND IS UNVERIFIED", "2^32 - 2"):
        assert words in text, words
    assert re.search(r"typedef struct lio_overlay_params \{", src)
    assert "#define LIO_OVERLAY_DRAW_ORDER 0" in src and "#define LIO_OVERLAY_NEAREST 1" in src


def test_symbols_are_exported_and_bound():
    L = _capi.lib()
    for name, nargs in NAMES.items():
        assert name in _capi.EXPORTS
        fn = getattr(L, name)
        assert fn.argtypes and len(fn.argtypes) == nargs and fn.restype is C.c_int, name
    assert (_capi.LIO_OVERLAY_DRAW_ORDER, _capi.LIO_OVERLAY_NEAREST) == (0, 1) == (CAM.ORDERS["draw"], CAM.ORDERS["nearest"])


def test_new_struct_is_under_a_third_abi_list(monkeypatch):
    L = _capi.lib()
    assert _capi._ABI_OVERLAY_STRUCTS == ("OverlayParams",)
    n = L.lio_abi_overlay_struct_sizes(None, 0)
    sizes = (C.c_int64 * n)()
    L.lio_abi_overlay_struct_sizes(sizes, n)
    assert list(sizes) == [C.sizeof(_capi.OverlayParams)] == [8]
    # the two earlier lists stay closed
    assert L.lio_abi_struct_sizes(None, 0) == len(_capi._ABI_STRUCTS) == 15 and L.lio_abi_camera_struct_sizes(None, 0) == 2
    _capi._check_abi(L)

    class WiderParams(C.Structure):
        _fields_ = _capi.OverlayParams._fields_ + [("thickness", C.c_int32)]

    monkeypatch.setattr(_capi, "OverlayParams", WiderParams)
    with pytest.raises(ImportError, match="ABI mismatch"):
        _capi._check_abi(L)


def test_argument_checks_come_before_the_device():
    """draw_points checks everything it is given before it creates a handle: these raise ValueError with or without
    a device"""
    cam = CAM.CameraModel(32, 24, 32, 24, 64, 48)
    img = np.zeros((48, 64, 3), np.uint8)
    pts = np.zeros((5, 3), np.float32)
    Rt = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    labels = np.zeros(5, np.int32)
    colors = np.zeros((5, 3), np.uint8)
    palette = np.zeros((2, 3), np.uint8)

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            CAM.draw_points(img, pts, cam, Rt, **kw)

    for radius in (-1, 16, 2.5):
        bad("0..15", radius=radius)
    bad("order", order="depth")
    bad("labels: shape", labels=labels[:4])
    bad("labels: shape", labels=np.zeros((5, 1), np.int32))
    bad("labels: dtype int32", labels=labels.astype(np.int64))
    bad("labels: dtype int32", labels=labels.astype(np.float32))
    bad("colors: shape", colors=colors[:4])
    bad("colors: shape", colors=np.zeros((5, 4), np.uint8))
    bad("colors: shape", colors=np.zeros(15, np.uint8))
    bad("colors: dtype uint8", colors=colors.astype(np.float32))
    bad("palette", palette=np.zeros((0, 3), np.uint8))
    bad("palette", palette=np.zeros((2, 4), np.uint8))
    bad("palette", palette=palette.astype(np.int32))
    bad("more than one colour source", colors=colors, labels=labels)
    bad("more than one colour source", colors=colors, palette=palette)
    bad("more than one colour source", colors=colors, labels=labels, palette=palette)
    with pytest.raises(ValueError, match="uint8"):
        CAM.draw_points(img.astype(np.float32), pts, cam, Rt)
    with pytest.raises(ValueError, match="shape"):
        CAM.draw_points(np.zeros((64, 48, 3), np.uint8), pts, cam, Rt)
    # what is legal gets as far as the handle
    sources = CAM._colour_sources(5, labels, None, palette)
    assert sources[0] is not None and sources[1] is None and sources[2].shape == (2, 3)
    assert CAM._colour_sources(5, None, None, None) == (None, None, None)
    p = CAM._overlay_params(15, "nearest")
    assert (p.radius, p.order) == (15, 1)


def test_cluster_palette_feeds_the_overlay_and_says_so():
    c = filters.cluster_palette(np.array([0, 11, -1], np.int32))
    assert c.dtype == np.uint8 and c.tolist() == [[255, 0, 0], [0, 255, 0], [0, 0, 0]]
    assert CAM._per_point(c, 3, np.uint8, 3, "colors") is not None
    doc = filters.cluster_palette.__doc__
    assert "the caller's" not in doc and "draw_points" in doc and "lidar_projection_overlay" in doc


def test_cpp_mirror_is_declared():
    src = open(os.path.join(ROOT, "include", "lio_gpu.hpp")).read()
    body = src[src.index("class PointOverlay"):]
    body = body[:body.index("\n};")]
    for m in ("setInputCloud", "setLabels", "setColors", "setPalette", "draw(", "drawUndistorted(", "lio_overlay_draw(",
              "lio_overlay_draw_undistorted(", "lio_overlay_set_palette("):
        assert m in body, m


def test_entries_fail_loudly_without_device():
    L = _capi.lib()
    if L.lio_device_count() > 0:
        pytest.skip("a device is visible; covered by the gpu tests")
    h = C.c_void_p()
    rc = L.lio_overlay_create(0, None, C.byref(h))
    assert rc == _capi.LIO_ERR_NODEV and not h.value
    assert b"no HIP device" in L.lio_last_error() or b"gfx950" in L.lio_last_error()
    bad = _capi.OverlayParams(99, 7)
    assert L.lio_overlay_create(0, C.byref(bad), C.byref(h)) == _capi.LIO_ERR_NODEV and not h.value
    n = C.c_int64(0)
    assert L.lio_overlay_set_cloud(None, None, 0, 3) == _capi.LIO_ERR_NODEV
    assert L.lio_overlay_set_labels(None, None, 0) == _capi.LIO_ERR_NODEV
    assert L.lio_overlay_set_colors(None, None, 0) == _capi.LIO_ERR_NODEV
    assert L.lio_overlay_set_palette(None, None, 0) == _capi.LIO_ERR_NODEV
    assert L.lio_overlay_draw(None, None, None, None, 0, None, 0, None, C.byref(n)) == _capi.LIO_ERR_NODEV
    assert L.lio_overlay_draw_undistorted(None, None, None, None, None, 0, None, 0, None, C.byref(n)) == _capi.LIO_ERR_NODEV
    assert L.lio_overlay_get_timing(None, None) == _capi.LIO_ERR_NODEV
    assert L.lio_overlay_destroy(None) == _capi.LIO_OK  # nothing to close
    cam = CAM.CameraModel(32, 24, 32, 24, 64, 48)
    Rt = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    with pytest.raises(_capi.LioError) as e:
        CAM.PointOverlay()
    assert e.value.code == _capi.LIO_ERR_NODEV
    with pytest.raises(_capi.LioError) as e:
        CAM.draw_points(np.zeros((48, 64, 3), np.uint8), np.zeros((4, 3), np.float32), cam, Rt)
    assert e.value.code == _capi.LIO_ERR_NODEV
    with pytest.raises(_capi.LioError) as e:
        CAM.lidar_projection_overlay(np.zeros((40, 3), np.float32), np.zeros((48, 64, 3), np.uint8), cam, Rt)
    assert e.value.code == _capi.LIO_ERR_NODEV
