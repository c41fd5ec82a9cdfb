"""CPU checks of the camera interface (lio_project_points, lio_colorizer_*): declared in the header with the
contract in words, exported and bound, the two new structs under the ABI guard, lio_gpu.camera's own argument
checks and host helpers, colorize_pcd's file round trip with the compute call stubbed, and LIO_ERR_NODEV without a
device — there is no CPU path behind any of it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lio_gpu import _capi
from lio_gpu import camera as CAM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"lio_abi_camera_struct_sizes": 2, "lio_project_points": 10, "lio_colorizer_create": 3, "lio_colorizer_destroy": 1,
         "lio_colorizer_set_params": 2, "lio_colorizer_set_cloud": 4, "lio_colorizer_add_frame": 6, "lio_colorizer_get": 4,
         "lio_colorizer_reset": 1, "lio_colorizer_get_timing": 2}


def test_header_declares_the_entries_and_the_contract():
    src = open(os.path.join(ROOT, "include", "lio_gpu.h")).read()
    for name, nargs in NAMES.items():
        decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    text = " ".join(src.replace("*", " ").split())
    for words in ("EVERY COMPARISON IS FALSE ON NaN", "TRUNCATION ONLY AFTER THE TEST", "is NOT reproduced",
                  "STRICT, SO ON A TIE THE EARLIER FRAME STAYS", "IN R G B ORDER", "zf <= (D[py][px] (1.0f + depth_rel)) + depth_abs",
                  "c_k = ((R[k][0] x + R[k][1] y) + R[k][2] z) + t[k]", "num = 1 + ((k3 r2 + k2) r2 + k1) r2"):
        assert words in text, words
    for struct in ("lio_camera", "lio_colorize_params"):
        assert re.search(r"typedef struct " + struct + r" \{", src), struct


def test_symbols_are_exported_and_bound():
    L = _capi.lib()
    for name, nargs in NAMES.items():
        assert name in _capi.EXPORTS
        fn = getattr(L, name)
        assert fn.argtypes and len(fn.argtypes) == nargs and fn.restype is C.c_int, name


def test_new_structs_are_under_the_abi_guard(monkeypatch):
    L = _capi.lib()
    assert _capi._ABI_CAMERA_STRUCTS == ("Camera", "ColorizeParams")
    n = L.lio_abi_camera_struct_sizes(None, 0)
    sizes = (C.c_int64 * n)()
    L.lio_abi_camera_struct_sizes(sizes, n)
    assert list(sizes) == [C.sizeof(_capi.Camera), C.sizeof(_capi.ColorizeParams)] == [112, 20]
    _capi._check_abi(L)

    class WiderCamera(C.Structure):
        _fields_ = _capi.Camera._fields_ + [("skew", C.c_double)]

    monkeypatch.setattr(_capi, "Camera", WiderCamera)
    with pytest.raises(ImportError, match="ABI mismatch"):
        _capi._check_abi(L)


def test_camera_model_checks_its_arguments():
    cam = CAM.CameraModel(1422.18129, 1421.822766, 2017.285053, 1232.094237, 4096, 2464)
    assert cam.dist == (0.0,) * 8 and cam.r2_max == np.inf
    c = cam._c()
    assert (c.fx, c.cy, c.width, c.height) == (1422.18129, 1232.094237, 4096, 2464) and list(c.dist) == [0.0] * 8
    d5 = CAM.CameraModel(1, 1, 0, 0, 4, 4, dist=(0.1, 0.2, 0.3, 0.4, 0.5))
    assert d5.dist == (0.1, 0.2, 0.3, 0.4, 0.5, 0.0, 0.0, 0.0)  # OpenCV's order: k1 k2 p1 p2 k3, then k4 k5 k6
    assert len(CAM.CameraModel(1, 1, 0, 0, 4, 4, dist=np.arange(8.0)).dist) == 8
    for bad in (dict(dist=(1, 2, 3)), dict(fx=np.nan), dict(cy=np.inf), dict(dist=(np.nan, 0, 0, 0)), dict(r2_max=-1.0),
                dict(r2_max=np.nan), dict(width=0), dict(height=-1), dict(width=2.5), dict(width=1 << 16, height=1 << 15)):
        a = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, width=4, height=4)
        a.update(bad)
        with pytest.raises(ValueError):
            CAM.CameraModel(**a)


def test_pose_forms_and_world_to_camera():
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    t = np.array([1.0, 2.0, 3.0])
    flat = np.concatenate([R.ravel(), t])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    for form in (flat, T[:3], T, list(flat)):
        np.testing.assert_array_equal(CAM._pose(form), flat)
    with pytest.raises(ValueError):
        CAM._pose(np.zeros((3, 3)))
    # the keyframe pose (LiDAR to world) undone, then the extrinsic (LiDAR to camera)
    ang = 0.7
    Tw = np.eye(4)
    Tw[:3, :3] = [[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]
    Tw[:3, 3] = [10.0, -4.0, 0.5]
    Rt = CAM.world_to_camera(Tw, T)
    assert Rt.shape == (12,) and Rt.dtype == np.float64
    p_lidar = np.array([1.5, -0.3, 0.8])
    p_world = Tw[:3, :3] @ p_lidar + Tw[:3, 3]
    np.testing.assert_allclose(Rt[:9].reshape(3, 3) @ p_world + Rt[9:], R @ p_lidar + t, atol=1e-14)
    np.testing.assert_allclose(CAM.world_to_camera(np.eye(4), T), flat, atol=0)
    with pytest.raises(ValueError):
        CAM.world_to_camera(np.eye(3), T)


def test_image_forms():
    cam = CAM.CameraModel(1, 1, 0, 0, 8, 4)
    buf = np.arange(4 * 40, dtype=np.uint8).reshape(4, 40)
    view = np.lib.stride_tricks.as_strided(buf, (4, 8, 3), (40, 3, 1))
    a, pitch = CAM._image(view, cam)
    assert pitch == 40 and a.ctypes.data == buf.ctypes.data  # a padded view goes up as it is
    a, pitch = CAM._image(np.zeros((4, 16, 3), np.uint8)[:, ::2], cam)
    assert pitch == 24 and a.flags.c_contiguous                # anything else is copied
    for bad in (np.zeros((4, 8, 3), np.float32), np.zeros((4, 8), np.uint8), np.zeros((8, 4, 3), np.uint8),
                np.zeros((4, 8, 4), np.uint8)):
        with pytest.raises(ValueError):
            CAM._image(bad, cam)


def test_colors_float_is_the_scripts_array():
    rgb = np.array([[255, 0, 51], [9, 9, 9], [0, 0, 0]], np.uint8)
    out = CAM.colors_float(rgb, np.array([0, -1, 3]))
    np.testing.assert_array_equal(out, [[1.0, 0.0, 51 / 255.0], [0.5, 0.5, 0.5], [0.0, 0.0, 0.0]])
    assert out.dtype == np.float64


def test_colorize_pcd_round_trip_with_the_compute_call_stubbed(tmp_path, monkeypatch):
    """the two device calls stubbed (decoding the input's points, the colours): what goes into the compute call and
    the binary PCD with x y z rgb that comes out (tests/test_gpu_colorize.py runs the same on files, unstubbed)"""
    xyz = np.array([[1.0, 2.0, 3.0], [-4.5, 0.25, 8.0], [0.0, 0.0, -1.0]], np.float32)
    src = tmp_path / "in.pcd"
    seen = {}

    def stub(pts, image, camera, Rt, **params):
        seen.update(pts=pts.copy(), params=params, image=image)
        return np.array([[255, 0, 0], [1, 2, 3], [77, 77, 77]], np.uint8), np.array([0, 0, -1], np.int32)

    monkeypatch.setattr(CAM, "_compute", stub)
    monkeypatch.setattr(CAM, "_read_xyz", lambda path: xyz.copy() if path == str(src) else None)
    cam = CAM.CameraModel(10, 10, 4, 2, 8, 4)
    img = np.zeros((4, 8, 3), np.uint8)
    dst = tmp_path / "out.pcd"
    n, coloured = CAM.colorize_pcd(str(src), img, cam, np.eye(4), str(dst), occlusion=True, splat_radius=2)
    assert (n, coloured) == (3, 2)
    np.testing.assert_array_equal(seen["pts"], xyz)
    assert seen["params"] == dict(occlusion=True, splat_radius=2) and seen["image"] is img
    raw = dst.read_bytes()
    head, data = raw.split(b"DATA binary\n", 1)
    assert b"FIELDS x y z rgb" in head and b"POINTS 3" in head
    rec = np.frombuffer(data, np.float32).reshape(3, 4)
    np.testing.assert_array_equal(rec[:, :3], xyz)
    # the third point was not seen: the script's grey
    np.testing.assert_array_equal(rec[:, 3].view(np.uint32), [0x00FF0000, 0x00010203, 0x00808080])


def test_cpp_mirror_is_declared():
    src = open(os.path.join(ROOT, "include", "lio_gpu.hpp")).read()
    assert "struct CameraModel" in src and "void project_points(" in src and "lio_project_points(" in src
    body = src[src.index("class Colorizer"):]
    body = body[:body.index("\n};")]
    for m in ("setInputCloud", "addFrame", "colors(", "reset()", "setOcclusion", "lio_colorizer_add_frame(", "lio_colorizer_get("):
        assert m in body, m


def test_entries_fail_loudly_without_device():
    L = _capi.lib()
    if L.lio_device_count() > 0:
        pytest.skip("a device is visible; covered by the gpu tests")
    h = C.c_void_p()
    rc = L.lio_colorizer_create(0, None, C.byref(h))
    assert rc == _capi.LIO_ERR_NODEV and not h.value
    assert b"no HIP device" in L.lio_last_error() or b"gfx950" in L.lio_last_error()
    n = C.c_int64(0)
    assert L.lio_colorizer_set_cloud(None, None, 0, 3) == _capi.LIO_ERR_NODEV
    assert L.lio_colorizer_add_frame(None, None, None, None, 0, C.byref(n)) == _capi.LIO_ERR_NODEV
    assert L.lio_colorizer_get(None, None, None, None) == _capi.LIO_ERR_NODEV
    assert L.lio_colorizer_reset(None) == _capi.LIO_ERR_NODEV
    pts = np.zeros((4, 3), np.float32)
    valid = np.zeros(4, np.uint8)
    cam = CAM.CameraModel(1, 1, 0, 0, 4, 4)._c()
    Rt = np.zeros(12)
    rc = L.lio_project_points(None, pts.ctypes.data_as(_capi.fp), 4, 3, C.byref(cam), Rt.ctypes.data_as(_capi.dp), None, None,
                              None, valid.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert rc == _capi.LIO_ERR_NODEV
    with pytest.raises(_capi.LioError) as e:
        CAM.Colorizer()
    assert e.value.code == _capi.LIO_ERR_NODEV
    with pytest.raises(_capi.LioError) as e:
        CAM.project_points(pts, CAM.CameraModel(1, 1, 0, 0, 4, 4), Rt)
    assert e.value.code == _capi.LIO_ERR_NODEV
