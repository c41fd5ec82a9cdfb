"""GPU checks of the image undistortion (lio_undistort.hip: lio_undistort_map, lio_undistorter_*) against the
contract restated in numpy (tests/undistort_ref.py; tests/test_undistort_ref.py holds that restatement against
itself).  Every output is compared bit for bit: both sides perform the same IEEE and integer operations."""
import ctypes as C

import numpy as np
import pytest

import colorize_ref as CR
import undistort_ref as UR
from lio_gpu import _capi
from lio_gpu import camera as CAM
from lio_gpu.filters import _Handle

pytestmark = pytest.mark.gpu

SCENES = UR.scenes()
BORDER = (7, 200, 31)
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def fh():
    return _Handle()


@pytest.fixture(scope="module")
def ud():
    u = CAM.Undistorter()
    yield u
    u.close()


def model(cam):
    return CAM.CameraModel(cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, cam.dist)


def dst_model(scene):
    return model(scene.dst) if scene.dst is not None else None


def b64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


_MAPS = {}


def ref_map(scene):
    """the restatement's map of a scene, computed once"""
    if scene.name not in _MAPS:
        _MAPS[scene.name] = UR.undistort_map(scene.src, scene.dst)
    return _MAPS[scene.name]


def check_map(fh, scene):
    uv, sxy, axy = CAM.undistort_map(model(scene.src), dst_model(scene), handle=fh)
    m = ref_map(scene)
    np.testing.assert_array_equal(b64(uv), b64(m.uv), err_msg=scene.name)
    np.testing.assert_array_equal(sxy, m.sxy, err_msg=scene.name)
    np.testing.assert_array_equal(axy, m.axy, err_msg=scene.name)
    return uv, sxy, axy


# ------------------------------------------------------------------------------------------------------- the map
@pytest.mark.parametrize("scene", SCENES, ids=lambda s: s.name)
def test_map_equals_the_restatement(fh, scene):
    check_map(fh, scene)


def test_map_far_pixels(fh):
    scene = SCENES[-1]
    _, sxy, axy = check_map(fh, scene)
    far = sxy[:, :, 0] == -2 ** 31
    assert far.sum() == 2 and far[24, 0] and (sxy[far] == -2 ** 31).all() and not axy[far].any()


def test_map_equals_the_projection_of_the_same_rays(fh):
    """The points (xn, yn, 1) under the identity pose reach lio_project_points' distortion stage with the map's
    operands wherever float32 holds xn and yn exactly: one device function, the same bits.  With small_cam (fx = cx =
    32, fy = cy = 24) and DIST8 as the raw camera, xn = (j - 32) / 32 is exact in every column, but yn = (i - 24) / 24 only
    in the rows where i - 24 is a multiple of 3 (k / 24 is no binary fraction otherwise).  So dst = src is compared on
    those 16 rows, and all 3072 pixels with a rectified camera of fy = 32, whose yn = (i - 24) / 32 is exact."""
    cam = CR.small_cam(dist=CR.DIST8)
    raw = CAM.CameraModel(cam.fx, cam.fy, cam.cx, cam.cy, 64, 48, cam.dist)
    jj, ii = np.meshgrid(np.arange(64, dtype=np.float64), np.arange(48, dtype=np.float64))
    for dst_fy, rows in ((24.0, np.arange(0, 48, 3)), (32.0, np.arange(48))):
        dst = UR.pinhole(32.0, dst_fy, 32.0, 24.0, 64, 48)
        uv, _, _ = CAM.undistort_map(raw, model(dst), handle=fh)
        xn, yn = ((jj - 32.0) / 32.0)[rows], ((ii - 24.0) / dst_fy)[rows]
        pts = np.stack([xn.ravel(), yn.ravel(), np.ones(xn.size)], 1).astype(np.float32)
        assert (pts[:, 0].astype(np.float64) == xn.ravel()).all() and (pts[:, 1].astype(np.float64) == yn.ravel()).all()
        pr = CAM.project_points(pts, raw, CR.IDENTITY, handle=fh)
        np.testing.assert_array_equal(b64(uv[rows].reshape(-1, 2)), b64(pr.uv))
        m = UR.undistort_map(cam, dst)
        np.testing.assert_array_equal(b64(uv), b64(m.uv))


def test_rounding_ties_go_to_even(fh):
    """every u * 32 is 32 j + 0.5 and every v * 32 is 32 i - 0.5: ties to even give ax = ay = 0, sx = j, sy = i; half
    up would give ax = 1, half away from zero sy = -1, ay = 31 at i = 0"""
    src = CR.small_cam()
    dst = UR.pinhole(32.0, 24.0, 32.0 - 1.0 / 64.0, 24.0 + 1.0 / 64.0, 64, 48)
    uv, sxy, axy = CAM.undistort_map(model(src), model(dst), handle=fh)
    jj, ii = np.meshgrid(np.arange(64), np.arange(48))
    np.testing.assert_array_equal(uv[:, :, 0] * 32.0, 32.0 * jj + 0.5)
    np.testing.assert_array_equal(uv[:, :, 1] * 32.0, 32.0 * ii - 0.5)
    np.testing.assert_array_equal(sxy[:, :, 0], jj)
    np.testing.assert_array_equal(sxy[:, :, 1], ii)
    assert not axy.any()


# ---------------------------------------------------------------------------------------------------- the images
def run_padded(ud, img, out_cam, channels):
    """through an output whose rows are padded by 5 bytes holding a sentinel, which must survive"""
    row = channels * out_cam.width
    buf = np.full((out_cam.height, row + 5), SENTINEL, np.uint8)
    shape = (out_cam.height, out_cam.width) if channels == 1 else (out_cam.height, out_cam.width, 3)
    strides = (row + 5, 1) if channels == 1 else (row + 5, 3, 1)
    out = np.lib.stride_tricks.as_strided(buf, shape, strides)
    got = ud(img, out=out)
    assert got is out and (buf[:, row:] == SENTINEL).all(), "the output's padding was written"
    return np.ascontiguousarray(out)


@pytest.mark.parametrize("scene", SCENES, ids=lambda s: s.name)
def test_images_equal_the_restatement(ud, scene):
    src, out_cam, m = scene.src, scene.out_cam, ref_map(scene)
    for channels in (3, 1):
        odd_pitch = channels * src.width + 7
        images = [UR.image(src, channels, seed=1), UR.image(src, channels, pitch=odd_pitch, seed=2),
                  np.full(UR.image(src, channels).shape, 255, np.uint8), np.zeros(UR.image(src, channels).shape, np.uint8)]
        for border in ((0, 0, 0), BORDER):
            ud.set_camera(model(src), dst_model(scene), channels=channels, border=border)
            for k, img in enumerate(images):
                want = UR.remap(img, m, src, border)
                msg = f"{scene.name} channels={channels} border={border} image {k}"
                np.testing.assert_array_equal(ud(img), want, err_msg=msg)
                np.testing.assert_array_equal(run_padded(ud, img, out_cam, channels), want, err_msg=msg + " (padded out)")


def test_one_channel_forms_and_the_one_shot(ud):
    scene = SCENES[2]
    img = UR.image(scene.src, 1, seed=3)
    want = UR.remap(img, ref_map(scene), scene.src, 77)
    ud.set_camera(model(scene.src), dst_model(scene), channels=1, border=77)
    assert ud(img).shape == (48, 64) and ud(img[:, :, None]).shape == (48, 64, 1)
    np.testing.assert_array_equal(ud(img[:, :, None])[:, :, 0], want)
    np.testing.assert_array_equal(CAM.undistort_image(img, model(scene.src), dst_model(scene), border=77), want)
    img3 = UR.image(scene.src, 3, seed=4)
    np.testing.assert_array_equal(CAM.undistort_image(img3, model(scene.src), model(scene.src).rectified(), BORDER),
                                  UR.undistort(img3, scene.src, None, BORDER))
    with pytest.raises(ValueError):
        ud(img3)  # the handle holds one channel


@pytest.mark.parametrize("cam", [CR.small_cam(), UR.Cam(*(k / 64.0 for k in UR.K8), 64, 38), UR.Cam(11.3, 9.7, 2.2, 3.9, 5, 7)],
                         ids=["64x48", "64x38", "5x7"])
def test_identity(ud, cam):
    """zero dist and dst = src: the output is the input, the last row and the last column included (their second
    taps lie outside the image with weight 0 and must not be loaded)"""
    for channels in (3, 1):
        img = UR.image(cam, channels, pitch=channels * cam.width + 3, seed=6)
        ud.set_camera(model(cam), None, channels=channels, border=BORDER)
        np.testing.assert_array_equal(ud(img), img)


# ---------------------------------------------------------------------------------------------------- the handle
def test_run_before_set_camera_is_a_state_error():
    u = CAM.Undistorter()
    try:
        with pytest.raises(_capi.LioError) as e:
            u(np.zeros((48, 64, 3), np.uint8))
        assert e.value.code == _capi.LIO_ERR_STATE and "set_camera" in str(e.value)
        # a refused set_camera does not make one
        with pytest.raises(_capi.LioError) as e:
            u.set_camera(model(CR.small_cam()), channels=2)
        assert e.value.code == _capi.LIO_ERR_ARG
        with pytest.raises(_capi.LioError) as e:
            u(np.zeros((48, 64, 3), np.uint8))
        assert e.value.code == _capi.LIO_ERR_STATE
    finally:
        u.close()


def test_pitch_errors_name_their_bound(ud):
    L = _capi.lib()
    cam = CR.small_cam()
    ud.set_camera(model(cam), model(UR.pinhole(20.0, 3.0, 33.0, 2.0, 67, 5)), channels=3)
    src = np.zeros(48 * 192, np.uint8)
    out = np.zeros(5 * 201, np.uint8)
    ps, po = src.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for pitch, out_pitch, word in ((191, 201, b"pitch must be at least channels x width bytes of the raw image"),
                                   (192, 200, b"out_pitch must be at least channels x width bytes of the rectified image"),
                                   (-192, 201, b"pitch must be at least"), (0, 201, b"pitch must be at least")):
        assert L.lio_undistorter_run(ud._h, ps, pitch, po, out_pitch) == _capi.LIO_ERR_ARG
        assert word in L.lio_last_error()
    assert L.lio_undistorter_run(ud._h, None, 192, po, 201) == _capi.LIO_ERR_ARG and b"image is NULL" in L.lio_last_error()
    assert L.lio_undistorter_run(ud._h, ps, 192, None, 201) == _capi.LIO_ERR_ARG and b"out is NULL" in L.lio_last_error()
    assert L.lio_undistorter_get_timing(ud._h, None) == _capi.LIO_ERR_ARG
    assert L.lio_undistorter_run(ud._h, ps, 192, po, 201) == _capi.LIO_OK


def test_two_cameras_in_turn_on_one_handle(ud):
    for scene in (SCENES[2], SCENES[3], SCENES[0], SCENES[3]):
        img = UR.image(scene.src, 3, seed=8)
        ud.set_camera(model(scene.src), dst_model(scene), border=BORDER)
        np.testing.assert_array_equal(ud(img), UR.remap(img, ref_map(scene), scene.src, BORDER), err_msg=scene.name)


def test_frames_of_one_size_allocate_nothing_and_repeat(ud):
    L = _capi.lib()
    scene = SCENES[2]
    ud.set_camera(model(scene.src), dst_model(scene), border=BORDER)
    frames = [UR.image(scene.src, 3, seed=20 + k % 3) for k in range(10)]  # frames 0, 3, 6, 9 are one image
    out = np.empty((48, 64, 3), np.uint8)
    first = ud(frames[0]).copy()
    after_first = L.lio_alloc_count()
    outs = [ud(f, out=out).copy() for f in frames]
    assert L.lio_alloc_count() == after_first
    for k in (0, 3, 6, 9):
        np.testing.assert_array_equal(outs[k], first)
    assert not np.array_equal(outs[1], first)
    np.testing.assert_array_equal(outs[1], UR.remap(frames[1], ref_map(scene), scene.src, BORDER))
    t = ud.timing()
    assert set(t) == {"upload_ms", "kernel_ms", "download_ms"}
    assert all(np.isfinite(v) and v >= 0.0 for v in t.values()), t


# ----------------------------------------------------------------------------------------------- a larger shape
def test_larger_shape(fh, ud):
    """1031 x 517: many workgroups, a width that is no multiple of 4, rows that start at every alignment"""
    scene = UR.large_scene()
    check_map(fh, scene)
    m = ref_map(scene)
    s = scene.src  # the 5-parameter model folds outwards again beyond its field: a wider view leaves the source on all sides
    wide = UR.Scene("1031x517 wide", UR.Cam(s.fx, s.fy, s.cx, s.cy, 1031, 517, UR.DIST5),
                    UR.pinhole(s.fx * 0.6, s.fy * 0.6, 515.0, 258.0, 1031, 517), ())
    mw = UR.undistort_map(wide.src, wide.dst)
    c = UR.classes(mw, wide.src)
    assert min(c["all_in"], c["left"], c["right"], c["top"], c["bottom"], c["all_out"]) > 0, c
    for channels in (3, 1):
        img = UR.image(scene.src, channels, pitch=channels * 1031 + 1, seed=9)
        ud.set_camera(model(scene.src), None, channels=channels, border=BORDER)
        np.testing.assert_array_equal(run_padded(ud, img, scene.src, channels), UR.remap(img, m, scene.src, BORDER))
        ud.set_camera(model(wide.src), model(wide.dst), channels=channels, border=BORDER)
        np.testing.assert_array_equal(ud(img), UR.remap(img, mw, wide.src, BORDER))
