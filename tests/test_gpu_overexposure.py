"""GPU checks of the stencil calls (lio_overexposure.hip: lio_exposure_recover, lio_exposure_gaussian_blur,
lio_exposure_recover_undistorted) against the contract restated in numpy (tests/overexposure_ref.py;
tests/test_overexposure_ref.py holds that restatement against scipy).  Every output is compared bit for bit: the device
side is integer-only but for the HSV -> BGR it shares with the other exposure calls."""
import ctypes as C

import numpy as np
import pytest

import exposure_ref as ER
import overexposure_ref as OR
import undistort_ref as UR
from lio_gpu import _capi
from lio_gpu import camera as CAM
from lio_gpu import exposure as EX

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
TILE_W, TILE_H = 64, 32  # the workgroup tile of ox_stencil_kernel as built (kOxTW, kOxTH)
# W x H: one pixel; two; a halo larger than the image (several reflections); ...; a width that is no multiple of 4 with
# a tile seam in both directions; one tile column
SHAPES = [(1, 1), (2, 1), (5, 7), (16, 15), (67, 38), (64, 48)]
DILATES = [1, 3, 5, 15]
KSIZES = [1, 3, 7, 15, 31]
SIGMAS = [0.0, 0.5, 2.6, 10.0]
THRESHOLDS = [0, 200, 254, 255]
IDENT = np.arange(256, dtype=np.uint8)


@pytest.fixture(scope="module")
def ex():
    e = EX.Exposure()
    yield e
    e.close()


def padded_out(width, height, channels):
    """an output whose rows are padded by 5 bytes holding a sentinel, which must survive"""
    row = channels * width
    buf = np.full((height, row + 5), SENTINEL, np.uint8)
    return buf, ER.strided(buf, width, height, channels)


def check_padding(buf, width, channels):
    assert (buf[:, channels * width:] == SENTINEL).all(), "the output's padding was written"


def check_pitches(ex, w, h, channels, seed):
    """both orders, an odd input pitch, a padded output"""
    img = ER.random_image(w, h, channels, pitch=channels * w + 7, seed=seed)
    for order in (0, 1):
        want = OR.recover(img, order=order)
        np.testing.assert_array_equal(ex.recover(img, order=order), want, err_msg=f"order {order}")
        buf, out = padded_out(w, h, channels)
        assert ex.recover(img, order=order, out=out) is out
        np.testing.assert_array_equal(out, want)
        check_padding(buf, w, channels)
    buf, out = padded_out(w, h, channels)
    ex.gaussian_blur(img, 15, out=out)
    np.testing.assert_array_equal(out, OR.gaussian_blur(img, 15))
    check_padding(buf, w, channels)


# ------------------------------------------------------------------------------------------------------- recover
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("channels", [3, 1])
def test_recover_equals_the_restatement(ex, shape, channels):
    w, h = shape
    for name, img in OR.images(w, h, channels).items():
        for order in (0, 1):
            np.testing.assert_array_equal(ex.recover(img, order=order), OR.recover(img, order=order), err_msg=f"{name} order {order}")
        np.testing.assert_array_equal(ex.recover(img, 100, 3, 7, 2.6), OR.recover(img, 100, 3, 7, 2.6), err_msg=name)
    check_pitches(ex, w, h, channels, seed=w + h)


@pytest.mark.parametrize("ksize", KSIZES)
@pytest.mark.parametrize("dilate", DILATES)
def test_recover_parameter_grid(ex, dilate, ksize):
    for (w, h), channels in (((67, 38), 3), ((67, 38), 1), ((5, 7), 3), ((16, 15), 1)):
        img = OR.images(w, h, channels)["sky" if channels == 3 else "random"]
        for sigma in SIGMAS:
            for thr in THRESHOLDS:
                np.testing.assert_array_equal(ex.recover(img, thr, dilate, ksize, sigma), OR.recover(img, thr, dilate, ksize, sigma),
                                              err_msg=f"{w}x{h}x{channels} threshold {thr} sigma {sigma}")


def test_larger_shape(ex):
    """1031 x 517: many workgroups, rows starting at every alignment, tile seams in both directions"""
    for channels in (3, 1):
        img = ER.random_image(1031, 517, channels, pitch=channels * 1031 + 1, seed=4 + channels)
        for order in (0, 1):
            want = OR.recover(img, 180, 5, 15, 0.0, order)
            buf, out = padded_out(1031, 517, channels)
            ex.recover(img, 180, 5, 15, 0.0, order, out=out)
            np.testing.assert_array_equal(out, want)
            check_padding(buf, 1031, channels)
        np.testing.assert_array_equal(ex.gaussian_blur(img, 31, 2.6), OR.gaussian_blur(img, 31, 2.6))


def test_strict_threshold(ex):
    """199..202 in stripes: at threshold 200 only 201 and 202 are masked"""
    for channels in (3, 1):
        img = OR.stripes(67, 38, channels)
        for thr in (198, 199, 200, 201, 202):
            for d in (1, 3):
                np.testing.assert_array_equal(ex.recover(img, thr, d, 15), OR.recover(img, thr, d, 15), err_msg=f"threshold {thr}")
    plane = OR.stripes(16, 4, 1)
    got = ex.recover(plane, 200, 1, 15)
    blurred = OR.gaussian_blur(plane, 15)
    np.testing.assert_array_equal(got, np.where(plane > 200, blurred, plane))
    assert (got[:, 0::4] == 199).all() and (got[:, 1::4] == 200).all()


@pytest.mark.parametrize("dilate", DILATES)
def test_footprint_of_bright_pixels(ex, dilate):
    """one bright pixel in each corner and in the centre of a dark ground: exactly the clipped dilate x dilate blocks
    are blended (on a plane nothing else is touched)"""
    rd = (dilate - 1) // 2
    for w, h in ((67, 38), (130, 70), (16, 15)):
        img = OR.bright_points(w, h, 1)
        got = ex.recover(img, 200, dilate, 15)
        np.testing.assert_array_equal(got, OR.recover(img, 200, dilate, 15))
        want = np.zeros((h, w), bool)
        for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)):
            want[max(y - rd, 0):y + rd + 1, max(x - rd, 0):x + rd + 1] = True
        np.testing.assert_array_equal(got, np.where(want, OR.gaussian_blur(img, 15), img))
        assert not (got != img)[~want].any() and (got != img)[h // 2, w // 2] and (got != img)[0, 0]
        img3 = OR.bright_points(w, h, 3)
        np.testing.assert_array_equal(ex.recover(img3, 200, dilate, 15), OR.recover(img3, 200, dilate, 15))


def test_steps_across_the_tile_seams(ex):
    """201 | 50 steps one pixel before, at and after the seam between two workgroup tiles, in both directions"""
    w, h = 2 * TILE_W + 3, 2 * TILE_H + 3
    for channels in (3, 1):
        for vertical, seam in ((False, TILE_W), (True, TILE_H)):
            for at in (seam - 1, seam, seam + 1):
                img = OR.step(w, h, channels, at, vertical)
                for d, k in ((5, 15), (15, 31), (1, 3)):
                    np.testing.assert_array_equal(ex.recover(img, 200, d, k), OR.recover(img, 200, d, k),
                                                  err_msg=f"vertical {vertical} at {at} dilate {d} ksize {k}")
                np.testing.assert_array_equal(ex.gaussian_blur(img, 15), OR.gaussian_blur(img, 15))


def test_every_entry_of_the_division_tables(ex):
    img = ER.vd_image()
    for order in (0, 1):
        np.testing.assert_array_equal(ex.recover(img, order=order), OR.recover(img, order=order))
        np.testing.assert_array_equal(ex.recover(img, 255, order=order), ex.remap(img, IDENT, None, order))


# ------------------------------------------------------------------------------------------- ties to the other calls
@pytest.mark.parametrize("shape", SHAPES + [(1031, 517)], ids=lambda s: "%dx%d" % s)
def test_no_mask_and_no_blur_are_the_round_trip(ex, shape):
    w, h = shape
    for channels in (3, 1):
        img = ER.random_image(w, h, channels, seed=w)
        for order in (0, 1):
            trip = ex.remap(img, IDENT, None, order)
            np.testing.assert_array_equal(ex.recover(img, 255, 5, 15, 0.0, order), trip, err_msg="threshold 255: an empty mask")
            np.testing.assert_array_equal(ex.recover(img, 200, 1, 1, 0.0, order), trip, err_msg="dilate 1, ksize 1")


# ------------------------------------------------------------------------------------------------- gaussian_blur
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("channels", [3, 1])
def test_gaussian_blur_equals_the_restatement(ex, shape, channels):
    w, h = shape
    imgs = ER.images(w, h, channels)
    for k in KSIZES:
        for sigma in SIGMAS:
            for name in ("random", "sky", "full"):
                np.testing.assert_array_equal(ex.gaussian_blur(imgs[name], k, sigma), OR.gaussian_blur(imgs[name], k, sigma),
                                              err_msg=f"{name} ksize {k} sigma {sigma}")
    for name, img in imgs.items():
        np.testing.assert_array_equal(ex.gaussian_blur(img, 1), img, err_msg=f"{name}: ksize 1 is the identity")
        np.testing.assert_array_equal(ex.gaussian_blur(img, 1, 2.6), img)


# ------------------------------------------------------------------------------------------------------- chained
@pytest.mark.parametrize("scene", [UR.scenes()[2], UR.scenes()[3]], ids=lambda s: s.name)  # 64 x 48 and 67 x 5 rectified
def test_recover_undistorted_equals_the_two_calls(ex, scene):
    def model(cam):
        return CAM.CameraModel(cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, cam.dist)

    ud = CAM.Undistorter()
    try:
        with pytest.raises(_capi.LioError) as e:
            ex.recover_undistorted(ud, np.zeros((48, 64, 3), np.uint8))
        assert e.value.code == _capi.LIO_ERR_STATE and "set_camera" in str(e.value)
        out_cam = scene.out_cam
        for channels in (3, 1):
            ud.set_camera(model(scene.src), model(scene.dst) if scene.dst is not None else None, channels=channels, border=(7, 200, 31))
            raw = UR.image(scene.src, channels, pitch=channels * scene.src.width + 7, seed=5)
            rect = ud(raw)
            np.testing.assert_array_equal(rect, UR.undistort(raw, scene.src, scene.dst, (7, 200, 31)))
            for order in (0, 1):
                two = ex.recover(rect, 150, 5, 15, 0.0, order)
                np.testing.assert_array_equal(two, OR.recover(rect, 150, 5, 15, 0.0, order))
                buf, out = padded_out(out_cam.width, out_cam.height, channels)
                ex.recover_undistorted(ud, raw, 150, 5, 15, 0.0, order, out=out)
                np.testing.assert_array_equal(out, two, err_msg=f"{scene.name} channels {channels} order {order}")
                check_padding(buf, out_cam.width, channels)
            np.testing.assert_array_equal(ud(raw), rect)  # the undistorter still serves its own calls
    finally:
        ud.close()


# ---------------------------------------------------------------------------------------------------- the handle
def test_frames_of_one_size_allocate_nothing_and_repeat():
    L = _capi.lib()
    e = EX.Exposure()
    try:
        frames = [ER.random_image(67, 38, 3, seed=20 + k % 3) for k in range(10)]  # frames 0, 3, 6, 9 are one image
        out = np.empty((38, 67, 3), np.uint8)
        first = e.recover(frames[0]).copy()
        after_first = L.lio_alloc_count()
        outs = [e.recover(f, out=out).copy() for f in frames]
        for f in frames[:3]:
            e.gaussian_blur(f, 15)
            e.recover(f, 100, 15, 31, 2.6)
        assert L.lio_alloc_count() == after_first
        for k in (0, 3, 6, 9):
            np.testing.assert_array_equal(outs[k], first)
        assert not np.array_equal(outs[1], first)
        np.testing.assert_array_equal(outs[1], OR.recover(frames[1]))
        t = e.stencil_timing()
        assert set(t) == {"upload_ms", "kernel_ms", "download_ms"}
        assert all(np.isfinite(v) and v >= 0.0 for v in t.values()), t
        np.testing.assert_array_equal(e.clahe(frames[0]), ER.clahe(frames[0]))  # the other calls share the staging
        assert L.lio_alloc_count() >= after_first
        again = e.recover(frames[0])
        np.testing.assert_array_equal(again, first)
    finally:
        e.close()


def test_handle_errors(ex):
    L = _capi.lib()
    img = np.zeros((48, 64, 3), np.uint8)
    p = img.ctypes.data_as(C.c_void_p)
    assert L.lio_exposure_recover(ex._h, p, 64, 48, 3, 191, 0, None, p, 192) == _capi.LIO_ERR_ARG
    assert b"pitch must be at least" in L.lio_last_error()
    assert L.lio_exposure_get_stencil_timing(ex._h, None) == _capi.LIO_ERR_ARG
    assert L.lio_exposure_recover_undistorted(ex._h, None, p, 192, 0, None, p, 192) == _capi.LIO_ERR_ARG
    assert b"undistorter is NULL" in L.lio_last_error()
    for kw in (dict(ksize=4), dict(dilate=2), dict(threshold=256), dict(sigma=float("inf"))):
        with pytest.raises(_capi.LioError) as e:
            ex.recover(img, **kw)
        assert e.value.code == _capi.LIO_ERR_ARG
