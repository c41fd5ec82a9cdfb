"""GPU checks of the exposure adaption (lio_exposure.hip: lio_exposure_*) against the contract restated in numpy
(tests/exposure_ref.py; tests/test_exposure_ref.py holds that restatement against itself).  Every output is compared
bit for bit: both sides perform the same integer and IEEE float32 operations."""
import ctypes as C

import numpy as np
import pytest

import exposure_ref as ER
import undistort_ref as UR
from lio_gpu import _capi
from lio_gpu import camera as CAM
from lio_gpu import exposure as EX

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
# (width, height, tiles_x, tiles_y): divisible; padded both ways; the whole-tile quirk pad; tiles 2 x 2 pixels after
# padding; one tile; tiles that divide neither way evenly
SHAPES = [(64, 48, 8, 8), (67, 38, 8, 8), (64, 38, 8, 8), (9, 7, 8, 6), (5, 7, 1, 1), (64, 48, 3, 5)]
CLIPS = [2.0, 0.0, 0.001, 40.0, 1e6]


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


# --------------------------------------------------------------------------------------------------------- CLAHE
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_%dx%d" % s)
@pytest.mark.parametrize("channels", [3, 1])
def test_clahe_equals_the_restatement(ex, shape, channels):
    w, h, tx, ty = shape
    for name, img in ER.images(w, h, channels).items():
        for clip in CLIPS:
            want = ER.clahe(img, clip, (tx, ty))
            np.testing.assert_array_equal(ex.clahe(img, clip, (tx, ty)), want, err_msg=f"{name} clip {clip}")
    # both orders, an odd input pitch, a padded output
    img = ER.random_image(w, h, channels, pitch=channels * w + 7, seed=w + h)
    for order in (0, 1):
        want = ER.clahe(img, 2.0, (tx, ty), order)
        np.testing.assert_array_equal(ex.clahe(img, 2.0, (tx, ty), order), want, err_msg=f"order {order}")
        buf, out = padded_out(w, h, channels)
        assert ex.clahe(img, 2.0, (tx, ty), order, out=out) is out
        np.testing.assert_array_equal(out, want)
        check_padding(buf, w, channels)


def test_constant_images_map_to_one_value(ex):
    for value in (0, 255, 77):
        for channels in (1, 3):
            img = np.full((48, 64) if channels == 1 else (48, 64, 3), value, np.uint8)
            out = ex.clahe(img, 2.0, (8, 8))
            assert len(np.unique(out)) == 1
            np.testing.assert_array_equal(out, ER.clahe(img, 2.0, (8, 8)))


def test_every_entry_of_the_division_tables(ex):
    """every (v, d) pair with the maximum on each channel: the identity table on V is the HSV round trip alone"""
    img = ER.vd_image()
    ident = np.arange(256, dtype=np.uint8)
    for order in (0, 1):
        np.testing.assert_array_equal(ex.remap(img, ident, None, order), ER.remap(img, ident, None, order))
    np.testing.assert_array_equal(ex.clahe(img, 2.0, (8, 8)), ER.clahe(img, 2.0, (8, 8)))


def test_larger_shape(ex):
    """1031 x 517 with 8 x 8 tiles: several workgroups per tile, a width that is no multiple of 4, padding both ways, rows
    that start at every alignment"""
    for channels in (3, 1):
        img = ER.random_image(1031, 517, channels, pitch=channels * 1031 + 1, seed=4 + channels)
        want = ER.clahe(img, 2.0, (8, 8))
        buf, out = padded_out(1031, 517, channels)
        ex.clahe(img, 2.0, (8, 8), out=out)
        np.testing.assert_array_equal(out, want)
        check_padding(buf, 1031, channels)
        hv, hg = ex.histograms(img)
        rv, rg = ER.histograms(img)
        np.testing.assert_array_equal(hv, rv)
        np.testing.assert_array_equal(hg, rg)
    sky = np.full((517, 1031, 3), 255, np.uint8)  # the LDS-atomic worst case on many workgroups
    hv, hg = ex.histograms(sky)
    assert hv[255] == hg[255] == 1031 * 517 and hv.sum() == hg.sum() == 1031 * 517


# ---------------------------------------------------------------------------------------------------- histograms
@pytest.mark.parametrize("shape", [(64, 48), (67, 38), (5, 7), (1, 1)], ids=lambda s: "%dx%d" % s)
def test_histograms(ex, shape):
    w, h = shape
    for channels in (3, 1):
        for name, img in ER.images(w, h, channels).items():
            for order in (0, 1):
                hv, hg = ex.histograms(img, order)
                rv, rg = ER.histograms(img, order)
                np.testing.assert_array_equal(hv, rv, err_msg=name)
                np.testing.assert_array_equal(hg, rg, err_msg=name)
                assert hv.sum() == hg.sum() == w * h
        img = ER.random_image(w, h, channels, pitch=channels * w + 3, seed=1)
        np.testing.assert_array_equal(ex.histograms(img)[1], ER.histograms(img)[1])


# --------------------------------------------------------------------------------------------------------- remap
@pytest.mark.parametrize("shape", [(64, 48), (67, 38), (5, 7)], ids=lambda s: "%dx%d" % s)
def test_remap(ex, shape):
    w, h = shape
    rng = np.random.default_rng(w)
    lut_v, lut_all = rng.integers(0, 256, 256, dtype=np.uint8), rng.integers(0, 256, 256, dtype=np.uint8)
    for channels in (3, 1):
        img = ER.random_image(w, h, channels, pitch=channels * w + 7, seed=2)
        for order in (0, 1):
            for lv, la in ((lut_v, None), (None, lut_all), (lut_v, lut_all)):
                want = ER.remap(img, lv, la, order)
                buf, out = padded_out(w, h, channels)
                ex.remap(img, lv, la, order, out=out)
                np.testing.assert_array_equal(out, want, err_msg=f"channels {channels} order {order}")
                check_padding(buf, w, channels)
    with pytest.raises(_capi.LioError) as e:
        ex.remap(img, None, None)
    assert e.value.code == _capi.LIO_ERR_ARG and "both NULL" in str(e.value)


def exposure_image(kind):
    """64 x 48 x 3 built to trigger one branch of detect_exposure"""
    rng = np.random.default_rng(12)
    img = rng.integers(60, 190, (48, 64, 3), dtype=np.uint8)
    if kind == "overexposed":
        img[:20] = rng.integers(215, 256, (20, 64, 3), dtype=np.uint8)
    if kind == "underexposed":
        img[:20] = rng.integers(0, 40, (20, 64, 3), dtype=np.uint8)
    return img


@pytest.mark.parametrize("kind", ["overexposed", "underexposed", "well-exposed"])
def test_correct_exposure_branches(ex, kind):
    img = exposure_image(kind)
    rv, rg = ER.histograms(img)
    assert EX.detect_exposure(rg) == kind
    got, state = EX.correct_exposure(img, handle=ex)
    assert state == kind
    if kind == "overexposed":
        want = ER.remap(img, EX.equalize_lut(rv), EX.gamma_lut(0.8))
        np.testing.assert_array_equal(EX.correct_overexposure(img, handle=ex), want)
    elif kind == "underexposed":
        want = ER.remap(img, EX.stretch_lut(rv, 5, 95), EX.gamma_lut(1.2))
        np.testing.assert_array_equal(EX.correct_underexposure(img, handle=ex), want)
    else:
        want = img
        assert got is not img
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(EX.adapt_exposure(img, handle=ex), ER.clahe(img, 2.0, (8, 8)))


# ------------------------------------------------------------------------------------------------------- chained
@pytest.mark.parametrize("scene", [UR.scenes()[2], UR.scenes()[3]], ids=lambda s: s.name)  # 64 x 48 and 67 x 5 rectified
def test_clahe_undistorted_equals_the_two_calls(ex, scene):
    def model(cam):
        return CAM.CameraModel(cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, cam.dist)

    ud = CAM.Undistorter()
    try:
        with pytest.raises(_capi.LioError) as e:
            ex.clahe_undistorted(ud, np.zeros((48, 64, 3), np.uint8))
        assert e.value.code == _capi.LIO_ERR_STATE and "set_camera" in str(e.value)
        out_cam = scene.out_cam
        for channels in (3, 1):
            ud.set_camera(model(scene.src), model(scene.dst) if scene.dst is not None else None, channels=channels, border=(7, 200, 31))
            raw = UR.image(scene.src, channels, pitch=channels * scene.src.width + 7, seed=5)
            rect = ud(raw)
            np.testing.assert_array_equal(rect, UR.undistort(raw, scene.src, scene.dst, (7, 200, 31)))
            for order in (0, 1):
                two = ex.clahe(rect, 2.0, (8, 8), order)
                np.testing.assert_array_equal(two, ER.clahe(rect, 2.0, (8, 8), order))
                buf, out = padded_out(out_cam.width, out_cam.height, channels)
                ex.clahe_undistorted(ud, raw, 2.0, (8, 8), order, out=out)
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
        first = e.clahe(frames[0]).copy()
        after_first = L.lio_alloc_count()
        outs = [e.clahe(f, out=out).copy() for f in frames]
        assert L.lio_alloc_count() == after_first
        for f in frames[:3]:  # the other entries share the staging and the arena of that first frame
            e.histograms(f)
            e.remap(f, np.arange(256, dtype=np.uint8), None)
        assert L.lio_alloc_count() == after_first
        for k in (0, 3, 6, 9):
            np.testing.assert_array_equal(outs[k], first)
        assert not np.array_equal(outs[1], first)
        np.testing.assert_array_equal(outs[1], ER.clahe(frames[1]))
        t = e.timing()
        assert set(t) == {"upload_ms", "hist_ms", "lut_ms", "apply_ms", "download_ms"}
        assert all(np.isfinite(v) and v >= 0.0 for v in t.values()), t
    finally:
        e.close()


def test_two_sizes_in_turn_on_one_handle(ex):
    for (w, h, tx, ty), channels in ((SHAPES[1], 3), (SHAPES[3], 1), (SHAPES[0], 3), (SHAPES[1], 1), (SHAPES[3], 3)):
        img = ER.random_image(w, h, channels, seed=w)
        np.testing.assert_array_equal(ex.clahe(img, 2.0, (tx, ty)), ER.clahe(img, 2.0, (tx, ty)))


def test_many_small_tiles(ex):
    """64 x 4 tiles of 3 x 3 pixels on 150 x 9 (padded by 42 columns and 3 rows), and the most tiles there are"""
    for (w, h, tx, ty) in ((150, 9, 64, 4), (130, 131, 64, 64)):
        for channels in (3, 1):
            img = ER.random_image(w, h, channels, seed=h)
            np.testing.assert_array_equal(ex.clahe(img, 2.0, (tx, ty)), ER.clahe(img, 2.0, (tx, ty)), err_msg=f"{w}x{h}")


def test_handle_errors(ex):
    L = _capi.lib()
    img = np.zeros((48, 64, 3), np.uint8)
    p = img.ctypes.data_as(C.c_void_p)
    assert L.lio_exposure_clahe(ex._h, p, 64, 48, 3, 191, 0, 2.0, 8, 8, p, 192) == _capi.LIO_ERR_ARG
    assert b"pitch must be at least" in L.lio_last_error()
    assert L.lio_exposure_get_timing(ex._h, None) == _capi.LIO_ERR_ARG
    assert L.lio_exposure_clahe_undistorted(ex._h, None, p, 192, 0, 2.0, 8, 8, p, 192) == _capi.LIO_ERR_ARG
    assert b"undistorter is NULL" in L.lio_last_error()
    with pytest.raises(_capi.LioError) as e:
        ex.clahe(np.zeros((7, 2), np.uint8), 2.0, (4, 1))
    assert e.value.code == _capi.LIO_ERR_ARG and "at most width - 1" in str(e.value)
