"""CPU checks of the numpy restatement of the overexposure contract (tests/overexposure_ref.py) against independent
formulations: scipy's mirror correlation and maximum filter, an impulse, the pinned weights; and of
lio_gaussian_weights from the built library (host only: no device is needed) against the restatement's weights."""
import ctypes as C

import numpy as np
import pytest
from scipy import ndimage

import exposure_ref as ER
import overexposure_ref as OR
from lio_gpu import _capi
from lio_gpu import exposure as EX

SHAPES = [(1, 1), (2, 1), (5, 7), (3, 20), (16, 15), (67, 38), (64, 48)]  # W x H


def test_pinned_weights():
    np.testing.assert_array_equal(OR.gaussian_weights(15, 0.0), OR.PINNED_15)
    np.testing.assert_array_equal(OR.gaussian_weights(15, -1.0), OR.PINNED_15)
    np.testing.assert_array_equal(OR.gaussian_weights(1, 0.0), [256])
    np.testing.assert_array_equal(OR.gaussian_weights(3, 0.0), [64, 128, 64])
    np.testing.assert_array_equal(OR.gaussian_weights(5, 0.0), [16, 64, 96, 64, 16])
    np.testing.assert_array_equal(OR.gaussian_weights(7, 0.0), [8, 28, 56, 72, 56, 28, 8])
    np.testing.assert_array_equal(OR.gaussian_weights(1, 2.6), [256])


@pytest.mark.parametrize("sigma", OR.SIGMAS)
def test_weights_sum_to_256_and_are_symmetric(sigma):
    for k in OR.KSIZES:
        w = OR.gaussian_weights(k, sigma)
        assert len(w) == k and w.sum() == 256 and (w >= 0).all(), (k, sigma, w)
        np.testing.assert_array_equal(w, w[::-1])


@pytest.mark.parametrize("sigma", OR.SIGMAS)
def test_library_weights_equal_the_restatement(sigma):
    """lio_gaussian_weights needs no device"""
    L = _capi.lib()
    for k in OR.KSIZES:
        w = np.full(32, 0xFFFF, np.uint16)
        assert L.lio_gaussian_weights(k, sigma, w.ctypes.data_as(C.POINTER(C.c_uint16))) == _capi.LIO_OK
        np.testing.assert_array_equal(w[:k], OR.gaussian_weights(k, sigma), err_msg=f"k {k} sigma {sigma}")
        assert (w[k:] == 0xFFFF).all()
        np.testing.assert_array_equal(EX.gaussian_weights(k, sigma), w[:k])
    np.testing.assert_array_equal(EX.gaussian_weights(15), OR.PINNED_15)


def test_refl_is_numpy_reflect_padding():
    for n in (1, 2, 3, 5, 16):
        base = np.arange(n)
        pad = 40
        want = np.pad(base, pad, mode="reflect") if n > 1 else np.zeros(n + 2 * pad, np.int64)
        np.testing.assert_array_equal(OR.refl(np.arange(-pad, n + pad), n), want)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_blur_equals_scipy_mirror_correlation(shape):
    w_, h_ = shape
    plane = np.random.default_rng(w_ * 100 + h_).integers(0, 256, (h_, w_)).astype(np.int64)
    for k, sigma in ((15, 0.0), (31, 10.0), (3, 0.0), (7, 0.5), (1, 0.0)):
        w = OR.gaussian_weights(k, sigma)
        rows = ndimage.correlate1d(plane, w, axis=1, mode="mirror")
        both = ndimage.correlate1d(rows, w, axis=0, mode="mirror")
        np.testing.assert_array_equal(OR.blur_plane(plane, w), (both + 32768) >> 16, err_msg=f"k {k}")
    np.testing.assert_array_equal(OR.blur_plane(plane, OR.gaussian_weights(1)), plane)


@pytest.mark.parametrize("d", [1, 3, 5, 15])
def test_dilate_equals_scipy_maximum_filter(d):
    for w_, h_ in SHAPES:
        mask = np.random.default_rng(d + w_).random((h_, w_)) < 0.1
        want = ndimage.maximum_filter(mask.astype(np.uint8), size=d, mode="constant", cval=0) > 0
        np.testing.assert_array_equal(OR.dilate(mask, d), want)


def test_impulse_blurs_to_the_outer_product():
    for k, sigma in ((15, 0.0), (7, 0.0), (31, 2.6)):
        w = OR.gaussian_weights(k, sigma)
        r = k // 2
        plane = np.zeros((2 * k + 3, 2 * k + 5), np.int64)
        cy, cx = k + 1, k + 2
        plane[cy, cx] = 255
        want = np.zeros_like(plane)
        want[cy - r:cy + r + 1, cx - r:cx + r + 1] = (255 * np.outer(w, w) + 32768) >> 16
        np.testing.assert_array_equal(OR.blur_plane(plane, w), want)


def test_constant_planes_are_fixed_points():
    for value in (0, 1, 77, 255):
        plane = np.full((9, 13), value, np.int64)
        for k in (1, 3, 15, 31):
            np.testing.assert_array_equal(OR.blur_plane(plane, OR.gaussian_weights(k)), plane)


def test_recover_properties():
    ident = np.arange(256, dtype=np.uint8)
    for channels in (3, 1):
        img = ER.images(67, 38, channels)["random"]
        for order in (0, 1):
            trip = ER.remap(img, ident, None, order)
            np.testing.assert_array_equal(OR.recover(img, 255, 5, 15, 0.0, order), trip)   # an empty mask
            np.testing.assert_array_equal(OR.recover(img, 200, 1, 1, 0.0, order), trip)    # the blur is the identity
        # threshold 0 on a plane without zeros: everything is masked
        bright = np.maximum(img, 1)
        if channels == 1:
            np.testing.assert_array_equal(OR.recover(bright, 0, 1, 15), OR.gaussian_blur(bright, 15))
    # the strict threshold: of 199..202 only 201 and 202 are masked
    st = OR.stripes(16, 4, 1)
    np.testing.assert_array_equal(OR.dilate(st.astype(np.int64) > 200, 1)[0, :4], [False, False, True, True])
    # the footprint of a bright pixel is the clipped dilate x dilate block
    pts = OR.bright_points(21, 17, 1)
    m = OR.dilate(pts.astype(np.int64) > 200, 5)
    assert m.sum() == 4 * 9 + 25 and m[:3, :3].all() and m[6:11, 8:13].all() and not m[3, 0] and not m[0, 3]
