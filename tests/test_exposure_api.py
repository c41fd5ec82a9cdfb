"""CPU checks of the exposure interface (lio_exposure_*): declared in the header with the contract in words, exported
and bound, no new struct, every argument error with the word that names its bound (they are made before the handle is
looked at, so they show without a device), and LIO_ERR_NODEV without a device, from C and from lio_gpu.exposure —
there is no CPU path behind any of it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lio_gpu import _capi
from lio_gpu import exposure as EX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"lio_exposure_create": 2, "lio_exposure_destroy": 1, "lio_exposure_histograms": 9, "lio_exposure_clahe": 12,
         "lio_exposure_remap": 11, "lio_exposure_clahe_undistorted": 10, "lio_exposure_get_timing": 2}


def test_header_declares_the_entries_and_the_contract():
    src = open(os.path.join(ROOT, "include", "lio_gpu.h")).read()
    for name, nargs in NAMES.items():
        decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    assert src.index("exposure adaption") > src.index("lio_icp_get_timing(lio_icp* h")  # after the timing section
    text = " ".join(src.replace("*", " ").split())
    for words in ("AGREEMENT WITH cv2 IS OUR READING OF ITS SOURCE AND IS UNVERIFIED", "TIES TO EVEN", "0 = B G R", "1 = R G B",
                  "sdiv[i] = rint((255 << 12) / i)", "hdiv[i] = rint((180 << 12) / (6 i))", "s = (d sdiv[v] + 2048) >> 12",
                  "h = (h0 hdiv[d] + 2048) >> 12", "if h < 0, h += 180", "0x1.111112p-5f", "0x1.010102p-8f",
                  "{1,3,0} {1,0,2} {3,0,1} {0,2,1} {0,1,3} {2,1,0}", "sat(rint(x 255.0f))", "REFLECT_101: x >= W reads 2 (W - 1) - x",
                  "PADDED BY A WHOLE tiles_x OR tiles_y", "clip = max((int)(clip_limit area / 256), 1)",
                  "step = max(256 / res, 1)", "k % step == 0 and k / step < res", "scale = 255.0f / (float)area",
                  "txf = (float)x (1.0f / (float)tw) - 0.5f", "gray = (3735 b + 19235 g + 9798 r + 16384) >> 15",
                  "ONE UPLOAD AND ONE DOWNLOAD", "1..32767", "1..64", "LIO_ERR_NODEV"):
        assert words in text, words
    assert "typedef struct lio_exposure lio_exposure;" in src


def test_symbols_are_exported_and_bound():
    L = _capi.lib()
    for name, nargs in NAMES.items():
        assert name in _capi.EXPORTS
        fn = getattr(L, name)
        assert fn.argtypes and len(fn.argtypes) == nargs and fn.restype is C.c_int, name


def test_no_new_struct():
    L = _capi.lib()
    assert len(_capi._ABI_STRUCTS) == 15 and L.lio_abi_struct_sizes(None, 0) == 15
    assert _capi._ABI_CAMERA_STRUCTS == ("Camera", "ColorizeParams") and L.lio_abi_camera_struct_sizes(None, 0) == 2
    src = open(os.path.join(ROOT, "include", "lio_gpu.h")).read()
    part = src[src.index("exposure adaption"):]
    assert "typedef struct lio_exposure lio_exposure;" in part and not re.search(r"typedef\s+struct\s+\w+\s*\{", part)


def expect_arg(rc, word):
    L = _capi.lib()
    assert rc == _capi.LIO_ERR_ARG, (rc, word, L.lio_last_error())
    assert word.encode() in L.lio_last_error(), (word, L.lio_last_error())


BUF = np.zeros(64 * 48 * 3 + 64, np.uint8)
P = BUF.ctypes.data_as(C.c_void_p)
LUT = np.arange(256, dtype=np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))


def image_args(**kw):
    a = dict(image=P, width=64, height=48, channels=3, pitch=192, order=0)
    a.update(kw)
    return [a[k] for k in ("image", "width", "height", "channels", "pitch", "order")]


# (overrides of the image arguments, the word of the message)
BAD_IMAGES = [
    (dict(image=None), "image is NULL"),
    (dict(width=0), "1..32767"), (dict(height=0), "1..32767"), (dict(width=32768), "1..32767"), (dict(height=-1), "1..32767"),
    (dict(channels=0), "channels must be 1 or 3"), (dict(channels=2), "channels must be 1 or 3"),
    (dict(channels=4), "channels must be 1 or 3"),
    (dict(order=2), "order must be 0 (B G R) or 1 (R G B)"), (dict(order=-1), "order must be 0"),
    (dict(pitch=191), "pitch must be at least channels x width bytes"), (dict(pitch=0), "pitch must be at least"),
    (dict(pitch=-192), "pitch must be at least"), (dict(channels=1, pitch=63), "pitch must be at least"),
]


@pytest.mark.parametrize("k", range(len(BAD_IMAGES)))
def test_image_errors_name_their_bound_before_any_handle(k):
    """with a NULL handle: LIO_ERR_ARG comes before the handle (and the device) is looked at"""
    L = _capi.lib()
    kw, word = BAD_IMAGES[k]
    a = image_args(**kw)
    expect_arg(L.lio_exposure_histograms(None, *a, None, None), word)
    expect_arg(L.lio_exposure_clahe(None, *a, 2.0, 8, 8, P, 192), word)
    expect_arg(L.lio_exposure_remap(None, *a, LUT, LUT, P, 192), word)


def test_the_other_argument_errors():
    L = _capi.lib()
    a = image_args()
    expect_arg(L.lio_exposure_create(0, None), "out is NULL")
    expect_arg(L.lio_exposure_get_timing(None, None), "ms5 is NULL")
    expect_arg(L.lio_exposure_clahe(None, *a, 2.0, 8, 8, None, 192), "out is NULL")
    expect_arg(L.lio_exposure_remap(None, *a, LUT, LUT, None, 192), "out is NULL")
    expect_arg(L.lio_exposure_clahe(None, *a, 2.0, 8, 8, P, 191), "out_pitch must be at least channels x width bytes")
    expect_arg(L.lio_exposure_remap(None, *a, LUT, None, P, 0), "out_pitch must be at least")
    expect_arg(L.lio_exposure_remap(None, *a, None, None, P, 192), "both NULL")
    for tx, ty in ((0, 8), (8, 0), (65, 8), (8, 65), (-1, 8)):
        expect_arg(L.lio_exposure_clahe(None, *a, 2.0, tx, ty, P, 192), "tiles_x and tiles_y must be in 1..64")
        expect_arg(L.lio_exposure_clahe_undistorted(None, None, P, 192, 0, 2.0, tx, ty, P, 192), "1..64")
    # the padding bound: 2 x 48 with 4 x 1 tiles would reflect 2 columns of a width of 2; 8 x 3 with 8 x 8 tiles pads the
    # evenly dividing width by a whole 8
    expect_arg(L.lio_exposure_clahe(None, *image_args(width=2, channels=1, pitch=2), 2.0, 4, 1, P, 2), "at most width - 1 and height - 1")
    expect_arg(L.lio_exposure_clahe(None, *image_args(width=8, height=3, channels=1, pitch=8), 2.0, 8, 8, P, 8), "at most width - 1")
    # the clip bounds
    expect_arg(L.lio_exposure_clahe(None, *a, float("nan"), 8, 8, P, 192), "below 2^31 and not NaN")
    expect_arg(L.lio_exposure_clahe(None, *a, 1e12, 8, 8, P, 192), "below 2^31 and not NaN")
    expect_arg(L.lio_exposure_clahe(None, *a, float("inf"), 8, 8, P, 192), "below 2^31")
    expect_arg(L.lio_exposure_clahe_undistorted(None, None, P, 192, 0, float("nan"), 8, 8, P, 192), "not NaN")
    expect_arg(L.lio_exposure_clahe_undistorted(None, None, None, 192, 0, 2.0, 8, 8, P, 192), "raw_image is NULL")
    expect_arg(L.lio_exposure_clahe_undistorted(None, None, P, 192, 0, 2.0, 8, 8, None, 192), "out is NULL")
    expect_arg(L.lio_exposure_clahe_undistorted(None, None, P, 192, 3, 2.0, 8, 8, P, 192), "order must be 0")
    # good arguments: the handle is next
    for rc in (L.lio_exposure_clahe(None, *a, 2.0, 8, 8, P, 192), L.lio_exposure_clahe(None, *a, -1.0, 64, 1, P, 197),
               L.lio_exposure_remap(None, *a, None, LUT, P, 192), L.lio_exposure_histograms(None, *a, None, None),
               L.lio_exposure_clahe_undistorted(None, None, P, 192, 1, 2.0, 8, 8, P, 192)):
        assert rc in (_capi.LIO_ERR_NODEV, _capi.LIO_ERR_ARG) and (rc == _capi.LIO_ERR_NODEV or b"handle is NULL" in L.lio_last_error())


def test_python_argument_forms():
    for bad in (np.zeros(256, np.uint16), np.zeros(255, np.uint8), np.zeros((2, 128), np.uint8)):
        with pytest.raises(ValueError):
            EX._table(bad, "lut_v")
    assert EX._table(None, "lut_v") == (None, None)
    with pytest.raises(ValueError):
        EX._out(np.zeros((4, 8, 3), np.uint8)[:, ::2], (4, 4, 3), 3, 4)  # pixels not packed
    with pytest.raises(ValueError):
        EX._out(np.zeros((4, 8), np.float32), (4, 8), 1, 8)
    with pytest.raises(ValueError):
        EX.equalize_lut(np.zeros(255))
    with pytest.raises(ValueError):
        EX.detect_exposure(np.zeros(256))


def test_cpp_mirror_is_declared():
    src = open(os.path.join(ROOT, "include", "lio_gpu.hpp")).read()
    for fn in ("inline ExposureLut equalize_lut(", "inline ExposureLut stretch_lut(", "inline ExposureLut gamma_lut(",
               "inline int detect_exposure(", "inline double hist_percentile("):
        assert fn in src, fn
    body = src[src.index("class Exposure {"):]
    body = body[:body.index("\n};")]
    for m in ("histograms(", "clahe(", "remap(", "claheUndistorted(", "timing()", "lio_exposure_histograms(", "lio_exposure_clahe(",
              "lio_exposure_remap(", "lio_exposure_clahe_undistorted(", "lio_exposure_get_timing("):
        assert m in body, m


def test_entries_fail_loudly_without_device():
    L = _capi.lib()
    if L.lio_device_count() > 0:
        pytest.skip("a device is visible; covered by the gpu tests")
    h = C.c_void_p()
    rc = L.lio_exposure_create(0, C.byref(h))
    assert rc == _capi.LIO_ERR_NODEV and not h.value
    assert b"no HIP device" in L.lio_last_error() or b"gfx950" in L.lio_last_error()
    a = image_args()
    ms = np.zeros(5)
    hist = np.zeros(256, np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    assert L.lio_exposure_histograms(None, *a, hist, hist) == _capi.LIO_ERR_NODEV
    assert L.lio_exposure_clahe(None, *a, 2.0, 8, 8, P, 192) == _capi.LIO_ERR_NODEV
    assert L.lio_exposure_remap(None, *a, LUT, LUT, P, 192) == _capi.LIO_ERR_NODEV
    assert L.lio_exposure_clahe_undistorted(None, None, P, 192, 0, 2.0, 8, 8, P, 192) == _capi.LIO_ERR_NODEV
    assert L.lio_exposure_get_timing(None, ms.ctypes.data_as(_capi.dp)) == _capi.LIO_ERR_NODEV
    assert L.lio_exposure_destroy(None) == _capi.LIO_OK
    img = np.zeros((48, 64, 3), np.uint8)
    for call in (EX.Exposure, lambda: EX.adapt_exposure(img), lambda: EX.correct_exposure(img), lambda: EX.correct_overexposure(img),
                 lambda: EX.correct_underexposure(img)):
        with pytest.raises(_capi.LioError) as e:
            call()
        assert e.value.code == _capi.LIO_ERR_NODEV
