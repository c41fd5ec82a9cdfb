"""CPU checks of the stencil interface (lio_gaussian_weights, lio_exposure_recover, lio_exposure_gaussian_blur,
lio_exposure_recover_undistorted, lio_exposure_get_stencil_timing): declared in the header with the contract in words,
exported and bound, every argument error with the word that names its bound (made before the handle is looked at, so
they show without a device), and LIO_ERR_NODEV without a device — there is no CPU path behind the frame calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lio_gpu import _capi
from lio_gpu import exposure as EX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fast-lio-sam_gps_amd", "lio_gpu", "_lib", "liblio_gpu.so")
NAMES = {"lio_gaussian_weights": 3, "lio_exposure_gaussian_blur": 10, "lio_exposure_recover": 10,
         "lio_exposure_recover_undistorted": 8, "lio_exposure_get_stencil_timing": 2}


def test_header_declares_the_entries_and_the_contract():
    src = open(os.path.join(ROOT, "include", "lio_gpu.h")).read()
    for name, nargs in NAMES.items():
        decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    part = src[src.index("overexposure recovery"):]
    assert src.index("overexposure recovery") > src.index("int lio_exposure_get_timing(")  # beside the exposure section
    text = " ".join(part.replace("*", " ").split())
    for words in ("AGREEMENT WITH cv2 IS OUR READING OF ITS SOURCE AND IS UNVERIFIED", "TIES TO EVEN", "STRICT", "1..32767",
                  "m0(x, y) = V(x, y) > threshold", "rd = (dilate - 1) / 2", "ONLY OVER POSITIONS INSIDE THE IMAGE",
                  "SUM TO 256", "{.0625, .25, .375, .25, .0625}", "{.03125, .109375, .21875, .28125, .21875, .109375, .03125}",
                  "((k - 1) 0.5 - 1) 0.3 + 0.8", "a = g[i] 256 + err", "w[k / 2] = 256 - 2 sum w[i]",
                  "1 3 6 12 20 30 36 40 36 30 20 12 6 3 1", "at most 65 280", "+ 32768) >> 16",
                  "REFLECT_101 APPLIED UNTIL THE INDEX IS IN RANGE", "q < n ? q : 2 (n - 1) - q", "V' = M ? B : V",
                  "ON EVERY PIXEL, MASKED OR NOT", "ONE UPLOAD AND ONE DOWNLOAD", "{200, 5, 15, 0}", "LIO_ERR_NODEV"):
        assert words in text, words
    fields = re.search(r"struct lio_recover_params \{([^}]*)\}", part).group(1)
    assert re.findall(r"(int|double)\s+(\w+);", fields) == [("int", "threshold"), ("int", "dilate"), ("int", "ksize"),
                                                           ("double", "sigma")]


def test_symbols_are_exported_bound_and_in_the_library():
    L = _capi.lib()
    raw = C.CDLL(LIB)  # the library itself, without the binding's declarations
    for name, nargs in NAMES.items():
        assert name in _capi.EXPORTS
        fn = getattr(L, name)
        assert fn.argtypes and len(fn.argtypes) == nargs and fn.restype is C.c_int, name
        assert getattr(raw, name), name
    assert C.sizeof(_capi.RecoverParams) == 24 and _capi.RecoverParams.sigma.offset == 16


def test_cpp_mirror_is_declared():
    src = open(os.path.join(ROOT, "include", "lio_gpu.hpp")).read()
    assert "struct RecoverParams {" in src and "inline std::vector<uint16_t> gaussian_weights(" in src
    body = src[src.index("class Exposure {"):]
    body = body[:body.index("\n};")]
    for m in ("recover(", "gaussian_blur(", "recover_undistorted(", "stencil_timing()", "lio_exposure_recover(",
              "lio_exposure_gaussian_blur(", "lio_exposure_recover_undistorted(", "lio_exposure_get_stencil_timing("):
        assert m in body, m


def expect_arg(rc, word):
    L = _capi.lib()
    assert rc == _capi.LIO_ERR_ARG, (rc, word, L.lio_last_error())
    assert word.encode() in L.lio_last_error(), (word, L.lio_last_error())


BUF = np.zeros(64 * 48 * 3 + 64, np.uint8)
P = BUF.ctypes.data_as(C.c_void_p)
W16 = np.zeros(32, np.uint16).ctypes.data_as(C.POINTER(C.c_uint16))


def image_args(**kw):
    a = dict(image=P, width=64, height=48, channels=3, pitch=192, order=0)
    a.update(kw)
    return [a[k] for k in ("image", "width", "height", "channels", "pitch", "order")]


def params(threshold=200, dilate=5, ksize=15, sigma=0.0):
    return C.byref(_capi.RecoverParams(threshold, dilate, ksize, sigma))


# (overrides of the image arguments, the word of the message)
BAD_IMAGES = [
    (dict(image=None), "image is NULL"),
    (dict(width=0), "1..32767"), (dict(height=0), "1..32767"), (dict(width=32768), "1..32767"), (dict(height=-1), "1..32767"),
    (dict(channels=0), "channels must be 1 or 3"), (dict(channels=2), "channels must be 1 or 3"),
    (dict(channels=4), "channels must be 1 or 3"),
    (dict(pitch=191), "pitch must be at least channels x width bytes"), (dict(pitch=0), "pitch must be at least"),
    (dict(pitch=-192), "pitch must be at least"), (dict(channels=1, pitch=63), "pitch must be at least"),
]


@pytest.mark.parametrize("k", range(len(BAD_IMAGES)))
def test_image_errors_name_their_bound_before_any_handle(k):
    """with a NULL handle: LIO_ERR_ARG comes before the handle (and the device) is looked at"""
    L = _capi.lib()
    kw, word = BAD_IMAGES[k]
    a = image_args(**kw)
    expect_arg(L.lio_exposure_recover(None, *a, None, P, 192), word)
    expect_arg(L.lio_exposure_recover(None, *a, params(), P, 192), word)
    expect_arg(L.lio_exposure_gaussian_blur(None, *a[:5], 15, 0.0, P, 192), word)


def test_order_errors():
    L = _capi.lib()
    for order in (2, -1):
        expect_arg(L.lio_exposure_recover(None, *image_args(order=order), None, P, 192), "order must be 0 (B G R) or 1 (R G B)")
        expect_arg(L.lio_exposure_recover_undistorted(None, None, P, 192, order, None, P, 192), "order must be 0")


BAD_PARAMS = [
    (dict(threshold=-1), "threshold must be in 0..255"), (dict(threshold=256), "threshold must be in 0..255"),
    (dict(dilate=0), "dilate must be odd and in 1..15"), (dict(dilate=4), "dilate must be odd and in 1..15"),
    (dict(dilate=17), "dilate must be odd and in 1..15"), (dict(dilate=-3), "dilate must be odd"),
    (dict(ksize=0), "ksize must be odd and in 1..31"), (dict(ksize=14), "ksize must be odd and in 1..31"),
    (dict(ksize=33), "ksize must be odd and in 1..31"), (dict(ksize=-5), "ksize must be odd"),
    (dict(sigma=float("nan")), "sigma must be finite"), (dict(sigma=float("inf")), "sigma must be finite"),
    (dict(sigma=float("-inf")), "sigma must be finite"),
]


@pytest.mark.parametrize("k", range(len(BAD_PARAMS)))
def test_parameter_errors_name_their_bound_before_any_handle(k):
    L = _capi.lib()
    kw, word = BAD_PARAMS[k]
    a = image_args()
    expect_arg(L.lio_exposure_recover(None, *a, params(**kw), P, 192), word)
    expect_arg(L.lio_exposure_recover_undistorted(None, None, P, 192, 0, params(**kw), P, 192), word)
    if "ksize" in kw or "sigma" in kw:
        expect_arg(L.lio_exposure_gaussian_blur(None, *a[:5], kw.get("ksize", 15), kw.get("sigma", 0.0), P, 192), word)
        expect_arg(L.lio_gaussian_weights(kw.get("ksize", 15), kw.get("sigma", 0.0), W16), word)


def test_the_other_argument_errors():
    L = _capi.lib()
    a = image_args()
    expect_arg(L.lio_gaussian_weights(15, 0.0, None), "w is NULL")
    expect_arg(L.lio_exposure_get_stencil_timing(None, None), "ms3 is NULL")
    expect_arg(L.lio_exposure_recover(None, *a, None, None, 192), "out is NULL")
    expect_arg(L.lio_exposure_gaussian_blur(None, *a[:5], 15, 0.0, None, 192), "out is NULL")
    expect_arg(L.lio_exposure_recover(None, *a, None, P, 191), "out_pitch must be at least channels x width bytes")
    expect_arg(L.lio_exposure_gaussian_blur(None, *a[:5], 15, 0.0, P, 0), "out_pitch must be at least")
    expect_arg(L.lio_exposure_recover_undistorted(None, None, None, 192, 0, None, P, 192), "raw_image is NULL")
    expect_arg(L.lio_exposure_recover_undistorted(None, None, P, 192, 0, None, None, 192), "out is NULL")
    # good arguments: the handle is next
    for rc in (L.lio_exposure_recover(None, *a, None, P, 192), L.lio_exposure_recover(None, *a, params(0, 15, 31, 10.0), P, 197),
               L.lio_exposure_recover(None, *a, params(255, 1, 1, -2.0), P, 192),
               L.lio_exposure_gaussian_blur(None, *a[:5], 1, 0.5, P, 192),
               L.lio_exposure_recover_undistorted(None, None, P, 192, 1, None, P, 192)):
        assert rc in (_capi.LIO_ERR_NODEV, _capi.LIO_ERR_ARG) and (rc == _capi.LIO_ERR_NODEV or b"handle is NULL" in L.lio_last_error())


def test_python_weights_errors():
    for k, s in ((4, 0.0), (0, 0.0), (33, 0.0), (15, float("nan"))):
        with pytest.raises(_capi.LioError) as e:
            EX.gaussian_weights(k, s)
        assert e.value.code == _capi.LIO_ERR_ARG


def test_entries_fail_loudly_without_device():
    L = _capi.lib()
    if L.lio_device_count() > 0:
        pytest.skip("a device is visible; covered by the gpu tests")
    a = image_args()
    ms = np.zeros(3)
    assert L.lio_exposure_recover(None, *a, None, P, 192) == _capi.LIO_ERR_NODEV
    assert L.lio_exposure_gaussian_blur(None, *a[:5], 15, 0.0, P, 192) == _capi.LIO_ERR_NODEV
    assert L.lio_exposure_recover_undistorted(None, None, P, 192, 0, None, P, 192) == _capi.LIO_ERR_NODEV
    assert L.lio_exposure_get_stencil_timing(None, ms.ctypes.data_as(_capi.dp)) == _capi.LIO_ERR_NODEV
    assert L.lio_gaussian_weights(15, 0.0, W16) == _capi.LIO_OK  # host only
