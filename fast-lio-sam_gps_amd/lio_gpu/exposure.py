"""Exposure adaption of camera frames: the step the reference runs on every rectified image
(post_process/exposure_adaption), over the C-ABI.

* :class:`Exposure` — ``histograms``, ``clahe``, ``remap``, ``clahe_undistorted`` (``lio_exposure_*``), and the stencil
  calls ``recover`` (``solve_overexposure``'s ``recover_overexposure``), ``gaussian_blur``, ``recover_undistorted``
* :func:`gaussian_weights` — the fixed-point weights of the 8-bit Gaussian blur
* :func:`equalize_lut`, :func:`stretch_lut`, :func:`gamma_lut`, :func:`detect_exposure` — the host side of
  ``correct_exposure``: 256-entry tables from a 256-bin histogram, a few hundred operations per frame
* :func:`adapt_exposure` — ``CLAHE_region_adjusted.py``'s function (clip 2.0, 8 x 8 tiles);
  :func:`correct_overexposure`, :func:`correct_underexposure`, :func:`correct_exposure` — ``correct_exposure``'s

Images are numpy arrays (``height x width`` or ``height x width x 3`` uint8, B G R by default as ``cv2.imread``
gives them).  Every result follows the contract of include/lio_gpu.h bit for bit; that the contract is what OpenCV
computes is a reading of its source and is unverified.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._capi import RecoverParams, check, lib
from .camera import _out, _plane
from .filters import _Handle

_i64p = C.POINTER(C.c_int64)
_u8p = C.POINTER(C.c_uint8)
BGR, RGB = 0, 1


# ------------------------------------------------------------------------------------------------ host helpers
def _hist(hist) -> np.ndarray:
    h = np.asarray(hist)
    if h.shape != (256,) or (h < 0).any():
        raise ValueError("a histogram of 256 non-negative counts is expected")
    h = h.astype(np.int64)
    if h.sum() < 1:
        raise ValueError("the histogram is empty")
    return h


def _sat_rint_f32(x) -> np.ndarray:
    return np.clip(np.rint(np.asarray(x, np.float32)), 0, 255).astype(np.uint8)


def equalize_lut(hist) -> np.ndarray:
    """our reading of ``cv2.equalizeHist``: ``i0`` is the first non-empty bin; if it holds every pixel the table maps
    everything to ``i0``; otherwise ``scale = 255.0f / (float)(total - hist[i0])``, ``lut[i <= i0] = 0`` and
    ``lut[i] = sat(rint((float)sum_{i0 < j <= i} hist[j] * scale))`` in float32"""
    h = _hist(hist)
    total = int(h.sum())
    i0 = int(np.flatnonzero(h)[0])
    if int(h[i0]) == total:
        return np.full(256, i0, np.uint8)
    scale = np.float32(255.0) / np.float32(total - int(h[i0]))
    tail = h.copy()
    tail[:i0 + 1] = 0
    return _sat_rint_f32(np.cumsum(tail).astype(np.float32) * scale)


def hist_percentile(hist, q: float) -> float:
    """``np.percentile(plane, q)`` (the default, linear method) from the plane's histogram: the position ``q / 100 *
    (n - 1)`` in the sorted values, computed as numpy computes it, ``(n - 1) * (q / 100)``, and numpy's
    interpolation ``a + (b - a) t``, or ``b - (b - a) (1 - t)`` when ``t >= 0.5``, in double"""
    h = _hist(hist)
    n = int(h.sum())
    pos = float(n - 1) * (float(q) / 100.0)
    pos = min(max(pos, 0.0), float(n - 1))
    lo = int(np.floor(pos))
    t = pos - lo
    cum = np.cumsum(h)
    a = float(np.searchsorted(cum, lo, side="right"))               # the sorted plane's value at index lo
    b = float(np.searchsorted(cum, min(lo + 1, n - 1), side="right"))
    d = b - a
    return b - d * (1.0 - t) if t >= 0.5 else a + d * t


def stretch_lut(hist, lo_pct: float = 5.0, hi_pct: float = 95.0) -> np.ndarray:
    """``correct_exposure:59-61``: ``lut[v] = uint8(clip((v - lo) / (hi - lo) * 255, 0, 255))`` in double, truncating,
    with ``lo``, ``hi`` the two percentiles of the plane whose histogram this is.  ``hi == lo`` is an error (the
    script divides by zero there)."""
    lo, hi = hist_percentile(hist, lo_pct), hist_percentile(hist, hi_pct)
    if hi == lo:
        raise ValueError(f"stretch_lut: the {lo_pct:g} and {hi_pct:g} percentiles are both {lo:g}")
    v = np.arange(256, dtype=np.float64)
    return np.clip((v - lo) / (hi - lo) * 255.0, 0.0, 255.0).astype(np.uint8)


def gamma_lut(gamma: float) -> np.ndarray:
    """``correct_exposure:48, 69``: ``uint8(clip((x / 255.0) ** gamma * 255.0, 0, 255))`` in double"""
    x = np.arange(256, dtype=np.float64)
    return np.clip(((x / 255.0) ** np.float64(gamma)) * 255.0, 0.0, 255.0).astype(np.uint8)


def detect_exposure(hist_gray) -> str:
    """``correct_exposure:19-30``: more than 0.3 of the pixels in bins ``[200:]``: "overexposed"; else more than 0.3 in
    bins ``[:50]``: "underexposed"; else "well-exposed".  The ratios are taken in double."""
    h = _hist(hist_gray)
    total = float(h.sum())
    if float(h[200:].sum()) / total > 0.3:
        return "overexposed"
    if float(h[:50].sum()) / total > 0.3:
        return "underexposed"
    return "well-exposed"


def gaussian_weights(ksize: int, sigma: float = 0.0) -> np.ndarray:
    """the ``ksize`` fixed-point weights (uint16, 8 fractional bits, their sum is 256) of the 8-bit Gaussian blur, from
    the library (``lio_gaussian_weights``; host only, no device is needed)"""
    w = np.zeros(max(int(ksize), 1), np.uint16)
    check(lib().lio_gaussian_weights(int(ksize), float(sigma), w.ctypes.data_as(C.POINTER(C.c_uint16))))
    return w


# ------------------------------------------------------------------------------------------------- the handle
def _table(lut, name):
    if lut is None:
        return None, None
    a = np.ascontiguousarray(lut)
    if a.dtype != np.uint8 or a.shape != (256,):
        raise ValueError(f"{name}: 256 uint8 values are expected")
    return a, a.ctypes.data_as(_u8p)


class Exposure(_Handle):
    """One handle for the exposure work on frames of any size: the staging is reused across frames.  ``order``:
    :data:`BGR` (0, OpenCV's) or :data:`RGB` (1); the output has the input's order."""

    _create, _destroy = "lio_exposure_create", "lio_exposure_destroy"

    @staticmethod
    def _image(image):
        a = np.asarray(image)
        if a.ndim not in (2, 3):
            raise ValueError("image: a height x width, height x width x 1 or height x width x 3 uint8 array is expected")
        return _plane(a, a.shape[1], a.shape[0])

    def histograms(self, image, order: int = BGR):
        """``(hist_v, hist_gray)``, 256 int64 each: of V (the channel maximum) and of OpenCV's gray; with one
        channel both are the plane's"""
        img, pitch, ch = self._image(image)
        hv, hg = np.zeros(256, np.int64), np.zeros(256, np.int64)
        check(lib().lio_exposure_histograms(self._h, img.ctypes.data_as(C.c_void_p), img.shape[1], img.shape[0], ch, pitch,
                                            int(order), hv.ctypes.data_as(_i64p), hg.ctypes.data_as(_i64p)))
        return hv, hg

    def clahe(self, image, clip_limit: float = 2.0, tiles=(8, 8), order: int = BGR, out=None) -> np.ndarray:
        """CLAHE of a plane, or of V of a 3-channel image with H and S kept (``adapt_exposure``).  ``tiles``:
        ``(tiles_x, tiles_y)``, OpenCV's ``tileGridSize``."""
        img, pitch, ch = self._image(image)
        h, w = img.shape[:2]
        out, o = _out(out, np.shape(image), ch, w)
        check(lib().lio_exposure_clahe(self._h, img.ctypes.data_as(C.c_void_p), w, h, ch, pitch, int(order), float(clip_limit),
                                       int(tiles[0]), int(tiles[1]), o.ctypes.data_as(C.c_void_p), o.strides[0]))
        return out

    def remap(self, image, lut_v=None, lut_all=None, order: int = BGR, out=None) -> np.ndarray:
        """``lut_v`` on V through the HSV round trip (on the plane with one channel), then ``lut_all`` on every channel
        (``cv2.LUT``); either may be None, not both"""
        img, pitch, ch = self._image(image)
        h, w = img.shape[:2]
        out, o = _out(out, np.shape(image), ch, w)
        _, pv = _table(lut_v, "lut_v")
        _, pa = _table(lut_all, "lut_all")
        check(lib().lio_exposure_remap(self._h, img.ctypes.data_as(C.c_void_p), w, h, ch, pitch, int(order), pv, pa,
                                       o.ctypes.data_as(C.c_void_p), o.strides[0]))
        return out

    def clahe_undistorted(self, undistorter, raw, clip_limit: float = 2.0, tiles=(8, 8), order: int = BGR, out=None) -> np.ndarray:
        """``undistorter(raw)`` followed by :meth:`clahe`, bit for bit, with one upload and one download: the rectified
        frame never leaves the device.  ``undistorter``: a :class:`lio_gpu.camera.Undistorter` after ``set_camera``."""
        if undistorter._shape is None:  # the library's state error, with its message
            z = np.zeros(1, np.uint8)
            check(lib().lio_exposure_clahe_undistorted(self._h, undistorter._h, z.ctypes.data_as(C.c_void_p), 0, int(order),
                                                       float(clip_limit), int(tiles[0]), int(tiles[1]),
                                                       z.ctypes.data_as(C.c_void_p), 0))
        sh, sw, dh, dw, ch = undistorter._shape
        img, pitch, c = _plane(raw, sw, sh)
        if c != ch:
            raise ValueError(f"raw: {c} channel(s), the undistorter was set up for {ch}")
        shape = (dh, dw) if np.ndim(raw) == 2 else (dh, dw, ch)
        out, o = _out(out, shape, ch, dw)
        check(lib().lio_exposure_clahe_undistorted(self._h, undistorter._h, img.ctypes.data_as(C.c_void_p), pitch, int(order),
                                                   float(clip_limit), int(tiles[0]), int(tiles[1]),
                                                   o.ctypes.data_as(C.c_void_p), o.strides[0]))
        return out

    def timing(self) -> dict:
        """device ms of the last run: upload (staging copy included), histogram, LUT, apply, download"""
        return self._timing("lio_exposure_get_timing", ("upload_ms", "hist_ms", "lut_ms", "apply_ms", "download_ms"))

    def recover(self, image, threshold: int = 200, dilate: int = 5, ksize: int = 15, sigma: float = 0.0, order: int = BGR,
                out=None) -> np.ndarray:
        """``solve_overexposure``'s ``recover_overexposure``: where the mask ``V > threshold``, dilated by ``dilate x
        dilate``, is set, V becomes its ``ksize x ksize`` Gaussian blur; H and S are kept (on a plane: the plane)"""
        img, pitch, ch = self._image(image)
        h, w = img.shape[:2]
        out, o = _out(out, np.shape(image), ch, w)
        p = RecoverParams(int(threshold), int(dilate), int(ksize), float(sigma))
        check(lib().lio_exposure_recover(self._h, img.ctypes.data_as(C.c_void_p), w, h, ch, pitch, int(order), C.byref(p),
                                         o.ctypes.data_as(C.c_void_p), o.strides[0]))
        return out

    def gaussian_blur(self, image, ksize: int, sigma: float = 0.0, out=None) -> np.ndarray:
        """``cv2.GaussianBlur(image, (ksize, ksize), sigma)`` of a uint8 image, every channel"""
        img, pitch, ch = self._image(image)
        h, w = img.shape[:2]
        out, o = _out(out, np.shape(image), ch, w)
        check(lib().lio_exposure_gaussian_blur(self._h, img.ctypes.data_as(C.c_void_p), w, h, ch, pitch, int(ksize), float(sigma),
                                               o.ctypes.data_as(C.c_void_p), o.strides[0]))
        return out

    def recover_undistorted(self, undistorter, raw, threshold: int = 200, dilate: int = 5, ksize: int = 15, sigma: float = 0.0,
                            order: int = BGR, out=None) -> np.ndarray:
        """``undistorter(raw)`` followed by :meth:`recover`, bit for bit, with one upload and one download"""
        p = RecoverParams(int(threshold), int(dilate), int(ksize), float(sigma))
        if undistorter._shape is None:  # the library's state error, with its message
            z = np.zeros(1, np.uint8)
            check(lib().lio_exposure_recover_undistorted(self._h, undistorter._h, z.ctypes.data_as(C.c_void_p), 0, int(order),
                                                         C.byref(p), z.ctypes.data_as(C.c_void_p), 0))
        sh, sw, dh, dw, ch = undistorter._shape
        img, pitch, c = _plane(raw, sw, sh)
        if c != ch:
            raise ValueError(f"raw: {c} channel(s), the undistorter was set up for {ch}")
        shape = (dh, dw) if np.ndim(raw) == 2 else (dh, dw, ch)
        out, o = _out(out, shape, ch, dw)
        check(lib().lio_exposure_recover_undistorted(self._h, undistorter._h, img.ctypes.data_as(C.c_void_p), pitch, int(order),
                                                     C.byref(p), o.ctypes.data_as(C.c_void_p), o.strides[0]))
        return out

    def stencil_timing(self) -> dict:
        """device ms of the last ``recover``, ``gaussian_blur`` or ``recover_undistorted``: upload (staging copy
        included; chained: the undistorter's upload and gather), the kernel, download"""
        return self._timing("lio_exposure_get_stencil_timing", ("upload_ms", "kernel_ms", "download_ms"))


# ------------------------------------------------------------------------------------------ the scripts' functions
def _with(handle, fn):
    if handle is not None:
        return fn(handle)
    ex = Exposure()
    try:
        return fn(ex)
    finally:
        ex.close()


def adapt_exposure(image, order: int = BGR, handle: Exposure | None = None) -> np.ndarray:
    """``CLAHE_region_adjusted.py:6-41``: CLAHE of V with clip 2.0 and 8 x 8 tiles (for many frames pass a ``handle``)"""
    return _with(handle, lambda ex: ex.clahe(image, 2.0, (8, 8), order))


def correct_overexposure(image, order: int = BGR, handle: Exposure | None = None, hist_v=None) -> np.ndarray:
    """``correct_exposure:32-49``: V equalised, then gamma 0.8: one histogram pass, one remap"""
    def run(ex):
        hv = ex.histograms(image, order)[0] if hist_v is None else hist_v
        return ex.remap(image, equalize_lut(hv), gamma_lut(0.8), order)
    return _with(handle, run)


def correct_underexposure(image, order: int = BGR, handle: Exposure | None = None, hist_v=None) -> np.ndarray:
    """``correct_exposure:51-70``: V stretched between its 5th and 95th percentile, then gamma 1.2"""
    def run(ex):
        hv = ex.histograms(image, order)[0] if hist_v is None else hist_v
        return ex.remap(image, stretch_lut(hv, 5.0, 95.0), gamma_lut(1.2), order)
    return _with(handle, run)


def correct_exposure(image, order: int = BGR, handle: Exposure | None = None):
    """``correct_exposure:86-99`` on one image: ``(corrected image, state)``; a well-exposed image comes back as a
    copy"""
    def run(ex):
        hv, hg = ex.histograms(image, order)
        state = detect_exposure(hg)
        if state == "overexposed":
            return correct_overexposure(image, order, ex, hv), state
        if state == "underexposed":
            return correct_underexposure(image, order, ex, hv), state
        return np.array(image, np.uint8, copy=True), state
    return _with(handle, run)
