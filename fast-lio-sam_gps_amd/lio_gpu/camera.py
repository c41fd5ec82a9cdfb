"""Camera projection and point cloud colorization from images: the camera step of the reference's offline leg
over the C-ABI.

* :class:`CameraModel` — pinhole intrinsics, OpenCV's 8-parameter rational distortion model
  (post_process/undistort_image.py:95-97) and the image size
* :func:`project_points` — the projection of post_process/colorize_pcd.py:31-47 (``lio_project_points``)
* :class:`Colorizer` — colours of a cloud from any number of frames, with an opt-in z-buffer (``lio_colorizer_*``)
* :func:`pack_rgb` — PCL's packed ``rgb`` field; :func:`colorize_pcd` — ``colorize_pcd.py`` on files
* :func:`world_to_camera` — the ``Rt`` of a keyframe from its pose and the LiDAR-to-camera extrinsic
* :func:`undistort_map`, :class:`Undistorter`, :func:`undistort_image` — the scripts' ``cv2.undistort(img, K, D, None,
  K)`` on every frame (post_process/undistort_image.py:21-27), as a 1/32-pixel map and an integer bilinear gather
  (``lio_undistort_map``, ``lio_undistorter_*``); :meth:`CameraModel.rectified` is the camera of its output
* :class:`PointOverlay`, :func:`draw_points` — the image with every projected point drawn as a filled disc, the
  output of the reference's projection tool (post_process/lidar_projection/src/lidar_projection.cpp:113-125;
  ``lio_overlay_*``); :func:`lidar_projection_overlay` — that tool from its k-means to the finished image

Images are numpy arrays (``height x width x 3`` uint8); decoding them is the caller's.  Every result follows the
contract of include/lio_gpu.h bit for bit: IEEE double operations in a written order, nothing fused.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field, replace

import numpy as np

from . import _capi
from ._capi import check, lib
from .filters import _Handle, _fp, _rows

_dp = C.POINTER(C.c_double)


@dataclass
class CameraModel:
    """``dist``: ``k1 k2 p1 p2 [k3 [k4 k5 k6]]`` in OpenCV's order (4, 5 or 8 numbers; none: a pinhole).
    ``r2_max`` bounds the squared normalised radius ``xn^2 + yn^2`` of a valid point (``inf``: no limit)."""
    fx: float
    fy: float
    cx: float
    cy: float
    width: int
    height: int
    dist: tuple = field(default_factory=tuple)
    r2_max: float = math.inf

    def __post_init__(self):
        d = np.asarray(self.dist, np.float64).ravel()
        if len(d) not in (0, 4, 5, 8):
            raise ValueError("CameraModel: dist takes 0, 4, 5 or 8 coefficients (k1 k2 p1 p2 k3 k4 k5 k6)")
        self.dist = tuple(float(v) for v in np.concatenate([d, np.zeros(8 - len(d))]))
        for name in ("fx", "fy", "cx", "cy"):
            setattr(self, name, float(getattr(self, name)))
            if not math.isfinite(getattr(self, name)):
                raise ValueError(f"CameraModel: {name} is not finite")
        if not all(math.isfinite(v) for v in self.dist):
            raise ValueError("CameraModel: a distortion coefficient is not finite")
        self.r2_max = float(self.r2_max)
        if not self.r2_max >= 0.0:
            raise ValueError("CameraModel: r2_max must be >= 0 (inf: no limit) and not NaN")
        if int(self.width) != self.width or int(self.height) != self.height or self.width < 1 or self.height < 1:
            raise ValueError("CameraModel: width and height must be integers of at least 1")
        self.width, self.height = int(self.width), int(self.height)
        if self.width * self.height >= 1 << 31:
            raise ValueError("CameraModel: width x height must be below 2^31")

    def _c(self) -> _capi.Camera:
        return _capi.Camera(self.fx, self.fy, self.cx, self.cy, (C.c_double * 8)(*self.dist), self.r2_max, self.width,
                            self.height)

    def rectified(self, **overrides) -> "CameraModel":
        """The pinhole camera of this camera's undistorted image: the same intrinsics and size with zero distortion
        (``overrides``: other ``fx fy cx cy width height``).  It is what :class:`Colorizer` takes for a rectified
        image, and the ``new_camera`` of :func:`undistort_image`."""
        return replace(self, **{"dist": (), **overrides})


def _pose(Rt) -> np.ndarray:
    """12 doubles, row-major R then t, from 12 numbers, a 3 x 4 ``[R | t]`` or a 4 x 4 homogeneous matrix"""
    a = np.asarray(Rt, np.float64)
    if a.shape == (4, 4):
        a = a[:3]
    if a.shape == (3, 4):
        a = np.concatenate([a[:, :3].ravel(), a[:, 3]])
    if a.shape != (12,):
        raise ValueError("Rt: 12 numbers (row-major R, then t), a 3 x 4 [R | t] or a 4 x 4 matrix is expected")
    return np.ascontiguousarray(a)


def world_to_camera(T_world_lidar, T_cam_lidar) -> np.ndarray:
    """The ``Rt`` (12 doubles) that maps MAP points to the camera frame of one keyframe: ``T_cam_lidar @
    inv(T_world_lidar)``, with the keyframe's pose ``T_world_lidar`` (LiDAR to world) and the rig's extrinsic
    ``T_cam_lidar`` (LiDAR to camera), both 4 x 4 rigid transforms.  A host helper in double: the inverse is the
    transpose form ``[R^T | -R^T t]``, not a general matrix inverse."""
    Tw, Tc = np.asarray(T_world_lidar, np.float64), np.asarray(T_cam_lidar, np.float64)
    if Tw.shape != (4, 4) or Tc.shape != (4, 4):
        raise ValueError("world_to_camera: two 4 x 4 transforms are expected")
    Rw, tw, Rc, tc = Tw[:3, :3], Tw[:3, 3], Tc[:3, :3], Tc[:3, 3]
    R = Rc @ Rw.T
    t = tc - R @ tw
    return np.concatenate([R.ravel(), t])


@dataclass
class Projection:
    """``uv``: n x 2 doubles; ``zc``: the depth along the optical axis; ``pix``: n x 2 int32 ``(px, py)``, -1 where
    the point is not valid; ``valid``: the script's mask"""
    uv: np.ndarray
    zc: np.ndarray
    pix: np.ndarray
    valid: np.ndarray


def project_points(pts, camera: CameraModel, Rt, handle: _Handle | None = None) -> Projection:
    """Point records (n x stride float32, x, y, z first) through ``Rt`` and the camera, by the contract of
    ``lio_project_points``: with no distortion ``u`` is bit for bit ``fx * (x / z) + cx`` of colorize_pcd.py:39."""
    h = handle or _Handle()
    p = _rows(pts)
    n = len(p)
    rt = _pose(Rt)
    uv, zc = np.zeros((n, 2), np.float64), np.zeros(n, np.float64)
    pix, valid = np.zeros((n, 2), np.int32), np.zeros(n, np.uint8)
    cam = camera._c()
    check(lib().lio_project_points(h._h, _fp(p), n, p.shape[1], C.byref(cam), rt.ctypes.data_as(_dp), uv.ctypes.data_as(_dp),
                                   zc.ctypes.data_as(_dp), pix.ctypes.data_as(C.POINTER(C.c_int32)),
                                   valid.ctypes.data_as(C.POINTER(C.c_uint8))))
    return Projection(uv, zc, pix, valid.astype(bool))


def _image(image, camera: CameraModel):
    """(array kept alive, row pitch in bytes) of a height x width x 3 uint8 image; a view whose pixels are packed
    (rows may be padded) is passed as it is, anything else is copied"""
    a = np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("image: a height x width x 3 uint8 array is expected")
    return _plane(a, camera.width, camera.height)[:2]


def _plane(image, width: int, height: int, what: str = "image"):
    """(array kept alive, row pitch in bytes, channels) of a height x width (x 1) or height x width x 3 uint8 image;
    a view whose pixels are packed (rows may be padded) is passed as it is, anything else is copied"""
    a = np.asarray(image)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    ch = 1 if a.ndim == 2 else 3
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise ValueError(f"{what}: a height x width, height x width x 1 or height x width x 3 uint8 array is expected")
    if a.shape[:2] != (height, width):
        raise ValueError(f"{what}: shape {a.shape[:2]} is not the camera's (height, width) = {(height, width)}")
    if a.strides[-1] != 1 or a.strides[1] != ch or a.strides[0] < ch * width:
        a = np.ascontiguousarray(a)
    return a, a.strides[0], ch


def _out(out, shape, ch, width):
    """(the array to return, the view handed to the library) of a result of ``shape``: ``out`` or a new array; its
    rows may be padded, its pixels not"""
    if out is None:
        out = np.empty(shape, np.uint8)
    if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.shape != shape or not out.flags.writeable:
        raise ValueError(f"out: a writeable uint8 array of shape {shape} is expected")
    o = out[:, :, 0] if (out.ndim == 3 and ch == 1) else out
    if o.strides[-1] != 1 or o.strides[1] != ch or o.strides[0] < ch * width:
        raise ValueError("out: the pixels of a row must be packed (rows may be padded)")
    return out, o


def undistort_map(src: CameraModel, dst: CameraModel | None = None, handle: _Handle | None = None):
    """The map of ``lio_undistort_map`` from the raw camera ``src`` to the rectified camera ``dst`` (none: ``src``'s
    intrinsics and size): ``(uv, sxy, axy)``, each ``height x width x 2`` of ``dst``: the unquantised source
    position (float64), its integer part (int32; ``INT32_MIN``: FAR) and its fraction in 1/32 pixel (uint8)."""
    h = handle or _Handle()
    d = dst or src
    uv = np.zeros((d.height, d.width, 2), np.float64)
    sxy = np.zeros((d.height, d.width, 2), np.int32)
    axy = np.zeros((d.height, d.width, 2), np.uint8)
    cs = src._c()
    cd = dst._c() if dst is not None else None
    check(lib().lio_undistort_map(h._h, C.byref(cs), C.byref(cd) if cd is not None else None, uv.ctypes.data_as(_dp),
                                  sxy.ctypes.data_as(C.POINTER(C.c_int32)), axy.ctypes.data_as(C.POINTER(C.c_uint8))))
    return uv, sxy, axy


class Undistorter(_Handle):
    """``cv2.undistort(img, K, D, None, K)`` per frame: ``set_camera`` once (the map stays on the device), then call
    the handle on every image.  Bilinear in 1/32 pixel with a constant ``border`` per tap, by the contract of
    include/lio_gpu.h (agreement with OpenCV is a reading of its source, not a test)."""

    _create, _destroy = "lio_undistorter_create", "lio_undistorter_destroy"

    def __init__(self, device: int = 0):
        self._shape = None  # (src height, src width, dst height, dst width, channels)
        super().__init__(device)

    def set_camera(self, camera: CameraModel, new_camera: CameraModel | None = None, channels: int = 3, border=(0, 0, 0)):
        """``camera``: the raw image's; ``new_camera``: the rectified image's pinhole (none: ``camera.rectified()``, the
        scripts' call); ``border``: one value, or one per channel"""
        b = np.zeros(3, np.uint8)
        b[:] = np.asarray(border, np.uint8).ravel()[:3] if np.ndim(border) else np.uint8(border)
        cs = camera._c()
        cd = new_camera._c() if new_camera is not None else None
        self._shape = None
        check(lib().lio_undistorter_set_camera(self._h, C.byref(cs), C.byref(cd) if cd is not None else None, int(channels),
                                               b.ctypes.data_as(C.POINTER(C.c_uint8))))
        d = new_camera or camera
        self._shape = (camera.height, camera.width, d.height, d.width, int(channels))

    def __call__(self, image, out=None) -> np.ndarray:
        """the rectified image, in the shape of the input (``h x w`` stays two-dimensional).  ``out``: a uint8 array
        of that shape to write into (its rows may be padded; the padding is not touched)."""
        if self._shape is None:  # the library's state error, with its message
            img = np.zeros(1, np.uint8)
            check(lib().lio_undistorter_run(self._h, img.ctypes.data_as(C.c_void_p), 0, img.ctypes.data_as(C.c_void_p), 0))
        sh, sw, dh, dw, ch = self._shape
        img, pitch, c = _plane(image, sw, sh)
        if c != ch:
            raise ValueError(f"image: {c} channel(s), the handle was set up for {ch}")
        shape = (dh, dw) if np.ndim(image) == 2 else (dh, dw, ch)
        out, o = _out(out, shape, ch, dw)
        check(lib().lio_undistorter_run(self._h, img.ctypes.data_as(C.c_void_p), pitch, o.ctypes.data_as(C.c_void_p),
                                        o.strides[0]))
        return out

    def timing(self) -> dict:
        """device ms of the last frame: upload (staging copy included), kernel, download"""
        return self._timing("lio_undistorter_get_timing", ("upload_ms", "kernel_ms", "download_ms"))


def undistort_image(image, camera: CameraModel, new_camera: CameraModel | None = None, border=(0, 0, 0)) -> np.ndarray:
    """one image through a fresh :class:`Undistorter` (for many frames of one camera keep the handle)"""
    a = np.asarray(image)
    ud = Undistorter()
    try:
        ud.set_camera(camera, new_camera, channels=3 if (a.ndim == 3 and a.shape[2] == 3) else 1, border=border)
        return ud(a)
    finally:
        ud.close()


class Colorizer(_Handle):
    """Colours of a cloud from camera frames: ``set_cloud`` once, ``add_frame`` per image; per point the nearest
    view wins (the smallest depth ``zc``; on a tie the earlier frame).  ``occlusion=False`` is the reference
    (colorize_pcd.py has none: points behind a wall take the wall's colour); ``occlusion=True`` builds a z-buffer
    per frame — every valid point splats its float depth over ``(2 splat_radius + 1)^2`` pixels — and colours a
    point only if ``zf <= D * (1 + depth_rel) + depth_abs`` at its own pixel.  ``bgr``: the image's channel order is
    OpenCV's (as in the script); the state is always R G B."""

    _create, _destroy = "lio_colorizer_create", "lio_colorizer_destroy"

    def __init__(self, occlusion: bool = False, splat_radius: int = 0, depth_rel: float = 0.0, depth_abs: float = 0.0,
                 bgr: bool = True, device: int = 0):
        self._n = 0
        p = _capi.ColorizeParams(int(bool(occlusion)), int(splat_radius), float(depth_rel), float(depth_abs), int(bool(bgr)))
        super().__init__(device, C.byref(p))

    def set_params(self, occlusion: bool = False, splat_radius: int = 0, depth_rel: float = 0.0, depth_abs: float = 0.0,
                   bgr: bool = True):
        p = _capi.ColorizeParams(int(bool(occlusion)), int(splat_radius), float(depth_rel), float(depth_abs), int(bool(bgr)))
        check(lib().lio_colorizer_set_params(self._h, C.byref(p)))

    def set_cloud(self, pts):
        p = _rows(pts)
        check(lib().lio_colorizer_set_cloud(self._h, _fp(p), len(p), p.shape[1]))
        self._n = len(p)

    def add_frame(self, camera: CameraModel, Rt, image) -> int:
        """one frame; returns the number of points whose colour it replaced"""
        img, pitch = _image(image, camera)
        rt = _pose(Rt)
        cam = camera._c()
        n = C.c_int64(0)
        check(lib().lio_colorizer_add_frame(self._h, C.byref(cam), rt.ctypes.data_as(_dp), img.ctypes.data_as(C.c_void_p), pitch,
                                            C.byref(n)))
        return int(n.value)

    def reset(self):
        check(lib().lio_colorizer_reset(self._h))

    def state(self):
        """(rgb n x 3 uint8, frame n int32, depth n float64) in one download"""
        n = max(self._n, 1)
        rgb, frame, depth = np.zeros((n, 3), np.uint8), np.zeros(n, np.int32), np.zeros(n, np.float64)
        check(lib().lio_colorizer_get(self._h, rgb.ctypes.data_as(C.POINTER(C.c_uint8)),
                                      frame.ctypes.data_as(C.POINTER(C.c_int32)), depth.ctypes.data_as(_dp)))
        return rgb[:self._n], frame[:self._n], depth[:self._n]

    @property
    def rgb(self) -> np.ndarray:
        return self.state()[0]

    @property
    def frame(self) -> np.ndarray:
        """per point the number of the frame that coloured it, -1: none (``frame >= 0`` is the script's mask)"""
        return self.state()[1]

    @property
    def depth(self) -> np.ndarray:
        """per point the depth ``zc`` in the frame that coloured it, ``inf``: none"""
        return self.state()[2]

    def colors_float(self) -> np.ndarray:
        """the script's n x 3 double colours: ``rgb / 255.0``, grey 0.5 where no frame saw the point"""
        rgb, frame, _ = self.state()
        return colors_float(rgb, frame)

    def timing(self) -> dict:
        """device ms of the last frame: upload (staging copy included), fill, splat, resolve (or the fused kernel)"""
        return self._timing("lio_colorizer_get_timing", ("upload_ms", "fill_ms", "splat_ms", "resolve_ms"))


def colors_float(rgb, frame) -> np.ndarray:
    """colorize_pcd.py:58-63: ``colors[:] = 0.5; colors[valid] = img[v, u, ::-1] / 255.0``"""
    rgb = np.asarray(rgb, np.uint8)
    out = np.full(rgb.shape, 0.5, np.float64)
    seen = np.asarray(frame) >= 0
    out[seen] = rgb[seen] / 255.0
    return out


def pack_rgb(rgb) -> np.ndarray:
    """n x 3 uint8 (r, g, b) -> PCL's packed ``rgb`` field: the uint32 ``r << 16 | g << 8 | b`` seen as float32"""
    c = np.asarray(rgb)
    if c.dtype != np.uint8 or c.ndim != 2 or c.shape[1] != 3:
        raise ValueError("pack_rgb: an n x 3 uint8 array is expected")
    c = c.astype(np.uint32)
    return ((c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]).astype(np.uint32).view(np.float32)


def _read_xyz(path: str) -> np.ndarray:
    """x y z of a PCD file"""
    from . import formats

    codec = formats.CloudCodec()
    try:
        return codec.read_pcd(path, want=("x", "y", "z"))
    finally:
        codec.close()


def _compute(xyz, image, camera, Rt, **params):
    """one cloud against one image: (rgb, frame)"""
    cz = Colorizer(**params)
    try:
        cz.set_cloud(xyz)
        cz.add_frame(camera, Rt, image)
        rgb, frame, _ = cz.state()
        return rgb, frame
    finally:
        cz.close()


def colorize_pcd(in_path: str, image, camera: CameraModel, Rt, out_path: str, default_rgb=(128, 128, 128), **params):
    """``colorize_pcd.py`` on files: x y z of ``in_path`` coloured from one image, written as a binary PCD with the
    fields ``x y z rgb`` (PCL's packed float).  Points outside the image take ``default_rgb`` (the script's grey).
    ``params``: :class:`Colorizer`'s.  Returns (points, coloured points)."""
    from . import formats

    xyz = _read_xyz(in_path)
    rgb, frame = _compute(xyz, image, camera, Rt, **params)
    rgb = np.where((np.asarray(frame) >= 0)[:, None], rgb, np.asarray(default_rgb, np.uint8)[None, :]).astype(np.uint8)
    rec = np.empty((len(xyz), 4), np.float32)
    rec[:, :3] = xyz
    rec[:, 3] = pack_rgb(rgb)
    formats.write_pcd_binary(out_path, rec, names=("x", "y", "z", "rgb"))
    return len(xyz), int(np.count_nonzero(np.asarray(frame) >= 0))


ORDERS = {"draw": _capi.LIO_OVERLAY_DRAW_ORDER, "nearest": _capi.LIO_OVERLAY_NEAREST}


def _overlay_params(radius, order) -> _capi.OverlayParams:
    if int(radius) != radius or not 0 <= radius <= 15:
        raise ValueError("radius: an integer in 0..15 is expected")
    if order not in ORDERS:
        raise ValueError("order: 'draw' (later points over earlier ones) or 'nearest' (the nearest point wins) is expected")
    return _capi.OverlayParams(int(radius), ORDERS[order])


def _per_point(a, n: int, dtype, cols: int, what: str) -> np.ndarray:
    """``a`` as it goes to the library: exactly ``dtype`` (nothing is cast: a float label is a mistake), one value per
    point (``cols`` 0) or ``cols`` of them"""
    a = np.asarray(a)
    if a.dtype != dtype:
        raise ValueError(f"{what}: dtype {np.dtype(dtype).name} is expected, not {a.dtype.name}")
    if a.shape != ((n, cols) if cols else (n,)):
        raise ValueError(f"{what}: shape {(n, cols) if cols else (n,)} is expected (one per point), not {a.shape}")
    return np.ascontiguousarray(a)


def _palette(palette) -> np.ndarray:
    p = np.asarray(palette)
    if p.dtype != np.uint8 or p.ndim != 2 or p.shape[1] != 3 or len(p) < 1:
        raise ValueError("palette: a P x 3 uint8 array with P >= 1 is expected")
    return np.ascontiguousarray(p)


def _colour_sources(n: int, labels, colors, palette):
    """the checked (labels, colors, palette) of a draw, each None where not given.  Exactly one source applies:
    ``colors``; or ``labels`` through ``palette``; or ``palette``'s row 0 (none: the handle's, green at first)"""
    if colors is not None and (labels is not None or palette is not None):
        raise ValueError("more than one colour source: give colors, or labels (with a palette), or a palette alone")
    return (_per_point(labels, n, np.int32, 0, "labels") if labels is not None else None,
            _per_point(colors, n, np.uint8, 3, "colors") if colors is not None else None,
            _palette(palette) if palette is not None else None)


class PointOverlay(_Handle):
    """The projection tool's output: every valid point of a cloud drawn on the image as a filled disc of ``radius``
    pixels (OpenCV's filled midpoint circle around the centre rounded to even, clipped to the image).  ``order="draw"``:
    later points over earlier ones, the tool's sequential loop; ``order="nearest"``: the nearest point wins a pixel.
    The colour of a point is three bytes in the image's own channel order: ``set_colors`` (one per point), or
    ``set_labels`` through ``set_palette`` (``palette[label % P]``; a point with a negative label is not drawn), or
    the palette's first row for every point (green at first, as the tool ships).  The cloud and the colour sources
    stay on the device between frames.  Every result follows the contract of include/lio_gpu.h bit for bit
    (agreement of the disc with OpenCV is a reading of its source, not a test)."""

    _create, _destroy = "lio_overlay_create", "lio_overlay_destroy"

    def __init__(self, radius: int = 3, order: str = "draw", device: int = 0):
        self._n = None
        p = _overlay_params(radius, order)
        super().__init__(device, C.byref(p))
        self.n_drawn = 0

    def set_cloud(self, pts):
        """uploads the cloud; the labels and per-point colours of the cloud before it are dropped"""
        p = _rows(pts)
        self._n = None
        check(lib().lio_overlay_set_cloud(self._h, _fp(p), len(p), p.shape[1]))
        self._n = len(p)

    def _need_cloud(self):
        if self._n is None:  # the library's state error, with its message
            check(lib().lio_overlay_set_labels(self._h, np.zeros(1, np.int32).ctypes.data_as(C.POINTER(C.c_int32)), 1))

    def set_labels(self, labels):
        """one int32 per point (none: dropped); negative: that point is not drawn"""
        self._need_cloud()
        a = _per_point(labels, self._n, np.int32, 0, "labels") if labels is not None else None
        check(lib().lio_overlay_set_labels(self._h, a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None,
                                           self._n if a is not None else 0))

    def set_colors(self, colors):
        """three uint8 per point in the image's channel order (none: dropped)"""
        self._need_cloud()
        a = _per_point(colors, self._n, np.uint8, 3, "colors") if colors is not None else None
        check(lib().lio_overlay_set_colors(self._h, a.ctypes.data_as(C.POINTER(C.c_uint8)) if a is not None else None,
                                           self._n if a is not None else 0))

    def set_palette(self, palette):
        p = _palette(palette)
        check(lib().lio_overlay_set_palette(self._h, p.ctypes.data_as(C.POINTER(C.c_uint8)), len(p)))

    def _draw(self, entry, head, camera, Rt, src, pitch, out, owner):
        rt = _pose(Rt)
        cam = camera._c()
        out, o = _out(out, (camera.height, camera.width, 3), 3, camera.width)
        own = np.empty((camera.height, camera.width), np.int32) if owner else None
        n = C.c_int64(0)
        check(entry(self._h, *head, C.byref(cam), rt.ctypes.data_as(_dp), src.ctypes.data_as(C.c_void_p), pitch,
                    o.ctypes.data_as(C.c_void_p), o.strides[0], own.ctypes.data_as(C.POINTER(C.c_int32)) if owner else None,
                    C.byref(n)))
        self.n_drawn = int(n.value)
        return (out, own) if owner else out

    def draw(self, camera: CameraModel, Rt, image, out=None, owner: bool = False):
        """the drawn image (``out``: a uint8 array of the image's shape to write into; its rows may be padded, the
        padding is not touched; it may be ``image``); with ``owner`` also the ``height x width`` int32 image of each
        pixel's owning point, -1 where none.  ``n_drawn``: the points that were valid and not skipped by their label."""
        img, pitch = _image(image, camera)
        return self._draw(lib().lio_overlay_draw, (), camera, Rt, img, pitch, out, owner)

    def draw_undistorted(self, undistorter: Undistorter, camera: CameraModel, Rt, raw_image, out=None, owner: bool = False):
        """``undistorter(raw_image)`` then :meth:`draw`, bit for bit, with one upload and one download.  ``camera``: the
        rectified image's (:meth:`CameraModel.rectified`)."""
        if undistorter._shape is None:  # the library's state error, with its message
            return self._draw(lib().lio_overlay_draw_undistorted, (undistorter._h,), camera, Rt, np.zeros(1, np.uint8), 0, out,
                              owner)
        sh, sw = undistorter._shape[:2]
        img, pitch, ch = _plane(raw_image, sw, sh, "raw_image")
        if ch != 3:
            raise ValueError("raw_image: a height x width x 3 uint8 array is expected")
        return self._draw(lib().lio_overlay_draw_undistorted, (undistorter._h,), camera, Rt, img, pitch, out, owner)

    def timing(self) -> dict:
        """device ms of the last draw: upload (staging copy included), fill, stamp, compose, download"""
        return self._timing("lio_overlay_get_timing", ("upload_ms", "fill_ms", "stamp_ms", "compose_ms", "download_ms"))


def draw_points(image, pts, camera: CameraModel, Rt, radius: int = 3, order: str = "draw", labels=None, colors=None,
                palette=None, owner: bool = False):
    """one image through a fresh :class:`PointOverlay` (for many frames of one cloud keep the handle): ``pts`` drawn
    on ``image`` as filled discs.  One colour source: ``colors`` (n x 3 uint8, e.g. ``filters.cluster_palette(labels)``),
    or ``labels`` (n int32) with a ``palette`` (P x 3 uint8; none: green), or ``palette``'s first row for every point
    (none: green, as the tool ships).  Returns the drawn image, with ``owner`` also the owner image.  Every argument is
    checked before the device is touched."""
    p = _rows(pts)
    _overlay_params(radius, order)
    labels, colors, palette = _colour_sources(len(p), labels, colors, palette)
    _image(image, camera)
    ov = PointOverlay(radius, order)
    try:
        ov.set_cloud(p)
        if palette is not None:
            ov.set_palette(palette)
        if labels is not None:
            ov.set_labels(labels)
        if colors is not None:
            ov.set_colors(colors)
        return ov.draw(camera, Rt, image, owner=owner)
    finally:
        ov.close()


def lidar_projection_overlay(pts, image, camera: CameraModel, Rt, K: int = 5, seed: int = 0, by_cluster: bool = False,
                             radius: int = 3):
    """The ``main`` of post_process/lidar_projection/src/lidar_projection.cpp from its k-means to the finished image
    (:82-125): :class:`lio_gpu.filters.KMeans` with the tool's criteria, :func:`lio_gpu.filters.cluster_palette`, then
    the overlay in draw order.  ``by_cluster=False`` is the tool as shipped: its palette call is commented out and
    every point is drawn green (0, 255, 0); ``True`` draws each point in its cluster's colour (B G R, for OpenCV's
    image).  Returns ``(drawn image, labels)``."""
    from . import filters

    p = _rows(pts)
    km = filters.KMeans(n_clusters=K, seed=seed)
    try:
        labels = km.fit(p)
    finally:
        km.close()
    if by_cluster:
        return draw_points(image, p, camera, Rt, radius=radius, colors=filters.cluster_palette(labels)), labels
    return draw_points(image, p, camera, Rt, radius=radius), labels
