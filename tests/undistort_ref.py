"""The contract of lio_undistort_map / lio_undistorter (include/lio_gpu.h) restated in numpy: elementwise IEEE
double operations in the written order, np.rint (ties to even), integer shifts and an integer bilinear sum.  Also
the scenes of the undistortion tests.  CPU only; tests/test_undistort_ref.py holds it against itself.  The cameras
are colorize_ref's (Cam, small_cam, K8, DIST8, DIST5)."""
import numpy as np

from colorize_ref import DIST5, DIST8, K8, Cam, small_cam  # noqa: F401  (K8: the timing script's and the large scene's)

f64 = np.float64
INT32_MIN = np.int32(-2 ** 31)
CLASSES = ("all_in", "left", "right", "top", "bottom", "all_out", "far")


class Map:
    """u, v (float64), sx, sy (int32, INT32_MIN where FAR), ax, ay (uint8), far (bool), each dst.height x dst.width"""

    def __init__(self, u, v, sx, sy, ax, ay, far):
        self.u, self.v, self.sx, self.sy, self.ax, self.ay, self.far = u, v, sx, sy, ax, ay, far

    @property
    def uv(self):
        return np.stack([self.u, self.v], -1)

    @property
    def sxy(self):
        return np.stack([self.sx, self.sy], -1)

    @property
    def axy(self):
        return np.stack([self.ax, self.ay], -1)


def undistort_map(src, dst=None):
    """one numpy operation per operation of the contract"""
    dst = src if dst is None else dst
    assert not any(dst.dist) or dst is src
    k1, k2, p1, p2, k3, k4, k5, k6 = (f64(v) for v in src.dist)
    fx, fy, cx, cy = f64(src.fx), f64(src.fy), f64(src.cx), f64(src.cy)
    j = np.arange(dst.width, dtype=f64)[None, :]
    i = np.arange(dst.height, dtype=f64)[:, None]
    with np.errstate(all="ignore"):
        xn = np.broadcast_to((j - f64(dst.cx)) / f64(dst.fx), (dst.height, dst.width))
        yn = np.broadcast_to((i - f64(dst.cy)) / f64(dst.fy), (dst.height, dst.width))
        r2 = xn * xn + yn * yn
        num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2
        rad = num / den
        a1, a2, a3 = (2.0 * xn) * yn, r2 + (2.0 * xn) * xn, r2 + (2.0 * yn) * yn
        xd = xn * rad + (p1 * a1 + p2 * a2)
        yd = yn * rad + (p1 * a3 + p2 * a1)
        u, v = fx * xd + cx, fy * yd + cy
        qu, qv = np.rint(u * 32.0), np.rint(v * 32.0)
        near = (np.abs(qu) < 2.0 ** 30) & (np.abs(qv) < 2.0 ** 30)  # false on NaN
        iu = np.where(near, qu, 0.0).astype(np.int64)
        iv = np.where(near, qv, 0.0).astype(np.int64)
    sx = np.where(near, iu >> 5, INT32_MIN).astype(np.int32)
    sy = np.where(near, iv >> 5, INT32_MIN).astype(np.int32)
    ax = np.where(near, iu & 31, 0).astype(np.uint8)
    ay = np.where(near, iv & 31, 0).astype(np.uint8)
    return Map(u, v, sx, sy, ax, ay, ~near)


def taps_inside(m, src):
    """the four taps' inside flags, in the order (sx, sy) (sx + 1, sy) (sx, sy + 1) (sx + 1, sy + 1)"""
    sx, sy = m.sx.astype(np.int64), m.sy.astype(np.int64)
    out = []
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = sx + dx, sy + dy
            out.append(~m.far & (x >= 0) & (x < src.width) & (y >= 0) & (y < src.height))
    return out


def remap(img, m, src, border=(0, 0, 0), scale=1, half=512, shift=10):
    """img: src.height x src.width [x channels] uint8 (any strides) -> the rectified image in the map's size.
    (scale, half, shift) = (32, 2 ** 14, 15) is OpenCV's table arithmetic, (1, 512, 10) the contract's line."""
    a = np.asarray(img)
    planar = a.ndim == 2
    a = a[:, :, None] if planar else a
    assert a.dtype == np.uint8 and a.shape[:2] == (src.height, src.width)
    ch = a.shape[2]
    b = np.broadcast_to(np.asarray(border, np.int64).ravel(), (3,)) if np.ndim(border) else np.full(3, border, np.int64)
    ax, ay = m.ax.astype(np.int64), m.ay.astype(np.int64)
    w = [(32 - ax) * (32 - ay), ax * (32 - ay), (32 - ax) * ay, ax * ay]
    sx, sy = m.sx.astype(np.int64), m.sy.astype(np.int64)
    inside = taps_inside(m, src)
    acc = np.zeros(m.sx.shape + (ch,), np.int64)
    for k, (dx, dy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        x = np.clip(sx + dx, 0, src.width - 1)
        y = np.clip(sy + dy, 0, src.height - 1)
        p = np.where(inside[k][:, :, None], a[y, x].astype(np.int64), b[None, None, :ch])
        acc += (scale * w[k])[:, :, None] * p
    out = ((acc + half) >> shift).astype(np.uint8)
    return out[:, :, 0] if planar else out


def undistort(img, src, dst=None, border=(0, 0, 0)):
    return remap(img, undistort_map(src, dst), src, border)


def classes(m, src):
    """pixel counts: every tap inside; some inside with the left / right / top / bottom taps outside (a corner pixel
    counts on two sides); none inside but not FAR; FAR"""
    t00, t10, t01, t11 = taps_inside(m, src)
    n_in = t00.astype(int) + t10 + t01 + t11
    part = (n_in > 0) & (n_in < 4)
    sx, sy = m.sx.astype(np.int64), m.sy.astype(np.int64)
    return dict(all_in=int((n_in == 4).sum()), left=int((part & (sx == -1)).sum()),
                right=int((part & (sx == src.width - 1)).sum()), top=int((part & (sy == -1)).sum()),
                bottom=int((part & (sy == src.height - 1)).sum()), all_out=int(((n_in == 0) & ~m.far).sum()),
                far=int(m.far.sum()), partial=int(part.sum()))


# ------------------------------------------------------------------------------------------------------ scenes
def pinhole(fx, fy, cx, cy, width, height):
    return Cam(fx=fx, fy=fy, cx=cx, cy=cy, width=width, height=height)


class Scene:
    """name, the raw camera, the rectified camera (None: the raw one's pinhole) and the classes it covers"""

    def __init__(self, name, src, dst, covers):
        self.name, self.src, self.dst, self.covers = name, src, dst, covers

    @property
    def out_cam(self):
        return self.dst if self.dst is not None else self.src


def scenes():
    """the 64 x 48 source of small_cam() in every scene"""
    return [
        Scene("dist8", small_cam(dist=DIST8), None, ("all_in",)),
        Scene("dist5", small_cam(dist=DIST5), None, ("all_in",)),
        # a wider field than the source: partial pixels on every side and pixels that see nothing
        Scene("wide", small_cam(dist=DIST8), pinhole(16.0, 12.0, 30.5, 25.25, 64, 48),
              ("all_in", "left", "right", "top", "bottom", "all_out")),
        # a width that is no multiple of 4, a partial last workgroup, partial pixels on both sides
        Scene("67x5", small_cam(dist=DIST8), pinhole(20.0, 3.0, 33.0, 2.0, 67, 5), ("all_in", "left", "right")),
        Scene("1x1", small_cam(dist=DIST8), pinhole(32.0, 24.0, 0.5, 0.5, 1, 1), ("all_in",)),
        # at j = 0, i = 24: xn = -1, yn = 0, r2 = 1, den = 1 + k4 = 0: u = -inf, v = NaN
        Scene("pole", small_cam(dist=(0, 0, 0, 0, 0, -1.0, 0, 0)), None, ("all_in", "far")),
    ]


def image(cam, channels=3, pitch=None, seed=0):
    """a random uint8 image as a view into rows of `pitch` bytes (None: packed); the padding holds other random bytes"""
    pitch = channels * cam.width if pitch is None else pitch
    buf = np.random.default_rng(seed).integers(0, 256, (cam.height, pitch), dtype=np.uint8)
    if channels == 1:
        return np.lib.stride_tricks.as_strided(buf, (cam.height, cam.width), (pitch, 1))
    return np.lib.stride_tricks.as_strided(buf, (cam.height, cam.width, channels), (pitch, channels, 1))


def large_scene():
    """1031 x 517 with the rig's 8-parameter calibration scaled to it: many workgroups, rows that start at any
    alignment"""
    s = 1031.0 / 4096.0
    return Scene("1031x517", Cam(fx=K8[0] * s, fy=K8[1] * s, cx=K8[2] * s, cy=K8[3] * s, width=1031, height=517, dist=DIST8),
                 None, ("all_in",))
