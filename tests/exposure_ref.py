"""The contract of lio_exposure_* (include/lio_gpu.h) restated in numpy: integer operations in int64, float operations
elementwise in float32 in the written order (numpy fuses nothing), np.rint (ties to even), a few loops over tiles.
No OpenCV.  CPU only; tests/test_exposure_ref.py holds it against itself.  Also the images of the exposure tests."""
import numpy as np

f32 = np.float32
HS = f32(float.fromhex("0x1.111112p-5"))  # the float nearest 1/30
K = f32(float.fromhex("0x1.010102p-8"))   # the float nearest 1/255
SECTORS = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])


def div_tables():
    """sdiv, hdiv: computed in double, rint ties to even"""
    i = np.arange(1, 256, dtype=np.float64)
    sdiv, hdiv = np.zeros(256, np.int64), np.zeros(256, np.int64)
    sdiv[1:] = np.rint(float(255 << 12) / i).astype(np.int64)
    hdiv[1:] = np.rint(float(180 << 12) / (6.0 * i)).astype(np.int64)
    return sdiv, hdiv


SDIV, HDIV = div_tables()


def sat_rint(x):
    """sat(rint(x)) of a float32 array"""
    assert x.dtype == np.float32
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def split(img, order=0):
    """b, g, r (int64) of a ... x 3 uint8 array whose bytes are B G R (order 0) or R G B (order 1)"""
    a = np.asarray(img).astype(np.int64)
    return (a[..., 2], a[..., 1], a[..., 0]) if order else (a[..., 0], a[..., 1], a[..., 2])


def merge(b, g, r, order=0):
    return np.stack((r, g, b) if order else (b, g, r), -1).astype(np.uint8)


def bgr2hsv(b, g, r):
    v = np.maximum(b, np.maximum(g, r))
    vmin = np.minimum(b, np.minimum(g, r))
    d = v - vmin
    s = (d * SDIV[v] + 2048) >> 12
    h0 = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (h0 * HDIV[d] + 2048) >> 12  # numpy's >> on int64 is arithmetic
    h = np.where(h < 0, h + 180, h)
    return h, s, v


def hsv2bgr(h, s, v):
    hf, sf, vf = h.astype(f32) * HS, s.astype(f32) * K, v.astype(f32) * K
    sec = np.floor(hf).astype(np.int64)
    f = hf - sec.astype(f32)
    wrap = sec >= 6
    sec = np.where(wrap, 0, sec)
    f = np.where(wrap, f32(0), f)
    one = f32(1)
    t = np.stack([vf, vf * (one - sf), vf * (one - sf * f), vf * (one - sf * (one - f))], -1)
    assert t.dtype == np.float32
    out = []
    for c in range(3):
        x = np.take_along_axis(t, SECTORS[sec, c][..., None], -1)[..., 0]
        x = np.where(s == 0, vf, x)
        out.append(sat_rint(x * f32(255.0)).astype(np.int64))
    return out  # b, g, r


def gray(b, g, r):
    return (3735 * b + 19235 * g + 9798 * r + 16384) >> 15


def value_plane(img, order=0):
    """V of an image: the plane itself with one channel"""
    a = np.asarray(img)
    return a.astype(np.int64) if a.ndim == 2 else bgr2hsv(*split(a, order))[2]


def gray_plane(img, order=0):
    a = np.asarray(img)
    return a.astype(np.int64) if a.ndim == 2 else gray(*split(a, order))


# ------------------------------------------------------------------------------------------------------- CLAHE
class Tiling:
    def __init__(self, width, height, clip_limit, tiles_x, tiles_y):
        self.tiles_x, self.tiles_y = tiles_x, tiles_y
        self.pad_w = self.pad_h = 0
        if width % tiles_x != 0 or height % tiles_y != 0:
            self.pad_w, self.pad_h = tiles_x - width % tiles_x, tiles_y - height % tiles_y
            if self.pad_w > width - 1 or self.pad_h > height - 1:
                raise ValueError("padding larger than the dimension - 1")
        self.ext_w, self.ext_h = width + self.pad_w, height + self.pad_h
        self.tw, self.th = self.ext_w // tiles_x, self.ext_h // tiles_y
        self.area = self.tw * self.th
        if clip_limit <= 0:
            self.clip = 0
        else:
            c = float(clip_limit) * float(self.area) / 256.0
            if not c < 2.0 ** 31:
                raise ValueError("clip out of range")
            self.clip = max(int(c), 1)


def redistribute_closed(hist, clip):
    """the contract's closed form on one 256-bin histogram (int64)"""
    excess = int(np.maximum(hist - clip, 0).sum())
    h = np.minimum(hist, clip)
    batch = excess // 256
    res = excess - 256 * batch
    h = h + batch
    if res > 0:
        step = max(256 // res, 1)
        k = np.arange(256)
        h = h + ((k % step == 0) & (k // step < res))
    return h


def redistribute_loop(hist, clip):
    """OpenCV's loop (clahe.cpp), for the test of the closed form"""
    h = [int(x) for x in hist]
    clipped = 0
    for i in range(256):
        if h[i] > clip:
            clipped += h[i] - clip
            h[i] = clip
    batch = clipped // 256
    residual = clipped - batch * 256
    for i in range(256):
        h[i] += batch
    if residual != 0:
        step = max(256 // residual, 1)
        i = 0
        while i < 256 and residual > 0:
            h[i] += 1
            i += step
            residual -= 1
    return np.array(h, np.int64)


def clahe_luts(plane, t):
    """uint8 [tiles_y][tiles_x][256] of an int plane"""
    ext = np.pad(plane, ((0, t.pad_h), (0, t.pad_w)), mode="reflect") if (t.pad_w or t.pad_h) else plane
    assert ext.shape == (t.ext_h, t.ext_w)
    scale = f32(255.0) / f32(t.area)
    luts = np.zeros((t.tiles_y, t.tiles_x, 256), np.uint8)
    for ty in range(t.tiles_y):
        for tx in range(t.tiles_x):
            tile = ext[ty * t.th:(ty + 1) * t.th, tx * t.tw:(tx + 1) * t.tw]
            hist = np.bincount(tile.ravel(), minlength=256).astype(np.int64)
            if t.clip > 0:
                hist = redistribute_closed(hist, t.clip)
            luts[ty, tx] = sat_rint(np.cumsum(hist).astype(f32) * scale)
    return luts


def _axis(n, inv, tiles):
    f = np.arange(n).astype(f32) * inv - f32(0.5)
    t1 = np.floor(f).astype(np.int64)
    a = f - t1.astype(f32)
    a1 = f32(1) - a
    t2 = np.minimum(t1 + 1, tiles - 1)
    t1 = np.maximum(t1, 0)
    assert a.dtype == np.float32 and a1.dtype == np.float32 and t1.max() <= tiles - 1
    return t1, t2, a, a1


def clahe_plane(plane, clip_limit, tiles_x, tiles_y):
    """int plane (H x W, values 0..255) -> int64 plane"""
    H, W = plane.shape
    t = Tiling(W, H, clip_limit, tiles_x, tiles_y)
    L = clahe_luts(plane, t).astype(f32)
    tx1, tx2, xa, xa1 = _axis(W, f32(1.0) / f32(t.tw), tiles_x)
    ty1, ty2, ya, ya1 = _axis(H, f32(1.0) / f32(t.th), tiles_y)
    p = plane
    Y1, Y2, X1, X2 = ty1[:, None], ty2[:, None], tx1[None, :], tx2[None, :]
    top = L[Y1, X1, p] * xa1[None, :] + L[Y1, X2, p] * xa[None, :]
    bot = L[Y2, X1, p] * xa1[None, :] + L[Y2, X2, p] * xa[None, :]
    res = top * ya1[:, None] + bot * ya[:, None]
    return sat_rint(res).astype(np.int64)


def clahe(img, clip_limit=2.0, tiles=(8, 8), order=0):
    """lio_exposure_clahe"""
    a = np.asarray(img)
    if a.ndim == 2:
        return clahe_plane(a.astype(np.int64), clip_limit, *tiles).astype(np.uint8)
    h, s, v = bgr2hsv(*split(a, order))
    return merge(*hsv2bgr(h, s, clahe_plane(v, clip_limit, *tiles)), order)


def remap(img, lut_v=None, lut_all=None, order=0):
    """lio_exposure_remap"""
    a = np.asarray(img)
    if a.ndim == 2:
        out = a
        if lut_v is not None:
            out = np.asarray(lut_v)[out]
        if lut_all is not None:
            out = np.asarray(lut_all)[out]
        return out.astype(np.uint8)
    out = a
    if lut_v is not None:
        h, s, v = bgr2hsv(*split(a, order))
        out = merge(*hsv2bgr(h, s, np.asarray(lut_v).astype(np.int64)[v]), order)
    if lut_all is not None:
        out = np.asarray(lut_all)[out]
    return out.astype(np.uint8)


def histograms(img, order=0):
    return (np.bincount(value_plane(img, order).ravel(), minlength=256).astype(np.int64),
            np.bincount(gray_plane(img, order).ravel(), minlength=256).astype(np.int64))


# ------------------------------------------------------------------------------------------------------ images
def strided(buf, width, height, channels):
    pitch = buf.shape[1]
    if channels == 1:
        return np.lib.stride_tricks.as_strided(buf, (height, width), (pitch, 1))
    return np.lib.stride_tricks.as_strided(buf, (height, width, channels), (pitch, channels, 1))


def random_image(width, height, channels=3, pitch=None, seed=0):
    """a random uint8 image as a view into rows of `pitch` bytes (None: packed); the padding holds other random bytes"""
    pitch = channels * width if pitch is None else pitch
    return strided(np.random.default_rng(seed).integers(0, 256, (height, pitch), dtype=np.uint8), width, height, channels)


def images(width, height, channels):
    """name -> image: random, a ramp, all 0, all 255, a sky (upper half 255), few distinct colours"""
    shape = (height, width) if channels == 1 else (height, width, channels)
    rng = np.random.default_rng(width * 1000 + height + channels)
    ramp = ((np.arange(width)[None, :] * 255) // max(width - 1, 1) + np.zeros((height, 1), np.int64)).astype(np.uint8)
    if channels == 3:
        ramp = np.stack([ramp, ramp[::-1], (ramp // 2 + 17).astype(np.uint8)], -1)
    sky = rng.integers(0, 120, shape, dtype=np.uint8)
    sky[:height // 2] = 255
    palette = rng.integers(0, 256, (4,) if channels == 1 else (4, channels), dtype=np.uint8)
    few = palette[rng.integers(0, 4, (height, width))]
    return {"random": rng.integers(0, 256, shape, dtype=np.uint8), "ramp": np.ascontiguousarray(ramp),
            "zeros": np.zeros(shape, np.uint8), "full": np.full(shape, 255, np.uint8), "sky": sky, "few": few}


def vd_image():
    """256 x 768 x 3: every (v, d) pair of the HSV division tables with the maximum on each channel in turn (columns
    0..255 red, 256..511 green, 512..767 blue); row v, column d (d > v wraps to v - d % (v + 1))"""
    v = np.arange(256)[:, None] + np.zeros((1, 256), np.int64)
    d = np.arange(256)[None, :] % (v + 1)
    lo, mid = v - d, v - d // 2
    blocks = [np.stack(c, -1) for c in ((lo, mid, v), (mid, v, lo), (v, lo, mid))]  # B G R: max on r, g, b
    return np.concatenate(blocks, 1).astype(np.uint8)
