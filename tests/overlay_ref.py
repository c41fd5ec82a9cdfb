"""The contract of lio_overlay (include/lio_gpu.h) restated in numpy: the projection of tests/colorize_ref.py, the
centre rounded to even, one half-width per row offset from OpenCV's filled midpoint circle, one uint64 key per pixel
with np.minimum.at.  Also the scene that tests/cpp/overlay.cpp builds with the same generator.  CPU only;
tests/test_overlay_ref.py holds it against a sequential loop that overwrites pixels in draw order."""
import numpy as np

import colorize_ref as CR

DRAW_ORDER, NEAREST = 0, 1
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
GREEN = np.array([[0, 255, 0]], np.uint8)  # the handle's first palette: the tool as shipped draws every point green


def half_widths(r):
    """hw[d]: the half-width of the rows cy - d and cy + d of the filled circle of radius r"""
    hw = [0] * (r + 1)
    err, dx, dy, plus, minus = 0, r, 0, 1, 2 * r - 1
    while dx >= dy:
        hw[dy] = max(hw[dy], dx)
        hw[dx] = max(hw[dx], dy)
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2
    return hw


def disc_offsets(r):
    hw = half_widths(r)
    return [(ox, oy) for oy in range(-r, r + 1) for ox in range(-hw[abs(oy)], hw[abs(oy)] + 1)]


def drawn_points(pr, labels=None, colors=None):
    """the mask of n_drawn: valid, and not skipped by a negative label (labels apply only without per-point colours)"""
    drawn = pr.valid.copy()
    if labels is not None and colors is None:
        drawn &= np.asarray(labels) >= 0
    return drawn


def centres(pr):
    """(cx, cy) int64 of every point, meaningful where valid: rint in double, ties to even, after the validity test"""
    with np.errstate(all="ignore"):
        u = np.where(pr.valid, pr.u, 0.0)
        v = np.where(pr.valid, pr.v, 0.0)
    return np.rint(u).astype(np.int64), np.rint(v).astype(np.int64)


def keys_of(pr, order):
    """key_i = (hi << 32) | (0xFFFFFFFF - i); hi = 0, or the bits of (float)zc"""
    n = len(pr.zc)
    lo = np.uint64(0xFFFFFFFF) - np.arange(n, dtype=np.uint64)
    if order == DRAW_ORDER:
        return lo
    with np.errstate(all="ignore"):
        hi = np.where(pr.valid, pr.zc, 1.0).astype(np.float32).view(np.uint32).astype(np.uint64)
    return (hi << np.uint64(32)) | lo


def colour_of(idx, labels=None, colors=None, palette=None):
    """the three bytes of the points idx"""
    if colors is not None:
        return np.asarray(colors, np.uint8)[idx]
    pal = GREEN if palette is None else np.asarray(palette, np.uint8)
    if labels is not None:
        return pal[np.asarray(labels, np.int64)[idx] % len(pal)]
    return np.broadcast_to(pal[0], (len(idx), 3))


def draw(pts, cam, Rt, image, radius=3, order=DRAW_ORDER, labels=None, colors=None, palette=None):
    """(drawn image as a new packed array, owner image int32, n_drawn)"""
    pr = CR.project(pts, cam, Rt)
    W, H = cam.width, cam.height
    i = np.flatnonzero(drawn_points(pr, labels, colors))
    cx, cy = centres(pr)
    key = keys_of(pr, order)
    K = np.full(H * W, EMPTY, np.uint64)
    for ox, oy in disc_offsets(radius):
        qx, qy = cx[i] + ox, cy[i] + oy
        ok = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)  # clipped, never wrapped
        np.minimum.at(K, qy[ok] * W + qx[ok], key[i][ok])
    owned = K != EMPTY
    owner = np.full(H * W, -1, np.int64)
    owner[owned] = 0xFFFFFFFF - (K[owned] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    out = np.array(image, np.uint8).reshape(H * W, 3).copy()
    out[owned] = colour_of(owner[owned], labels, colors, palette)
    return out.reshape(H, W, 3), owner.astype(np.int32).reshape(H, W), len(i)


# ------------------------------------------------------------------------------- the scene of tests/cpp/overlay.cpp
class Lcg:
    """the generator of tests/cpp/overlay.cpp: doubles in [0, 1) that both languages compute alike"""

    def __init__(self, state=24680):
        self.s = state

    def __call__(self):
        self.s = (self.s * 1664525 + 1013904223) & 0xFFFFFFFF
        return float(self.s >> 8) * (1.0 / 16777216.0)


CPP_PITCH = 300
CPP_RT = np.array([0.96875, 0.0, 0.25, 0.0, 1.0, 0.0, -0.25, 0.0, 0.96875, 0.05, -0.05, 1.25])  # not a rotation: any Rt is legal
CPP_PALETTE = np.array([[255, 0, 0], [0, 0, 255], [255, 255, 0]], np.uint8)


def cpp_cam():
    return CR.Cam(70.0, 71.0, 47.3, 32.6, 96, 64, (-0.2972345646, 0.08469466538, -0.0004248149362, -0.000175399726), 1.5)


def cpp_scene():
    """(image as a 64 x 96 x 3 view into rows of 300 bytes, records n x 4, labels), drawn in the driver's order of
    calls to the generator"""
    rnd = Lcg()
    buf = np.array([int(256.0 * rnd()) for _ in range(64 * CPP_PITCH)], np.uint8).reshape(64, CPP_PITCH)
    image = np.lib.stride_tricks.as_strided(buf, (64, 96, 3), (CPP_PITCH, 3, 1))
    n = 1500
    rec = np.zeros((n, 4), np.float32)
    labels = np.zeros(n, np.int32)
    for i in range(n):
        z = -3.0 if i % 50 == 0 else 1.5 + 4.0 * rnd()
        rec[i] = (np.float32(6.0 * (rnd() - 0.5)), np.float32(4.0 * (rnd() - 0.5)), np.float32(z), np.float32(255.0 * rnd()))
        labels[i] = int(7.0 * rnd()) - 1  # -1 .. 5: some are skipped, some wrap around the 3-row palette
    return image, rec, labels


def fnv1a(a) -> int:
    """FNV-1a over the bytes of a, as the driver prints it"""
    h = 0xCBF29CE484222325
    for b in np.ascontiguousarray(a).view(np.uint8).ravel().tolist():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h
