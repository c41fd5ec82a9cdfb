"""The numpy restatement of the overlay contract (tests/overlay_ref.py) against a second formulation written plainly:
a sequential loop over the points that runs the midpoint iteration literally and overwrites pixels in draw order, as
the tool's cv::circle loop does (post_process/lidar_projection/src/lidar_projection.cpp:113-125).  CPU only."""
import numpy as np
import pytest

import colorize_ref as CR
import overlay_ref as OR

POSE = CR.pose([1, 2, 3], 0.3, [0.1, -0.2, 0.3])


def hline(canvas, owner, y, x0, x1, colour, i):
    H, W = owner.shape
    if 0 <= y < H:
        for x in range(max(x0, 0), min(x1, W - 1) + 1):
            canvas[y, x] = colour
            owner[y, x] = i


def circle(canvas, owner, cx, cy, r, colour, i):
    """OpenCV's filled circle, its iteration as it stands"""
    err, dx, dy, plus, minus = 0, r, 0, 1, 2 * r - 1
    while dx >= dy:
        hline(canvas, owner, cy - dy, cx - dx, cx + dx, colour, i)
        hline(canvas, owner, cy + dy, cx - dx, cx + dx, colour, i)
        hline(canvas, owner, cy - dx, cx - dy, cx + dy, colour, i)
        hline(canvas, owner, cy + dx, cx - dy, cx + dy, colour, i)
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2


def sequential(pts, cam, Rt, image, radius, sequence=None, labels=None, colors=None, palette=None):
    """the tool's loop: the points of `sequence` (none: 0 .. n - 1) one after the other, each circle over what is there"""
    pr = CR.project(pts, cam, Rt)
    canvas = np.array(image, np.uint8)
    owner = np.full((cam.height, cam.width), -1, np.int32)
    drawn = 0
    for i in (range(len(pr.zc)) if sequence is None else sequence):
        if not pr.valid[i] or (labels is not None and colors is None and labels[i] < 0):
            continue
        drawn += 1
        # Python's round is ties-to-even on a float, as rint
        circle(canvas, owner, round(float(pr.u[i])), round(float(pr.v[i])), radius, OR.colour_of(np.array([i]), labels, colors, palette)[0], i)
    return canvas, owner, drawn


def scene(n=400, seed=3, dist=CR.DIST5):
    cam = CR.small_cam(dist=dist)
    rec = CR.records(CR.small_scene(n, cam, POSE, seed=seed), 4)
    img = CR.padded_image(48, 64, 200, seed=seed)
    return cam, rec, img


def same(a, b):
    for x, y in zip(a[:2], b[:2]):
        np.testing.assert_array_equal(x, y)
    assert a[2] == b[2]


@pytest.mark.parametrize("radius", [0, 1, 2, 3, 4, 15])
def test_restatement_equals_the_sequential_loop(radius):
    cam, rec, img = scene()
    rng = np.random.default_rng(radius)
    labels = rng.integers(-1, 12, len(rec)).astype(np.int32)
    colors = rng.integers(0, 256, (len(rec), 3)).astype(np.uint8)
    palette = rng.integers(0, 256, (5, 3)).astype(np.uint8)
    for src in (dict(), dict(labels=labels, palette=palette), dict(colors=colors), dict(palette=palette[2:])):
        got = OR.draw(rec, cam, POSE, img, radius, OR.DRAW_ORDER, **src)
        same(got, sequential(rec, cam, POSE, img, radius, **src))
        assert 0 < got[2] < len(rec) and (got[1] >= 0).any()
    # discs that leave the image on every side are in the scene: centres within `radius` of each border
    pr = CR.project(rec, cam, POSE)
    cx, cy = OR.centres(pr)
    v = pr.valid
    if radius >= 3:
        assert (cx[v] < radius).any() and (cx[v] > 63 - radius).any() and (cy[v] < radius).any() and (cy[v] > 47 - radius).any()


@pytest.mark.parametrize("radius,pixels", [(0, 1), (1, 5), (2, 13), (3, 29), (4, 49)])
def test_pixel_counts_and_half_widths(radius, pixels):
    want = {0: [0], 1: [1, 0], 2: [2, 1, 0], 3: [3, 2, 2, 0], 4: [4, 3, 3, 2, 0]}[radius]
    assert OR.half_widths(radius) == want
    assert len(OR.disc_offsets(radius)) == pixels == len(set(OR.disc_offsets(radius)))
    # one point in the middle of an empty image owns exactly that many pixels
    cam = CR.small_cam()
    out, owner, n = OR.draw(np.array([[0, 0, 2]], np.float32), cam, CR.IDENTITY, np.zeros((48, 64, 3), np.uint8), radius)
    assert n == 1 and (owner == 0).sum() == pixels and (out[owner == 0] == (0, 255, 0)).all() and not out[owner < 0].any()


@pytest.mark.parametrize("radius", range(16))
def test_half_width_tables_are_symmetric_under_transposition(radius):
    offs = set(OR.disc_offsets(radius))
    assert {(oy, ox) for ox, oy in offs} == offs
    assert {(-ox, oy) for ox, oy in offs} == offs and {(ox, -oy) for ox, oy in offs} == offs
    hw = OR.half_widths(radius)
    assert hw[0] == radius and len(hw) == radius + 1 and all(a >= b for a, b in zip(hw, hw[1:]))


@pytest.mark.parametrize("radius", [0, 3, 15])
def test_nearest_equals_drawing_sorted_by_depth(radius):
    cam, rec, img = scene(seed=7)
    # duplicates and equal float depths with different double depths: the index decides
    rec = np.concatenate([rec, rec[:40]])
    pr = CR.project(rec, cam, POSE)
    zf = pr.zc.astype(np.float32)
    seq = sorted(range(len(rec)), key=lambda i: (-float(zf[i]) if pr.valid[i] else 0.0, i))
    labels = np.random.default_rng(1).integers(-1, 4, len(rec)).astype(np.int32)
    for src in (dict(), dict(labels=labels, palette=CR.padded_image(1, 6, 18)[0])):
        got = OR.draw(rec, cam, POSE, img, radius, OR.NEAREST, **src)
        same(got, sequential(rec, cam, POSE, img, radius, sequence=seq, **src))
    assert (got[1] >= len(rec) - 40).any()  # a duplicate's second copy owns pixels


def test_cpp_scene_is_stable():
    """the scene shared with tests/cpp/overlay.cpp: its generator's first values and what it exercises"""
    rnd = OR.Lcg()
    s1 = (24680 * 1664525 + 1013904223) & 0xFFFFFFFF
    assert rnd() == (s1 >> 8) / 16777216.0 and rnd.s == s1
    img, rec, labels = OR.cpp_scene()
    assert img.shape == (64, 96, 3) and img.strides == (300, 3, 1) and rec.shape == (1500, 4)
    assert labels.min() == -1 and labels.max() == 5
    _, owner, n = OR.draw(rec, OR.cpp_cam(), OR.CPP_RT, img, 3, OR.NEAREST, labels=labels, palette=OR.CPP_PALETTE)
    assert 300 < n < 1400 and (owner >= 0).sum() > 1000 and (owner < 0).sum() > 100
