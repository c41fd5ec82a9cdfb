"""GPU checks of the point overlay (lio_overlay.hip: lio_overlay_*) against the contract restated in numpy
(tests/overlay_ref.py; tests/test_overlay_ref.py holds that restatement against a sequential loop).  Every output is
compared bit for bit: the owner image first, then the image, then n_drawn."""
import ctypes as C

import numpy as np
import pytest

import colorize_ref as CR
import overlay_ref as OR
from lio_gpu import _capi
from lio_gpu import camera as CAM
from lio_gpu import filters

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 5000]  # those of tests/test_gpu_colorize.py
PITCH = 200                                    # bytes per row of the 64 x 48 test image (3 * 64 = 192)
POSE = CR.pose([1, 2, 3], 0.3, [0.1, -0.2, 0.3])
ORDER = {OR.DRAW_ORDER: "draw", OR.NEAREST: "nearest"}


def model(cam):
    return CAM.CameraModel(cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, cam.dist, cam.r2_max)


@pytest.fixture(scope="module")
def overlays():
    """one handle per (radius, order), made when first asked for"""
    made = {}

    def get(radius, order):
        if (radius, order) not in made:
            made[radius, order] = CAM.PointOverlay(radius, ORDER[order])
        return made[radius, order]

    yield get
    for ov in made.values():
        ov.close()


def same(ov, got, exp, msg=""):
    out, owner = got
    np.testing.assert_array_equal(owner, exp[1], err_msg=msg + " (owner)")
    np.testing.assert_array_equal(out, exp[0], err_msg=msg + " (image)")
    assert ov.n_drawn == exp[2], msg + " (n_drawn)"


def draw(ov, rec, cam, Rt, img, labels=None, colors=None, palette=None):
    """the cloud and its sources set anew, one draw with the owner image"""
    ov.set_cloud(rec)
    ov.set_palette(OR.GREEN if palette is None else palette)
    if labels is not None:
        ov.set_labels(labels)
    if colors is not None:
        ov.set_colors(colors)
    return ov.draw(model(cam), Rt, img, owner=True)


def check(ov, rec, cam, Rt, img, radius, order, msg="", **src):
    exp = OR.draw(rec, cam, Rt, img, radius, order, **src)
    same(ov, draw(ov, rec, cam, Rt, img, **src), exp, msg)
    return exp


# ----------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("radius", [0, 1, 3, 15])
@pytest.mark.parametrize("n", SIZES)
def test_shapes_strides_radii_and_orders(overlays, n, radius):
    """every size with strides 3, 4 and 8, the rig's 5-parameter distortion, an image whose pitch exceeds 3 x width,
    both orders; the restatement is computed once per order and shared by the strides (the fields after x y z must
    not matter)"""
    cam = CR.small_cam(dist=CR.DIST5)
    img = CR.padded_image(48, 64, PITCH, seed=n)
    xyz = CR.small_scene(n, cam, POSE, seed=n + radius)
    for order in (OR.DRAW_ORDER, OR.NEAREST):
        exp = OR.draw(xyz, cam, POSE, img, radius, order)
        if n >= 255:
            assert 0 < exp[2] < n
        for stride in (3, 4, 8):
            ov = overlays(radius, order)
            same(ov, draw(ov, CR.records(xyz, stride, seed=stride), cam, POSE, img), exp, f"n={n} r={radius} order={order} stride={stride}")


# --------------------------------------------------------------------------------------------- centre rounding
@pytest.mark.parametrize("radius", [0, 1, 3])
def test_centres_round_to_even_after_the_validity_test(overlays, radius):
    """a pinhole with fx = fy = 1, cx = cy = 0 and points at z = 1: u = x, v = y"""
    cam = CR.Cam(1.0, 1.0, 0.0, 0.0, 64, 48)
    W, H = 64, 48
    xyz = np.array([[2.5, 8, 1], [3.5, 16, 1], [0.4, 24, 1], [W - 0.4, 32, 1], [-0.4, 40, 1],  # on u
                    [10, 2.5, 1], [20, 3.5, 1], [30, 0.4, 1], [40, H - 0.4, 1], [50, -0.4, 1]], np.float32)  # on v
    pr = CR.project(xyz, cam, CR.IDENTITY)
    assert list(pr.valid) == [True, True, True, True, False] * 2
    cx, cy = OR.centres(pr)
    assert list(cx[:4]) == [2, 4, 0, W] and list(cy[5:9]) == [2, 4, 0, H]  # ties to even; a centre on x == width
    ov = overlays(radius, OR.DRAW_ORDER)
    _, owner, n = check(ov, xyz, cam, CR.IDENTITY, np.zeros((H, W, 3), np.uint8), radius, OR.DRAW_ORDER)
    assert n == 8                                               # the centres outside the image are drawn points
    hw = OR.half_widths(radius)
    assert owner[8, 2] == 0 and owner[16, 4] == 1 and owner[2, 10] == 5 and owner[4, 20] == 6
    assert owner[8, 2 + radius] == 0 and (radius == 0 or owner[8, 3 + radius] == -1)
    assert (owner == 2).sum() == sum(hw[abs(d)] + 1 for d in range(-radius, radius + 1))  # clipped on the left, not wrapped
    assert (owner == 7).sum() == (owner == 2).sum()                                        # and at the top
    assert (owner[:, W - 1] == 3).sum() == (2 * radius - 1 if radius else 0)              # centre W: the column W - 1 of the rows |d| < r
    assert (owner == 3).sum() == sum(hw[abs(d)] for d in range(-radius, radius + 1))
    assert (owner == 8).sum() == (owner == 3).sum() and (radius == 0 or owner[H - 1, 40] == 8)
    assert not np.isin(owner, [4, 9]).any()                                                # u = -0.4, v = -0.4: invalid


# -------------------------------------------------------------------------------------------------------- ties
def test_duplicates_give_the_higher_index_in_both_orders(overlays):
    cam = CR.small_cam()
    xyz = CR.small_scene(300, cam, POSE, seed=5)
    rec = CR.records(np.concatenate([xyz, xyz]), 4)
    for order in (OR.DRAW_ORDER, OR.NEAREST):
        _, owner, _ = check(overlays(3, order), rec, cam, POSE, CR.padded_image(48, 64, PITCH, seed=1), 3, order)
        assert owner.max() >= 300 and not ((owner >= 0) & (owner < 300)).any()


def test_equal_float_depth_is_decided_by_the_index(overlays):
    """zc = 1e-9 x + z: the two depths differ in double and are one float; in double the lower index is nearer"""
    cam = CR.small_cam()
    Rt = CR.IDENTITY.copy()
    Rt[6] = 1e-9
    xyz = np.array([[0, 0, 2], [0.125, 0, 2]], np.float32)
    pr = CR.project(xyz, cam, Rt)
    assert pr.zc[0] < pr.zc[1] and np.float32(pr.zc[0]) == np.float32(pr.zc[1])
    cx, _ = OR.centres(pr)
    assert cx[1] - cx[0] == 2
    _, owner, _ = check(overlays(3, OR.NEAREST), xyz, cam, Rt, np.zeros((48, 64, 3), np.uint8), 3, OR.NEAREST)
    assert owner[24, cx[0] + 1] == 1 and owner[24, cx[0] - 3] == 0 and (owner == 1).sum() == 29


def test_a_covered_disc_owns_nothing_when_nearest_and_everything_when_drawn_later(overlays):
    cam = CR.small_cam()
    xyz = np.array([[0, 0, 1], [0, 0, 2]], np.float32)  # one centre; the far point is drawn later
    img = CR.padded_image(48, 64, PITCH, seed=2)
    _, owner, n = check(overlays(3, OR.NEAREST), xyz, cam, CR.IDENTITY, img, 3, OR.NEAREST)
    assert n == 2 and (owner == 0).sum() == 29 and not (owner == 1).any()
    _, owner, n = check(overlays(3, OR.DRAW_ORDER), xyz, cam, CR.IDENTITY, img, 3, OR.DRAW_ORDER)
    assert n == 2 and (owner == 1).sum() == 29 and not (owner == 0).any()


# ----------------------------------------------------------------------------------------------- colour sources
def test_colour_sources(overlays):
    cam = CR.small_cam(dist=CR.DIST5)
    n = 600
    rec = CR.records(CR.small_scene(n, cam, POSE, seed=11), 4)
    img = CR.padded_image(48, 64, PITCH, seed=11)
    rng = np.random.default_rng(11)
    palette = rng.integers(0, 256, (4, 3)).astype(np.uint8)
    labels = rng.integers(-1, 9, n).astype(np.int32)  # -1: skipped; 4 .. 8 wrap around the 4 rows
    pr = CR.project(rec, cam, POSE)
    last = int(np.flatnonzero(pr.valid)[-1])
    labels[last] = -1  # it would win every pixel of its disc in draw order
    colors = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    for order in (OR.DRAW_ORDER, OR.NEAREST):
        ov = overlays(3, order)
        plain = check(ov, rec, cam, POSE, img, 3, order, palette=palette[1:])  # a constant colour: the palette's row 0
        assert set(map(tuple, plain[0][plain[1] >= 0])) == {tuple(palette[1])}
        exp = check(ov, rec, cam, POSE, img, 3, order, labels=labels, palette=palette)
        assert exp[2] == int(pr.valid.sum()) - int((labels[pr.valid] < 0).sum()) < plain[2]
        assert not np.isin(exp[1], np.flatnonzero(labels < 0)).any() and (labels[exp[1][exp[1] >= 0]] >= 4).any()
        check(ov, rec, cam, POSE, img, 3, order, colors=colors)
    # the premise of `last`: without its label it owns its whole clipped disc in draw order
    assert (OR.draw(rec, cam, POSE, img, 3, OR.DRAW_ORDER)[1] == last).any()


def test_palette_row_change_between_two_draws_is_the_only_upload(overlays):
    cam = CR.small_cam()
    rec = CR.records(CR.small_scene(400, cam, POSE, seed=12), 3)
    img = CR.padded_image(48, 64, PITCH, seed=12)
    labels = np.random.default_rng(12).integers(0, 3, 400).astype(np.int32)
    palette = np.array([[1, 2, 3], [40, 50, 60], [7, 8, 9]], np.uint8)
    ov = overlays(1, OR.NEAREST)
    same(ov, draw(ov, rec, cam, POSE, img, labels=labels, palette=palette), OR.draw(rec, cam, POSE, img, 1, OR.NEAREST, labels=labels, palette=palette))
    palette[1] = (200, 100, 0)
    ov.set_palette(palette)
    exp = OR.draw(rec, cam, POSE, img, 1, OR.NEAREST, labels=labels, palette=palette)
    same(ov, ov.draw(model(cam), POSE, img, owner=True), exp)
    assert (exp[0] == (200, 100, 0)).all(axis=2).any()


# ------------------------------------------------------------------------------------------------ source pixels
def test_untouched_pixels_and_the_callers_padding(overlays):
    cam = CR.small_cam()
    rec = CR.records(CR.small_scene(40, cam, POSE, seed=13), 4)
    img = CR.padded_image(48, 64, PITCH, seed=13)
    exp = OR.draw(rec, cam, POSE, img, 3, OR.DRAW_ORDER)
    assert 100 < (exp[1] < 0).sum() < 64 * 48 - 100
    buf = np.full((48, 208), 0xA5, np.uint8)  # the caller's rows: 16 bytes of padding each, another pitch than the input's
    out = np.lib.stride_tricks.as_strided(buf, (48, 64, 3), (208, 3, 1))
    ov = overlays(3, OR.DRAW_ORDER)
    ov.set_cloud(rec)
    ov.set_palette(OR.GREEN)
    got = ov.draw(model(cam), POSE, img, out=out, owner=True)
    assert got[0] is out
    same(ov, got, exp)
    np.testing.assert_array_equal(out[exp[1] < 0], np.asarray(img)[exp[1] < 0])
    assert (buf[:, 192:] == 0xA5).all()
    # in place: out is the image
    buf2 = np.lib.stride_tricks.as_strided(np.asarray(img), (48, PITCH), (PITCH, 1)).copy()
    work = np.lib.stride_tricks.as_strided(buf2, (48, 64, 3), (PITCH, 3, 1))
    pad = buf2[:, 192:].copy()
    same(ov, ov.draw(model(cam), POSE, work, out=work, owner=True), exp)
    np.testing.assert_array_equal(buf2[:, 192:], pad)


# --------------------------------------------------------------------------------------------- draw_undistorted
def test_draw_undistorted_equals_undistorter_then_draw(overlays):
    """the rig's 8-parameter model on a 1/16-scale camera: one upload and one download, the bits of the two calls"""
    K = [k / 16 for k in CR.K8]
    raw_cam = CAM.CameraModel(*K, 256, 154, CR.DIST8)
    rect = CR.Cam(*K, 256, 154)
    Rt = CR.script_Rt()
    rec = CR.records(CR.script_scene(5000, seed=5), 4)
    raw = CR.padded_image(154, 256, 800, seed=9)
    ud = CAM.Undistorter()
    ud.set_camera(raw_cam)
    rectified = ud(raw)
    assert (rectified != np.asarray(raw)).any()
    for order in (OR.DRAW_ORDER, OR.NEAREST):
        ov = overlays(3, order)
        exp = check(ov, rec, rect, Rt, rectified, 3, order)
        assert 500 < exp[2] < 4500
        same(ov, ov.draw_undistorted(ud, model(rect), Rt, raw, owner=True), exp)
        t = ov.timing()
        assert set(t) == {"upload_ms", "fill_ms", "stamp_ms", "compose_ms", "download_ms"} and t["stamp_ms"] > 0
    ud.close()


# --------------------------------------------------------------------------------- allocation, cloud change
def test_second_frame_of_one_size_allocates_nothing_and_the_cloud_may_change():
    cam = CR.small_cam(dist=CR.DIST5)
    L = _capi.lib()
    ov = CAM.PointOverlay(3, "nearest")
    imgs = [CR.padded_image(48, 64, PITCH, seed=20 + k) for k in range(3)]
    rec = CR.records(CR.small_scene(5000, cam, POSE, seed=20), 4)
    ov.set_cloud(rec)
    first = ov.draw(model(cam), POSE, imgs[0], owner=True)
    settled = L.lio_alloc_count()
    for img in imgs[1:] + imgs[:1]:
        got = ov.draw(model(cam), POSE, img, owner=True)
        assert L.lio_alloc_count() == settled, "a frame of a size seen before allocated"
    same(ov, got, OR.draw(rec, cam, POSE, imgs[0], 3, OR.NEAREST))
    np.testing.assert_array_equal(got[0], first[0])  # repeated draws give identical bits
    np.testing.assert_array_equal(got[1], first[1])
    # another cloud of another size between draws, smaller and larger; the sources of the old cloud are gone
    ov.set_labels(np.full(5000, -1, np.int32))
    for n in (300, 7000):
        rec = CR.records(CR.small_scene(n, cam, POSE, seed=n), 3)
        ov.set_cloud(rec)
        exp = OR.draw(rec, cam, POSE, imgs[1], 3, OR.NEAREST)
        same(ov, ov.draw(model(cam), POSE, imgs[1], owner=True), exp)
        assert exp[2] > 0
    ov.close()


# --------------------------------------------------------------------------------------------------- the tool
def test_lidar_projection_overlay_equals_the_three_calls_by_hand():
    cam = CR.small_cam()
    xyz = CR.small_scene(1200, cam, POSE, seed=31)
    img = CR.padded_image(48, 64, PITCH, seed=31)
    km = filters.KMeans(n_clusters=5, seed=0)
    labels = km.fit(xyz)
    km.close()
    colors = filters.cluster_palette(labels)
    by_hand = CAM.draw_points(img, xyz, model(cam), POSE, radius=3, colors=colors)
    got, got_labels = CAM.lidar_projection_overlay(xyz, img, model(cam), POSE, K=5, seed=0, by_cluster=True)
    np.testing.assert_array_equal(got_labels, labels)
    np.testing.assert_array_equal(got, by_hand)
    np.testing.assert_array_equal(got, OR.draw(xyz, cam, POSE, img, 3, OR.DRAW_ORDER, colors=colors)[0])
    assert len(set(map(tuple, colors))) == 5
    # as shipped: every point green
    shipped, _ = CAM.lidar_projection_overlay(xyz, img, model(cam), POSE)
    exp = OR.draw(xyz, cam, POSE, img, 3, OR.DRAW_ORDER)
    np.testing.assert_array_equal(shipped, exp[0])
    assert (shipped[exp[1] >= 0] == (0, 255, 0)).all()
    # the one-shot with labels and a palette, and its owner image
    out, owner = CAM.draw_points(img, xyz, model(cam), POSE, radius=1, order="nearest", labels=labels,
                                 palette=filters.CLUSTER_PALETTE_BGR, owner=True)
    exp = OR.draw(xyz, cam, POSE, img, 1, OR.NEAREST, labels=labels, palette=filters.CLUSTER_PALETTE_BGR)
    np.testing.assert_array_equal(owner, exp[1])
    np.testing.assert_array_equal(out, exp[0])


# --------------------------------------------------------------------------------------------- argument errors
def _err(rc, code, *words):
    msg = _capi.lib().lio_last_error().decode()
    assert rc == code, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_argument_errors_name_their_bound():
    L = _capi.lib()
    ARG, STATE = _capi.LIO_ERR_ARG, _capi.LIO_ERR_STATE
    dp, i32p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    h = C.c_void_p()
    for p, word in ((_capi.OverlayParams(16, 0), "0..15"), (_capi.OverlayParams(-1, 0), "0..15"), (_capi.OverlayParams(3, 2), "order")):
        _err(L.lio_overlay_create(0, C.byref(p), C.byref(h)), ARG, word)
        assert not h.value
    _err(L.lio_overlay_create(0, None, None), ARG, "out is NULL")
    assert L.lio_overlay_create(0, None, C.byref(h)) == 0
    try:
        cam = model(CR.small_cam())._c()
        Rt = CR.IDENTITY.copy()
        rtp = Rt.ctypes.data_as(dp)
        img = np.zeros((48, PITCH), np.uint8)
        out = np.zeros((48, PITCH), np.uint8)
        ip, op = img.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
        nd = C.c_int64(-7)
        pts = np.zeros((4, 8), np.float32)
        pts[:, 2] = 2.0
        fp = pts.ctypes.data_as(_capi.fp)
        labels = np.zeros(4, np.int32)
        colors = np.zeros((4, 3), np.uint8)
        lp, cp = labels.ctypes.data_as(i32p), colors.ctypes.data_as(u8p)
        _err(L.lio_overlay_draw(h, C.byref(cam), rtp, ip, PITCH, op, PITCH, None, C.byref(nd)), STATE, "lio_overlay_set_cloud")
        _err(L.lio_overlay_set_labels(h, lp, 4), STATE, "lio_overlay_set_cloud")
        _err(L.lio_overlay_set_colors(h, cp, 4), STATE, "lio_overlay_set_cloud")
        _err(L.lio_overlay_set_cloud(h, None, 4, 3), ARG, "pts is NULL")
        _err(L.lio_overlay_set_cloud(h, fp, -1, 3), ARG, "2^32 - 2")
        _err(L.lio_overlay_set_cloud(h, fp, (1 << 32) - 1, 3), ARG, "2^32 - 2")
        _err(L.lio_overlay_set_cloud(h, fp, 4, 2), ARG, "3..8")
        _err(L.lio_overlay_set_cloud(h, fp, 4, 9), ARG, "3..8")
        assert L.lio_overlay_set_cloud(h, fp, 4, 8) == 0
        _err(L.lio_overlay_set_labels(h, lp, 3), ARG, "number of points")
        _err(L.lio_overlay_set_colors(h, cp, 5), ARG, "number of points")
        assert L.lio_overlay_set_labels(h, lp, 4) == 0
        _err(L.lio_overlay_set_colors(h, cp, 4), ARG, "one colour source")
        assert L.lio_overlay_set_labels(h, None, 0) == 0 and L.lio_overlay_set_colors(h, cp, 4) == 0
        _err(L.lio_overlay_set_labels(h, lp, 4), ARG, "one colour source")
        assert L.lio_overlay_set_colors(h, None, 0) == 0
        _err(L.lio_overlay_set_palette(h, None, 1), ARG, "palette is NULL")
        _err(L.lio_overlay_set_palette(h, cp, 0), ARG, "at least 1")
        _err(L.lio_overlay_draw(h, None, rtp, ip, PITCH, op, PITCH, None, C.byref(nd)), ARG, "cam is NULL")
        _err(L.lio_overlay_draw(h, C.byref(cam), None, ip, PITCH, op, PITCH, None, C.byref(nd)), ARG, "Rt is NULL")
        _err(L.lio_overlay_draw(h, C.byref(cam), rtp, None, PITCH, op, PITCH, None, C.byref(nd)), ARG, "image is NULL")
        _err(L.lio_overlay_draw(h, C.byref(cam), rtp, ip, PITCH, None, PITCH, None, C.byref(nd)), ARG, "out is NULL")
        _err(L.lio_overlay_draw(h, C.byref(cam), rtp, ip, PITCH, op, PITCH, None, None), ARG, "n_drawn is NULL")
        _err(L.lio_overlay_draw(h, C.byref(cam), rtp, ip, 191, op, PITCH, None, C.byref(nd)), ARG, "pitch")
        _err(L.lio_overlay_draw(h, C.byref(cam), rtp, ip, PITCH, op, 191, None, C.byref(nd)), ARG, "out_pitch")
        _err(L.lio_overlay_draw_undistorted(h, None, C.byref(cam), rtp, ip, PITCH, op, PITCH, None, C.byref(nd)), ARG, "undistorter is NULL")
        _err(L.lio_overlay_get_timing(h, None), ARG, "ms5 is NULL")
        assert nd.value == -7  # nothing ran
        assert L.lio_overlay_draw(h, C.byref(cam), rtp, ip, 192, op, 192, None, C.byref(nd)) == 0 and nd.value == 4
        # an empty cloud is a cloud: the image comes back as it went in
        assert L.lio_overlay_set_cloud(h, None, 0, 3) == 0
        img[:] = 77
        assert L.lio_overlay_draw(h, C.byref(cam), rtp, ip, PITCH, op, PITCH, None, C.byref(nd)) == 0 and nd.value == 0
        assert (out[:, :192] == 77).all()
        # an undistorter of another size or of one channel
        ud = CAM.Undistorter()
        _err(L.lio_overlay_draw_undistorted(h, ud._h, C.byref(cam), rtp, ip, PITCH, op, PITCH, None, C.byref(nd)), STATE, "lio_undistorter_set_camera")
        ud.set_camera(CAM.CameraModel(32, 24, 32, 24, 64, 48), channels=1)
        _err(L.lio_overlay_draw_undistorted(h, ud._h, C.byref(cam), rtp, ip, PITCH, op, PITCH, None, C.byref(nd)), ARG, "3 channels")
        ud.set_camera(CAM.CameraModel(16, 12, 16, 12, 32, 24))
        _err(L.lio_overlay_draw_undistorted(h, ud._h, C.byref(cam), rtp, ip, PITCH, op, PITCH, None, C.byref(nd)), ARG, "rectified image")
        ud.close()
    finally:
        L.lio_overlay_destroy(h)
    _err(L.lio_overlay_get_timing(None, None), ARG, "handle is NULL")
