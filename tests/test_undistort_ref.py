"""The numpy restatement of the undistortion contract (tests/undistort_ref.py) held against itself: the identity, the
two forms of the fixed-point sum, and every scene of the GPU tests producing the classes of pixels it is there for.
CPU only."""
import numpy as np
import pytest

import undistort_ref as UR


@pytest.mark.parametrize("cam", [UR.small_cam(), UR.Cam(*(k / 64.0 for k in UR.K8), 64, 38),
                                 UR.Cam(1422.18129, 1421.822766, 2017.285053, 1232.094237, 97, 61)])
def test_no_distortion_and_the_same_camera_return_the_input(cam):
    """u differs from j by rounding in the last bits where the intrinsics are not round numbers; the 1/32-pixel
    rounding absorbs it, so every pixel is its own source with weight 1024 — the last row and column included, whose
    second taps are outside and carry weight 0"""
    m = UR.undistort_map(cam)
    jj, ii = np.meshgrid(np.arange(cam.width), np.arange(cam.height))
    assert np.abs(m.u - jj).max() < 1e-9 and np.abs(m.v - ii).max() < 1e-9
    np.testing.assert_array_equal(m.sx, jj)
    np.testing.assert_array_equal(m.sy, ii)
    assert not m.ax.any() and not m.ay.any() and not m.far.any()
    for channels in (1, 3):
        img = UR.image(cam, channels, seed=channels)
        np.testing.assert_array_equal(UR.remap(img, m, cam, border=(9, 99, 199)), img)


def test_the_table_form_of_the_sum_gives_the_same_bytes():
    """OpenCV's table holds 32 w of 2^15 and rounds with 2^14 >> 15; the contract says (w, 512, >> 10)"""
    for s in UR.scenes():
        m = UR.undistort_map(s.src, s.dst)
        for img in (UR.image(s.src, 3, seed=5), np.full((s.src.height, s.src.width, 3), 255, np.uint8)):
            np.testing.assert_array_equal(UR.remap(img, m, s.src, (7, 200, 31), scale=32, half=2 ** 14, shift=15),
                                          UR.remap(img, m, s.src, (7, 200, 31)), err_msg=s.name)
    # every pair of fractions against every pair of extreme neighbours
    a = np.arange(32, dtype=np.int64)
    ax, ay = np.meshgrid(a, a)
    w = [(32 - ax) * (32 - ay), ax * (32 - ay), (32 - ax) * ay, ax * ay]
    assert (sum(w) == 1024).all()
    for taps in np.ndindex(2, 2, 2, 2):
        acc = sum(wk * 255 * t for wk, t in zip(w, taps))
        np.testing.assert_array_equal((32 * acc + 2 ** 14) >> 15, (acc + 512) >> 10)


@pytest.mark.parametrize("scene", UR.scenes() + [UR.large_scene()], ids=lambda s: s.name)
def test_every_scene_produces_the_classes_it_covers(scene):
    c = UR.classes(UR.undistort_map(scene.src, scene.dst), scene.src)
    for name in scene.covers:
        assert c[name] > 0, (scene.name, name, c)
    out = scene.out_cam
    assert c["all_in"] + c["partial"] + c["all_out"] + c["far"] == out.width * out.height


def test_the_counts_of_the_two_scenes_the_contract_quotes():
    by = {s.name: UR.classes(UR.undistort_map(s.src, s.dst), s.src) for s in UR.scenes()}
    w = by["wide"]
    assert (w["all_in"], w["partial"], w["left"], w["right"], w["top"], w["bottom"], w["all_out"]) == (2491, 237, 42, 57, 80, 58, 344)
    assert by["pole"]["far"] == 2
    m = UR.undistort_map(UR.scenes()[-1].src)
    assert m.far[24, 0] and m.u[24, 0] == -np.inf and np.isnan(m.v[24, 0])
    assert m.sx[24, 0] == m.sy[24, 0] == -2 ** 31 and m.ax[24, 0] == m.ay[24, 0] == 0


def test_rounding_ties_go_to_even():
    """no distortion, dst.cx = 32 - 1/64, dst.cy = 24 + 1/64: every u * 32 is 32 j + 0.5 and every v * 32 is
    32 i - 0.5, exactly; ties to even give ax = ay = 0, sx = j, sy = i (half up: ax = 1; half away: sy = -1, ay = 31 at
    i = 0)"""
    src = UR.small_cam()
    dst = UR.pinhole(32.0, 24.0, 32.0 - 1.0 / 64.0, 24.0 + 1.0 / 64.0, 64, 48)
    m = UR.undistort_map(src, dst)
    jj, ii = np.meshgrid(np.arange(64), np.arange(48))
    np.testing.assert_array_equal(m.u * 32.0, 32.0 * jj + 0.5)
    np.testing.assert_array_equal(m.v * 32.0, 32.0 * ii - 0.5)
    np.testing.assert_array_equal(m.sx, jj)
    np.testing.assert_array_equal(m.sy, ii)
    assert not m.ax.any() and not m.ay.any()


def test_a_tap_outside_takes_the_border_whatever_its_weight():
    """one pixel per side, fractions chosen: the weights of the outside taps go to the border value"""
    src = UR.small_cam()
    img = np.full((48, 64, 3), 200, np.uint8)
    m = UR.Map(None, None, np.array([[-1, 63, 10, 10]], np.int32), np.array([[5, 5, -1, 47]], np.int32),
               np.array([[8, 8, 0, 0]], np.uint8), np.array([[0, 0, 24, 24]], np.uint8), np.zeros((1, 4), bool))
    out = UR.remap(img, m, src, border=(0, 100, 200))
    # left: the inside tap has weight 8 * 32; right: 24 * 32; top: 24 * 32; bottom: 8 * 32
    for k, w_in in enumerate((256, 768, 768, 256)):
        for c, b in enumerate((0, 100, 200)):
            assert out[0, k, c] == (w_in * 200 + (1024 - w_in) * b + 512) >> 10
