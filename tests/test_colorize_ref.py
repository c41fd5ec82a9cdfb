"""The numpy restatement of the colorize contract (tests/colorize_ref.py) against the script's own formulation
(post_process/colorize_pcd.py:31-63), written out plainly here: R @ P.T + t through BLAS, fx * (x / z) + cx, the
mask, astype(int32), img[v, u, ::-1] / 255.0.  With the script's extrinsic and intrinsics on a seeded 200 000-point
scene and a seeded random image: masks, pixel indices and double colours equal, u and v within 1e-9.  CPU only."""
import numpy as np
import pytest

import colorize_ref as CR

N = 200_000


@pytest.fixture(scope="module")
def scene():
    pts = CR.script_scene(N, seed=7)
    cam = CR.script_cam()
    img = np.random.default_rng(11).integers(0, 256, (cam.height, cam.width, 3), dtype=np.uint8)
    return pts, cam, img


def script(points, img, R, t, fx, fy, cx, cy):
    """colorize_pcd.py:31-63 on float64 points, as the script has them from Open3D"""
    img_h, img_w = img.shape[:2]
    with np.errstate(all="ignore"):
        points_cam = (R @ points.T + t.reshape(3, 1)).T
        x, y, z = points_cam[:, 0], points_cam[:, 1], points_cam[:, 2]
        u = fx * (x / z) + cx
        v = fy * (y / z) + cy
        valid = (z > 0) & (u >= 0) & (u < img_w) & (v >= 0) & (v < img_h)
    colors = np.zeros_like(points)
    colors[:] = [0.5, 0.5, 0.5]
    u_valid = u[valid].astype(np.int32)
    v_valid = v[valid].astype(np.int32)
    colors[valid] = img[v_valid, u_valid, ::-1] / 255.0
    return u, v, valid, u_valid, v_valid, colors


def test_restatement_equals_the_script(scene):
    pts, cam, img = scene
    u, v, valid, u_valid, v_valid, colors = script(pts.astype(np.float64), img, CR.SCRIPT_R, CR.SCRIPT_T, *CR.SCRIPT_K)
    pr = CR.project(pts, cam, CR.script_Rt())
    share = valid.mean()
    print(f"valid share {share:.3f}")
    assert 0.2 < share < 0.8  # the scene exercises both sides of the mask
    # no point within 1e-9 of a pixel edge: a last-bit difference of BLAS cannot move a point across one
    for w in (u[valid], v[valid]):
        assert np.abs(w - np.rint(w)).min() > 1e-9
    np.testing.assert_array_equal(pr.valid, valid)
    np.testing.assert_array_equal(pr.px[valid], u_valid)
    np.testing.assert_array_equal(pr.py[valid], v_valid)
    assert (pr.px[~valid] == -1).all() and (pr.py[~valid] == -1).all()
    err = max(np.abs(pr.u[valid] - u[valid]).max(), np.abs(pr.v[valid] - v[valid]).max())
    print(f"max |u, v| difference from the BLAS formulation: {err:.3g}")
    assert err < 1e-9
    # one frame, no occlusion, BGR input: the script's double colours, identical
    st = CR.State(len(pts))
    n_up = st.add_frame(pts, cam, CR.script_Rt(), img, bgr=True)
    assert n_up == np.count_nonzero(valid)
    np.testing.assert_array_equal(st.frame >= 0, valid)
    np.testing.assert_array_equal(st.colors_float().view(np.uint64), colors.view(np.uint64))


def test_zero_distortion_is_the_scripts_pinhole_bit_for_bit(scene):
    """with all-zero dist, rad == 1 and the tangential term is +0: u is fx * (x / z) + cx computed from the
    contract's own xc, yc, zc — an identity of the one code path, not a second path"""
    pts, cam, _ = scene
    Rt = CR.script_Rt()
    R, t = Rt[:9].reshape(3, 3), Rt[9:]
    p = pts.astype(np.float64)
    c = [((R[k, 0] * p[:, 0] + R[k, 1] * p[:, 1]) + R[k, 2] * p[:, 2]) + t[k] for k in range(3)]
    with np.errstate(all="ignore"):
        u = cam.fx * (c[0] / c[2]) + cam.cx
        v = cam.fy * (c[1] / c[2]) + cam.cy
    pr = CR.project(pts, cam, Rt)
    np.testing.assert_array_equal(pr.u.view(np.uint64), u.view(np.uint64))
    np.testing.assert_array_equal(pr.v.view(np.uint64), v.view(np.uint64))
    np.testing.assert_array_equal(pr.zc.view(np.uint64), c[2].view(np.uint64))


def test_distortion_moves_points_and_r2_max_cuts_the_fold_back():
    """the rig's 8- and 5-parameter sets: on the axis nothing moves, off it the pixel moves by the model's amount
    (checked against the formula written out for one point), and r2_max removes points beyond it"""
    for K, dist in ((CR.K8, CR.DIST8), (CR.K5, CR.DIST5)):
        cam = CR.Cam(*K, 4096, 2464, dist)
        pin = CR.Cam(*K, 4096, 2464)
        pts = np.array([[0, 0, 5], [1, 0.5, 5], [-2, 1, 4]], np.float32)
        a, b = CR.project(pts, cam, CR.IDENTITY), CR.project(pts, pin, CR.IDENTITY)
        assert a.u[0] == b.u[0] == K[2] and a.v[0] == K[3]
        assert abs(a.u[1] - b.u[1]) > 1.0  # tens of pixels on this lens
        k1, k2, p1, p2, k3, k4, k5, k6 = cam.dist
        xn, yn = 1 / 5, 0.5 / 5
        r2 = xn * xn + yn * yn
        rad = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
        xd = xn * rad + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn)
        assert abs(a.u[1] - (K[0] * xd + K[2])) < 1e-9
        cut = CR.Cam(*K, 4096, 2464, dist, r2_max=0.04)
        c = CR.project(pts, cut, CR.IDENTITY)
        assert list(c.valid) == [True, False, False] and list(a.valid) == [True, True, True]


def test_edge_cases_hold_their_premises():
    assert len(CR.edge_cases()) >= 12  # each case asserts its own premise while it is built


def test_occlusion_restatement_hides_the_back_wall():
    cam = CR.occlusion_cam()
    for radius in (0, 1, 3):
        xyz, parts = CR.occlusion_scene(radius, 0.25, 0.125)
        pr = CR.project(xyz, cam, CR.OCC_RT)
        vis = CR.visible(pr, cam, radius, 0.25, 0.125)
        assert vis[parts["probe_visible"]].all() and not vis[parts["probe_hidden"]].any()
        assert vis[parts["front"]].all()
        back = parts["back"]
        # behind the front wall's footprint, shrunk by the splat, nothing of the back wall is visible
        inside = CR.behind_front(pr, parts, radius)
        assert inside.sum() > 100 and not vis[back][inside].any()
        assert vis[back].sum() > 500  # the rest of it is seen
        # border pixels hold points: their splats are clipped on all four sides
        v = pr.valid
        assert (pr.px[v] == 0).any() and (pr.px[v] == 63).any() and (pr.py[v] == 0).any() and (pr.py[v] == 47).any()
        # a pair with equal float depths and different double depths in one pixel, both visible
        f = parts["front"]
        key = pr.py[f].astype(np.int64) * 64 + pr.px[f]
        zf = pr.zc[f].astype(np.float32)
        order = np.lexsort((zf, key))
        same = (key[order][1:] == key[order][:-1]) & (zf[order][1:] == zf[order][:-1]) & \
            (pr.zc[f][order][1:] != pr.zc[f][order][:-1])
        assert same.any()


def test_frames_keep_the_nearest_view_and_the_earlier_frame_on_a_tie():
    cam = CR.small_cam()
    Rt = CR.pose([1, 2, 3], 0.3, [0.1, -0.2, 0.3])
    pts = CR.small_scene(500, cam, Rt, seed=3)
    img0, img1 = CR.padded_image(48, 64, 200, seed=1), CR.padded_image(48, 64, 200, seed=2)
    st = CR.State(len(pts))
    n0 = st.add_frame(pts, cam, Rt, img0)
    first = st.rgb.copy()
    assert n0 > 100 and st.add_frame(pts, cam, Rt, img1) == 0  # the same pose again: every depth ties
    np.testing.assert_array_equal(st.rgb, first)
    assert set(np.unique(st.frame)) == {-1, 0}
    # RGB input of the channel-swapped image gives the same state
    st2 = CR.State(len(pts))
    st2.add_frame(pts, cam, Rt, img0[:, :, ::-1], bgr=False)
    np.testing.assert_array_equal(st2.rgb, first)


def test_pack_rgb_against_hand_written_values():
    from lio_gpu.camera import pack_rgb

    rgb = np.array([[0, 0, 0], [255, 255, 255], [1, 2, 3], [128, 128, 128], [255, 0, 0], [0, 0, 255]], np.uint8)
    want = np.array([0x00000000, 0x00FFFFFF, 0x00010203, 0x00808080, 0x00FF0000, 0x000000FF], np.uint32)
    got = pack_rgb(rgb)
    assert got.dtype == np.float32 and got.shape == (6,)
    np.testing.assert_array_equal(got.view(np.uint32), want)
    # PCL's value for pure red: 0x00ff0000 as a float is 2.3418052e-38
    assert got[4] == np.float32(2.3418052e-38)
    with pytest.raises(ValueError):
        pack_rgb(np.zeros((3, 3), np.float32))
