"""GPU checks of the camera projection and the colorizer (lio_colorize.hip: lio_project_points, lio_colorizer_*)
against the contract restated in numpy (tests/colorize_ref.py; tests/test_colorize_ref.py holds that restatement
against the script's own formulation).  Every output is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import colorize_ref as CR
from lio_gpu import _capi
from lio_gpu import camera as CAM
from lio_gpu.filters import _Handle

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)
u8p = C.POINTER(C.c_uint8)

SIZES = [1, 63, 64, 65, 255, 256, 257, 5000]  # around one wave and one 256-thread block, and twenty blocks
PITCH = 200                                    # bytes per row of the 64 x 48 test image (3 * 64 = 192)
POSE = CR.pose([1, 2, 3], 0.3, [0.1, -0.2, 0.3])


@pytest.fixture(scope="module")
def fh():
    return _Handle()


def model(cam):
    return CAM.CameraModel(cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, cam.dist, cam.r2_max)


def b64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_projection(fh, rec, cam, Rt, msg=""):
    got = CAM.project_points(rec, model(cam), Rt, handle=fh)
    exp = CR.project(rec, cam, Rt)
    np.testing.assert_array_equal(got.valid, exp.valid, err_msg=msg)
    np.testing.assert_array_equal(b64(got.uv[:, 0]), b64(exp.u), err_msg=msg)
    np.testing.assert_array_equal(b64(got.uv[:, 1]), b64(exp.v), err_msg=msg)
    np.testing.assert_array_equal(b64(got.zc), b64(exp.zc), err_msg=msg)
    np.testing.assert_array_equal(got.pix[:, 0], exp.px, err_msg=msg)
    np.testing.assert_array_equal(got.pix[:, 1], exp.py, err_msg=msg)
    return exp


def check_state(cz, st, msg=""):
    rgb, frame, depth = cz.state()
    np.testing.assert_array_equal(frame, st.frame, err_msg=msg)
    np.testing.assert_array_equal(rgb, st.rgb, err_msg=msg)
    np.testing.assert_array_equal(b64(depth), b64(st.best_z), err_msg=msg)
    np.testing.assert_array_equal(b64(cz.colors_float()), b64(st.colors_float()), err_msg=msg)


def run(rec, frames, **params):
    """frames: (cam, Rt, image) in order, on a fresh handle; the state and every n_updated against the restatement"""
    ref = dict(occlusion=params.get("occlusion", False), radius=params.get("splat_radius", 0),
               depth_rel=params.get("depth_rel", 0.0), depth_abs=params.get("depth_abs", 0.0), bgr=params.get("bgr", True))
    cz = CAM.Colorizer(**params)
    cz.set_cloud(rec)
    st = CR.State(len(rec))
    for k, (cam, Rt, img) in enumerate(frames):
        assert cz.add_frame(model(cam), Rt, img) == st.add_frame(rec, cam, Rt, img, **ref), f"n_updated of frame {k}"
    check_state(cz, st)
    return cz, st


# ----------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("n", SIZES)
def test_shapes_and_strides(fh, n):
    """every size with strides 3, 4 and 8, the rig's 5-parameter distortion, an image whose pitch exceeds 3 x width:
    the projection alone, one fused frame, and one frame through the z-buffer"""
    cam = CR.small_cam(dist=CR.DIST5)
    img = CR.padded_image(48, 64, PITCH, seed=n)
    for stride in (3, 4, 8):
        rec = CR.records(CR.small_scene(n, cam, POSE, seed=n + stride), stride, seed=stride)
        exp = check_projection(fh, rec, cam, POSE, f"n={n} stride={stride}")
        if n >= 255:
            assert 0 < exp.valid.sum() < n
        run(rec, [(cam, POSE, img)])
        run(rec, [(cam, POSE, img)], occlusion=True, splat_radius=1, depth_rel=0.01)


# ------------------------------------------------------------------------------------------- edges of validity
def test_project_points_on_the_edges_of_validity(fh):
    for name, cam, Rt, xyz, want in CR.edge_cases():
        exp = check_projection(fh, xyz, cam, Rt, name)
        np.testing.assert_array_equal(exp.valid, want, err_msg=name)


def test_colorizer_on_the_edges_of_validity():
    cz = CAM.Colorizer()
    for k, (name, cam, Rt, xyz, want) in enumerate(CR.edge_cases()):
        img = CR.padded_image(48, 64, PITCH, seed=k)
        cz.set_cloud(xyz)
        st = CR.State(len(xyz))
        assert cz.add_frame(model(cam), Rt, img) == st.add_frame(xyz, cam, Rt, img) == int(want.sum()), name
        check_state(cz, st, name)
        np.testing.assert_array_equal(st.frame >= 0, want, err_msg=name)
    # zc = 1e-300 underflows to a float depth of 0: still visible through the z-buffer
    name, cam, Rt, xyz, want = [c for c in CR.edge_cases() if c[0] == "zc = 1e-300"][0]
    run(xyz, [(cam, Rt, CR.padded_image(48, 64, PITCH))], occlusion=True, splat_radius=2)


# -------------------------------------------------------------------------------------------------- distortion
@pytest.mark.parametrize("K,dist", [(CR.K8, CR.DIST8), (CR.K5, CR.DIST5)], ids=["rational8", "radtan5"])
def test_the_rigs_distortion_models(fh, K, dist):
    """the 8-parameter set of undistort_image.py:97 and the 5-parameter one (k4..k6 = 0) at the rig's image size,
    with and without a bound on r2; colours from a 1/16-scale camera of the same model"""
    Rt = CR.script_Rt()
    pts = CR.script_scene(5000, seed=5)
    for r2_max in (np.inf, 1.2):
        cam = CR.Cam(*K, 4096, 2464, dist, r2_max)
        exp = check_projection(fh, pts, cam, Rt)
        assert 500 < exp.valid.sum() < 4500
    small = CR.Cam(K[0] / 16, K[1] / 16, K[2] / 16, K[3] / 16, 256, 154, dist, 1.2)
    run(CR.records(pts, 4), [(small, Rt, CR.padded_image(154, 256, 800, seed=9))])


# --------------------------------------------------------------------------------------------------- occlusion
@pytest.mark.parametrize("radius", [0, 1, 3])
def test_occlusion_hides_the_back_wall(radius):
    """two parallel walls and an oblique one: splats clipped at all four borders, equal float depths in one pixel,
    a probe on each side of the visibility bound (tests/test_colorize_ref.py asserts the scene holds all of these)"""
    cam = CR.occlusion_cam()
    xyz, parts = CR.occlusion_scene(radius, 0.25, 0.125)
    img = CR.padded_image(48, 64, PITCH, seed=radius)
    cz, st = run(CR.records(xyz, 4), [(cam, CR.OCC_RT, img)], occlusion=True, splat_radius=radius, depth_rel=0.25,
                 depth_abs=0.125)
    frame = cz.frame
    pr = CR.project(xyz, cam, CR.OCC_RT)
    assert (frame[parts["back"]][CR.behind_front(pr, parts, radius)] == -1).all()  # the hidden wall stays uncoloured
    assert (frame[parts["front"]] == 0).all()
    assert frame[parts["probe_visible"]][0] == 0 and frame[parts["probe_hidden"]][0] == -1
    # without occlusion the same frame colours the hidden wall too (the reference's behaviour)
    cz2, _ = run(CR.records(xyz, 4), [(cam, CR.OCC_RT, img)])
    assert (cz2.frame[parts["back"]][pr.valid[parts["back"]]] == 0).all()


def test_zero_tolerance_sees_exactly_the_front_of_each_pixel():
    cam = CR.occlusion_cam()
    xyz, _ = CR.occlusion_scene(0, 0.0, 0.0)
    run(xyz, [(cam, CR.OCC_RT, CR.padded_image(48, 64, PITCH))], occlusion=True)
    run(xyz, [(cam, CR.OCC_RT, CR.padded_image(48, 64, PITCH))], occlusion=True, splat_radius=8)


# ------------------------------------------------------------------------------------------------------ frames
def frames3():
    cam = CR.small_cam()
    poses = [POSE, CR.pose([0, 1, 0], -0.4, [0.5, 0.1, 1.0]), CR.pose([1, 0, 1], 0.2, [-0.3, 0.2, 2.5])]
    return cam, poses, [CR.padded_image(48, 64, PITCH, seed=40 + k) for k in range(4)]


@pytest.mark.parametrize("occlusion", [False, True])
def test_frames_accumulate_the_nearest_view(occlusion):
    cam, poses, imgs = frames3()
    rec = CR.records(CR.small_scene(3000, cam, POSE, seed=21), 4)
    params = dict(occlusion=True, splat_radius=1, depth_rel=0.05) if occlusion else {}
    ref = dict(occlusion=occlusion, radius=1 if occlusion else 0, depth_rel=0.05 if occlusion else 0.0)
    # three poses, then the first pose again with another image: every depth ties, the first frame is kept
    seq = [(poses[0], imgs[0]), (poses[1], imgs[1]), (poses[2], imgs[2]), (poses[0], imgs[3])]
    cz = CAM.Colorizer(**params)
    cz.set_cloud(rec)
    st = CR.State(len(rec))
    ups = []
    for Rt, img in seq:
        ups.append(cz.add_frame(model(cam), Rt, img))
        assert ups[-1] == st.add_frame(rec, cam, Rt, img, **ref)
    assert ups[0] > 0 and ups[1] > 0 and ups[3] == 0
    check_state(cz, st)
    assert set(np.unique(st.frame)) == {-1, 0, 1, 2}
    forward = cz.state()
    # reset, then the reverse order: the frame numbers restart and the nearest view still wins
    cz.reset()
    st.reset()
    check_state(cz, st)
    for Rt, img in seq[::-1]:
        assert cz.add_frame(model(cam), Rt, img) == st.add_frame(rec, cam, Rt, img, **ref)
    check_state(cz, st)
    np.testing.assert_array_equal(b64(cz.depth), b64(forward[2]))  # the nearest depth does not depend on the order


def test_bgr_and_rgb_input_give_the_same_colours():
    cam, poses, imgs = frames3()
    rec = CR.records(CR.small_scene(1000, cam, POSE, seed=22), 3)
    a, _ = run(rec, [(cam, poses[0], imgs[0])], bgr=True)
    swapped = np.ascontiguousarray(imgs[0][:, :, ::-1])
    b, _ = run(rec, [(cam, poses[0], swapped)], bgr=False)
    np.testing.assert_array_equal(a.rgb, b.rgb)
    np.testing.assert_array_equal(a.frame, b.frame)


# ----------------------------------------------------------------------------------------------- repeatability
def test_same_sequence_twice_is_identical_and_allocates_nothing():
    cam, poses, imgs = frames3()
    rec = CR.records(CR.small_scene(5000, cam, POSE, seed=23), 4)
    L = _capi.lib()
    cz = CAM.Colorizer(occlusion=True, splat_radius=3, depth_rel=0.02)
    runs = []
    for rep in range(2):
        cz.set_cloud(rec)
        ups = [cz.add_frame(model(cam), poses[0], imgs[0])]
        after_first = L.lio_alloc_count()
        ups += [cz.add_frame(model(cam), Rt, img) for Rt, img in zip(poses[1:], imgs[1:])]
        assert L.lio_alloc_count() == after_first, "a frame of a size seen before allocated"
        if rep == 1:
            assert after_first == settled, "the second pass allocated"
        settled = L.lio_alloc_count()
        runs.append((ups, [a.copy() for a in cz.state()]))
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))


# --------------------------------------------------------------------------------------------- argument errors
def _err(rc, code, *words):
    msg = _capi.lib().lio_last_error().decode()
    assert rc == code, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_argument_errors_name_their_bound(fh):
    L = _capi.lib()
    ARG, STATE = _capi.LIO_ERR_ARG, _capi.LIO_ERR_STATE
    pts = np.zeros((4, 8), np.float32)
    pts[:, 2] = 2.0
    good = model(CR.small_cam())._c()
    Rt = CR.IDENTITY.copy()
    rtp = Rt.ctypes.data_as(dp)
    valid = np.zeros(4, np.uint8)
    vp_ = valid.ctypes.data_as(u8p)
    fp = pts.ctypes.data_as(_capi.fp)

    def proj(cam=good, rt=rtp, p=fp, n=4, stride=3, v=vp_):
        return L.lio_project_points(fh._h, p, n, stride, C.byref(cam) if cam is not None else None, rt, None, None, None, v)

    assert proj() == 0
    _err(proj(cam=None), ARG, "cam is NULL")
    _err(proj(rt=None), ARG, "Rt is NULL")
    _err(proj(p=None), ARG, "pts is NULL")
    _err(proj(v=None), ARG, "valid is NULL")
    _err(proj(n=-1), ARG, "2^31")
    _err(proj(n=1 << 31), ARG, "2^31")
    _err(proj(stride=2), ARG, "3..8")
    _err(proj(stride=9), ARG, "3..8")

    def cam_with(**kw):
        c = model(CR.small_cam())._c()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    _err(proj(cam=cam_with(width=0)), ARG, "at least 1")
    _err(proj(cam=cam_with(height=-3)), ARG, "at least 1")
    _err(proj(cam=cam_with(width=1 << 16, height=1 << 15)), ARG, "below 2^31")
    _err(proj(cam=cam_with(fx=np.nan)), ARG, "intrinsic")
    _err(proj(cam=cam_with(cy=np.inf)), ARG, "intrinsic")
    bad = cam_with()
    bad.dist[5] = np.nan
    _err(proj(cam=bad), ARG, "distortion")
    _err(proj(cam=cam_with(r2_max=np.nan)), ARG, "r2_max")
    _err(proj(cam=cam_with(r2_max=-1.0)), ARG, "r2_max")
    for k in (0, 11):
        rt = Rt.copy()
        rt[k] = np.inf
        _err(proj(rt=rt.ctypes.data_as(dp)), ARG, "pose")

    # the colorizer
    h = C.c_void_p()
    for p, word in ((_capi.ColorizeParams(1, 9, 0, 0, 1), "0..8"), (_capi.ColorizeParams(1, -1, 0, 0, 1), "0..8"),
                    (_capi.ColorizeParams(1, 1, -0.5, 0, 1), "depth_rel"), (_capi.ColorizeParams(1, 1, 0, np.nan, 1), "depth_abs"),
                    (_capi.ColorizeParams(1, 1, np.inf, 0, 1), "finite")):
        _err(L.lio_colorizer_create(0, C.byref(p), C.byref(h)), ARG, word)
        assert not h.value
    _err(L.lio_colorizer_create(0, None, None), ARG, "out is NULL")
    assert L.lio_colorizer_create(0, None, C.byref(h)) == 0
    try:
        _err(L.lio_colorizer_set_params(h, C.byref(_capi.ColorizeParams(0, 9, 0, 0, 1))), ARG, "0..8")
        _err(L.lio_colorizer_set_params(h, None), ARG, "params is NULL")
        img = np.zeros((48, PITCH), np.uint8)
        ip = img.ctypes.data_as(C.c_void_p)
        nup = C.c_int64(-7)
        rgb = np.zeros((4, 3), np.uint8)
        # before set_cloud
        _err(L.lio_colorizer_add_frame(h, C.byref(good), rtp, ip, PITCH, C.byref(nup)), STATE, "lio_colorizer_set_cloud")
        _err(L.lio_colorizer_get(h, rgb.ctypes.data_as(u8p), None, None), STATE, "lio_colorizer_set_cloud")
        _err(L.lio_colorizer_set_cloud(h, None, 4, 3), ARG, "pts is NULL")
        _err(L.lio_colorizer_set_cloud(h, fp, -1, 3), ARG, "2^31")
        _err(L.lio_colorizer_set_cloud(h, fp, 1 << 31, 3), ARG, "2^31")
        _err(L.lio_colorizer_set_cloud(h, fp, 4, 2), ARG, "3..8")
        _err(L.lio_colorizer_set_cloud(h, fp, 4, 9), ARG, "3..8")
        assert L.lio_colorizer_set_cloud(h, fp, 4, 8) == 0
        _err(L.lio_colorizer_add_frame(h, None, rtp, ip, PITCH, C.byref(nup)), ARG, "cam is NULL")
        _err(L.lio_colorizer_add_frame(h, C.byref(good), None, ip, PITCH, C.byref(nup)), ARG, "Rt is NULL")
        _err(L.lio_colorizer_add_frame(h, C.byref(good), rtp, None, PITCH, C.byref(nup)), ARG, "image is NULL")
        _err(L.lio_colorizer_add_frame(h, C.byref(good), rtp, ip, PITCH, None), ARG, "n_updated is NULL")
        _err(L.lio_colorizer_add_frame(h, C.byref(good), rtp, ip, 191, C.byref(nup)), ARG, "pitch", "3 x width")
        _err(L.lio_colorizer_add_frame(h, C.byref(cam_with(width=0)), rtp, ip, PITCH, C.byref(nup)), ARG, "at least 1")
        _err(L.lio_colorizer_add_frame(h, C.byref(cam_with(r2_max=-1.0)), rtp, ip, PITCH, C.byref(nup)), ARG, "r2_max")
        _err(L.lio_colorizer_add_frame(h, C.byref(cam_with(fy=np.nan)), rtp, ip, PITCH, C.byref(nup)), ARG, "intrinsic")
        _err(L.lio_colorizer_get(h, None, None, None), ARG, "rgb is NULL")
        assert nup.value == -7  # nothing ran
        assert L.lio_colorizer_add_frame(h, C.byref(good), rtp, ip, 192, C.byref(nup)) == 0 and nup.value == 4
        assert L.lio_colorizer_get(h, rgb.ctypes.data_as(u8p), None, None) == 0
        # an empty cloud is a cloud
        assert L.lio_colorizer_set_cloud(h, None, 0, 3) == 0
        assert L.lio_colorizer_add_frame(h, C.byref(good), rtp, ip, PITCH, C.byref(nup)) == 0 and nup.value == 0
    finally:
        L.lio_colorizer_destroy(h)
    _err(L.lio_colorizer_reset(None), ARG, "handle is NULL")


def test_python_mirror_rejects_a_wrong_image():
    cam = model(CR.small_cam())
    cz = CAM.Colorizer()
    cz.set_cloud(np.zeros((1, 3), np.float32))
    with pytest.raises(ValueError, match="uint8"):
        cz.add_frame(cam, CR.IDENTITY, np.zeros((48, 64, 3), np.float32))
    with pytest.raises(ValueError, match="shape"):
        cz.add_frame(cam, CR.IDENTITY, np.zeros((64, 48, 3), np.uint8))
    # a non-contiguous view (every second column) is copied, not misread
    wide = CR.padded_image(48, 128, 400, seed=3)
    pts = np.array([[0, 0, 2]], np.float32)
    cz.set_cloud(pts)
    assert cz.add_frame(cam, CR.IDENTITY, wide[:, ::2]) == 1
    np.testing.assert_array_equal(cz.rgb[0], wide[24, 64, ::-1])


def test_colorize_pcd_on_files(tmp_path):
    """colorize_pcd.py on files: a binary PCD in, x y z rgb out, read back with the library's own reader"""
    from lio_gpu import formats

    cam = CR.small_cam()
    rec = CR.records(CR.small_scene(700, cam, POSE, seed=31), 4)
    img = CR.padded_image(48, 64, PITCH, seed=31)
    src, dst = str(tmp_path / "map.pcd"), str(tmp_path / "coloured.pcd")
    formats.write_pcd_binary(src, rec)
    n, coloured = CAM.colorize_pcd(src, img, model(cam), POSE, dst)
    st = CR.State(len(rec))
    assert (n, coloured) == (700, st.add_frame(rec, cam, POSE, img)) and 0 < coloured < n
    codec = formats.CloudCodec()
    out = codec.read_pcd(dst, want=("x", "y", "z", "rgb"))
    codec.close()
    np.testing.assert_array_equal(out[:, :3], rec[:, :3])
    want = np.where((st.frame >= 0)[:, None], st.rgb, np.uint8(128))
    np.testing.assert_array_equal(out[:, 3].view(np.uint32), CAM.pack_rgb(want.astype(np.uint8)).view(np.uint32))
