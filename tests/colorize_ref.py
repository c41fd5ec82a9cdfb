"""The contract of lio_project_points / lio_colorizer (include/lio_gpu.h) restated in numpy: elementwise IEEE
double operations in the written order, a float32 depth image, np.minimum.at for the splat.  Also the scene
builders of the colorize tests.  CPU only; tests/test_colorize_ref.py holds it against the script's own
formulation (post_process/colorize_pcd.py:31-63)."""
from dataclasses import dataclass, field

import numpy as np

f64, f32 = np.float64, np.float32
INF_BITS = np.uint32(0x7F800000)

# the script's LiDAR-to-camera extrinsic and intrinsics (colorize_pcd.py:11-21); its image is 4096 x 2464
SCRIPT_R = np.array([[-0.86900, 0.49480, 0.00251], [-0.00257, 0.00055, -1.00000], [-0.49480, -0.86901, 0.00079]], f64)
SCRIPT_T = np.array([0.01791, -0.32026, -0.22659], f64)
SCRIPT_K = (1422.18129, 1421.822766, 2017.285053, 1232.094237)
SCRIPT_SIZE = (4096, 2464)
# the rig's calibrations (undistort_image.py:83-97): fx fy cx cy and k1 k2 p1 p2 k3 [k4 k5 k6]
K5 = (1417.541654, 1418.002061, 2089.904695, 1235.591032)
DIST5 = (-0.2972345646, 0.08469466538, -0.0004248149362, -0.000175399726, 0.0)
K8 = (1419.488223, 1419.783836, 2091.72389, 1231.71474)
DIST8 = (0.4765817545, 0.0267510319, 1.495544387e-07, -2.581193063e-07, 8.833337814e-05, 0.8074516265, 0.1103335164,
         0.001695886702)


@dataclass
class Cam:
    fx: float
    fy: float
    cx: float
    cy: float
    width: int
    height: int
    dist: tuple = ()
    r2_max: float = np.inf

    def __post_init__(self):
        self.dist = tuple(self.dist) + (0.0,) * (8 - len(self.dist))


def script_cam():
    return Cam(*SCRIPT_K, *SCRIPT_SIZE)


def script_Rt():
    return np.concatenate([SCRIPT_R.ravel(), SCRIPT_T])


@dataclass
class Proj:
    u: np.ndarray
    v: np.ndarray
    zc: np.ndarray
    r2: np.ndarray
    valid: np.ndarray
    px: np.ndarray
    py: np.ndarray


def project(pts, cam, Rt):
    """§4g's projection, one numpy operation per operation of the contract"""
    p = np.asarray(pts, f32)
    Rt = np.asarray(Rt, f64).ravel()
    R, t = Rt[:9].reshape(3, 3), Rt[9:]
    x, y, z = p[:, 0].astype(f64), p[:, 1].astype(f64), p[:, 2].astype(f64)
    k1, k2, p1, p2, k3, k4, k5, k6 = (f64(v) for v in cam.dist)
    fx, fy, cx, cy = f64(cam.fx), f64(cam.fy), f64(cam.cx), f64(cam.cy)
    with np.errstate(all="ignore"):
        c = [((R[k, 0] * x + R[k, 1] * y) + R[k, 2] * z) + t[k] for k in range(3)]
        xc, yc, zc = c
        xn, yn = xc / zc, yc / zc
        r2 = xn * xn + yn * yn
        num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2
        rad = num / den
        a1, a2, a3 = (2.0 * xn) * yn, r2 + (2.0 * xn) * xn, r2 + (2.0 * yn) * yn
        xd = xn * rad + (p1 * a1 + p2 * a2)
        yd = yn * rad + (p1 * a3 + p2 * a1)
        u, v = fx * xd + cx, fy * yd + cy
        valid = (zc > 0) & (r2 <= f64(cam.r2_max)) & (u >= 0) & (u < f64(cam.width)) & (v >= 0) & (v < f64(cam.height))
        px = np.where(valid, u, -1.0).astype(np.int32)
        py = np.where(valid, v, -1.0).astype(np.int32)
    return Proj(u, v, zc, r2, valid, px, py)


def depth_image(pr, cam, radius):
    """D: height x width uint32, the minimum of bits((float)zc) over every valid point's clipped splat"""
    D = np.full(cam.height * cam.width, INF_BITS, np.uint32)
    i = np.flatnonzero(pr.valid)
    with np.errstate(all="ignore"):
        zb = pr.zc[i].astype(f32).view(np.uint32)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            qx, qy = pr.px[i] + dx, pr.py[i] + dy
            ok = (qx >= 0) & (qx < cam.width) & (qy >= 0) & (qy < cam.height)
            np.minimum.at(D, qy[ok].astype(np.int64) * cam.width + qx[ok], zb[ok])
    return D.reshape(cam.height, cam.width)


def visible(pr, cam, radius, depth_rel, depth_abs, D=None):
    """valid and zf <= (D[py][px] * (1.0f + depth_rel)) + depth_abs, in float32"""
    D = depth_image(pr, cam, radius) if D is None else D
    vis = np.zeros(len(pr.zc), bool)
    i = np.flatnonzero(pr.valid)
    with np.errstate(all="ignore"):
        zf = pr.zc[i].astype(f32)
        d = D[pr.py[i], pr.px[i]].view(f32)
        bound = (d * (f32(1.0) + f32(depth_rel))) + f32(depth_abs)
    vis[i] = zf <= bound
    return vis


@dataclass
class State:
    n: int
    best_z: np.ndarray = field(init=False)
    rgb: np.ndarray = field(init=False)
    frame: np.ndarray = field(init=False)
    frames: int = 0

    def __post_init__(self):
        self.reset()

    def reset(self):
        self.best_z = np.full(self.n, np.inf, f64)
        self.rgb = np.zeros((self.n, 3), np.uint8)
        self.frame = np.full(self.n, -1, np.int32)
        self.frames = 0

    def add_frame(self, pts, cam, Rt, img, bgr=True, occlusion=False, radius=0, depth_rel=0.0, depth_abs=0.0):
        """one frame of the accumulation; img: height x width x 3 uint8 (any row pitch).  Returns n_updated."""
        pr = project(pts, cam, Rt)
        cand = visible(pr, cam, radius, depth_rel, depth_abs) if occlusion else pr.valid
        rep = np.zeros(self.n, bool)
        rep[cand] = pr.zc[cand] < self.best_z[cand]
        pix = img[pr.py[rep], pr.px[rep]]
        self.rgb[rep] = pix[:, ::-1] if bgr else pix
        self.best_z[rep] = pr.zc[rep]
        self.frame[rep] = self.frames
        self.frames += 1
        return int(np.count_nonzero(rep))

    def colors_float(self):
        out = np.full((self.n, 3), 0.5, f64)
        s = self.frame >= 0
        out[s] = self.rgb[s] / 255.0
        return out


# ---------------------------------------------------------------------------------------------- scene builders
def records(xyz, stride, seed=0):
    """n x stride float32 records, x y z first, the other fields random (they must not matter)"""
    xyz = np.asarray(xyz, f32)
    rec = np.random.default_rng(seed).uniform(-100, 100, (len(xyz), stride)).astype(f32)
    rec[:, :3] = xyz
    return rec


def padded_image(height, width, pitch, seed=0):
    """a random uint8 image as a view into rows of `pitch` bytes; the padding holds other random bytes"""
    buf = np.random.default_rng(seed).integers(0, 256, (height, pitch), dtype=np.uint8)
    return np.lib.stride_tricks.as_strided(buf, (height, width, 3), (pitch, 3, 1))


def script_scene(n, seed=0):
    """points in the LiDAR frame around the script's camera: about half of them land in its 4096 x 2464 image, the
    rest is behind the camera or outside the image"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    # two thirds of the directions pulled towards the optical axis (the third row of R), the rest anywhere
    pull = rng.random(n) < 0.67
    d[pull] = d[pull] * 0.9 + SCRIPT_R[2]
    return (d * rng.uniform(1.5, 60.0, (n, 1))).astype(f32)


def small_cam(**kw):
    """64 x 48 with fx = cx = 32 and fy = cy = 24 (or as given): u = 0 and v = height lie on the rays xn = -1 and
    yn = 1, which float32 coordinates hold exactly"""
    a = dict(fx=32.0, fy=24.0, cx=32.0, cy=24.0, width=64, height=48)
    a.update(kw)
    return Cam(**a)


IDENTITY = np.concatenate([np.eye(3).ravel(), np.zeros(3)])


def small_scene(n, cam, Rt, seed=0):
    """n points spread so that about half of them land in the camera's image"""
    rng = np.random.default_rng(seed)
    Rt = np.asarray(Rt, f64)
    R, t = Rt[:9].reshape(3, 3), Rt[9:]
    z = rng.uniform(-2.0, 12.0, n)
    xn = rng.uniform(-1.4, 1.4, n) * (cam.width / 2) / cam.fx
    yn = rng.uniform(-1.4, 1.4, n) * (cam.height / 2) / cam.fy
    pc = np.stack([xn * z, yn * z, z], 1)
    return ((pc - t) @ R).astype(f32)  # R^T (pc - t)


def rot(axis, ang):
    a = np.asarray(axis, f64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def pose(axis, ang, t):
    return np.concatenate([rot(axis, ang).ravel(), np.asarray(t, f64)])


def edge_cases():
    """(name, cam, Rt, xyz, expected valid) around every term of the validity test, built by back-projecting chosen
    (u, v, zc) through an identity rotation onto rays that float32 holds exactly; each case asserts its own premise"""
    cam = small_cam()
    nb = np.nextafter
    out = []

    def case(name, xyz, want, cam=cam, Rt=IDENTITY, premise=None):
        xyz = np.asarray(xyz, f32).reshape(-1, 3)
        pr = project(xyz, cam, Rt)
        assert premise is None or premise(pr), name
        assert list(pr.valid) == list(want), (name, pr.valid)
        out.append((name, cam, np.asarray(Rt, f64), xyz, np.asarray(want, bool)))

    case("u exactly 0", [[-2, 0, 2], [-1e6, 0.5, 1e6]], [True, True], premise=lambda p: (p.u == 0.0).all() and (p.px == 0).all())
    x = nb(f32(2), f32(0))
    case("u just below width", [[x, 0, 2]], [True], premise=lambda p: 64 - 1e-5 < p.u[0] < 64 and p.px[0] == 63)
    case("u exactly width", [[2, 0, 2]], [False], premise=lambda p: p.u[0] == 64.0)
    Rt = IDENTITY.copy()
    Rt[9] = -6.25e-15
    case("u = -1e-13", [[-2, 0, 2]], [False], Rt=Rt, premise=lambda p: -2e-13 < p.u[0] < 0)
    case("v exactly 0 and just below height", [[0, -2, 2], [0, x, 2]], [True, True],
         premise=lambda p: p.v[0] == 0.0 and p.py[1] == 47)
    case("v = height", [[0, 2, 2]], [False], premise=lambda p: p.v[0] == 48.0)
    case("zc = 0", [[0, 0, 0], [1, 1, 0]], [False, False], premise=lambda p: (p.zc == 0).all())
    case("zc < 0", [[0, 0, -2], [0.5, 0.5, -1e-3]], [False, False])
    Rt = IDENTITY.copy()
    Rt[11] = 1e-300
    case("zc = 1e-300", [[1, 0, 0], [0, 0, 0]], [False, True], Rt=Rt,
         premise=lambda p: (p.zc == 1e-300).all() and not np.isfinite(p.u[0]) and p.u[1] == 32.0)
    case("a NaN coordinate", [[np.nan, 0, 2], [0, np.nan, 2], [0, 0, np.nan], [0, 0, 2]], [False, False, False, True])
    case("an infinite coordinate", [[np.inf, 0, 2], [0, 0, np.inf]], [False, False])
    lim = small_cam(r2_max=0.5)
    y = nb(f32(1), f32(2))
    case("r2 just inside r2_max", [[1, 1, 2], [nb(f32(1), f32(0)), 1, 2]], [True, True], cam=lim,
         premise=lambda p: p.r2[0] == 0.5 and p.r2[1] < 0.5)
    case("r2 just outside r2_max", [[y, 1, 2]], [False], cam=lim,
         premise=lambda p: 0.5 < p.r2[0] < 0.5 + 1e-6 and 0 <= p.u[0] < 64 and 0 <= p.v[0] < 48)
    return out


def occlusion_cam():
    return Cam(fx=40.0, fy=40.0, cx=32.0, cy=24.0, width=64, height=48)


# a rotation of 1e-6 rad about y: along the front wall zc changes by less than a float32 ulp across a pixel, so
# points with equal float depths and different double depths share pixels
OCC_RT = pose([0, 1, 0], 1e-6, [0.01, -0.02, 0.03])


def occlusion_scene(radius, depth_rel, depth_abs):
    """Two parallel walls and an oblique one in front of occlusion_cam() under OCC_RT, and two probe points behind
    the front wall on each side of the visibility bound.  Returns (xyz, parts): parts maps a name to the indices of
    its points.  The back wall overshoots the image on all four sides, so border pixels hold points and their
    splats are clipped."""
    def grid(x0, x1, nx, y0, y1, ny, zf):
        gx, gy = np.meshgrid(np.linspace(x0, x1, nx), np.linspace(y0, y1, ny))
        return np.stack([gx.ravel(), gy.ravel(), zf(gx.ravel())], 1)

    front = grid(-0.6, 0.2, 40, -0.5, 0.5, 50, lambda x: np.full_like(x, 2.0))
    back = grid(-3.4, 3.4, 100, -2.6, 2.6, 76, lambda x: np.full_like(x, 4.0))
    oblique = grid(0.3, 1.2, 45, -0.9, 0.9, 60, lambda x: 3.0 + 0.8 * x)
    xyz = np.concatenate([front, back, oblique]).astype(f32)
    parts, at = {}, 0
    for name, a in (("front", front), ("back", back), ("oblique", oblique)):
        parts[name] = np.arange(at, at + len(a))
        at += len(a)
    cam = occlusion_cam()
    pr = project(xyz, cam, OCC_RT)
    D = depth_image(pr, cam, radius)
    # the probes sit behind the middle of the front wall, in pixel (28, 24)
    px, py = 28, 24
    with np.errstate(all="ignore"):
        bound = (D[py, px].view(f32) * (f32(1.0) + f32(depth_rel))) + f32(depth_abs)
    x, y = (px + 0.5 - cam.cx) / cam.fx, (py + 0.5 - cam.cy) / cam.fy
    near = far = None
    z0 = f32(float(bound) - 0.03)
    zs = [z0]
    for _ in range(16):
        zs.insert(0, np.nextafter(zs[0], f32(0)))
        zs.append(np.nextafter(zs[-1], f32(np.inf)))
    for z in zs:
        p = np.array([[x * float(bound), y * float(bound), z]], f32)
        q = project(p, cam, OCC_RT)
        assert q.valid[0] and (q.px[0], q.py[0]) == (px, py)
        if q.zc[0].astype(f32) <= bound:
            near = p
        elif far is None:
            far = p
    assert near is not None and far is not None
    parts["probe_visible"] = np.array([len(xyz)])
    parts["probe_hidden"] = np.array([len(xyz) + 1])
    return np.concatenate([xyz, near, far]).astype(f32), parts


def behind_front(pr, parts, radius):
    """mask over parts["back"]: the points whose pixel lies inside the front wall's footprint shrunk by the splat
    radius (the front wall covers every pixel of its footprint: 0.4 px between its points)"""
    f, b = parts["front"], parts["back"]
    x0, x1, y0, y1 = pr.px[f].min(), pr.px[f].max(), pr.py[f].min(), pr.py[f].max()
    return pr.valid[b] & (pr.px[b] >= x0 + radius) & (pr.px[b] <= x1 - radius) & (pr.py[b] >= y0 + radius) & \
        (pr.py[b] <= y1 - radius)
