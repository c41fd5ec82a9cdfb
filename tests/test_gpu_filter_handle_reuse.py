"""One lio_filter handle through every stage that keeps scratch in it — voxel grid, statistical outlier
removal, first-seed radius query, intensity map denoise, Euclidean clusters, DBSCAN, plane segmentation — over
clouds that make every scratch regrow (4097 crosses the 4096-point floor, 6200 is just over 1.5 x 4096, the second
plane call goes from 64 to 1100 hypotheses past the 1024 floor) and shrink again.  A stale arena pointer after
a regrow, or a scratch that one stage leaves in a state the next cannot use, shows as an output that differs
from the same call on a fresh handle: every comparison is bit for bit.  A second round on the same handle must
reproduce the first and allocate nothing (lio_alloc_count).

The arenas that are sized per call — GPS alignment / pair fit, and the one lio_project_points and
lio_undistort_map share — start at 1 MiB (1 048 576 bytes) and grow to max(need, 1.5 x old), so the sizes above
never move them.  OFFLINE is their ladder; each slot is its field rounded up to 256 bytes:
  projection, 33 bytes per point (uv 16, zc 8, pix 8, valid 1), then the map, 26 bytes per pixel (uv 16, sxy 8,
  axy 2), in the same arena, in this order:
    257 points, 33 x 17      9 472 and 15 104 bytes: the 1 MiB floor
    40 000, 320 x 200        1 320 192 > 1 048 576 -> 1 572 864; then 1 664 000 > 1 572 864 -> 2 359 296
    80 000, 480 x 300        2 640 128 > 2 359 296 -> 3 538 944; then 3 744 000 > 3 538 944 -> 5 308 416
    257, 33 x 17             reused
  so each of the two calls regrows the arena twice, right after the other has.
  GPS alignment with n = m, 76 bytes per point and 12 per point and chunk of the nearest-neighbour partials:
    257 (1 chunk)            24 832 bytes: the 1 MiB floor
    20 000 (10 chunks)       3 923 968 > 1 048 576 -> 3 923 968
    40 000 (14 chunks)       9 767 680 > 1.5 x 3 923 968 -> 9 767 680
    257                      reused
  The pair fit (no chunks: 1 523 968 and 3 047 680 bytes) follows the alignment in the arena it has just grown,
  and the georeferencing of the step's cloud grows its plain buffers by 1.5 x."""
import numpy as np
import pytest

from lio_gpu import _capi
from lio_gpu import camera as CAM
from lio_gpu import filters as FL
from lio_gpu import georef as GR
from test_gpu_denoise import make_cloud

pytestmark = pytest.mark.gpu
SIZES = (257, 4097, 6200, 257)
# (points of the cloud, width x height of the map, points of each trajectory)
OFFLINE = ((257, (33, 17), 257), (40000, (320, 200), 20000), (80000, (480, 300), 40000), (257, (33, 17), 257))
DENOISE = dict(seed_thres=8.0, cluster_seed_radius=2.0, denoise_radius=1.0, noise_thres=0.0, mean_k=5, stddev_mul=1.0)
CAMERA = CAM.CameraModel(300.0, 310.0, 322.5, 238.25, 640, 480, dist=(-0.28, 0.07, 0.0008, -0.0004, 0.01))
RT = np.concatenate([np.eye(3).ravel(), [0.5, -0.25, 12.0]])  # the cloud's z in -10 .. 10: every point in front


def make_tracks(n):
    """(gps_xy, slam_xy), n points each: a winding track, and its noisy copy turned, scaled and moved to grid
    coordinates"""
    rng = np.random.default_rng(77 + n)
    s = np.linspace(0.0, 1.0, n)
    slam = np.column_stack([400.0 * s, 60.0 * np.sin(5.0 * s)]) + rng.normal(0, 0.05, (n, 2))
    c, sn = np.cos(0.3), np.sin(0.3)
    gps = 1.02 * slam @ np.array([[c, -sn], [sn, c]]).T + np.array([836000.0, 818000.0]) + rng.normal(0, 0.3, (n, 2))
    return gps, slam


def raw_camera(width, height):
    return CAM.CameraModel(0.8 * width, 0.8 * width, 0.5 * width - 0.25, 0.5 * height + 0.5, width, height,
                           dist=(-0.2, 0.05, 0.001, -0.001, 0.0))


def on_handle(cls, h, *args):
    """a wrapper object of cls working on h's handle, which h keeps owning"""
    w = cls(*args)
    w.close()
    w._h = h._h
    w.close = lambda: None
    return w


class Stages:
    """the wrappers of every stage on one handle, made once (making a wrapper opens and closes a handle of its own)"""

    def __init__(self):
        self.h = h = FL._Handle()
        self.voxel = on_handle(FL.VoxelGrid, h, 0.5)
        self.sor = on_handle(FL.StatisticalOutlierRemoval, h, 5, 1.0)
        self.ece = on_handle(FL.EuclideanClusterExtraction, h, 1.2, 2)
        self.dbscan = on_handle(FL.DBSCAN, h, 1.2, 4)
        self.seg = on_handle(FL.PlaneSegmentation, h)
        self.aligner = on_handle(GR.GpsAligner, h, 3)

    def __call__(self, pts):
        """every stage once; the outputs as a flat list of (name, array)"""
        h, sor, ece, db, seg = self.h, self.sor, self.ece, self.dbscan, self.seg
        out = [("voxel_grid", self.voxel.filter(pts))]
        out += [("sor", sor.filter(pts)), ("sor.distances", sor.distances), ("sor.stats", sor.stats)]
        seed, d2 = FL.radius_first_seed(pts, pts[:64, :3], 0.5, h)
        out += [("seed", seed), ("seed.d2", d2)]
        den, counts = FL.denoise_slam_map(pts, handle=h, **DENOISE)
        out += [("denoise", den), ("denoise.counts", counts)]
        ece.extract(pts)
        out += [("labels", ece.labels), ("indices", ece.indices), ("offsets", ece.offsets), ("aabb", ece.aabb),
                ("cluster.stats", ece.stats)]
        db.fit(pts)
        out += [("dbscan.labels", db.labels_), ("dbscan.core", db.core_sample_indices_), ("dbscan.indices", db.indices),
                ("dbscan.offsets", db.offsets), ("dbscan.aabb", db.aabb), ("dbscan.stats", db.stats)]
        for k in (64, 1100):
            plane, inliers = seg.segment_plane(pts, 0.2, 3, k, seed=7)
            out += [(f"plane{k}", plane), (f"plane{k}.inliers", inliers), (f"plane{k}.counts", seg.counts),
                    (f"plane{k}.sq", seg.sq), (f"plane{k}.mask", seg.mask), (f"plane{k}.refit", seg.refit)]
        return out

    def offline(self, step):
        """the stages whose arenas are sized per call, once, for one step of OFFLINE"""
        n, (width, height), nt = step
        h, pts = self.h, make_cloud("uniform", n)
        gps, slam = make_tracks(nt)
        res = self.aligner.align(gps, slam)
        out = [("align.aligned", res.aligned), ("align.nn", res.nn), ("align.out", res.out)]
        sim = GR.fit_pairs(slam, gps, h)
        out += [("fit.scale", np.float64(sim.scale)), ("fit.R", sim.R), ("fit.t", sim.t)]
        geo, xy = GR.georeference(pts, sim.scale, sim.R, sim.t, origin=(836000.0, 818000.0), return_f64=True, handle=h)
        out += [("georef", geo), ("georef.xy", xy)]
        pr = CAM.project_points(pts, CAMERA, RT, h)
        out += [("project.uv", pr.uv), ("project.zc", pr.zc), ("project.pix", pr.pix), ("project.valid", pr.valid)]
        uv, sxy, axy = CAM.undistort_map(raw_camera(width, height), handle=h)
        out += [("map.uv", uv), ("map.sxy", sxy), ("map.axy", axy)]
        return [(name, np.asarray(a)) for name, a in out]


def assert_same(got, ref, what):
    assert [name for name, _ in got] == [name for name, _ in ref]
    for (name, a), (_, b) in zip(got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {name}"
        assert a.tobytes() == b.tobytes(), f"{what}: {name} differs from a fresh handle's"


@pytest.fixture(scope="module")
def fresh():
    """per size the outputs of a handle that has seen nothing else (computed once, not modified)"""
    ref = {}
    for n in set(SIZES):
        ref[n] = Stages()(make_cloud("uniform", n))
    for step in set(OFFLINE):
        ref[step] = Stages().offline(step)
    return ref


def test_fresh_outputs_exercise_every_stage(fresh):
    by = dict(fresh[6200])
    assert 0 < len(by["voxel_grid"]) < 6200
    assert 0 < len(by["sor"]) < 6200
    assert (by["seed"] >= 0).any() and (by["seed"] < 0).any()
    seeds, segmented, after_sor, denoised, remained = by["denoise.counts"]
    assert seeds > 0 and segmented > 0 and 0 < after_sor <= segmented and remained > 0
    assert by["cluster.stats"][2] > 0 and (by["labels"] < 0).any()
    assert by["dbscan.stats"][2] > 0 and len(by["dbscan.core"]) > 0 and (by["dbscan.labels"] < 0).any()
    assert len(by["plane64.inliers"]) > 0 and len(by["plane1100.inliers"]) >= len(by["plane64.inliers"])
    by = dict(fresh[OFFLINE[2]])
    assert by["align.out"][_capi.GPSALIGN_ITERATIONS] == 3 and len(np.unique(by["align.nn"])) > 1000
    assert abs(by["fit.scale"] - 1.02) < 0.01 and np.abs(by["georef.xy"]).max() < 1000.0
    assert by["project.valid"].any() and not by["project.valid"].all()
    assert (by["project.pix"][by["project.valid"]] >= 0).all() and (by["project.pix"][~by["project.valid"]] == -1).all()
    assert by["map.axy"].max() < 32 and len(np.unique(by["map.sxy"])) > 100


def test_one_handle_through_regrowth_matches_fresh_handles(fresh):
    L = _capi.lib()
    stages = Stages()
    for n in SIZES:
        assert_same(stages(make_cloud("uniform", n)), fresh[n], f"first round, n = {n}")
    for step in OFFLINE:
        assert_same(stages.offline(step), fresh[step], f"first round, offline step {step}")
    a1 = L.lio_alloc_count()
    for n in SIZES:
        assert_same(stages(make_cloud("uniform", n)), fresh[n], f"second round, n = {n}")
    for step in OFFLINE:
        assert_same(stages.offline(step), fresh[step], f"second round, offline step {step}")
    assert L.lio_alloc_count() == a1  # every scratch is at its largest: the second round allocates nothing
