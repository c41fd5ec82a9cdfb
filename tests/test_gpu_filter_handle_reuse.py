"""One lio_filter handle through every stage that keeps scratch in it — voxel grid, statistical outlier
removal, first-seed radius query, intensity map denoise, Euclidean clusters, plane segmentation — over clouds
that make every scratch regrow (4097 crosses the 4096-point floor, 6200 is just over 1.5 x 4096, the second
plane call goes from 64 to 1100 hypotheses past the 1024 floor) and shrink again.  A stale arena pointer after
a regrow, or a scratch that one stage leaves in a state the next cannot use, shows as an output that differs
from the same call on a fresh handle: every comparison is bit for bit.  A second round on the same handle must
reproduce the first and allocate nothing (lio_alloc_count)."""
import numpy as np
import pytest

from lio_gpu import _capi
from lio_gpu import filters as FL
from test_gpu_denoise import make_cloud

pytestmark = pytest.mark.gpu
SIZES = (257, 4097, 6200, 257)
DENOISE = dict(seed_thres=8.0, cluster_seed_radius=2.0, denoise_radius=1.0, noise_thres=0.0, mean_k=5, stddev_mul=1.0)


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
        self.seg = on_handle(FL.PlaneSegmentation, h)

    def __call__(self, pts):
        """every stage once; the outputs as a flat list of (name, array)"""
        h, sor, ece, seg = self.h, self.sor, self.ece, self.seg
        out = [("voxel_grid", self.voxel.filter(pts))]
        out += [("sor", sor.filter(pts)), ("sor.distances", sor.distances), ("sor.stats", sor.stats)]
        seed, d2 = FL.radius_first_seed(pts, pts[:64, :3], 0.5, h)
        out += [("seed", seed), ("seed.d2", d2)]
        den, counts = FL.denoise_slam_map(pts, handle=h, **DENOISE)
        out += [("denoise", den), ("denoise.counts", counts)]
        ece.extract(pts)
        out += [("labels", ece.labels), ("indices", ece.indices), ("offsets", ece.offsets), ("aabb", ece.aabb),
                ("cluster.stats", ece.stats)]
        for k in (64, 1100):
            plane, inliers = seg.segment_plane(pts, 0.2, 3, k, seed=7)
            out += [(f"plane{k}", plane), (f"plane{k}.inliers", inliers), (f"plane{k}.counts", seg.counts),
                    (f"plane{k}.sq", seg.sq), (f"plane{k}.mask", seg.mask), (f"plane{k}.refit", seg.refit)]
        return out


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
    return ref


def test_fresh_outputs_exercise_every_stage(fresh):
    by = dict(fresh[6200])
    assert 0 < len(by["voxel_grid"]) < 6200
    assert 0 < len(by["sor"]) < 6200
    assert (by["seed"] >= 0).any() and (by["seed"] < 0).any()
    seeds, segmented, after_sor, denoised, remained = by["denoise.counts"]
    assert seeds > 0 and segmented > 0 and 0 < after_sor <= segmented and remained > 0
    assert by["cluster.stats"][2] > 0 and (by["labels"] < 0).any()
    assert len(by["plane64.inliers"]) > 0 and len(by["plane1100.inliers"]) >= len(by["plane64.inliers"])


def test_one_handle_through_regrowth_matches_fresh_handles(fresh):
    L = _capi.lib()
    stages = Stages()
    for n in SIZES:
        assert_same(stages(make_cloud("uniform", n)), fresh[n], f"first round, n = {n}")
    a1 = L.lio_alloc_count()
    for n in SIZES:
        assert_same(stages(make_cloud("uniform", n)), fresh[n], f"second round, n = {n}")
    assert L.lio_alloc_count() == a1  # every scratch is at its largest: the second round allocates nothing
