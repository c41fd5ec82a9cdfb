"""GPU normal estimation (lio_estimate_normals, lio_gpu.filters.NormalEstimation) against tests/normals_ref.py, the
numpy restatement of its contract.  Every comparison is exact: normals and curvature as float bits (NaN where there
is no normal), counts and stats."""
import numpy as np
import pytest

import normals_ref as NR
from lio_gpu import _capi
from lio_gpu import filters as FL

pytestmark = pytest.mark.gpu
f32 = np.float32

# k alone (k > n included at the small sizes), the radius alone, the hybrid search
MODES = (dict(k=3), dict(k=16), dict(k=255), dict(radius=0.5, k=0), dict(radius=0.5, k=30))


@pytest.fixture(scope="module")
def ne():
    h = FL.NormalEstimation()
    yield h
    h.close()


def check(ne, pts, viewpoint=None, **mode):
    ne.k, ne.radius = mode.get("k", 0), mode.get("radius", 0.0)
    got = ne.compute(pts, viewpoint)
    ref = NR.estimate_normals(pts, ne.radius, ne.k, viewpoint)
    assert np.array_equal(ne.counts, ref["counts"]), mode
    assert np.array_equal(got.view(np.uint32), ref["normals"].view(np.uint32)), mode
    assert np.array_equal(ne.curvature.view(np.uint32), ref["curvature"].view(np.uint32)), mode
    assert np.array_equal(ne.stats, ref["stats"]), (mode, ne.stats, ref["stats"])
    return ref


def plane_cloud(n, seed=1, offset=(100.0, -50.0, 3.0), stride=3, density=37.5):
    """a noisy plane of about `density` points per square metre (the 600-point plane of test_normals_ref.py at
    n = 600), with attribute columns behind x y z"""
    rng = np.random.default_rng(seed)
    half = max(np.sqrt(n / density) / 2, 1e-3)
    p = np.stack([rng.uniform(-half, half, n), rng.uniform(-half, half, n), rng.normal(0, 0.01, n)], axis=1)
    out = rng.uniform(-1, 1, (n, stride)).astype(f32)
    out[:, :3] = (p + np.array(offset)).astype(f32)
    return out


@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 4097])
def test_sizes_modes_strides(ne, n):
    for t, mode in enumerate(MODES):
        pts = plane_cloud(n, seed=n + t, stride=3 + (n + t) % 6)
        ref = check(ne, pts, **mode)
        if n >= 255 and mode.get("k", 0) in (0, 16, 30):
            assert ref["stats"][1] > n // 2  # the case computes normals, not NaN


def test_size_20001(ne):
    pts = plane_cloud(20001, seed=7, stride=4)
    for mode in (dict(k=16), dict(radius=0.5, k=0), dict(radius=0.5, k=30)):
        ref = check(ne, pts, **mode)
        assert ref["stats"][1] > 19000


@pytest.mark.parametrize("n", [3, 65, 257, 4097])
def test_non_finite_rows(ne, n):
    pts = plane_cloud(n, seed=n, stride=5)
    pts[0, 0] = np.nan
    pts[n - 1, 2] = np.inf
    pts[n // 2::97, 1] = -np.inf
    pts[1::2, 4] = np.nan  # an attribute is not a coordinate
    for mode in (dict(k=16), dict(radius=0.5, k=0), dict(radius=0.5, k=30)):
        ref = check(ne, pts, **mode)
        assert ref["counts"][0] == 0 and ref["counts"][n - 1] == 0 and ref["stats"][0] < n
    check(ne, np.full((70, 3), np.nan, f32), k=5)  # no finite point at all


def lattice_cloud():
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3)
    return (0.25 * g).astype(f32)


def test_lattice_ties(ne):
    pts = lattice_cloud()
    for mode in (dict(k=10), dict(k=27), dict(radius=0.5, k=0), dict(radius=0.5, k=10), dict(radius=0.25, k=0),
                 dict(radius=0.25, k=5)):
        check(ne, pts, **mode)
    check(ne, pts[np.random.default_rng(3).permutation(len(pts))], k=10)  # the index rule under another order
    ne.k, ne.radius = 0, 0.25
    ne.compute(pts)
    assert (ne.counts == 1).all()  # the radius test is strict


def test_degenerate_clouds(ne):
    dup = np.tile(np.array([[1.5, -2.0, 0.25]], f32), (5, 1))
    for mode in (dict(k=5), dict(k=3), dict(radius=0.5, k=0), dict(radius=0.5, k=4)):
        ref = check(ne, dup, **mode)
        assert ref["stats"][3] == 5
    many = np.concatenate([np.tile(np.array([[0.5, 0.5, 0.5]], f32), (300, 1)), plane_cloud(400, offset=(0, 0, 0))])
    for mode in (dict(k=16), dict(k=255), dict(radius=0.5, k=0), dict(radius=0.5, k=30)):
        check(ne, many, **mode)
    t = np.linspace(-1, 1, 21)
    line = (t[:, None] * (np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5]))[None, :] + [3.0, 4.0, 5.0]).astype(f32)
    for mode in (dict(k=7), dict(radius=0.45, k=0)):
        check(ne, line, **mode)
    axis = np.zeros((40, 3), f32)
    axis[:, 0] = np.arange(40) * 0.125  # exactly collinear on an axis: a zero eigenvalue twice over
    check(ne, axis, k=9)
    planar = plane_cloud(2000, seed=2, offset=(0, 0, 0))
    planar[:, 2] = 0.25  # z constant: the smallest eigenvalue is exactly 0
    for mode in (dict(k=16), dict(radius=0.5, k=0), dict(radius=0.5, k=30)):
        ref = check(ne, planar, **mode)
        nz = ref["normals"][ref["counts"] >= 3, 2]
        assert (nz == 1.0).all()


def test_dense_cell_overflows_the_candidate_buffer(ne):
    """1500 points within 5 cm among 4097: one cell of the density grid holds more than the 512 candidate keys of a
    wave, so the buffer is sorted and cut (repeatedly) and filtered against the running bound; with the radius
    alone every one of the 1500 has a neighbourhood of about 1500"""
    rng = np.random.default_rng(11)
    pts = plane_cloud(4097, seed=5, offset=(0, 0, 0), stride=4)
    pts[1000:2500, :3] = (rng.normal(0, 0.012, (1500, 3)) + [0.3, 0.3, 0.0]).astype(f32)
    for mode in (dict(k=3), dict(k=50), dict(k=255), dict(radius=0.5, k=0), dict(radius=0.5, k=255)):
        ref = check(ne, pts, **mode)
    assert check(ne, pts, radius=0.5, k=0)["counts"].max() >= 1500


def test_far_clusters(ne):
    """clusters far apart: a query's k-th neighbour may lie many empty cells away, and with a radius the walk stops
    at it instead"""
    rng = np.random.default_rng(13)
    centres = rng.uniform(-300, 300, (12, 3))
    sizes = [2, 3, 5, 9, 17, 40, 100, 200, 400, 800, 1200, 1321]
    pts = np.concatenate([c + rng.normal(0, 0.2, (s, 3)) for c, s in zip(centres, sizes)]).astype(f32)
    pts = pts[rng.permutation(len(pts))]
    assert len(pts) == 4097
    for mode in (dict(k=3), dict(k=16), dict(k=255), dict(radius=0.5, k=0), dict(radius=0.5, k=30)):
        check(ne, pts, **mode)


def test_large_offsets(ne):
    for off in ((8e5, -8e5, 300.0), (-8e5, 8e5, -8e5)):
        pts = plane_cloud(4097, seed=17, offset=off)
        for mode in (dict(k=16), dict(radius=0.5, k=0), dict(radius=0.5, k=30)):
            ref = check(ne, pts, **mode)
            assert ref["stats"][1] > 3000


def knn_cell_edge(pts, k):
    """lio_normals.hip's grid for a k search — dn_build_grid with target k — restated: the largest of the volume,
    face and edge density estimates (float64, cast to float32) and the grid dimensions it gives; grown=True when
    the grid would exceed n + 64 cells, where the library enlarges the edge"""
    xyz = np.asarray(pts, f32)[:, :3]
    lo, hi = xyz.min(0), xyz.max(0)
    ex, ey, ez = (hi.astype(np.float64) - lo.astype(np.float64))
    n, t = np.float64(len(pts)), np.float64(k)
    c3 = np.cbrt(ex * ey * ez * t / (27.0 * n))
    c2 = np.sqrt(max(ex * ey, ey * ez, ex * ez) * t / (9.0 * n))
    c1 = max(ex, ey, ez) * t / (3.0 * n)
    cell = f32(max(c3, c2, c1))
    dims = np.floor((hi - lo) * (f32(1.0) / cell)).astype(np.int64) + 1
    return cell, lo, dims, int(np.prod(dims)) > len(pts) + 64


@pytest.mark.parametrize("scale,shift", [(1.0, 0.0), (0.5, 3.0)])
def test_points_on_cell_faces(ne, scale, shift):
    """The cell-face construction of test_sor_points_on_cell_faces for this search's grid (target k): a 9 x 9 x 9
    lattice of spacing `scale` spans 8 scale, and with n = 8^3 k / 27 = 1024 points at k = 54 the volume estimate
    is `scale` exactly; 729 cells, under the n + 64 cap.  Every lattice point lies on cell faces on all three axes —
    what the stop rule and its margin have to get right, now with the strict comparison at tied distances — and the
    rest sits one float step either side of a face, or anywhere inside."""
    n, k = 1024, 54
    rng = np.random.default_rng(n + k)
    g = np.stack(np.meshgrid(*[np.arange(9)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(f32)
    extra = rng.uniform(0, 8, (n - 729, 3)).astype(f32)
    near = rng.integers(1, 8, (len(extra) // 2, 3)).astype(f32)
    extra[: len(near)] = near
    xyz = (np.concatenate([g, extra]) * f32(scale) + f32(shift)).astype(f32)  # exact: small dyadic numbers
    side = np.where(rng.random(near.shape) < 0.5, f32(-99), f32(99)).astype(f32)
    xyz[729:729 + len(near)] = np.nextafter(xyz[729:729 + len(near)], side)
    pts = xyz[rng.permutation(n)]
    cell, lo, dims, grown = knn_cell_edge(pts, k)
    assert cell == f32(scale) and not grown and tuple(dims) == (9, 9, 9)
    kk = (pts - lo) * (f32(1.0) / cell)
    assert (kk == np.floor(kk)).all(1).sum() >= 729
    check(ne, pts, k=k)
    check(ne, pts, k=k, radius=2.5 * scale)
    check(ne, pts, k=7)


def test_orientation(ne):
    pts = plane_cloud(4097, seed=19, stride=4)
    rng = np.random.default_rng(19)
    one = np.array([100.0, -50.0, -10.0], f32)  # below the plane: every normal turns down
    per_point = (pts[:, :3] + rng.normal(0, 5, (len(pts), 3))).astype(f32)
    per_point[::50] = pts[::50, :3]  # the viewpoint at the point itself: s = 0 flips nothing
    per_point[7::300, 0] = np.nan    # a NaN s flips nothing
    for mode in (dict(k=16), dict(radius=0.5, k=0), dict(radius=0.5, k=30)):
        none = check(ne, pts, **mode)
        down = check(ne, pts, one, **mode)
        each = check(ne, pts, per_point, **mode)
        ok = ~np.isnan(none["normals"][:, 0])
        assert (none["normals"][ok, 2] > 0).all() and (down["normals"][ok, 2] < 0).all()
        flipped = (each["normals"][ok] != none["normals"][ok]).any(axis=1)
        assert 0.2 < flipped.mean() < 0.8
        assert np.array_equal(each["curvature"], none["curvature"], equal_nan=True)
    with pytest.raises(ValueError):
        ne.compute(pts, np.zeros((5, 3), f32))


def test_handle_reuse_repeatability_and_alloc_count():
    L = _capi.lib()
    h = FL.NormalEstimation()
    small, large = plane_cloud(700, seed=23), plane_cloud(9000, seed=29, stride=6)
    vps = np.zeros((9000, 3), f32)
    runs = []
    for pts, vp, mode in ((small, None, dict(k=16)), (large, vps, dict(radius=0.5, k=30)), (small, None, dict(radius=0.5, k=0)),
                          (large, None, dict(k=255)), (small, vps[0], dict(k=16))):
        check(h, pts, vp, **mode)
    a1 = L.lio_alloc_count()
    for _ in range(2):  # one size again, in every mode: nothing is allocated, and the bits repeat
        for mode in (dict(k=16), dict(radius=0.5, k=0), dict(radius=0.5, k=30)):
            h.k, h.radius = mode["k"], mode.get("radius", 0.0)
            nrm = h.compute(large, vps)
            runs.append((nrm.tobytes(), h.curvature.tobytes(), h.counts.tobytes(), h.stats.tobytes()))
    assert L.lio_alloc_count() == a1
    assert runs[:3] == runs[3:]
    # the other filters of the handle's kind still work beside it (one scratch for the grid)
    sor = FL.StatisticalOutlierRemoval(20, 2.0)
    kept = sor.filter(small)
    sor.close()
    assert 0 < len(kept) <= len(small)
    h.close()


def test_with_normals_round_trip(ne):
    pts = plane_cloud(300, seed=31, stride=4)
    ne.k, ne.radius = 16, 0.0
    nrm = ne.compute(pts)
    rows = FL.with_normals(pts, nrm, ne.curvature)
    assert rows.shape == (300, 8) and np.array_equal(rows[:, 4:7], nrm) and np.array_equal(rows[:, 7], ne.curvature)
