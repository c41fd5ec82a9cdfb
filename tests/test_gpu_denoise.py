"""GPU checks of the statistical outlier removal, the first-seed radius query and the intensity map denoise
(lio_denoise.hip) against numpy restatements written here — float32 arithmetic in the stated order, brute
force over all pairs, sequential float64 sums (np.cumsum).  Every comparison is bit-exact.

Squared distance: float32 ((dx*dx + dy*dy) + dz*dz).  SOR [U: PCL 1.10]: the mean_k + 1 smallest per finite
point, the first dropped, float64 square roots added in ascending order, / mean_k, cast to float32; the
threshold loop in index order with the float32 product d*d.  Radius query [U: FLANN]: d2 < float32(r*r) strict,
lowest seed index.  denoise_slam_map: the reference's loops (fast_lio_sam.cpp:941-1008, 575-646) written
literally — seed loop in order, radius hits in ascending distance (ties by index: the library's contract),
mark-by-zeroing — against the library's set formulation.
"""
import numpy as np
import pytest

from lio_gpu import _capi
from lio_gpu import filters as FL

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
NS = (1, 2, 63, 64, 65, 257, 4097)
MEAN_KS = (1, 5, 50, 200, 255)


# ------------------------------------------------------------------ references
def sqdist3(a, b):
    """float32 ((dx*dx + dy*dy) + dz*dz) of every row of a against every row of b"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def sorted_d2(pts, kmax=256):
    """finite rows' indices and, per finite row, its min(nf, kmax) smallest squared distances, ascending"""
    xyz = np.asarray(pts, f32)[:, :3]
    fin = np.flatnonzero(np.isfinite(xyz).all(1))
    q = xyz[fin]
    keep = min(len(fin), kmax)
    S = np.empty((len(fin), keep), f32)
    for i0 in range(0, len(fin), 512):
        D = sqdist3(q[i0:i0 + 512], q)
        if keep < D.shape[1]:
            D = np.partition(D, keep - 1, axis=1)[:, :keep]
        S[i0:i0 + 512] = np.sort(D, axis=1)
    return fin, S


def ref_sor_distances(pts, mean_k, cache=None):
    """(distances, counted)"""
    n = len(pts)
    fin, S = cache if cache is not None else sorted_d2(pts)
    dist, counted = np.zeros(n, f32), np.zeros(n, bool)
    if len(fin) >= mean_k + 1:
        roots = np.sqrt(S[:, 1:mean_k + 1].astype(f64))
        dist[fin] = (np.cumsum(roots, axis=1)[:, -1] / f64(mean_k)).astype(f32)
        counted[fin] = True
    return dist, counted


def ref_sor_threshold(dist, counted, stddev_mul):
    with np.errstate(all="ignore"):
        nv = f64(counted.sum())
        s = np.cumsum(dist.astype(f64))[-1] if len(dist) else f64(0)
        sq = np.cumsum((dist * dist).astype(f64))[-1] if len(dist) else f64(0)
        mean = s / nv
        var = (sq - s * s / nv) / (nv - f64(1))
        sd = np.sqrt(var)
        return np.array([mean, sd, mean + f64(stddev_mul) * sd, nv], f64)


def ref_sor_filter(pts, mean_k, stddev_mul, negative=False, cache=None):
    dist, counted = ref_sor_distances(pts, mean_k, cache)
    stats = ref_sor_threshold(dist, counted, stddev_mul)
    d = dist.astype(f64)
    with np.errstate(invalid="ignore"):
        removed = (d <= stats[2]) if negative else (d > stats[2])
    return np.asarray(pts, f32)[~removed], dist, stats


def ref_radius_first_seed(pts, seeds, radius):
    pts, seeds = np.asarray(pts, f32), np.asarray(seeds, f32).reshape(-1, 3)
    r = f32(radius)
    r2 = f32(f64(r) * f64(r))
    seed, d2 = np.full(len(pts), -1, np.int32), np.zeros(len(pts), f32)
    if len(seeds) == 0 or len(pts) == 0:
        return seed, d2
    with np.errstate(invalid="ignore"):
        D = sqdist3(pts[:, :3], seeds)
        hit = (D < r2) & np.isfinite(pts[:, :3]).all(1)[:, None] & np.isfinite(seeds).all(1)[None, :]
    first = hit.argmax(1)
    has = hit.any(1)
    seed[has] = first[has]
    d2[has] = D[has, first[has]]
    return seed, d2


def ref_denoise_slam_map(pts, seed_thres, cluster_seed_radius, denoise_radius, noise_thres, mean_k, stddev_mul):
    """FastLioSam::denoise_slam_map, its loops as written (kd-tree radius search = brute force, hits in
    ascending distance then index)"""
    pts = np.asarray(pts, f32)
    inten = pts[:, 3].copy()
    fin = np.isfinite(pts[:, :3]).all(1)
    seeds = np.flatnonzero(inten > f32(seed_thres))

    def radius_hits(cloud_xyz, cloud_fin, s, r):
        r32 = f32(r)
        r2 = f32(f64(r32) * f64(r32))
        with np.errstate(invalid="ignore"):
            d2 = sqdist3(pts[s:s + 1, :3], cloud_xyz)[0]
            hit = np.flatnonzero(cloud_fin & (d2 < r2))
        return hit[np.lexsort((hit, d2[hit]))]

    segmented = []
    for s in seeds:  # "for (const auto& pt : seed_points)"
        if not fin[s]:
            continue
        for j in radius_hits(pts[:, :3], fin, s, cluster_seed_radius):
            if inten[j] == 0.0:
                continue
            segmented.append(j)
            inten[j] = 0.0
    remained = pts[inten != 0.0]
    seg = pts[np.asarray(segmented, np.int64)] if segmented else np.zeros((0, 4), f32)
    sor = ref_sor_filter(seg, mean_k, f64(f32(stddev_mul)))[0] if len(seg) else seg
    sor_i = sor[:, 3].copy()
    sor_fin = np.isfinite(sor[:, :3]).all(1)
    for s in seeds:  # denoise_map's intensity loop
        if not fin[s] or not len(sor):
            continue
        for j in radius_hits(sor[:, :3], sor_fin, s, denoise_radius):
            if sor_i[j] == 0.0:
                continue
            if sor_i[j] < f32(noise_thres):
                sor_i[j] = 0.0
    denoised = sor[sor_i != 0.0]
    counts = np.array([len(seeds), len(seg), len(sor), len(denoised), len(remained)], np.int64)
    return np.concatenate([denoised, remained]), counts


# ---------------------------------------------------------------------- inputs
def make_cloud(kind, n, seed=0):
    rng = np.random.default_rng(1000 * seed + n)
    if kind == "uniform":
        p = rng.uniform(-10, 10, (n, 4))
    elif kind == "clustered":  # 20 clusters of sigma = 1 cm in a 50 m box
        c = rng.uniform(0, 50, (20, 3))
        p = np.concatenate([c[rng.integers(0, 20, n)] + rng.normal(0, 0.01, (n, 3)), rng.uniform(0, 1, (n, 1))], 1)
    elif kind == "dense":  # two clusters of 1500 points, each inside one grid cell, in a sparse background
        c = np.array([[5.0, 5.0, 5.0], [31.0, 40.0, 12.0]])
        who = np.minimum(np.arange(n) // 1500, 2)
        p = np.where((who < 2)[:, None], c[np.minimum(who, 1)] + rng.normal(0, 0.01, (n, 3)), rng.uniform(0, 50, (n, 3)))
        p = np.concatenate([p, rng.uniform(0, 1, (n, 1))], 1)
    elif kind == "lattice":  # integer coordinates: every distance many times (ties)
        m = int(round(n ** (1 / 3)))
        g = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
        p = np.concatenate([g, np.ones((len(g), 1))], 1)
    elif kind == "duplicates":
        p = np.tile([[1.5, -2.25, 0.75, 7.0]], (n, 1))
    else:
        raise ValueError(kind)
    return p.astype(f32)


def make_scene(seed=3):
    """20 000 PointXYZI: a ground plane (intensity 500-2000), two 1 m signboards above 2800 with a halo of
    2000-2700 around them, and a sprinkle of intensity-0 points"""
    rng = np.random.default_rng(seed)
    ground = np.column_stack([rng.uniform(-20, 20, (17000, 2)), rng.normal(0, 0.02, 17000), rng.uniform(500, 2000, 17000)])
    parts = [ground]
    for cx, cy in ((3.0, 4.0), (-6.0, 1.5)):
        u, v = rng.uniform(-0.5, 0.5, 600), rng.uniform(1.0, 2.0, 600)
        parts.append(np.column_stack([cx + u, cy + rng.normal(0, 0.005, 600), v, rng.uniform(2801, 3500, 600)]))
        hu, hv = rng.uniform(-0.7, 0.7, 500), rng.uniform(0.8, 2.2, 500)
        parts.append(np.column_stack([cx + hu, cy + rng.normal(0, 0.06, 500), hv, rng.uniform(2000, 2700, 500)]))
    zero = np.column_stack([rng.uniform(-8, 8, (800, 2)), rng.uniform(0, 2.5, 800), np.zeros(800)])
    pts = np.concatenate(parts + [zero]).astype(f32)
    return pts[rng.permutation(len(pts))]


SHIPPED = dict(seed_thres=2800.0, cluster_seed_radius=0.1, denoise_radius=0.5, noise_thres=2700.0, mean_k=200,
               stddev_mul=0.2)  # config.yaml:32-42
SOURCE_DEFAULTS = dict(SHIPPED, mean_k=50, stddev_mul=1.0, cluster_seed_radius=1.0)  # fast_lio_sam.cpp:89-96


@pytest.fixture(scope="module")
def sor():
    return FL.StatisticalOutlierRemoval()


@pytest.fixture(scope="module")
def handle():
    return FL._Handle()


def check_sor(sor, pts, mean_ks, muls=(0.2, 1.0)):
    cache = sorted_d2(pts)
    for k in mean_ks:
        sor.setMeanK(k)
        for mul in muls:
            for neg in (False, True):
                sor.setStddevMulThresh(mul)
                sor.setNegative(neg)
                got = sor.filter(pts)
                kept, dist, stats = ref_sor_filter(pts, k, mul, neg, cache)
                np.testing.assert_array_equal(sor.distances, dist, err_msg=f"k={k}")
                np.testing.assert_array_equal(sor.stats, stats, err_msg=f"k={k} mul={mul}")
                np.testing.assert_array_equal(got, kept, err_msg=f"k={k} mul={mul} neg={neg}")
        # negative is the complement wherever a threshold exists; without one both keep everything
        sor.setNegative(False)
        a = len(sor.filter(pts))
        sor.setNegative(True)
        b = len(sor.filter(pts))
        assert a + b == (len(pts) if np.isfinite(sor.stats[2]) else 2 * len(pts))


# ----------------------------------------------------------------------- tests
@pytest.mark.parametrize("n", NS)
def test_sor_uniform(sor, n):
    """every n x mean_k, mean_k + 1 > n included (all distances 0, nothing counted, every point kept)"""
    pts = make_cloud("uniform", n)
    check_sor(sor, pts, MEAN_KS)
    if n < 256:
        sor.setMeanK(255)
        sor.setNegative(False)
        np.testing.assert_array_equal(sor.filter(pts), pts)
        assert not sor.distances.any() and sor.stats[3] == 0


@pytest.mark.parametrize("n", NS)
def test_sor_nan_rows(sor, n):
    pts = make_cloud("uniform", n, seed=1)
    pts[::97, 1] = np.nan
    check_sor(sor, pts, MEAN_KS)


def test_sor_clustered(sor):
    """clusters far apart: a query's neighbours beyond its own cluster lie many empty cells away"""
    check_sor(sor, make_cloud("clustered", 4097), MEAN_KS)


def test_sor_dense_cells_overflow_the_candidate_buffer(sor):
    """1500 points in one cell: more than the 1024 candidates a wave holds, so the buffer is cut to the
    mean_k + 1 smallest and filtered against the running bound (nothing truncated: still bit-exact)"""
    check_sor(sor, make_cloud("dense", 4097), (1, 50, 255), muls=(0.2,))


def test_sor_duplicates_and_lattice(sor):
    pts = make_cloud("duplicates", 300)
    sor.setMeanK(200)
    sor.setNegative(False)
    sor.setStddevMulThresh(0.2)
    np.testing.assert_array_equal(sor.filter(pts), pts)
    assert not sor.distances.any() and sor.stats[3] == 300
    check_sor(sor, pts, (200, 255), muls=(0.2,))
    check_sor(sor, make_cloud("lattice", 4096), (5, 26, 50, 200), muls=(1.0,))
    planar = make_cloud("uniform", 2000, seed=2)
    planar[:, 2] = 0.25
    check_sor(sor, planar, (5, 200), muls=(1.0,))


def sor_cell_edge(pts, mean_k):
    """lio_denoise.hip's cell edge for the SOR grid, restated: the largest of the volume, face and edge density
    estimates (float64, cast to float32), and the grid dimensions it gives; grown=True when the grid would
    exceed n + 64 cells, where the library enlarges the edge"""
    xyz = np.asarray(pts, f32)[:, :3]
    xyz = xyz[np.isfinite(xyz).all(1)]
    lo, hi = xyz.min(0), xyz.max(0)
    ex, ey, ez = (hi.astype(f64) - lo.astype(f64))
    n, t = f64(len(pts)), f64(mean_k + 1)
    c3 = np.cbrt(ex * ey * ez * t / (27.0 * n))
    c2 = np.sqrt(max(ex * ey, ey * ez, ex * ez) * t / (9.0 * n))
    c1 = max(ex, ey, ez) * t / (3.0 * n)
    cell = f32(max(c3, c2, c1))
    inv = f32(1.0) / cell
    dims = np.floor((hi - lo) * inv).astype(np.int64) + 1
    return cell, lo, dims, int(np.prod(dims)) > len(pts) + 64


@pytest.mark.parametrize("n,mean_k,scale,shift", [(1024, 53, 1.0, 0.0), (4096, 215, 1.0, -4.0), (1024, 53, 0.5, 3.0)])
def test_sor_points_on_cell_faces(sor, n, mean_k, scale, shift):
    """Points on integer multiples of the cell size.  The cloud is built so that the library's edge formula
    gives a power of two without growth: a 9 x 9 x 9 lattice of spacing `scale` spans an extent of 8 scale,
    and with t = mean_k + 1 and n = 8^3 t / 27 points the volume estimate is cbrt(8^3 scale^3 t / (27 n)) =
    scale exactly; the grid is 9^3 = 729 cells, under the n + 64 cap.  Every lattice point then lies on cell
    faces (o + k cell on all three axes) — what the stop rule and its margin have to get right — and the
    rest of the cloud sits one float step either side of a face, or anywhere inside."""
    rng = np.random.default_rng(n + mean_k)
    g = np.stack(np.meshgrid(*[np.arange(9)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(f32)
    extra = rng.uniform(0, 8, (n - 729, 3)).astype(f32)
    near = rng.integers(1, 8, (len(extra) // 2, 3)).astype(f32)  # on faces here, moved one float step below
    extra[: len(near)] = near
    xyz = (np.concatenate([g, extra]) * f32(scale) + f32(shift)).astype(f32)  # exact: small dyadic numbers
    side = np.where(rng.random(near.shape) < 0.5, f32(-99), f32(99)).astype(f32)
    xyz[729:729 + len(near)] = np.nextafter(xyz[729:729 + len(near)], side)  # ... either side of the face
    pts = np.column_stack([xyz, np.ones(n, f32)]).astype(f32)[rng.permutation(n)]
    cell, lo, dims, grown = sor_cell_edge(pts, mean_k)
    assert cell == f32(scale) and not grown and tuple(dims) == (9, 9, 9)
    k = (pts[:, :3] - lo) * (f32(1.0) / cell)  # the library's float cell coordinate before floor
    on_faces = (k == np.floor(k)).all(1)
    assert on_faces.sum() >= 729
    off = np.abs(k - np.rint(k))
    assert ((off > 0) & (off < 1e-5)).any(1).sum() >= len(near) // 2  # and points a float step off a face
    check_sor(sor, pts, (mean_k,), muls=(1.0,))


@pytest.mark.parametrize("r", [0.5, 0.1])
def test_radius_first_seed_points_on_cell_faces(handle, r):
    """Seeds and points at origin + k r: the seed grid's cell edge is the radius and its origin the seeds'
    minimum (4^3 = 64 cells for the 64 seeds, under the ns + 64 cap, so the edge is not enlarged), so every
    one of them lies on cell faces and axis neighbours are at the radius itself (d2 = r2 for r = 0.5: the
    strict comparison on a face)."""
    r32 = f32(r)
    lat = lambda a, b: np.stack(np.meshgrid(*[np.arange(a, b)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(f32)
    seeds = (lat(0, 4) * r32).astype(f32)
    grid_pts = (lat(-2, 7) * r32).astype(f32)
    rng = np.random.default_rng(5)
    step = np.nextafter(grid_pts[:300], np.where(rng.random((300, 3)) < 0.5, f32(-9), f32(9)).astype(f32))
    inside = rng.uniform(-2 * r, 6 * r, (500, 3)).astype(f32)
    pts = np.concatenate([grid_pts, step, inside]).astype(f32)
    lo = seeds.min(0)
    inv = f32(1.0) / r32
    dims = np.floor((seeds.max(0) - lo) * inv).astype(np.int64) + 1
    assert int(np.prod(dims)) <= len(seeds) + 64
    k = (pts - lo) * inv
    assert (k == np.floor(k)).all(1).sum() >= (len(grid_pts) if r == 0.5 else 64)
    got_s, got_d = FL.radius_first_seed(pts, seeds, r, handle)
    ref_s, ref_d = ref_radius_first_seed(pts, seeds, r)
    np.testing.assert_array_equal(got_s, ref_s)
    np.testing.assert_array_equal(got_d, ref_d)
    if r == 0.5:
        D = sqdist3(pts, seeds)
        assert (D == f32(0.25)).any(1).sum() >= 64 and (ref_s < 0).any() and (ref_d == 0)[ref_s >= 0].any()


def test_sor_strides(sor):
    rng = np.random.default_rng(8)
    for stride in (3, 5, 8):
        pts = rng.uniform(-3, 3, (700, stride)).astype(f32)
        check_sor(sor, pts, (5, 50), muls=(1.0,))


@pytest.mark.parametrize("ns", [0, 1, 64, 700])
@pytest.mark.parametrize("r", [0.1, 0.5])
def test_radius_first_seed(handle, ns, r):
    rng = np.random.default_rng(ns + int(r * 10))
    n = 5000
    pts = rng.uniform(-4, 4, (n, 4)).astype(f32)
    pts[:, 2] *= 0.25
    pts[::211, 0] = np.nan
    seeds = pts[rng.choice(n, ns, replace=False), :3].copy() if ns else np.zeros((0, 3), f32)  # d2 = 0 hits
    if ns >= 64:
        seeds[40] = seeds[7]  # a seed at two indices: the lowest wins
        seeds[13, 2] = np.inf  # never matches
        # pairs whose float d2 equals r2 exactly: the comparison is strict
        r32 = f32(r)
        r2 = f32(f64(r32) * f64(r32))
        for t in range(10):  # seeds at x = 0, so that the float difference is r itself
            seeds[20 + t] = [0.0, 3.0 - 0.6 * t, 0.9]
            for u, dx in enumerate((np.nextafter(r32, f32(0)), r32, np.nextafter(r32, f32(9)))):
                pts[100 + 3 * t + u, :3] = [dx, 3.0 - 0.6 * t, 0.9]
        d_pin = sqdist3(pts[100:130, :3], seeds[20:30])
        assert (d_pin == r2).sum() >= 10 and (d_pin < r2).sum() >= 10
    got_s, got_d = FL.radius_first_seed(pts, seeds, r, handle)
    ref_s, ref_d = ref_radius_first_seed(pts, seeds, r)
    np.testing.assert_array_equal(got_s, ref_s)
    np.testing.assert_array_equal(got_d, ref_d)
    if ns:
        assert (ref_s >= 0).any() and (ref_d[ref_s >= 0] == 0).any()
    if ns >= 64:
        assert not (ref_s == 40).any() and not (ref_s == 13).any()


@pytest.fixture(scope="module")
def scene():
    return make_scene()


@pytest.mark.parametrize("cfg", [SHIPPED, SOURCE_DEFAULTS], ids=["config_yaml", "source_defaults"])
def test_denoise_slam_map(handle, scene, cfg):
    out, counts = FL.denoise_slam_map(scene, handle=handle, **cfg)
    ref, ref_counts = ref_denoise_slam_map(scene, **cfg)
    np.testing.assert_array_equal(counts, ref_counts)
    np.testing.assert_array_equal(out, ref)
    seeds, seg, after_sor, denoised, remained = counts
    assert seg > 0  # segmented is non-empty
    assert 0 < after_sor < seg  # SOR removes some points but not all
    assert denoised < after_sor  # the noise_thres step removes some points
    assert len(out) == denoised + remained


def test_denoise_no_seed_and_empty(handle, scene):
    low = scene.copy()
    low[:, 3] = np.minimum(low[:, 3], 2500.0)
    out, counts = FL.denoise_slam_map(low, handle=handle, **SHIPPED)
    np.testing.assert_array_equal(out, low[low[:, 3] != 0])
    np.testing.assert_array_equal(counts, [0, 0, 0, 0, len(out)])
    out, counts = FL.denoise_slam_map(np.zeros((0, 4), f32), handle=handle, **SHIPPED)
    assert out.shape == (0, 4) and not counts.any()
    s, d = FL.radius_first_seed(np.zeros((0, 3), f32), np.zeros((0, 3), f32), 0.5, handle)
    assert len(s) == 0 and len(d) == 0
    sor = FL.StatisticalOutlierRemoval(5)
    assert sor.filter(np.zeros((0, 3), f32)).shape == (0, 3)


def test_scratch_regrowth_and_alloc_count(scene):
    """a larger, then a smaller cloud on one handle: the scratch regrows once and the third call allocates nothing"""
    L = _capi.lib()
    h = FL._Handle()
    small, large = scene[:6000], scene
    ref_small = ref_denoise_slam_map(small, **SOURCE_DEFAULTS)
    out, counts = FL.denoise_slam_map(small, handle=h, **SOURCE_DEFAULTS)
    np.testing.assert_array_equal(out, ref_small[0])
    a1 = L.lio_alloc_count()
    FL.denoise_slam_map(large, handle=h, **SOURCE_DEFAULTS)
    a2 = L.lio_alloc_count()
    assert a2 > a1
    out, counts = FL.denoise_slam_map(small, handle=h, **SOURCE_DEFAULTS)
    assert L.lio_alloc_count() == a2
    np.testing.assert_array_equal(out, ref_small[0])
    np.testing.assert_array_equal(counts, ref_small[1])
