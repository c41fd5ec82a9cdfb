"""GPU checks of the RANSAC plane segmentation (lio_plane.hip, lio_segment_plane) against a numpy restatement of
its contract written here.  Every comparison is exact except the refit.

Reference [U: Open3D PointCloud::SegmentPlane, restated as the contract of include/lio_gpu.h]: the counter-based
sampler in numpy uint64 (wrapping) arithmetic; `planes` (float32 cross product, normalised; degenerate unless
the length is finite and > 0 and d is finite); `evaluate` (float32 |((a x + b y) + c z) + d| < thr, strict; the
fixed-point sum of floor(float64(float32(dist * dist)) * 2^(32 - e)) over the inliers, thr * thr = m 2^e); the
winner by lexsort((t, sq, -count)) over the non-degenerate hypotheses; its inliers; for the refit
numpy.linalg.eigh of the float64 covariance of the inliers about their mean.

REFIT BOUND.  Angle between the normals <= 1e-9 rad and |delta d| <= 1e-9 (1 + max |coordinate|): the double
accumulation over <= 4097 terms carries a relative error <= 4097 * 2^-53 ~ 5e-13, the eigen-gap ratio of the
street scene is about 1, so Davis-Kahan bounds the angle near 1e-12; three orders of margin are left for the
host eigen solver.
"""
import ctypes as C
import math

import numpy as np
import pytest

from lio_gpu import _capi
from lio_gpu import filters as FL

pytestmark = pytest.mark.gpu
f32, f64, u64 = np.float32, np.float64, np.uint64
NS = (0, 1, 2, 3, 63, 64, 65, 257, 4097)  # the point tile is 1024, a workgroup's chunk 2048: 4097 = 2 chunks + 1
KS = (1, 255, 256, 257, 1000)


# ------------------------------------------------------------------ reference
def _mix(z):
    z = (z ^ (z >> u64(30))) * u64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> u64(27))) * u64(0x94D049BB133111EB)
    return z ^ (z >> u64(31))


def sample_triples(seed, n, k):
    if n < 3:
        return np.zeros((0, 3), np.int64)
    with np.errstate(over="ignore"):
        c = np.arange(3 * k, dtype=u64)
        r = _mix(np.array(seed, u64) + (c + u64(1)) * u64(0x9E3779B97F4A7C15)).reshape(k, 3)
    i0 = (r[:, 0] % u64(n)).astype(np.int64)
    i1 = (r[:, 1] % u64(n - 1)).astype(np.int64)
    i1 += i1 >= i0
    i2 = (r[:, 2] % u64(n - 2)).astype(np.int64)
    lo, hi = np.minimum(i0, i1), np.maximum(i0, i1)
    i2 += i2 >= lo
    i2 += i2 >= hi
    return np.stack([i0, i1, i2], 1)


def planes(xyz, tr):  # float32 throughout
    with np.errstate(all="ignore"):
        p0, p1, p2 = xyz[tr[:, 0]], xyz[tr[:, 1]], xyz[tr[:, 2]]
        e1, e2 = p1 - p0, p2 - p0
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        a, b, c = nx / ln, ny / ln, nz / ln
        d = -((a * p0[:, 0] + b * p0[:, 1]) + c * p0[:, 2])
        ok = np.isfinite(ln) & (ln > 0) & np.isfinite(d)
    assert all(v.dtype == f32 for v in (a, b, c, d))
    return np.stack([a, b, c, d], 1), ok


def distances(xyz, pl):
    """float32 |((a x + b y) + c z) + d| of every point (columns) to every plane (rows)"""
    with np.errstate(all="ignore"):
        x, y, z = xyz[None, :, 0], xyz[None, :, 1], xyz[None, :, 2]
        return np.abs(((pl[:, 0:1] * x + pl[:, 1:2] * y) + pl[:, 2:3] * z) + pl[:, 3:4])


def evaluate(xyz, pl, ok, thr):
    thr = f32(thr)
    thr2 = thr * thr
    _, e = math.frexp(float(thr2))
    S = 2.0 ** (32 - e)
    counts, sq = np.zeros(len(pl), np.int64), np.zeros(len(pl), u64)
    for h0 in range(0, len(pl), 128):
        dist = distances(xyz, pl[h0:h0 + 128])
        assert dist.dtype == f32
        with np.errstate(all="ignore"):
            inl = dist < thr
            q = np.floor((dist * dist).astype(f64) * S)
        q = np.where(inl, q, 0.0).astype(u64)
        counts[h0:h0 + 128] = inl.sum(1)
        sq[h0:h0 + 128] = q.sum(1, dtype=u64)
    counts[~ok] = 0
    sq[~ok] = 0
    return counts, sq


def xyz_of(pts):
    pts = np.asarray(pts, f32)
    return np.ascontiguousarray(pts.reshape(len(pts), pts.shape[-1])[:, :3])


class Ref:
    def __init__(self, pts, thr, k, seed=0, triples=None):
        xyz = xyz_of(pts)
        n = len(xyz)
        self.n, self.k = n, k
        self.plane, self.best = np.zeros(4, f32), -1
        self.inliers, self.mask = np.zeros(0, np.int32), np.zeros(n, np.uint8)
        self.counts, self.sq, self.degenerate = np.zeros(k, np.int64), np.zeros(k, u64), np.ones(k, np.uint8)
        if n < 3:  # no hypothesis at all
            return
        tr = sample_triples(seed, n, k) if triples is None else np.asarray(triples, np.int64)
        pl, ok = planes(xyz, tr)
        self.degenerate = (~ok).astype(np.uint8)
        self.counts, self.sq = evaluate(xyz, pl, ok, thr)
        self.planes = pl
        cand = np.flatnonzero(ok)
        if len(cand):
            order = np.lexsort((cand, self.sq[cand], -self.counts[cand]))
            self.best = int(cand[order[0]])
            self.plane = pl[self.best]
            self.mask = (distances(xyz, pl[self.best:self.best + 1])[0] < f32(thr)).astype(np.uint8)
            self.inliers = np.flatnonzero(self.mask).astype(np.int32)
            assert len(self.inliers) == self.counts[self.best]

    def top_ties(self):
        ok = self.degenerate == 0
        return int((self.counts[ok] == self.counts[ok].max()).sum()) if ok.any() else 0


_refs = {}


def reference(key, pts, thr, k, seed):
    """the sampler's reference, computed once per input at the largest K and shared: hypothesis t depends on
    (seed, t) alone, so a smaller K is a prefix"""
    kk = (key, len(pts), float(thr), seed)
    if kk not in _refs or _refs[kk].k < k:
        _refs[kk] = Ref(pts, thr, max(k, 1000), seed)
    full = _refs[kk]
    if full.k == k:
        return full
    r = Ref.__new__(Ref)
    r.n, r.k = full.n, k
    r.counts, r.sq, r.degenerate = full.counts[:k], full.sq[:k], full.degenerate[:k]
    r.plane, r.best, r.inliers, r.mask = np.zeros(4, f32), -1, np.zeros(0, np.int32), np.zeros(full.n, np.uint8)
    cand = np.flatnonzero(r.degenerate == 0)
    if len(cand):
        xyz = xyz_of(pts)
        order = np.lexsort((cand, r.sq[cand], -r.counts[cand]))
        r.best = int(cand[order[0]])
        r.plane = full.planes[r.best]
        r.mask = (distances(xyz, full.planes[r.best:r.best + 1])[0] < f32(thr)).astype(np.uint8)
        r.inliers = np.flatnonzero(r.mask).astype(np.int32)
    return r


# ---------------------------------------------------------------------- inputs
def street(n, seed=0):
    """60 % ground, 15 % wall, the rest 12 blobs; rows permuted; a 4th column of intensity"""
    rng = np.random.default_rng(1000 * seed + n)
    ng, nw = int(0.6 * n), int(0.15 * n)
    nb = n - ng - nw
    ground = np.stack([rng.uniform(-20, 20, ng), rng.uniform(-20, 20, ng), rng.normal(0, 0.02, ng)], 1)
    wall = np.stack([rng.uniform(-20, 20, nw), 15 + rng.normal(0, 0.02, nw), rng.uniform(0, 8, nw)], 1)
    centres = rng.uniform([-18, -12, 0.5], [18, 12, 2.5], (12, 3))
    blobs = centres[rng.integers(0, 12, nb)] + rng.normal(0, 0.15, (nb, 3))
    xyz = np.concatenate([ground, wall, blobs])[rng.permutation(n)]
    return np.concatenate([xyz, rng.uniform(0, 1, (n, 1))], 1).astype(f32)


def lattice():
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([g, np.ones((len(g), 1))], 1).astype(f32)


@pytest.fixture(scope="module")
def seg():
    return FL.PlaneSegmentation()


def check(seg, pts, ref, thr, k, seed=0, triples=None):
    plane, inl = seg.segment_plane(pts, thr, 3, k, seed, triples)
    msg = f"n={len(pts)} K={k} thr={thr} seed={seed}"
    np.testing.assert_array_equal(seg.degenerate, ref.degenerate, err_msg=msg)
    np.testing.assert_array_equal(seg.counts, ref.counts, err_msg=msg)
    np.testing.assert_array_equal(seg.sq, ref.sq, err_msg=msg)
    assert seg.best_iteration == ref.best, msg
    assert plane.tobytes() == np.asarray(ref.plane, f32).tobytes(), (msg, plane, ref.plane)  # bit for bit
    np.testing.assert_array_equal(inl, ref.inliers, err_msg=msg)
    np.testing.assert_array_equal(seg.mask, ref.mask, err_msg=msg)
    assert len(inl) == int(seg.mask.sum())
    if ref.best < 0:
        assert len(inl) == 0 and not plane.any() and not seg.refit.any(), msg
    elif len(inl) < 3:
        np.testing.assert_array_equal(seg.refit, plane.astype(f64), err_msg=msg)
    return plane, inl


# ----------------------------------------------------------------------- tests
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_street(seg, n, k):
    pts = street(n)
    ref = reference("street", pts, 0.2, k, 7)
    check(seg, pts, ref, 0.2, k, 7)
    if n < 3:
        assert ref.best == -1 and ref.degenerate.all()
    if k == 1000 and n >= 65:  # the count alone does not decide the winner: sq does
        assert ref.top_ties() > 1, ref.top_ties()
        top = np.flatnonzero((ref.counts == ref.counts.max()) & (ref.degenerate == 0))
        assert len(np.unique(ref.sq[top])) > 1 and ref.sq[ref.best] == ref.sq[top].min()


def test_lattice_ties_and_degenerates(seg):
    """an 8 x 8 x 4 integer grid: many hypotheses tie in count AND in sq (the lowest index wins), and collinear
    triples are skipped"""
    pts = lattice()
    ref = Ref(pts, 0.2, 257, 3)
    check(seg, pts, ref, 0.2, 257, 3)
    top = np.flatnonzero((ref.counts == ref.counts.max()) & (ref.degenerate == 0))
    same = top[ref.sq[top] == ref.sq[top].min()]
    assert len(same) > 1 and ref.best == same.min() and ref.degenerate.sum() >= 1
    # computed with this restatement on the host: 16 hypotheses tied at count 64 with one common sq, 1 degenerate
    assert (len(top), int(ref.counts.max()), len(same), int(ref.degenerate.sum()), ref.best) == (16, 64, 16, 1, 2)
    print("lattice: tied at the top count", len(top), "count", ref.counts.max(), "with the winner's sq", len(same),
          "degenerate", int(ref.degenerate.sum()))


@pytest.mark.parametrize("n", [3, 65, 4097])
@pytest.mark.parametrize("kind", ["duplicates", "collinear"])
def test_all_degenerate_is_no_plane(seg, kind, n):
    if kind == "duplicates":
        pts = np.tile(np.array([[1.5, -2.25, 0.75, 7.0]], f32), (n, 1))
    else:  # exactly representable multiples of one direction
        pts = np.zeros((n, 4), f32)
        pts[:, :3] = np.arange(n, dtype=f32)[:, None] * np.array([0.5, -0.25, 2.0], f32)
    ref = Ref(pts, 0.2, 257, 1)
    assert ref.best == -1 and ref.degenerate.all()
    plane, inl = check(seg, pts, ref, 0.2, 257, 1)
    assert seg.best_iteration == -1 and len(inl) == 0 and not seg.mask.any() and not seg.counts.any()


@pytest.mark.parametrize("n", NS)
def test_nan_and_inf_rows(seg, n):
    rng = np.random.default_rng(1000 + n)  # test_gpu_cluster.test_nan_and_inf_rows' cloud and rows
    pts = rng.uniform(-10, 10, (n, 4)).astype(f32)
    pts[::97, 1] = np.nan
    pts[50::97, 0] = np.inf
    pts[60::97, 2] = -np.inf
    ref = Ref(pts, 1.0, 257, 5)
    plane, inl = check(seg, pts, ref, 1.0, 257, 5)
    bad = ~np.isfinite(pts[:, :3]).all(1)
    assert not seg.mask[bad].any()
    if n >= 3:
        tr = sample_triples(5, n, 257)
        holds_bad = bad[tr].any(1)
        assert holds_bad.any() and seg.degenerate[holds_bad].all()


@pytest.mark.parametrize("n", [257, 4097])
def test_large_coordinates(seg, n):
    """1e6 m from the origin the float spacing is 0.0625 m: still exact"""
    pts = street(n)
    pts[:, :3] = (pts[:, :3].astype(f64) + 1e6).astype(f32)
    ref = Ref(pts, 0.2, 1000, 7)
    check(seg, pts, ref, 0.2, 1000, 7)
    assert ref.best >= 0 and ref.counts[ref.best] > 0.3 * n


def test_explicit_triples(seg):
    pts = street(4097)
    ref = reference("street", pts, 0.2, 257, 7)
    tr = sample_triples(7, len(pts), 257).astype(np.int32)
    np.testing.assert_array_equal(tr, FL.sample_triples(7, len(pts), 257))
    check(seg, pts, ref, 0.2, 257, 99, triples=tr)  # the seed is not used
    hand = np.array([[0, 1, 2], [5, 4, 3], [10, 20, 4096], [7, 8, 9]], np.int32)  # a hand-made set, all legal
    check(seg, pts, Ref(pts, 0.2, 4, triples=hand), 0.2, 4, triples=hand)
    L = _capi.lib()
    for bad in ([10, 20, 4097], [-1, 2, 3], [5, 5, 6], [5, 6, 5], [6, 5, 5]):
        t2 = hand.copy()
        t2[2] = bad
        with pytest.raises(_capi.LioError) as e:
            seg.segment_plane(pts, 0.2, 3, 4, 0, t2)
        assert e.value.code == _capi.LIO_ERR_ARG and b"lio_segment_plane" in L.lio_last_error()
    check(seg, pts, ref, 0.2, 257, 7)  # the handle is still usable


@pytest.mark.parametrize("stride", [3, 4, 8])
def test_strides(seg, stride):
    rng = np.random.default_rng(stride)
    pts = rng.uniform(-4, 4, (700, stride)).astype(f32)
    pts[:400, 2] = rng.normal(0, 0.05, 400)
    check(seg, pts, Ref(pts, 0.2, 300, 2), 0.2, 300, 2)


def test_threshold_is_strict(seg):
    """one hypothesis; a point at float distance exactly thr is no inlier, one float step above it is"""
    pts = street(257)
    tr = np.array([[3, 100, 200]], np.int32)
    pl, ok = planes(pts[:, :3], tr.astype(np.int64))
    assert ok[0]
    dist = distances(np.ascontiguousarray(pts[:, :3]), pl)[0]
    i = int(np.argsort(dist)[len(dist) // 2])
    at = dist[i]
    assert at > 0
    above = np.nextafter(at, f32(np.inf))
    below = np.nextafter(at, f32(0))
    for thr, inside in ((at, False), (above, True), (below, False)):
        ref = Ref(pts, float(thr), 1, triples=tr)
        _, inl = check(seg, pts, ref, float(thr), 1, triples=tr)
        assert (i in inl) == inside and bool(seg.mask[i]) == inside


def test_three_calls_are_identical(seg):
    pts = street(4097)
    runs = []
    for _ in range(3):
        plane, inl = seg.segment_plane(pts, 0.2, 3, 1000, 7)
        runs.append((plane.copy(), inl.copy(), seg.counts.copy(), seg.sq.copy(), seg.degenerate.copy(), seg.mask.copy(),
                     seg.refit.copy(), np.array(seg.best_iteration)))
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert a.tobytes() == b.tobytes()
    assert runs[0][6].any()


def test_no_allocation_on_a_second_or_smaller_call():
    L = _capi.lib()
    h = FL.PlaneSegmentation()
    large, small = street(4097), street(257)
    a0 = L.lio_alloc_count()
    h.segment_plane(large, 0.2, 3, 1000, 7)
    a1 = L.lio_alloc_count()
    assert a1 > a0
    h.segment_plane(large, 0.2, 3, 1000, 7)
    assert L.lio_alloc_count() == a1
    h.segment_plane(small, 0.2, 3, 1000, 7)
    h.segment_plane(large, 0.2, 3, 255, 7)
    assert L.lio_alloc_count() == a1
    check(h, small, reference("street", small, 0.2, 257, 7), 0.2, 257, 7)
    assert L.lio_alloc_count() == a1


def test_bad_arguments_leave_the_handle_usable():
    L = _capi.lib()
    h = FL.PlaneSegmentation()
    pts = street(257)
    plane, inl = np.zeros(4, f32), np.zeros(len(pts), np.int32)
    best, m = C.c_int64(0), C.c_int64(0)
    fp, ip = pts.ctypes.data_as(_capi.fp), inl.ctypes.data_as(C.POINTER(C.c_int32))
    pp = plane.ctypes.data_as(_capi.fp)

    def call(n=len(pts), stride=4, thr=0.2, ransac_n=3, k=100, plane_p=pp, best_p=C.byref(best), inl_p=ip,
             m_p=C.byref(m), pts_p=fp):
        return L.lio_segment_plane(h._h, pts_p, n, stride, thr, ransac_n, k, 0, None, plane_p, best_p, inl_p, m_p,
                                   None, None, None, None, None)

    bad = [dict(thr=0.0), dict(thr=-1.0), dict(thr=float("nan")), dict(thr=float("inf")), dict(stride=2), dict(stride=9),
           dict(n=-1), dict(n=2**31), dict(k=0), dict(k=-5), dict(k=2**20 + 1), dict(ransac_n=2), dict(ransac_n=4),
           dict(plane_p=None), dict(best_p=None), dict(m_p=None), dict(inl_p=None), dict(pts_p=None)]
    for kw in bad:
        assert call(**kw) == _capi.LIO_ERR_ARG, kw
        assert b"lio_segment_plane" in L.lio_last_error()
    assert call(n=0) == 0 and best.value == -1 and m.value == 0  # legal: no plane
    assert call(n=2) == 0 and best.value == -1 and m.value == 0
    assert call() == 0 and best.value >= 0 and m.value > 0  # the minimal call: every optional output NULL
    check(h, pts, reference("street", pts, 0.2, 257, 7), 0.2, 257, 7)


def ref_refit(pts, inl, winner):
    x = np.asarray(pts, f32)[inl, :3].astype(f64)
    mean = x.mean(0)
    d = x - mean
    w, v = np.linalg.eigh(d.T @ d / len(x))
    nrm = v[:, 0]
    if nrm @ winner[:3].astype(f64) < 0:
        nrm = -nrm
    return np.concatenate([nrm, [-(nrm @ mean)]]), w


@pytest.mark.parametrize("shift", [0.0, 1e6])
@pytest.mark.parametrize("n", [257, 4097])
def test_refit(seg, n, shift):
    pts = street(n)
    pts[:, :3] = (pts[:, :3].astype(f64) + shift).astype(f32)
    plane, inl = seg.segment_plane(pts, 0.2, 3, 1000, 7)
    assert len(inl) > 0.3 * n
    ref, w = ref_refit(pts, inl, plane)
    got = seg.refit
    angle = math.atan2(np.linalg.norm(np.cross(got[:3], ref[:3])), got[:3] @ ref[:3])
    dd = abs(got[3] - ref[3])
    bound_d = 1e-9 * (1 + (1e6 if shift else np.abs(pts[:, :3]).max()))
    print(f"refit n={n} shift={shift}: angle {angle:.3e} rad, |delta d| {dd:.3e} (bound {bound_d:.3e}), eigenvalues {w}")
    assert abs(np.linalg.norm(got[:3]) - 1) < 1e-12 and got[:3] @ plane[:3].astype(f64) >= 0
    assert angle <= 1e-9 and dd <= bound_d


def test_cluster_objects_equals_the_pieces():
    """post_process/clustering.py's main block: SOR -> plane -> drop the inliers -> clusters -> boxes, indices
    mapped back to rows of the input"""
    pts = street(4097)
    out = FL.cluster_objects(pts)
    sor = FL.StatisticalOutlierRemoval(20, 2.0)
    filtered = sor.filter(pts)
    kept = np.flatnonzero(~(sor.distances.astype(f64) > sor.stats[2]))
    np.testing.assert_array_equal(pts[kept], filtered)
    np.testing.assert_array_equal(out["kept"], kept)
    seg = FL.PlaneSegmentation()
    plane, inl = seg.segment_plane(filtered, 0.2, 3, 1000, 0)
    assert out["plane"].tobytes() == plane.tobytes()
    np.testing.assert_array_equal(out["ground"], kept[inl])
    rest = np.setdiff1d(np.arange(len(filtered)), inl)
    ec = FL.EuclideanClusterExtraction(0.5, 10, 10000)
    found = ec.extract(filtered[rest])
    assert len(found) == len(out["clusters"]) and len(found) >= 5
    for a, b in zip(out["clusters"], found):
        np.testing.assert_array_equal(a, kept[rest[b]])
        np.testing.assert_array_equal(pts[a], filtered[rest[b]])  # rows of the input
    np.testing.assert_array_equal(out["aabb"], ec.aabb)
    ground = set(out["ground"].tolist())
    assert all(not (set(c.tolist()) & ground) for c in out["clusters"])
