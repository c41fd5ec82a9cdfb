"""GPU checks of the Euclidean cluster extraction (lio_cluster.hip, lio_euclidean_clusters) against a numpy / scipy
restatement written here.  Every comparison is exact.

Reference [U: PCL 1.10 EuclideanClusterExtraction::extract, restated as sets]: brute-force float32
((dx*dx + dy*dy) + dz*dz) over all pairs of finite points in row chunks of 512, an edge where
d2 < float32(float64(r) * r) (strict), scipy.sparse.csgraph.connected_components, the size filter
min_size <= size <= max_size, clusters by (-size, lowest member index), indices ascending inside a cluster,
labels -1 for non-finite points and for points of rejected components, float32 min / max per cluster.
"""
import ctypes as C

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from lio_gpu import _capi
from lio_gpu import filters as FL

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
NS = (0, 1, 2, 63, 64, 65, 257, 4097)


# ------------------------------------------------------------------ reference
def sqdist3(a, b):
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def ref_components(pts, tolerance):
    """per point the lowest index of its component (-1: non-finite point)"""
    xyz = np.asarray(pts, f32)[:, :3]
    fin = np.flatnonzero(np.isfinite(xyz).all(1))
    q = xyz[fin]
    r = f32(tolerance)
    r2 = f32(f64(r) * f64(r))
    rows, cols = [], []
    for i0 in range(0, len(q), 512):
        a, b = np.nonzero(sqdist3(q[i0:i0 + 512], q) < r2)
        rows.append(a + i0)
        cols.append(b)
    root = np.full(len(xyz), -1, np.int64)
    if len(q):
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        g = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(len(q), len(q)))
        _, comp = connected_components(g, directed=False)
        low = np.full(comp.max() + 1, len(xyz), np.int64)
        np.minimum.at(low, comp, fin)
        root[fin] = low[comp]
    return root


class Ref:
    def __init__(self, pts, root, min_size, max_size):
        xyz = np.asarray(pts, f32)[:, :3]
        n = len(xyz)
        roots, sizes = np.unique(root[root >= 0], return_counts=True)
        ok = (sizes >= min_size) & (sizes <= max_size)
        order = np.lexsort((roots[ok], -sizes[ok]))
        acc_roots, acc_sizes = roots[ok][order], sizes[ok][order]
        rank = {int(r): k for k, r in enumerate(acc_roots)}
        self.labels = np.array([rank.get(int(r), -1) for r in root], np.int32).reshape(n)
        self.offsets = np.concatenate([[0], np.cumsum(acc_sizes)]).astype(np.int64)
        by_label = np.argsort(self.labels, kind="stable")  # indices ascending inside a cluster
        self.indices = by_label[self.labels[by_label] >= 0].astype(np.int32)
        self.clusters = [self.indices[self.offsets[k]:self.offsets[k + 1]] for k in range(len(acc_roots))]
        self.aabb = np.array([np.concatenate([xyz[c].min(0), xyz[c].max(0)]) for c in self.clusters], f32).reshape(-1, 6)
        self.stats = np.array([(root >= 0).sum(), len(roots), len(acc_roots), acc_sizes.sum()], np.int64)
        self.sizes = sizes


_roots = {}


def components(key, pts, tolerance):
    """the reference's components, computed once per input and shared"""
    k = (key, len(pts), float(tolerance))
    if k not in _roots:
        _roots[k] = ref_components(pts, tolerance)
    return _roots[k]


# ---------------------------------------------------------------------- inputs
def make_cloud(kind, n, seed=0):
    rng = np.random.default_rng(1000 * seed + n)  # test_gpu_denoise.make_cloud's seed rule
    if kind == "uniform":
        p = rng.uniform(-10, 10, (n, 4))
    elif kind == "blobs":  # 40 blobs of sigma 0.15 m in a 50 m box, skewed membership
        c = rng.uniform(0, 50, (40, 3))
        u = rng.uniform(0, 1, n)
        who = np.minimum((u * u * 40).astype(np.int64), 39)
        p = np.concatenate([c[who] + rng.normal(0, 0.15, (n, 3)), rng.uniform(0, 1, (n, 1))], 1)
    elif kind == "chain":  # 0.45 m apart along a line, input order shuffled
        p = np.zeros((n, 4))
        p[:, 0] = 0.45 * rng.permutation(n)
        p[:, 1], p[:, 2] = 3.0, -1.0
    elif kind == "lattice":  # integer coordinates
        m = int(round(n ** (1 / 3)))
        g = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
        p = np.concatenate([g, np.ones((len(g), 1))], 1)[rng.permutation(len(g))]
    elif kind == "duplicates":
        p = np.tile([[1.5, -2.25, 0.75, 7.0]], (n, 1))
    elif kind == "far":  # two blobs 1e5 m apart
        p = rng.normal(0, 0.01, (n, 4))
        p[n // 2:, 0] += 1e5
    else:
        raise ValueError(kind)
    return p.astype(f32)


@pytest.fixture(scope="module")
def ec():
    return FL.EuclideanClusterExtraction()


def size_pairs(n):
    return ((1, max(n, 1)), (10, 250), (1, 1), (5, 2))  # the last: min > max, no cluster


def check(ec, pts, root, tolerance, min_size, max_size, cap=None):
    ref = Ref(pts, root, min_size, max_size)
    ec.setClusterTolerance(tolerance)
    ec.setMinClusterSize(min_size)
    ec.setMaxClusterSize(max_size)
    got = ec.extract(pts, cap)
    msg = f"n={len(pts)} tol={tolerance} sizes=({min_size}, {max_size}) cap={cap}"
    k = len(ref.clusters) if cap is None else min(cap, len(ref.clusters))
    assert ec.n_clusters == len(ref.clusters), msg
    np.testing.assert_array_equal(ec.stats, ref.stats, err_msg=msg)
    np.testing.assert_array_equal(ec.labels, ref.labels, err_msg=msg)
    np.testing.assert_array_equal(ec.indices, ref.indices, err_msg=msg)  # complete whatever the capacity
    np.testing.assert_array_equal(ec.offsets, ref.offsets[: k + 1], err_msg=msg)
    np.testing.assert_array_equal(ec.aabb, ref.aabb[:k], err_msg=msg)
    assert len(got) == k
    for t in range(k):  # the outputs agree with one another
        np.testing.assert_array_equal(got[t], ref.clusters[t], err_msg=msg)
        assert (ec.labels[got[t]] == t).all() and (np.diff(got[t]) > 0).all()
    assert (ec.labels >= 0).sum() == ref.stats[3]
    return ref


def check_all(ec, key, pts, tolerance, pairs=None):
    root = components(key, pts, tolerance)
    n = len(pts)
    refs = [check(ec, pts, root, tolerance, lo, hi) for lo, hi in (pairs or size_pairs(n))]
    for cap in (0, 1, n):
        check(ec, pts, root, tolerance, 1, max(n, 1), cap)
    return refs


# ----------------------------------------------------------------------- tests
@pytest.mark.parametrize("tolerance", [0.5, 1.0, 1.6])
@pytest.mark.parametrize("n", NS)
def test_uniform(ec, n, tolerance):
    pts = make_cloud("uniform", n)
    refs = check_all(ec, "uniform", pts, tolerance)
    assert refs[3].stats[2] == 0 and (refs[3].labels == -1).all()  # min > max
    if n == 4097 and tolerance == 1.0:  # many components of equal size: the tie-break decides their order
        s = np.sort(refs[0].sizes)[::-1]
        assert len(s) == 1165 and tuple(s[:4]) == (90, 79, 58, 58) and refs[1].stats[2] == 87
    if n == 4097 and tolerance == 1.6:
        assert refs[0].sizes.max() == 4089


@pytest.mark.parametrize("n", NS)
def test_blobs(ec, n):
    pts = make_cloud("blobs", n)
    refs = check_all(ec, "blobs", pts, 0.5)
    if n == 4097:
        s = np.sort(refs[0].sizes)[::-1]
        assert len(s) == 40 and tuple(s[:4]) == (660, 262, 220, 168) and s.min() >= 10
        # min 10, max 250: the two largest components are rejected by max_size alone; their points come out
        # -1 and join no other cluster
        assert refs[1].stats[2] == 38 and refs[1].stats[3] == 4097 - 660 - 262
        big = np.concatenate(refs[0].clusters[:2])
        assert len(big) == 660 + 262 and (refs[1].labels[big] == -1).all()
        ec.setMinClusterSize(10)
        ec.setMaxClusterSize(250)
        ec.extract(pts)
        assert (ec.labels[big] == -1).all() and (ec.labels >= 0).sum() == 4097 - 660 - 262


def test_blob_boxes_in_rank_order(ec):
    """the boxes walk `indices` in rank order (size descending), which is not the root order of the sorted runs:
    clusters of 660 down to 10 points change inside and across the 64-position groups of the box kernel"""
    pts = make_cloud("blobs", 4097)
    root = components("blobs", pts, 0.5)
    ref = check(ec, pts, root, 0.5, 1, 4097)
    roots = np.array([c[0] for c in ref.clusters])
    assert len(ref.clusters) == 40 and (np.diff(roots) < 0).any()  # rank order differs from root order
    check(ec, pts, root, 0.5, 1, 4097, cap=3)
    np.testing.assert_array_equal(ec.aabb, ref.aabb[:3])


def test_two_point_clusters(ec):
    """1300 clusters of two points: a cluster boundary at every second position of `indices`, in lockstep across
    the box kernel's 1024-position chunks"""
    rng = np.random.default_rng(1300)
    site = 5.0 * np.stack(np.meshgrid(*[np.arange(11)] * 3, indexing="ij"), -1).reshape(-1, 3)[:1300]
    p = np.concatenate([site, site + [0.1, 0.0, 0.0]])
    pts = np.concatenate([p, np.ones((len(p), 1))], 1)[rng.permutation(len(p))].astype(f32)
    ref = check(ec, pts, components("pairs", pts, 0.5), 0.5, 2, 2)
    assert ref.stats[1] == 1300 and ref.stats[2] == 1300 and ref.stats[3] == 2600
    assert (np.diff(ref.offsets) == 2).all()


@pytest.mark.parametrize("n", NS)
def test_chain(ec, n):
    """one component through every cell and every workgroup: a union that hooks once without finding the roots
    again, or a flatten that stops early, splits it"""
    pts = make_cloud("chain", n)
    refs = check_all(ec, "chain", pts, 0.5, pairs=((1, max(n, 1)), (1, 1)))
    if n:
        assert refs[0].stats[1] == 1 and refs[0].stats[3] == n


@pytest.mark.parametrize("n", [27, 125, 4096])
def test_lattice(ec, n):
    """integer coordinates: d2 = 1 is not < 1 (n singletons); one float step above, one component"""
    pts = make_cloud("lattice", n)
    refs = check_all(ec, "lattice", pts, 1.0, pairs=((1, n), (1, 1), (2, n)))
    assert refs[0].stats[1] == n and refs[0].stats[2] == n and refs[2].stats[2] == 0
    np.testing.assert_array_equal(refs[0].labels, np.arange(n))  # equal sizes: ordered by index
    up = float(np.nextafter(f32(1), f32(2)))
    refs = check_all(ec, "lattice", pts, up, pairs=((1, n), (1, 1)))
    assert refs[0].stats[1] == 1 and refs[0].stats[3] == n and refs[1].stats[2] == 0


@pytest.mark.parametrize("n", NS)
def test_duplicates(ec, n):
    pts = make_cloud("duplicates", n)
    refs = check_all(ec, "duplicates", pts, 0.5, pairs=((1, max(n, 1)), (2, 5000)))
    if n:
        assert refs[0].stats[1] == 1


@pytest.mark.parametrize("n", NS)
def test_nan_and_inf_rows(ec, n):
    pts = make_cloud("uniform", n, seed=1)
    pts[::97, 1] = np.nan
    pts[50::97, 0] = np.inf
    pts[60::97, 2] = -np.inf
    refs = check_all(ec, "nan", pts, 1.0)
    bad = ~np.isfinite(pts[:, :3]).all(1)
    assert refs[0].stats[0] == n - bad.sum() and (refs[0].labels[bad] == -1).all()
    if n:
        assert bad.any() and (ec.labels[bad] == -1).all()


def test_far_apart(ec):
    """two blobs 1e5 m apart at tolerance 0.01: the cell cap grows the cell by orders of magnitude above the
    tolerance, so a cell holds many points that are not neighbours"""
    pts = make_cloud("far", 257)
    refs = check_all(ec, "far", pts, 0.01, pairs=((1, 257), (2, 50)))
    assert 2 < refs[0].stats[1] < 257


@pytest.mark.parametrize("n", [257, 4097])
def test_large_coordinates(ec, n):
    """1e6 m from the origin the float spacing is 0.0625 m: what the margin of the scanned cell range is for"""
    pts = make_cloud("uniform", n)
    pts[:, :3] = (pts[:, :3].astype(f64) + 1e6).astype(f32)
    refs = check_all(ec, "large", pts, 0.5)
    assert refs[0].stats[1] < n


@pytest.mark.parametrize("stride", [3, 4, 8])
def test_strides(ec, stride):
    rng = np.random.default_rng(stride)
    pts = rng.uniform(-4, 4, (700, stride)).astype(f32)
    check_all(ec, f"stride{stride}", pts, 0.7, pairs=((1, 700), (3, 40)))


def test_count_only_call(ec):
    """cap_clusters = 0 with NULLs: labels, the count and nothing else"""
    pts = make_cloud("blobs", 4097)
    ref = Ref(pts, components("blobs", pts, 0.5), 10, 250)
    labels = np.full(len(pts), -7, np.int32)
    m = C.c_int64(-1)
    rc = _capi.lib().lio_euclidean_clusters(ec._h, pts.ctypes.data_as(_capi.fp), len(pts), 4, 0.5, 10, 250,
                                            labels.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(m), 0, None, None,
                                            None, None)
    assert rc == 0 and m.value == ref.stats[2]
    np.testing.assert_array_equal(labels, ref.labels)


def test_three_calls_are_identical(ec):
    pts = make_cloud("uniform", 4097)
    ec.setClusterTolerance(1.0)
    ec.setMinClusterSize(2)
    ec.setMaxClusterSize(60)
    runs = []
    for _ in range(3):
        ec.extract(pts)
        runs.append((ec.labels.copy(), ec.offsets.copy(), ec.indices.copy(), ec.aabb.copy(), ec.stats.copy()))
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("kind,tolerance", [("uniform", 1.0), ("blobs", 0.5), ("chain", 0.5)])
def test_input_permutation_gives_the_same_sets(ec, kind, tolerance):
    pts = make_cloud(kind, 4097)
    perm = np.random.default_rng(9).permutation(len(pts))
    ec.setClusterTolerance(tolerance)
    ec.setMinClusterSize(2)
    ec.setMaxClusterSize(len(pts))  # the chain is one component of all points
    a = {frozenset(c.tolist()) for c in ec.extract(pts)}
    sizes_a = np.diff(ec.offsets)
    b = {frozenset(perm[c].tolist()) for c in ec.extract(pts[perm])}  # row k of the permuted cloud is point perm[k]
    assert a == b and len(a) > 0
    np.testing.assert_array_equal(sizes_a, np.diff(ec.offsets))


def test_no_allocation_on_a_second_or_smaller_call():
    L = _capi.lib()
    h = FL.EuclideanClusterExtraction(1.0, 1, 100)
    large, small = make_cloud("uniform", 4097), make_cloud("uniform", 257)
    a0 = L.lio_alloc_count()
    h.extract(large)
    a1 = L.lio_alloc_count()
    assert a1 > a0
    h.extract(large)
    assert L.lio_alloc_count() == a1
    h.extract(small)
    assert L.lio_alloc_count() == a1
    check(h, small, components("uniform", small, 1.0), 1.0, 1, 100)
    assert L.lio_alloc_count() == a1


def test_bad_arguments_leave_the_handle_usable():
    L = _capi.lib()
    h = FL.EuclideanClusterExtraction(1.0, 1, 100)
    pts = make_cloud("uniform", 257)
    labels = np.zeros(len(pts), np.int32)
    m = C.c_int64(0)
    fp, lp = pts.ctypes.data_as(_capi.fp), labels.ctypes.data_as(C.POINTER(C.c_int32))

    def call(n=len(pts), stride=4, tolerance=1.0, min_size=1, max_size=100, lab=lp):
        return L.lio_euclidean_clusters(h._h, fp, n, stride, tolerance, min_size, max_size, lab, C.byref(m), 0, None,
                                        None, None, None)

    bad = [dict(tolerance=0.0), dict(tolerance=-1.0), dict(tolerance=float("nan")), dict(tolerance=float("inf")),
           dict(min_size=0), dict(min_size=-3), dict(stride=2), dict(stride=9), dict(n=-1), dict(n=2**31),
           dict(lab=None)]
    for kw in bad:
        assert call(**kw) == _capi.LIO_ERR_ARG, kw
        assert b"lio_euclidean_clusters" in L.lio_last_error()
    assert call(min_size=5, max_size=2) == 0 and m.value == 0  # legal: no cluster
    assert call(n=0) == 0 and m.value == 0
    check(h, pts, components("uniform", pts, 1.0), 1.0, 1, 100)
