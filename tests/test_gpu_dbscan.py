"""GPU checks of DBSCAN (lio_dbscan.hip, lio_dbscan) against the contract restated as sets in numpy / scipy
(tests/dbscan_ref.py dbscan_sets; tests/test_dbscan_ref.py holds that reference against the sequential procedure
and against scikit-learn on the CPU).  Every comparison is exact: labels, core flags, counts, grouped indices,
offsets and boxes, at cluster capacities 0 / 1 / n / default and through the count-only call."""
import ctypes as C

import numpy as np
import pytest

import dbscan_cases as DC
import test_gpu_cluster as EC
from dbscan_cases import NS
from lio_gpu import _capi
from lio_gpu import filters as FL
from test_gpu_cluster import make_cloud

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
i32p, i64p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def db():
    return FL.DBSCAN()


def check(db, pts, exp, eps, min_samples, cap=None):
    db.eps, db.min_samples = eps, min_samples
    got = db.fit(pts, cap)
    msg = f"n={len(pts)} eps={eps} min_samples={min_samples} cap={cap}"
    k = exp.stats[2] if cap is None else min(cap, exp.stats[2])
    assert db.n_clusters == exp.stats[2], msg
    np.testing.assert_array_equal(db.stats, exp.stats, err_msg=msg)
    np.testing.assert_array_equal(db.labels_, exp.labels, err_msg=msg)
    np.testing.assert_array_equal(db.core_sample_indices_, exp.core_indices, err_msg=msg)
    np.testing.assert_array_equal(db.indices, exp.indices, err_msg=msg)  # complete whatever the capacity
    np.testing.assert_array_equal(db.offsets, exp.offsets[: k + 1], err_msg=msg)
    np.testing.assert_array_equal(db.aabb, exp.aabb[:k], err_msg=msg)
    assert len(got) == k
    for t in range(k):  # the outputs agree with one another
        np.testing.assert_array_equal(got[t], exp.clusters[t], err_msg=msg)
        assert (db.labels_[got[t]] == t).all() and (np.diff(got[t]) > 0).all()


def count_only(db, pts, eps, min_samples):
    """cap_clusters = 0 with NULLs: labels, the count and nothing else"""
    labels = np.full(len(pts), -7, np.int32)
    m = C.c_int64(-1)
    rc = _capi.lib().lio_dbscan(db._h, pts.ctypes.data_as(_capi.fp), len(pts), pts.shape[1], eps, min_samples,
                                labels.ctypes.data_as(i32p), None, C.byref(m), 0, None, None, None, None)
    assert rc == 0
    return labels, m.value


def check_all(db, key, pts, eps, min_samples):
    exp, details = DC.reference(key, pts, eps, min_samples)
    n = len(pts)
    for cap in (None, 0, 1, n):
        check(db, pts, exp, eps, min_samples, cap)
    labels, m = count_only(db, pts, eps, min_samples)
    assert m == exp.stats[2]
    np.testing.assert_array_equal(labels, exp.labels)
    return exp, details


# ----------------------------------------------------------------------- tests
@pytest.mark.parametrize("eps,min_samples", [(1.0, 4), (1.6, 10), (1.0, 1), (0.5, 10)])
@pytest.mark.parametrize("n", NS)
def test_uniform(db, n, eps, min_samples):
    pts = make_cloud("uniform", n)
    exp, details = check_all(db, "uniform", pts, eps, min_samples)
    if n == 4097:  # the reference's figures: clusters, core, border (contested among them), noise
        got = (exp.stats[2], exp.n_core, exp.n_border, details["contested"], exp.n_noise)
        want = {(1.0, 4): (297, 1339, 1037, 48, 1721), (1.6, 10): (18, 1691, 1843, 61, 563),
                (0.5, 10): (0, 0, 0, 0, 4097), (1.0, 1): (got[0], 4097, 0, 0, 0)}[(eps, min_samples)]
        assert got == want
        assert db.stats[1] == want[1] and db.stats[0] - db.stats[3] == want[4]


@pytest.mark.parametrize("eps,min_samples", [(0.5, 10), (0.3, 3)])
@pytest.mark.parametrize("n", NS)
def test_blobs(db, n, eps, min_samples):
    pts = make_cloud("blobs", n)
    exp, _ = check_all(db, "blobs", pts, eps, min_samples)
    if n == 4097 and eps == 0.5:
        assert exp.stats[2] == 40
    if n == 4097 and eps == 0.3:
        assert exp.n_border > 0 and exp.n_noise > 0


@pytest.mark.parametrize("n", NS)
def test_chain(db, n):
    """0.45 m apart, shuffled: with min_samples 3 every inner point is core, so one cluster runs through every cell
    and every workgroup, and the two end points are border; with 4 nobody is core"""
    pts = make_cloud("chain", n)
    exp, _ = check_all(db, "chain", pts, 0.5, 3)
    if n >= 3:
        ends = np.argsort(pts[:, 0])[[0, -1]]
        assert exp.stats[2] == 1 and exp.n_core == n - 2 and exp.n_border == 2 and not exp.core[ends].any()
        assert (db.labels_ == 0).all()
    exp, _ = check_all(db, "chain", pts, 0.5, 4)
    assert exp.stats[2] == 0 and exp.n_core == 0 and (db.labels_ == -1).all()


@pytest.mark.parametrize("n", [27, 125, 4096])
def test_lattice(db, n):
    """integer coordinates: d2 = 1 IS a neighbour (the inclusive test), so an inner point has 7 neighbours, a face
    point 6, an edge point 5, a corner 4; one float step below 1 a point has itself only"""
    pts = make_cloud("lattice", n)
    want = {7: (2744, 1176, 176, 1), 5: (4088, 8, 0, 1), 4: (4096, 0, 0, 1)}
    for ms in (7, 5, 4):
        exp, _ = check_all(db, "lattice", pts, 1.0, ms)
        if n == 4096:
            assert (exp.n_core, exp.n_border, exp.n_noise, exp.stats[2]) == want[ms]
    exp, _ = check_all(db, "lattice", pts, DC.BELOW_ONE, 2)
    assert exp.stats[2] == 0 and exp.n_noise == n and (db.labels_ == -1).all()


@pytest.mark.parametrize("swap", [False, True])
def test_contested_border_point(db, swap):
    """a non-core point within eps of a core point of two clusters joins the one with the lower core index, in
    either input order, and unites nothing"""
    pts = DC.contested_cloud(swap)
    exp, details = check_all(db, f"contested{int(swap)}", pts, 1.0, 5)
    mid = 11
    assert details["contested"] == 1 and exp.stats[2] == 2 and exp.n_core == 22 and exp.n_border == 1
    assert db.n_clusters == 2 and db.labels_[mid] == 0 and db.labels_[0] == 0 and db.labels_[12] == 1
    assert mid not in db.core_sample_indices_
    # whichever clump comes first in the input holds core index 0 and takes the point
    assert (pts[db.labels_ == 0, 0] < 1.5).sum() == (12 if not swap else 1)


@pytest.mark.parametrize("n", NS)
def test_duplicates(db, n):
    pts = make_cloud("duplicates", n)
    for ms in sorted({1, max(n, 1)}):  # min_samples <= n: one cluster, all core
        exp, _ = check_all(db, "duplicates", pts, 0.5, ms)
        if n:
            assert exp.stats[2] == 1 and exp.n_core == n and (db.labels_ == 0).all()
    exp, _ = check_all(db, "duplicates", pts, 0.5, n + 1)  # nobody has n + 1 neighbours
    assert exp.stats[2] == 0 and exp.n_core == 0 and (db.labels_ == -1).all()


@pytest.mark.parametrize("n", NS)
def test_nan_and_inf_rows(db, n):
    pts = DC.nan_cloud(n)
    exp, _ = check_all(db, "nan", pts, 1.0, 4)
    bad = ~np.isfinite(pts[:, :3]).all(1)
    assert exp.stats[0] == n - bad.sum() and (exp.labels[bad] == -1).all() and not exp.core[bad].any()
    if n:
        assert bad.any() and (db.labels_[bad] == -1).all() and not np.isin(np.flatnonzero(bad), db.core_sample_indices_).any()
    # not counted as anyone's neighbour: the finite rows alone give the same result for the finite rows
    alone = FL.DBSCAN(1.0, 4)
    alone.fit(pts[~bad])
    np.testing.assert_array_equal(alone.labels_, db.labels_[~bad])
    np.testing.assert_array_equal(np.flatnonzero(~bad)[alone.core_sample_indices_], db.core_sample_indices_)
    alone.close()


def test_far_apart(db):
    """two blobs 1e5 m apart at eps 0.01: the cell cap grows the cell by orders of magnitude above eps, so a cell
    holds many points that are not neighbours"""
    exp, _ = check_all(db, "far", make_cloud("far", 257), 0.01, 3)
    assert exp.stats[2] == 2 and exp.n_noise > 0  # one cluster per blob


@pytest.mark.parametrize("n", [257, 4097])
def test_large_coordinates(db, n):
    """1e6 m from the origin the float spacing is 0.0625 m: what the margin of the scanned cell range is for"""
    exp, _ = check_all(db, "large", DC.large_cloud(n), 0.5, 2)
    if n == 4097:
        assert exp.stats[2] > 0 and exp.n_noise > 0


@pytest.mark.parametrize("stride", [3, 4, 8])
def test_strides(db, stride):
    exp, _ = check_all(db, f"stride{stride}", DC.stride_cloud(stride), 0.7, 4)
    assert exp.stats[2] > 0 and exp.n_border > 0 and exp.n_noise > 0


def test_three_calls_are_identical(db):
    pts = make_cloud("uniform", 4097)
    db.eps, db.min_samples = 1.0, 4
    runs = []
    for _ in range(3):
        db.fit(pts)
        runs.append((db.labels_.copy(), db.core_sample_indices_.copy(), db.offsets.copy(), db.indices.copy(),
                     db.aabb.copy(), db.stats.copy()))
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            np.testing.assert_array_equal(a, b)


def test_input_permutation_gives_the_same_core_set(db):
    """The core set and the clusters' core members do not depend on the input order; a contested border point may
    change sides with it (the contract numbers clusters by input index), so clusters are compared by their core
    points, and the border and noise points as sets."""
    pts = make_cloud("uniform", 4097)
    perm = np.random.default_rng(9).permutation(len(pts))  # row k of the permuted cloud is point perm[k]
    db.eps, db.min_samples = 1.0, 4
    found = db.fit(pts)
    core_a = set(db.core_sample_indices_.tolist())
    a = {frozenset(core_a.intersection(c.tolist())) for c in found}
    clustered_a = set(db.indices.tolist())
    found = db.fit(pts[perm])
    core_b = set(perm[db.core_sample_indices_].tolist())
    b = {frozenset(core_b.intersection(perm[c].tolist())) for c in found}
    assert core_a == core_b and a == b and len(a) == 297
    assert clustered_a == set(perm[db.indices].tolist())
    check(db, pts[perm], DC.reference("uniform-permuted", pts[perm], 1.0, 4)[0], 1.0, 4)


def test_no_allocation_on_a_second_or_smaller_call():
    L = _capi.lib()
    h = FL.DBSCAN(1.0, 4)
    large, small = make_cloud("uniform", 4097), make_cloud("uniform", 257)
    a0 = L.lio_alloc_count()
    h.fit(large)
    a1 = L.lio_alloc_count()
    assert a1 > a0
    h.fit(large)
    assert L.lio_alloc_count() == a1
    h.fit(small)
    assert L.lio_alloc_count() == a1
    check(h, small, DC.reference("uniform", small, 1.0, 4)[0], 1.0, 4)
    assert L.lio_alloc_count() == a1
    # the Euclidean clusters and DBSCAN alternating on ONE handle (they share its arenas): each still equals its
    # reference, and nothing is allocated
    ref = EC.Ref(large, EC.components("uniform", large, 1.0), 2, 60)
    for _ in range(2):
        labels = np.full(len(large), -7, np.int32)
        m = C.c_int64(-1)
        assert L.lio_euclidean_clusters(h._h, large.ctypes.data_as(_capi.fp), len(large), 4, 1.0, 2, 60,
                                        labels.ctypes.data_as(i32p), C.byref(m), 0, None, None, None, None) == 0
        assert m.value == ref.stats[2]
        np.testing.assert_array_equal(labels, ref.labels)
        check(h, large, DC.reference("uniform", large, 1.0, 4)[0], 1.0, 4)
    assert L.lio_alloc_count() == a1
    h.close()


def test_bad_arguments_leave_the_handle_usable():
    L = _capi.lib()
    h = FL.DBSCAN(1.0, 4)
    pts = make_cloud("uniform", 257)
    labels = np.zeros(len(pts), np.int32)
    m = C.c_int64(0)
    fp, lp = pts.ctypes.data_as(_capi.fp), labels.ctypes.data_as(i32p)

    def call(p=fp, n=len(pts), stride=4, eps=1.0, min_samples=4, lab=lp, count=C.byref(m), cap=0):
        return L.lio_dbscan(h._h, p, n, stride, eps, min_samples, lab, None, count, cap, None, None, None, None)

    bad = [dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")), dict(min_samples=0),
           dict(min_samples=-3), dict(stride=2), dict(stride=9), dict(n=-1), dict(n=2**31), dict(cap=-1),
           dict(count=None), dict(p=None), dict(lab=None)]
    for kw in bad:
        assert call(**kw) == _capi.LIO_ERR_ARG, kw
        assert b"lio_dbscan" in L.lio_last_error()
    assert call(n=0) == 0 and m.value == 0
    assert call(n=0, p=None, lab=None) == 0 and m.value == 0
    assert call(min_samples=2**40) == 0 and m.value == 0  # legal: nobody is core
    check(h, pts, DC.reference("uniform", pts, 1.0, 4)[0], 1.0, 4)
    h.close()


def make_scene():
    """a 12 m x 12 m ground plane (z noise 2 cm), six objects of 150 points standing on it, sprinkled points"""
    rng = np.random.default_rng(5)
    ground = np.concatenate([rng.uniform(-6, 6, (3000, 2)), rng.normal(0, 0.02, (3000, 1))], 1)
    centres = np.array([[-4, -4, 1.0], [-4, 3, 1.2], [0, 0, 0.9], [3, -3, 1.5], [4, 4, 1.1], [1, 4, 2.0]])
    objects = np.concatenate([c + rng.normal(0, 0.12, (150, 3)) for c in centres])
    sprinkle = np.concatenate([rng.uniform(-6, 6, (60, 2)), rng.uniform(0.6, 3, (60, 1))], 1)
    xyz = np.concatenate([ground, objects, sprinkle])
    return np.concatenate([xyz, rng.uniform(0, 1, (len(xyz), 1))], 1).astype(f32)[rng.permutation(len(xyz))]


def test_pipeline_with_dbscan_equals_its_stages():
    pts = make_scene()
    out = FL.cluster_objects(pts, 20, 8.0, seed=3, method="dbscan", tolerance=0.5, min_samples=10)
    assert set(out) == {"clusters", "aabb", "plane", "ground", "kept", "noise"}
    sor = FL.StatisticalOutlierRemoval(20, 8.0)  # a wide threshold: the sprinkled points stay, for DBSCAN to call noise
    filtered = sor.filter(pts)
    kept = np.flatnonzero(~(sor.distances.astype(f64) > sor.stats[2]))
    seg = FL.PlaneSegmentation()
    plane, inl = seg.segment_plane(filtered, 0.2, 3, 1000, 3)
    rest = np.flatnonzero(seg.mask == 0)
    stage = FL.DBSCAN(0.5, 10)
    found = stage.fit(filtered[rest])
    np.testing.assert_array_equal(out["kept"], kept)
    np.testing.assert_array_equal(out["plane"], plane)
    np.testing.assert_array_equal(out["ground"], kept[inl])
    np.testing.assert_array_equal(out["aabb"], stage.aabb)
    np.testing.assert_array_equal(out["noise"], kept[rest][stage.labels_ < 0])
    assert len(out["clusters"]) == len(found) == 6 and len(out["noise"]) > 0
    for a, b in zip(out["clusters"], found):
        np.testing.assert_array_equal(a, kept[rest][b])
    # and the stage itself against the reference
    check(stage, filtered[rest], DC.reference("scene", filtered[rest], 0.5, 10)[0], 0.5, 10)
    # the default method is the Euclidean stage, with the dict it always returned
    default = FL.cluster_objects(pts, 20, 8.0, seed=3)
    ec = FL.EuclideanClusterExtraction(0.5, 10, 10000)
    found = ec.extract(filtered[rest])
    assert set(default) == {"clusters", "aabb", "plane", "ground", "kept"}
    np.testing.assert_array_equal(default["aabb"], ec.aabb)
    np.testing.assert_array_equal(default["kept"], kept)
    np.testing.assert_array_equal(default["ground"], kept[inl])
    assert len(default["clusters"]) == len(found) > 0
    for a, b in zip(default["clusters"], found):
        np.testing.assert_array_equal(a, kept[rest][b])
    for h in (sor, seg, stage, ec):
        h.close()
