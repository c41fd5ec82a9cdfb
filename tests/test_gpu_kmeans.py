"""GPU checks of k-means (lio_kmeans.hip, lio_kmeans) against tests/kmeans_ref.py, the numpy restatement of its
contract (tests/test_kmeans_ref.py checks that file on the CPU).  EVERY comparison is exact: labels, centres as
float bits, compactness and the per-attempt integer sums, iterations, seeds, counts, boxes as float bits, stats.

The shapes are the smallest at which a kernel can go wrong: the seeding passes take 1024 points per workgroup
(256 threads x 4), the prefix search is two levels of 1024, the assign kernel walks rows of 256 and adds per
wave of 64 — so n runs over K, K + 1, 63 / 64 / 65, 255 / 256 / 257, 4097 (four chunks and one point) and
70 001 (69 chunks, a ragged tail; 274 rows for the assign kernel)."""
import ctypes as C

import numpy as np
import pytest

import kmeans_ref as R
from lio_gpu import _capi
from lio_gpu import filters as FL

pytestmark = pytest.mark.gpu
fp, i32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def handle():
    h = FL.KMeans()
    yield h
    h.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sprinkle(pts, every=37):
    """non-finite points, index 0 and n - 1 among them (the caller leaves at least K finite ones)"""
    pts = pts.copy()
    pts[0, 0] = np.nan
    pts[-1, 2] = -np.inf
    pts[5::every, 1] = np.inf
    return pts


def check(h, pts, K=5, max_iter=100, eps=0.1, attempts=3, seed=0, init=None):
    h.n_clusters, h.max_iter, h.eps, h.attempts, h.seed = K, max_iter, eps, attempts, seed
    labels = h.fit(pts, init)
    ref = R.kmeans(pts, K, max_iter, eps, attempts, seed, init)
    what = f"n={len(pts)} K={K} max_iter={max_iter} eps={eps} attempts={attempts} seed={seed}"
    np.testing.assert_array_equal(h.stats, ref["stats"], err_msg=what)
    np.testing.assert_array_equal(h.seeds, ref["seeds"], err_msg=what)
    np.testing.assert_array_equal(h.attempt_iters, ref["attempt_iters"], err_msg=what)
    np.testing.assert_array_equal(h.attempt_q, ref["attempt_q"], err_msg=what)
    np.testing.assert_array_equal(labels, ref["labels"], err_msg=what)
    np.testing.assert_array_equal(_bits(h.cluster_centers_), _bits(ref["centers"]), err_msg=what)
    assert h.inertia_ == ref["compactness"], what
    np.testing.assert_array_equal(h.counts, ref["counts"], err_msg=what)
    np.testing.assert_array_equal(_bits(h.aabb), _bits(ref["aabb"]), err_msg=what)
    assert (h.best_attempt, h.n_iter_) == (int(ref["stats"][1]), int(ref["stats"][2]))
    return ref


@pytest.mark.parametrize("n", ["K", "K+1", 63, 64, 65, 255, 256, 257, 4097, 70001])
@pytest.mark.parametrize("K", [1, 2, 5])
def test_sizes(handle, n, K):
    n = {"K": K, "K+1": K + 1}.get(n, n)
    stride = (3, 4, 8)[(n + K) % 3]
    check(handle, R.uniform_cloud(n, seed=n + K, stride=stride), K)


@pytest.mark.parametrize("n,attempts", [(64, 3), (65, 3), (257, 16), (4097, 3)])
def test_64_clusters(handle, n, attempts):
    ref = check(handle, R.uniform_cloud(n, seed=3, stride=4), 64, attempts=attempts)
    if n == 257:
        assert ref["stats"][1] == 11  # the best of 16 attempts is not the first


@pytest.mark.parametrize("n,K,stride", [(63, 5, 3), (257, 5, 4), (4097, 5, 8), (4097, 64, 4), (70001, 2, 4)])
def test_non_finite_points_take_no_part(handle, n, K, stride):
    pts = _sprinkle(R.uniform_cloud(n, seed=11, stride=stride))
    ref = check(handle, pts, K)
    assert ref["stats"][0] < n and (ref["labels"][[0, 5, n - 1]] == -1).all()


@pytest.mark.parametrize("seed", [2, 6])  # attempt_q of these clouds: the best attempt is 1, then 2
def test_the_best_attempt_is_not_the_first(handle, seed):
    ref = check(handle, R.uniform_cloud(257, seed=seed), 5)
    assert ref["stats"][1] == {2: 1, 6: 2}[seed]
    check(handle, R.uniform_cloud(257, seed=seed), 5, attempts=1)
    check(handle, R.uniform_cloud(257, seed=seed), 5, seed=2**64 - 1)


@pytest.mark.parametrize("max_iter,eps", [(1, 0.1), (2, 0.1), (3, 0.1), (100, 0.0), (100, 1000.0)])
def test_stop_rules(handle, max_iter, eps):
    ref = check(handle, R.uniform_cloud(4097, stride=4), 5, max_iter, eps)
    if max_iter <= 2 or eps == 1000.0:  # max(max_iter, 2); a shift below eps^2 at the first check
        assert ref["attempt_iters"].tolist() == [2, 2, 2]
    if eps == 0.0:
        assert (ref["attempt_iters"] > 3).all()


def test_map_coordinates_use_another_coordinate_scale(handle):
    ref = check(handle, R.blobs(4097, 5, 1.0, 1, 4, (836000.0, 822000.0, 10.0)), 5)
    assert ref["stats"][4] == 20 and ref["stats"][5] == 14


@pytest.mark.parametrize("sigma", [1.0, 4.0])
def test_blobs(handle, sigma):
    check(handle, R.blobs(4097, 5, sigma, seed=1), 5, 100, 0.0)


def test_all_points_identical(handle):
    pts = np.tile(np.array([[1.5, -2.25, 0.75]], np.float32), (64, 1))
    ref = check(handle, pts, 5, attempts=1)
    assert ref["counts"].tolist() == [60, 1, 1, 1, 1] and ref["stats"].tolist() == [64, 0, 2, 4, 2, 0]
    check(handle, pts, 5, attempts=3)
    check(handle, np.zeros((70, 3), np.float32), 64, attempts=2)  # A = 0: ec = 0


def test_n_equals_k(handle):
    ref = check(handle, R.uniform_cloud(5), 5)
    assert ref["counts"].tolist() == [1] * 5
    check(handle, R.uniform_cloud(64, stride=8), 64)


def test_a_tie_goes_to_the_lowest_k(handle):
    xs, ys = np.meshgrid(np.arange(9), np.arange(5), indexing="ij")
    pts = np.stack([xs.ravel(), ys.ravel(), np.zeros(45)], 1).astype(np.float32)
    init = np.array([[[2, 2, 0], [6, 2, 0]]], np.float32)
    ref = check(handle, pts, 2, 1, 0.0, 1, 0, init)
    assert ref["labels"].reshape(9, 5)[:, 0].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1]
    check(handle, pts, 2, 1, 0.0, 1, 0, init[:, ::-1])
    check(handle, pts, 2, 100, 0.0, 1, 0, init)


@pytest.mark.parametrize("n", [257, 4097])
def test_centres_outside_the_cloud_are_repaired(handle, n):
    pts = R.uniform_cloud(n, seed=7, stride=4)
    init = np.array([[pts[0, :3], pts[1, :3], pts[2, :3], [1e4, 1e4, 1e4], [-1e4, 1e4, 0]]], np.float32)
    ref = check(handle, pts, 5, 100, 0.1, 1, 0, init)
    assert ref["stats"][3] == 2
    # every centre far away, one of them at a float distance that overflows: all points to cluster 0, four repairs
    far = np.array([[[1e4, 0, 0], [1e30, 0, 0], [2e4, 0, 0], [3e4, 0, 0], [4e4, 0, 0]]], np.float32)
    ref = check(handle, _sprinkle(pts), 5, 100, 0.1, 1, 0, far)
    assert ref["stats"][3] == 4


def test_init_centers_replace_the_seeding(handle):
    pts = R.uniform_cloud(4097, stride=4)
    seeded = check(handle, pts, 5)
    init = np.stack([pts[s, :3] for s in seeded["seeds"]])
    given = check(handle, pts, 5, init=init)
    np.testing.assert_array_equal(given["labels"], seeded["labels"])
    assert (given["seeds"] == -1).all()


def _raw(h, pts, K, opt=True, attempts=3):
    """lio_kmeans through ctypes with canaries in every output -> (status, outputs)"""
    n = len(pts)
    out = dict(labels=np.full(n, -7, np.int32), centers=np.full((K, 3), -7, np.float32), counts=np.full(K, -7, np.int64),
               aabb=np.full((K, 6), -7, np.float32), seeds=np.full((attempts, K), -7, np.int32),
               attempt_q=np.full(attempts, 7, np.uint64), attempt_iters=np.full(attempts, -7, np.int32),
               stats=np.full(6, -7, np.int64))
    comp = C.c_double(-7.0)
    rc = _capi.lib().lio_kmeans(
        h._h, pts.ctypes.data_as(fp), n, pts.shape[1], K, 100, 0.1, attempts, 0, None, out["labels"].ctypes.data_as(i32p),
        out["centers"].ctypes.data_as(fp), C.byref(comp), out["counts"].ctypes.data_as(i64p) if opt else None,
        out["aabb"].ctypes.data_as(fp) if opt else None, out["seeds"].ctypes.data_as(i32p) if opt else None,
        out["attempt_q"].ctypes.data_as(C.POINTER(C.c_uint64)) if opt else None,
        out["attempt_iters"].ctypes.data_as(i32p) if opt else None, out["stats"].ctypes.data_as(i64p) if opt else None)
    out["compactness"] = comp.value
    return rc, out


def test_every_optional_output_null_at_once(handle):
    pts = _sprinkle(R.uniform_cloud(4097, stride=4))
    rc, out = _raw(handle, pts, 5, opt=False)
    assert rc == 0, _capi.lib().lio_last_error()
    ref = R.kmeans(pts, 5)
    np.testing.assert_array_equal(out["labels"], ref["labels"])
    np.testing.assert_array_equal(_bits(out["centers"]), _bits(ref["centers"]))
    assert out["compactness"] == ref["compactness"]
    for name in ("counts", "aabb", "seeds", "attempt_iters", "stats"):
        assert (out[name] == -7).all(), name


def test_repeated_calls_are_identical_and_allocate_nothing(handle):
    pts = _sprinkle(R.uniform_cloud(70001, stride=4))
    rc, a = _raw(handle, pts, 5)
    assert rc == 0, _capi.lib().lio_last_error()
    before = _capi.lib().lio_alloc_count()
    rc, b = _raw(handle, pts, 5)
    assert rc == 0 and _capi.lib().lio_alloc_count() == before
    for name in a:
        np.testing.assert_array_equal(np.atleast_1d(a[name]).view(np.uint8), np.atleast_1d(b[name]).view(np.uint8), err_msg=name)
    rc, c = _raw(handle, pts[:4097], 64)  # a smaller call on the same handle: still nothing
    assert rc == 0 and _capi.lib().lio_alloc_count() == before


def test_fewer_finite_points_than_clusters(handle):
    pts = R.uniform_cloud(64, stride=4)
    pts[3:, 1] = np.nan  # n >= K, nf = 3 < K = 5: found by the counting pass
    rc, out = _raw(handle, pts, 5)
    assert rc == _capi.LIO_ERR_ARG and b"fewer finite points than clusters" in _capi.lib().lio_last_error()
    assert out["compactness"] == -7.0 and (out["attempt_q"] == 7).all()
    for name in ("labels", "centers", "counts", "aabb", "seeds", "attempt_iters", "stats"):
        assert (out[name] == -7).all(), name
    pts[3:5, 1] = 0.0  # nf = K
    rc, out = _raw(handle, pts, 5)
    assert rc == 0 and out["stats"][0] == 5 and sorted(out["labels"][:5].tolist()) == [0, 1, 2, 3, 4]
