"""CPU checks of tests/kmeans_ref.py, the numpy restatement of lio_kmeans' contract (include/lio_gpu.h) that
tests/test_gpu_kmeans.py holds the library to: its own invariants (every centre the fixed-point mean of its
members, sums independent of the point order, fixed draws), agreement with scikit-learn's Lloyd from the same
initial centres, and the edge cases with their figures recorded."""
import math

import numpy as np
import pytest

import kmeans_ref as R


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_every_centre_is_the_fixed_point_mean_of_its_members():
    pts = R.uniform_cloud(4097, stride=4)
    pts[[0, 77, 4096], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    r = R.kmeans(pts, 5, 100, 0.1, 3, 0)
    nf, ec = int(r["stats"][0]), int(r["stats"][4])
    assert nf == 4094 and (r["labels"][[0, 77, 4096]] == -1).all() and (r["labels"] >= 0).sum() == nf
    for k in range(5):
        members = pts[r["labels"] == k, :3]
        S = R.quant_x(members, ec).sum(0)
        assert len(members) == r["counts"][k]
        np.testing.assert_array_equal(_bits(R.mean_of(S, len(members), ec)), _bits(r["centers"][k]))
    # the compactness is the winning attempt's integer sum, scaled
    a = int(r["stats"][1])
    assert r["attempt_q"][a] == r["attempt_q"].min() and a == int(np.argmin(r["attempt_q"]))
    assert r["compactness"] == math.ldexp(float(int(r["attempt_q"][a])), int(r["stats"][5]) - 31)


def test_sums_do_not_depend_on_the_point_order():
    pts = R.uniform_cloud(4097)
    first = R.kmeans(pts, 5, 100, 0.1, 3, 0)
    init = np.stack([pts[s, :3] for s in first["seeds"]])
    base = R.kmeans(pts, 5, 100, 0.1, 3, 0, init)
    # the seeding's centres given as init_centers reproduce the seeded run
    np.testing.assert_array_equal(base["labels"], first["labels"])
    np.testing.assert_array_equal(base["attempt_q"], first["attempt_q"])
    assert (base["seeds"] == -1).all()
    perm = np.random.default_rng(5).permutation(len(pts))
    other = R.kmeans(pts[perm], 5, 100, 0.1, 3, 0, init)
    np.testing.assert_array_equal(_bits(other["centers"]), _bits(base["centers"]))
    np.testing.assert_array_equal(other["attempt_q"], base["attempt_q"])
    np.testing.assert_array_equal(other["attempt_iters"], base["attempt_iters"])
    np.testing.assert_array_equal(other["labels"], base["labels"][perm])
    np.testing.assert_array_equal(_bits(other["aabb"]), _bits(base["aabb"]))


def test_the_draws_are_fixed():
    # splitmix64 of seed + (c + 1) * golden: the first outputs of the generator for seed 0 (its published vector)
    assert R.draw(0, 0) == 0xE220A8397B1DCDAF and R.draw(0, 1) == 0x6E789E6AA1B965F4
    r = R.kmeans(R.uniform_cloud(4097), 5, 100, 0.1, 3, 0)
    assert r["seeds"].tolist() == [[3293, 438, 3126, 3129, 2887], [1828, 3469, 2727, 1687, 2616],
                                   [185, 1627, 1728, 1227, 125]]
    assert r["attempt_iters"].tolist() == [24, 25, 16]
    assert r["attempt_q"].tolist() == [125298042561, 125298042561, 126488385448]
    assert r["stats"].tolist() == [4097, 0, 24, 0, 6, 14]  # equal cq: the lowest attempt
    assert r["counts"].tolist() == [736, 908, 767, 699, 987]
    # centre 0 of attempt a is the (r mod nf)-th FINITE point
    pts = R.uniform_cloud(4097)
    pts[:100, 1] = np.nan
    s = R.kmeans(pts, 5, 2, 0.1, 2, 0)["seeds"]
    assert s[0, 0] == 100 + R.draw(0, 0) % 3997 and s[1, 0] == 100 + R.draw(0, 15) % 3997


@pytest.mark.parametrize("sigma", [1.0, 4.0])
def test_agreement_with_scikit_learn(sigma):
    """Our side: eps 0, max_iter 100, seeded by our own k-means++.  Their side: Lloyd from the same points as
    initial centres, in double, tol 0.  ALL labels equal, centres within 1e-5 m, for each of three attempts."""
    cluster = pytest.importorskip("sklearn.cluster")
    pts = R.blobs(4097, 5, sigma, seed=1)
    r = R.kmeans(pts, 5, 100, 0.0, 3, 0)
    X = pts[:, :3].astype(np.float64)
    for a in range(3):
        labels, centers = r["per_attempt"][a]
        assert 2 < r["attempt_iters"][a] < 100
        km = cluster.KMeans(5, init=X[r["seeds"][a]], n_init=1, algorithm="lloyd", tol=0, max_iter=300).fit(X)
        assert km.n_iter_ < 300
        diff = float(np.abs(km.cluster_centers_ - centers.astype(np.float64)).max())
        print(f"sigma {sigma} attempt {a}: {r['attempt_iters'][a]} iterations, {(km.labels_ != labels).sum()} labels "
              f"differ, largest centre difference {diff:.3g} m")
        np.testing.assert_array_equal(km.labels_, labels)
        assert diff <= 1e-5


def test_all_points_identical():
    pts = np.tile(np.array([[1.5, -2.25, 0.75]], np.float32), (64, 1))
    r = R.kmeans(pts, 5, 100, 0.1, 1, 0)
    assert r["counts"].tolist() == [60, 1, 1, 1, 1]
    assert r["stats"].tolist() == [64, 0, 2, 4, 2, 0]  # four repairs, ec = 2 (2.25 = 0.5625 * 2^2), ed = 0
    assert r["attempt_q"].tolist() == [0] and r["compactness"] == 0.0
    # sum0 = 0: every further centre is the lowest finite index; the repairs move the lowest indices
    assert r["seeds"].tolist() == [[int(R.draw(0, 0) % 64), 0, 0, 0, 0]]
    assert r["labels"][:5].tolist() == [1, 2, 3, 4, 0]
    np.testing.assert_array_equal(_bits(r["centers"]), _bits(np.tile(pts[:1], (5, 1))))


def test_n_equals_k():
    pts = R.uniform_cloud(5)
    r = R.kmeans(pts, 5)
    assert sorted(r["labels"].tolist()) == [0, 1, 2, 3, 4] and r["counts"].tolist() == [1] * 5
    assert r["attempt_q"].tolist() == [0, 0, 0] and r["stats"].tolist() == [5, 0, 2, 0, 5, 13]
    np.testing.assert_array_equal(_bits(r["centers"][r["labels"]]), _bits(pts))
    with pytest.raises(ValueError):
        R.kmeans(pts, 6)
    pts[2, 0] = np.nan
    with pytest.raises(ValueError):
        R.kmeans(pts, 5)


def test_a_tie_goes_to_the_lowest_k():
    xs, ys = np.meshgrid(np.arange(9), np.arange(5), indexing="ij")
    pts = np.stack([xs.ravel(), ys.ravel(), np.zeros(45)], 1).astype(np.float32)
    init = np.array([[[2, 2, 0], [6, 2, 0]]], np.float32)  # the column x = 4 is equidistant
    r = R.kmeans(pts, 2, 1, 0.0, 1, 0, init)
    assert r["labels"].reshape(9, 5)[:, 0].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1]
    assert r["counts"].tolist() == [25, 20] and r["stats"].tolist() == [45, 0, 2, 0, 4, 7]
    assert r["centers"].tolist() == [[2.0, 2.0, 0.0], [6.5, 2.0, 0.0]] and r["attempt_q"].tolist() == [2768240640]
    # swapped centres: still the lowest k
    r = R.kmeans(pts, 2, 1, 0.0, 1, 0, init[:, ::-1])
    assert r["labels"].reshape(9, 5)[:, 0].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0]


def test_centres_outside_the_cloud_are_repaired():
    pts = R.uniform_cloud(257, seed=7)
    init = np.array([[pts[0, :3], pts[1, :3], pts[2, :3], [1e4, 1e4, 1e4], [-1e4, 1e4, 0]]], np.float32)
    r = R.kmeans(pts, 5, 100, 0.1, 1, 0, init)
    assert r["stats"].tolist() == [257, 0, 12, 2, 6, 14]  # two repairs
    assert r["counts"].tolist() == [68, 51, 63, 36, 39] and r["attempt_q"].tolist() == [7701066098]
    assert (r["seeds"] == -1).all()
