"""The references the GPU DBSCAN is held against (tests/dbscan_ref.py) are themselves checked here, on the CPU:
the contract as sets and the literal sequential procedure agree exactly on every cloud of the GPU tests, and both
equal scikit-learn's DBSCAN where it is installed."""
import numpy as np
import pytest

import dbscan_cases as DC
import dbscan_ref as R
from test_gpu_cluster import make_cloud

f64 = np.float64


def test_sets_and_sequential_agree_on_every_cloud_of_the_gpu_tests():
    seen = dict(clusters=0, border=0, noise=0, contested=0)
    for key, pts, eps, ms in DC.all_cases():
        exp, details = DC.reference(key, pts, eps, ms)
        fin, g = DC.graph(key, pts, eps)
        labels, core = R.dbscan_sequential(len(pts), fin, g, ms)
        msg = f"{key} n={len(pts)} eps={eps} min_samples={ms}"
        np.testing.assert_array_equal(labels, exp.labels, err_msg=msg)
        np.testing.assert_array_equal(core, exp.core, err_msg=msg)
        seen["clusters"] += exp.stats[2]
        seen["border"] += exp.n_border
        seen["noise"] += exp.n_noise
        seen["contested"] += details["contested"]
    assert all(v > 0 for v in seen.values()), seen  # the list exercises every part of the contract


def test_the_figures_the_gpu_tests_assert():
    pts = make_cloud("uniform", 4097)
    for (eps, ms), want in {(1.0, 4): (297, 1339, 1037, 48, 1721), (1.6, 10): (18, 1691, 1843, 61, 563)}.items():
        exp, details = DC.reference("uniform", pts, eps, ms)
        assert (exp.stats[2], exp.n_core, exp.n_border, details["contested"], exp.n_noise) == want
    exp, _ = DC.reference("uniform", pts, 0.5, 10)
    assert exp.stats[2] == 0 and (exp.labels == -1).all() and not exp.core.any()
    exp, _ = DC.reference("uniform", pts, 1.0, 1)
    assert exp.core.all()
    exp, _ = DC.reference("blobs", make_cloud("blobs", 4097), 0.5, 10)
    assert exp.stats[2] == 40


@pytest.mark.parametrize("eps,min_samples", [(0.3, 3), (0.5, 10), (1.0, 4), (1.6, 10)])
@pytest.mark.parametrize("n", [257, 4097])
@pytest.mark.parametrize("kind", ["uniform", "blobs"])
def test_both_equal_scikit_learn(kind, n, eps, min_samples):
    cluster = pytest.importorskip("sklearn.cluster")
    pts = make_cloud(kind, n)
    x = pts[:, :3].astype(f64)
    # float32 and float64 cannot disagree about <=: no pair lies within 1e-6 (relative) of the radius
    e2 = f64(eps) * f64(eps)
    for i0 in range(0, n, 512):
        d2 = ((x[i0:i0 + 512, None, :] - x[None, :, :]) ** 2).sum(-1)
        assert not (np.abs(d2 - e2) <= 1e-6 * e2).any()
    sk = cluster.DBSCAN(eps=eps, min_samples=min_samples).fit(x)
    exp, _ = DC.reference(kind, pts, eps, min_samples)
    np.testing.assert_array_equal(sk.labels_, exp.labels)
    np.testing.assert_array_equal(sk.core_sample_indices_, exp.core_indices)
    fin, g = DC.graph(kind, pts, eps)
    labels, core = R.dbscan_sequential(n, fin, g, min_samples)
    np.testing.assert_array_equal(sk.labels_, labels)
    np.testing.assert_array_equal(sk.core_sample_indices_, np.flatnonzero(core))
