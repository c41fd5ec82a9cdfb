"""The clouds and parameters of the DBSCAN tests (tests/test_gpu_dbscan.py runs them on the GPU,
tests/test_dbscan_ref.py holds the two references of tests/dbscan_ref.py against each other on the same list), and
the references' results, computed once per cloud and shared.  Test infrastructure only."""
import numpy as np

import dbscan_ref as R
from test_gpu_cluster import make_cloud  # the clouds of the Euclidean tests, same seed rule

f32, f64 = np.float32, np.float64
NS = (0, 1, 2, 63, 64, 65, 257, 4097)
BELOW_ONE = float(np.nextafter(f32(1), f32(0)))  # one float step below 1


def nan_cloud(n):
    pts = make_cloud("uniform", n, seed=1)
    pts[::97, 1] = np.nan
    pts[50::97, 0] = np.inf
    pts[60::97, 2] = -np.inf
    return pts


def large_cloud(n):
    pts = make_cloud("uniform", n)
    pts[:, :3] = (pts[:, :3].astype(f64) + 1e6).astype(f32)
    return pts


def stride_cloud(stride):
    return np.random.default_rng(stride).uniform(-4, 4, (700, stride)).astype(f32)


def contested_cloud(swap):
    """Two clumps of core points and one non-core point within eps = 1 of a core point of each (min_samples 5):
    10 points at x = -0.9 and one at 0 (11 neighbours each), mirrored at x = 2.9 and 2, and the contested point at
    x = 1 with 3 neighbours.  swap: the right clump comes first in the input, so it holds the lower core index."""
    left = np.array([[-0.9, 0, 0]] * 10 + [[0.0, 0, 0]], f64)
    right = np.array([[2.9, 0, 0]] * 10 + [[2.0, 0, 0]], f64)
    mid = np.array([[1.0, 0, 0]], f64)
    xyz = np.concatenate([right, mid, left] if swap else [left, mid, right])
    return np.concatenate([xyz, np.ones((len(xyz), 1))], 1).astype(f32)


_graphs, _results = {}, {}


def reference(key, pts, eps, min_samples):
    """(Expected, details) of dbscan_sets for this cloud; the neighbour graph is shared between min_samples"""
    gk = (key, len(pts), float(eps))
    if gk not in _graphs:
        _graphs[gk] = R.neighbour_graph(pts, eps)
    rk = gk + (int(min_samples),)
    if rk not in _results:
        fin, g = _graphs[gk]
        details = {}
        labels, core = R.dbscan_sets(len(pts), fin, g, min_samples, details)
        _results[rk] = (R.Expected(pts, labels, core), details)
    return _results[rk]


def graph(key, pts, eps):
    reference(key, pts, eps, 1)
    return _graphs[(key, len(pts), float(eps))]


def all_cases():
    """(key, cloud, eps, min_samples) of every GPU comparison"""
    out = []
    for n in NS:
        for eps, ms in ((1.0, 4), (1.6, 10), (1.0, 1), (0.5, 10)):
            out.append(("uniform", make_cloud("uniform", n), eps, ms))
        for eps, ms in ((0.5, 10), (0.3, 3)):
            out.append(("blobs", make_cloud("blobs", n), eps, ms))
        for ms in (3, 4):
            out.append(("chain", make_cloud("chain", n), 0.5, ms))
        for ms in sorted({1, max(n, 1), n + 1}):
            out.append(("duplicates", make_cloud("duplicates", n), 0.5, ms))
        out.append(("nan", nan_cloud(n), 1.0, 4))
    for n in (27, 125, 4096):
        for ms in (7, 5, 4):
            out.append(("lattice", make_cloud("lattice", n), 1.0, ms))
        out.append(("lattice", make_cloud("lattice", n), BELOW_ONE, 2))
    for swap in (False, True):
        out.append((f"contested{int(swap)}", contested_cloud(swap), 1.0, 5))
    out.append(("far", make_cloud("far", 257), 0.01, 3))
    for n in (257, 4097):
        out.append(("large", large_cloud(n), 0.5, 2))
    for stride in (3, 4, 8):
        out.append((f"stride{stride}", stride_cloud(stride), 0.7, 4))
    return out
