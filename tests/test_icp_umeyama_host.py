"""Host half of the float fidelity orders, bit for bit (no device needed).

lio_icp_umeyama_pcl_float_order turns the 16 floats of a correspondence pass into the incremental transform
through a float JacobiSVD.  Fed the numpy restatement of those 16 floats (tests/icp_stats_ref.py), it must
equal the oracle's pcl::umeyama restatement on the same pairs in every bit — on generic clouds at the pair
counts where the statistics change path (3 and 4: the smallest; 13 / 14: the lazy product ends; 48: the
depth blocking starts; 681: the second depth block at order 2; 5000: many blocks) and on the degenerate
inputs where the SVD's sign and ordering decisions matter: planar, collinear, all-identical, reflected and
single-target-point pairs.
"""
import numpy as np
import pytest

import icp_stats_ref as R
from lio_gpu import _capi

GENERIC_N = [3, 4, 13, 14, 48, 681, 5000]
DEGENERATE = ["planar", "collinear", "identical", "reflected", "one_target"]


def _rot(axis, ang):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def _pairs(case):
    """(src, tgt) float32 (n, 3): a cloud and its moved, noisy copy"""
    n = case if isinstance(case, int) else 500
    rng = np.random.default_rng(1000 + (n if isinstance(case, int) else DEGENERATE.index(case)))
    src = rng.standard_normal((n, 3)) * [8.0, 5.0, 1.5] + [30.0, -12.0, 2.0]
    Rm, t = _rot(rng.standard_normal(3), rng.uniform(0.01, 0.3)), rng.uniform(-2, 2, 3)
    if case == "planar":
        src[:, 2] = 2.0
    elif case == "collinear":
        src = np.outer(rng.uniform(-20, 20, n), [1.0, 0.5, -0.25]) + [3.0, 1.0, 2.0]
    elif case == "identical":
        src = np.tile([[3.0, -1.0, 2.0]], (n, 1))
    tgt = src @ Rm.T + t
    if case not in ("planar", "collinear", "identical"):
        tgt = tgt + rng.standard_normal((n, 3)) * 0.01
    if case == "reflected":
        tgt[:, 2] = -tgt[:, 2]
    elif case == "one_target":
        tgt = np.tile([[1.0, 2.0, 3.0]], (n, 1))
    return src.astype(np.float32), tgt.astype(np.float32)


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("case", GENERIC_N + DEGENERATE)
def test_umeyama_host_bit_equal_to_oracle(oracle, case, order):
    src, tgt = _pairs(case)
    s16 = R.stats16(src, tgt, order)
    assert int(s16[6:7].view(np.uint32)[0]) == len(src)
    T = np.zeros(16, np.float32)
    L = _capi.lib()
    assert L.lio_icp_umeyama_pcl_float_order(s16.ctypes.data_as(_capi.fp), order, T.ctypes.data_as(_capi.fp)) == 0
    To, sm, dm, sigma = oracle.umeyama_float(src, tgt, order, stats=True)
    # the restated statistics first (so a mismatch names its half): means and sigma as the oracle has them
    oon = np.float32(1) / np.float32(len(src))
    np.testing.assert_array_equal((s16[0:3] * oon).view(np.uint32), sm.view(np.uint32))
    np.testing.assert_array_equal((s16[3:6] * oon).view(np.uint32), dm.view(np.uint32))
    # (+ 0: a chain of -0 products is -0 from its first element and +0 from a zeroed accumulator, which is how
    # the oracle's order 1 starts; the transform below is compared with its signs)
    sg = (s16[7:16] * oon if order == 1 else s16[7:16]) + np.float32(0)
    so = np.ascontiguousarray(sigma).reshape(9) + np.float32(0)
    np.testing.assert_array_equal(sg.view(np.uint32), so.view(np.uint32))
    assert np.all(np.isfinite(To))
    np.testing.assert_array_equal(T.view(np.uint32), np.ascontiguousarray(To).reshape(16).view(np.uint32))
