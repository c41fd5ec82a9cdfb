"""The seeded near kNN pass (later kNN evaluations of a scan against an unchanged map) and the far queue's entries.

The seeded pass bounds a query by the exact squared distances of its previous five neighbours, re-gathered by id
(group_knn_seeded); queries it cannot finish go to the far pass as one 64-byte entry each (index, world point,
list).  Every case runs a first evaluation, then one or more seeded ones at other poses, and compares the lists
and their d2 with oracle.OracleMap.knn at the same world points, bit for bit.
"""
import numpy as np
import pytest

import knn_scenes as S
from lio_gpu import frontend as F
from lio_gpu import synth

pytestmark = pytest.mark.gpu

RANGE_SQ = 5.0


@pytest.fixture(scope="module")
def c1(oracle):
    """C1: 200 k map, 16,384-point scan; the oracle map and the first pose are shared (read-only)"""
    _, m, scans = synth.make_config("C1", n_scans=1)
    sc = scans[0]
    return m, sc.body, synth.initial_state(sc.pos_init, sc.rot_init), oracle.OracleMap(m)


def _model(m, body, cell=1.0):
    tree = F.IkdTreeGPU(cell_size=cell)
    tree.Build(m)
    hm = F.HShareModelGPU(tree)
    hm.set_scan(body)
    return hm


def _moved(st, shift=(0.0, 0.0, 0.0), rotvec=None):
    st2 = dict(st)
    st2["pos"] = np.asarray(st["pos"]) + np.asarray(shift, np.float64)
    if rotvec is not None:
        st2["rot"] = synth.quat_mul(st["rot"], synth.rotvec_to_quat(rotvec))
    return st2


def _knn_eval_exact(oracle, om, hm, body, p24, msg=""):
    """one kNN evaluation at p24: the lists and their d2 are the oracle's"""
    hm(p24, converge=True)
    gi, gd = hm.nearest_points()
    oi, od = om.knn(oracle.body_to_world(p24, body), 5, RANGE_SQ)
    np.testing.assert_array_equal(gi, oi, err_msg=msg)
    np.testing.assert_array_equal(gd, od, err_msg=msg)
    return gi, gd


@pytest.mark.parametrize("rotvec", [(0.0, 0.0, np.deg2rad(1.0)), (np.deg2rad(0.5), 0.0, 0.0)], ids=["yaw1", "roll0.5"])
def test_seeded_after_rotation(oracle, c1, rotvec):
    """A pure rotation between the evaluations: the displacement grows with range."""
    m, body, st, om = c1
    hm = _model(m, body)
    hm(synth.pose24(st), converge=True)
    _knn_eval_exact(oracle, om, hm, body, synth.pose24(_moved(st, rotvec=rotvec)))
    hm.close()


def test_seeded_zero_change(oracle, c1):
    """The same pose again: the bound equals the old 5th key exactly, and that neighbour must be kept."""
    m, body, st, om = c1
    hm = _model(m, body)
    p24 = synth.pose24(st)
    i0, d0 = _knn_eval_exact(oracle, om, hm, body, p24)
    i1, d1 = _knn_eval_exact(oracle, om, hm, body, p24)
    np.testing.assert_array_equal(i1, i0)
    np.testing.assert_array_equal(d1, d0)
    hm.close()


def test_seeded_beyond_range(oracle, c1):
    """A 3 m shift: the previous neighbours lie beyond the gate for most queries, which fall back to the range."""
    m, body, st, om = c1
    hm = _model(m, body)
    hm(synth.pose24(st), converge=True)
    p2 = synth.pose24(_moved(st, (3.0, 0.0, 0.0)))
    gi, gd = _knn_eval_exact(oracle, om, hm, body, p2)
    # the premise: for most queries the previous fifth neighbour is now outside the range
    prev = om.knn(oracle.body_to_world(synth.pose24(st), body), 5, RANGE_SQ)[0]
    w2 = oracle.body_to_world(p2, body)
    full = prev[:, 4] >= 0
    d = w2[full] - m[prev[full, 4]]
    assert ((d * d).sum(axis=1) > RANGE_SQ).mean() > 0.5
    hm.close()


def _lattice():
    """a 0.5 m lattice, every point stored twice (two ids): most candidates tie in d2 with others"""
    ax, az = np.arange(0.0, 10.01, 0.5), np.arange(0.0, 4.01, 0.5)
    g = np.stack(np.meshgrid(ax, ax, az, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    pts = np.concatenate([g, g[::-1]])
    rng = np.random.default_rng(7)
    q = rng.integers(4, 36, (1500, 3)).astype(np.float32) * np.float32(0.25)  # lattice points, edge and face centres
    q[:, 2] = np.minimum(q[:, 2], np.float32(3.75))
    return S.Scene("lattice-dup", 1.0, pts, q, np.zeros(3))


def test_seeded_ties_at_the_bound(oracle):
    """Candidates that tie with the bound in d2 are ordered by id against the (bound, none) filler."""
    sc = _lattice()
    body = sc.body()
    om = oracle.OracleMap(sc.pts)
    hm = _model(sc.pts, body)
    hm(S.pose24(sc), converge=True)
    for shift in ((0.0, 0.0, 0.0), (0.25, 0.0, 0.0), (0.25, -0.5, 0.25)):  # exact in float: the ties survive
        p2 = S.pose24(sc, shift)
        gi, gd = _knn_eval_exact(oracle, om, hm, body, p2, msg=f"shift {shift}")
        assert (gd[:, 4] == gd[:, 3]).mean() > 0.5  # ties at the fifth place
    hm.close()


@pytest.mark.parametrize("kind", ["plane", "one"])
def test_seeded_previous_lists_not_full(oracle, kind):
    """A thin map: many previous lists are not full, those queries start from the range."""
    sc = S.thin(1.0, kind)
    body = sc.body()
    om = oracle.OracleMap(sc.pts)
    hm = _model(sc.pts, body)
    i0, _ = _knn_eval_exact(oracle, om, hm, body, S.pose24(sc))
    assert (i0[:, 4] < 0).sum() >= 50
    for s in (0.02, 0.3):
        _knn_eval_exact(oracle, om, hm, body, S.pose24(sc, (s, -0.5 * s, 0.25 * s)), msg=f"shift {s}")
    hm.close()


@pytest.mark.parametrize("scale", [1.0, 0.05])
def test_seeded_far_queue_entries(oracle, c1, scale):
    """A sparse map queues many queries for the far pass (index, world point and list travel in the queue entry);
    with the bound shrunk (scale 0.05) the seeded pass's guard queues them with the whole-box bit."""
    m, body, st, _ = c1
    sparse, body = np.ascontiguousarray(m[::4]), body[:4096]  # every list still full, ~30 % of the queries queued
    om = oracle.OracleMap(sparse)
    hm = _model(sparse, body)
    hm.set_seed_scale(scale)
    p2 = synth.pose24(_moved(st, (0.05, -0.03, 0.02), (0.0, 0.0, np.deg2rad(0.3))))
    queued = int((hm.knn_stats(p2)[1][:, 2] == 2).sum())  # unseeded walk at that pose: left to the far pass
    assert queued >= 50, queued
    hm.set_scan(body)
    _knn_eval_exact(oracle, om, hm, body, synth.pose24(st))
    _knn_eval_exact(oracle, om, hm, body, p2)
    hm.close()


@pytest.mark.parametrize("n", [5, 33, 16384 - 7])
def test_seeded_block_edges(oracle, c1, n):
    """A partial block, a partial second block and a ragged tail of the 32-query blocks."""
    m, body, st, om = c1
    body = body[:n]
    hm = _model(m, body)
    hm(synth.pose24(st), converge=True)
    _knn_eval_exact(oracle, om, hm, body, synth.pose24(_moved(st, (0.1, -0.08, 0.05), (0.0, 0.0, np.deg2rad(0.5)))))
    hm.close()


def test_seeded_three_in_a_row(oracle, c1):
    """The second seeded pass seeds from lists the first seeded pass wrote."""
    m, body, st, om = c1
    hm = _model(m, body)
    hm(synth.pose24(st), converge=True)
    _knn_eval_exact(oracle, om, hm, body, synth.pose24(_moved(st, (0.1, -0.08, 0.05), (0.0, 0.0, np.deg2rad(0.5)))))
    _knn_eval_exact(oracle, om, hm, body, synth.pose24(_moved(st, (0.13, -0.07, 0.04), (0.002, 0.0, np.deg2rad(0.45)))))
    hm.close()
