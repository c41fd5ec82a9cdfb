"""The grid searches on the constructed scenes of tests/knn_scenes.py against the brute-force reference
(tests/knn_ref.py brute_knn, tests/icp_stats_ref.py brute_nn): points on cell faces and one float either side,
far offsets and a 20 km extent (where the computed faces round), every cell population 0..70 and shell-1 table
size 1..70, flat and thin grids, a table that grows its cell, and rows that are not finite.

Ids and squared distances are compared with assert_array_equal: there is no tolerance in this file (the sums of
an evaluation keep test_gpu_parity's 1e-9, the order of a double sum).  tests/test_knn_ref.py proves the
reference against the oracle's kd-tree on the same scenes and counts what each scene holds.
"""
import time

import numpy as np
import pytest

import knn_scenes as S
from icp_stats_ref import brute_nn
from knn_ref import F32, brute_knn
from lio_gpu import frontend as F
from lio_gpu import loop_closure as LC
from test_gpu_icp import check_nn
from test_gpu_map import _knn_parity, _same_map
from test_gpu_parity import _check_sums, _oracle_eval

pytestmark = pytest.mark.gpu

NAMES = list(S.SCENES)
FAR_AWAY = np.float32(9.0e8)  # stands in for a row that is not finite where the oracle needs finite input


def _build(sc):
    tree = F.IkdTreeGPU(cell_size=sc.cell)
    tree.Build(sc.pts)
    g = tree.grid()
    np.testing.assert_array_equal(g["origin"].astype(np.float32), sc.origin)  # the scene was placed by this grid
    np.testing.assert_array_equal(g["dims"], sc.dims)
    assert g["cell"] == sc.cell_eff
    assert tree.size() == int(np.isfinite(sc.pts).all(axis=1).sum()) and tree.num_ids() == len(sc.pts)
    return tree


def _finite_or_far(a):
    a = np.array(a, np.float32)
    a[~np.isfinite(a).all(axis=1)] = FAR_AWAY
    return a


def _shifts(sc):
    ulp = float(np.spacing(F32(max(1.0, np.abs(sc.centre).max()))))
    return (ulp, 0.02, 0.3)


@pytest.mark.parametrize("name", NAMES)
def test_front_end_and_seeded_lists_exact(oracle, name):
    sc = S.SCENES[name]()
    tree = _build(sc)
    q = sc.queries if sc.queries_far is None else np.concatenate([sc.queries, sc.queries_far])
    body = sc.body(q)
    bad = ~np.isfinite(body).all(axis=1)
    hm = F.HShareModelGPU(tree)
    hm.set_scan(body)
    p24 = S.pose24(sc)
    g = hm(p24, converge=True)
    world = oracle.body_to_world(p24, body)
    np.testing.assert_array_equal(world[~bad], q[~bad])  # the pose gives the scene's queries back bit for bit
    np.testing.assert_array_equal(hm.world()[~bad], world[~bad])
    bi, bd = S.scene_knn(sc, 5, S.RANGE_SQ) if q is sc.queries else brute_knn(q, sc.pts, 5, S.RANGE_SQ)
    gi, gd = hm.nearest_points()
    np.testing.assert_array_equal(gi, bi)
    np.testing.assert_array_equal(gd, bd)
    assert (gi[bad] == -1).all()
    # sel and the sums: the oracle's h_share_model over the same scan, rows that are not finite moved far away
    om = oracle.OracleMap(_finite_or_far(sc.pts))
    o, nn, sel, _ = _oracle_eval(oracle, om, _finite_or_far(body), p24)
    np.testing.assert_array_equal(nn, bi)
    gsel = hm.normvec()[1]
    np.testing.assert_array_equal(gsel, sel)
    assert not gsel[bad].any()
    _check_sums(g, o)
    # seeded second evaluations of the same context: one float of the offset, 2 cm, 30 cm
    for hm2, scale in ((hm, 1.0), (F.HShareModelGPU(tree), 0.5)):
        if hm2 is not hm:  # the guard: a bound shrunk below the true 5th distance goes to the whole-box far pass
            hm2.set_seed_scale(scale)
            hm2.set_scan(body)
            hm2(p24, converge=True)
        for s in _shifts(sc):
            p2 = S.pose24(sc, (s, -0.5 * s, 0.25 * s))
            hm2(p2, converge=True)
            w2 = oracle.body_to_world(p2, body)
            ri, rd = brute_knn(w2, sc.pts, 5, S.RANGE_SQ)
            gi, gd = hm2.nearest_points()
            np.testing.assert_array_equal(gi, ri, err_msg=f"seed scale {scale} shift {s}")
            np.testing.assert_array_equal(gd, rd, err_msg=f"seed scale {scale} shift {s}")
        hm2.close()


@pytest.mark.parametrize("name", NAMES)
def test_nearest_search_exact(name):
    sc = S.SCENES[name]()
    tree = _build(sc)
    for max_dist in (np.inf, 2.0, 0.3):
        q = sc.queries
        if sc.queries_far is not None and np.isfinite(max_dist):
            q = np.concatenate([q, sc.queries_far])
        rs = np.inf if np.isinf(max_dist) else F32(max_dist) * F32(max_dist)
        b5 = brute_knn(q, sc.pts, 5, rs) if (q is not sc.queries or np.isfinite(rs)) else S.scene_knn(sc, 5, np.inf)
        for k in (1, 3, 5):
            gi, gd = tree.Nearest_Search(q, k, max_dist)
            np.testing.assert_array_equal(gi, b5[0][:, :k], err_msg=f"k {k} max_dist {max_dist}")
            np.testing.assert_array_equal(gd, b5[1][:, :k], err_msg=f"k {k} max_dist {max_dist}")


@pytest.mark.parametrize("name", S.ICP_SCENES)
def test_icp_nn_exact(name):
    sc = S.SCENES[name]()
    lc = LC.LoopClosure(LC.LoopClosureConfig(), cell_size=sc.cell)
    lc.setInputSource(sc.queries)
    lc.setInputTarget(sc.pts)
    lc.align(guess=np.eye(4, dtype=np.float32))
    ids, d2 = lc.correspondences()
    check_nn(lc, ids, d2, sc.pts)


@pytest.mark.parametrize("cell", S.CELLS)
def test_icp_nn_exact_without_the_rows_that_are_not_finite(cell):
    sc = S.nonfinite(cell, "scan")
    src = sc.queries[np.isfinite(sc.queries).all(axis=1)]  # as the caller would
    lc = LC.LoopClosure(LC.LoopClosureConfig(), cell_size=cell)
    lc.setInputSource(src)
    lc.setInputTarget(sc.pts)
    lc.align(guess=np.eye(4, dtype=np.float32))
    ids, d2 = lc.correspondences()
    bi, bd = brute_nn(lc.getFinalAlignedCloud(), sc.pts)
    np.testing.assert_array_equal(d2, bd)
    np.testing.assert_array_equal(ids, bi)


def _device_free_bytes():
    """hipMemGetInfo of the runtime the library runs on (0 where its symbols are not global)"""
    import ctypes as C

    try:
        free, total = C.c_size_t(0), C.c_size_t(0)
        C.CDLL(None).hipMemGetInfo(C.byref(free), C.byref(total))
        return int(free.value)
    except (AttributeError, OSError):
        return 0


def _brute_parity(tree, om, q):
    """the updated map's kNN against the reference over the oracle's content (deleted ids are no candidates)"""
    xyz, alive = om.by_id()
    pts = np.where(alive[:, None], xyz, np.float32(np.nan))
    for k, md in ((5, np.inf), (5, 2.0), (1, np.inf)):
        gi, gd = tree.Nearest_Search(q, k, md)
        bi, bd = brute_knn(q, pts, k, np.inf if np.isinf(md) else F32(md) * F32(md))
        np.testing.assert_array_equal(gi, bi)
        np.testing.assert_array_equal(gd, bd)


def test_map_maintenance_at_an_offset(oracle):
    """Build half, Add_Points the rest without and with downsampling, delete a box over one cluster: content and
    kNN against OracleDynMap after each step, 1e5 / -2e5 m from the origin, cell 0.6."""
    sc = S.faces(0.6, S.OFFSETS[2])
    rng = np.random.default_rng(7)
    perm = rng.permutation(len(sc.pts))
    half, rest = sc.pts[perm[: len(perm) // 2]], sc.pts[perm[len(perm) // 2:]]
    tree = F.IkdTreeGPU(cell_size=0.6, downsample_size=0.5)
    tree.Build(half)
    om = oracle.OracleDynMap(half)
    q = sc.queries

    def same():
        _same_map(tree, om)
        _knn_parity(tree, om, q)
        _brute_parity(tree, om, q)

    same()
    a, b = rest[: len(rest) // 2], rest[len(rest) // 2:]
    assert tree.Add_Points(a, False) == om.add(a, False, 0.5)
    same()
    assert tree.Add_Points(b, True) == om.add(b, True, 0.5)
    same()
    lo = sc.centre + 2.0 * 0.6
    box = np.concatenate([lo, lo + 5.0 * 0.6])[None]
    n_del = tree.Delete_Point_Boxes(box)
    assert n_del == om.delete_boxes(box) and n_del > 100
    same()


def test_grown_cell_map_add_points(oracle, capsys):
    """The table of the 1.0 m grid would exceed 2^29 cells: Build doubles the cell.  An Add_Points batch into the
    second cluster keeps the content and the kNN exact.  Prints the device memory and the time of the Build."""
    sc = S.grown()
    free0 = _device_free_bytes()
    t0 = time.perf_counter()
    tree = _build(sc)
    dt = time.perf_counter() - t0
    used = free0 - _device_free_bytes()
    g = tree.grid()
    assert g["cell"] == 2.0 and np.array_equal(g["dims"], sc.dims)
    om = oracle.OracleDynMap(sc.pts)
    add = sc.info["add"]
    t0 = time.perf_counter()
    n_gpu = tree.Add_Points(add, False)
    dt_add = time.perf_counter() - t0
    with capsys.disabled():
        print(f"\n[grown cell] Build {dt * 1e3:.1f} ms, Add_Points {dt_add * 1e3:.1f} ms, device memory "
              f"{used / 2**30:.2f} GiB, dims {sc.dims.tolist()}")
    assert n_gpu == om.add(add, False, 0.5)
    _same_map(tree, om)
    _knn_parity(tree, om, sc.queries)
    _brute_parity(tree, om, sc.queries)
    assert tree.grid()["cell"] == 2.0
