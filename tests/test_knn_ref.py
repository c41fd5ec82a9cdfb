"""The brute-force kNN reference (tests/knn_ref.py) against the oracle's kd-tree on every constructed scene of
tests/knn_scenes.py, bit for bit, and every scene's "teeth": the counts, computed by the reference alone, that
show the scene holds what it was built for.  No GPU: this proves the reference and the scenes before
tests/test_gpu_knn_faces.py holds the HIP searches against them.

Scene (b) and the stop rules.  The fixed face slack 1e-3 + 1e-4 * cell was documented for |v| < 1e4 m, and one
could expect every cell size that is not a power of two to lose neighbours from 3e4 m on, where one float
spacing (1.95 mm) exceeds it.  Searching every face of every far scene with the walk's own float arithmetic
(own, own + cell, the 0.999999f factor: knn_scenes._trap_combos) shows it is narrower than that: inside one
binade the points, the origin and the faces share one float lattice, v - o is exact, and rounding a face to that
lattice never puts it past the first lattice point of the next cell.  What remains is the second rounding in
lo + cell followed by the off-lattice + cell of the block rule (own + cell), which over-reaches only where the
lattice spacing exceeds the slack AND cell / spacing has a large fractional part, and the rounding of
(float)k * cell once the extent is large.  Over-reaching faces exist at (1e6, 1e6) with cell 0.6, at
(1e5, -2e5) with cell 2.3 and in the 20 km extent scene; none at 3e4 m (cell 0.6: a spacing of 1.95 mm leaves at
most half of it, 0.98 mm, of over-reach against a slack of 1.06 mm) nor, within the own-cell and block rules, at the other
combinations.  The trapped scenes assert at least 50 dropped neighbours under the fixed slack; the others assert
that no face of the scene over-reaches and that the restated rules drop nothing.
"""
import numpy as np
import pytest

import knn_scenes as S
from knn_ref import brute_knn, cell_of, grid_geom, grid_margin

BOUNDS = (S.RANGE_SQ, np.inf)


def _finite_map(sc):
    """(finite rows, their ids): the oracle's kd-tree is built over the finite points only"""
    keep = np.nonzero(np.isfinite(sc.pts).all(axis=1))[0]
    return sc.pts[keep], keep.astype(np.int32)


@pytest.mark.parametrize("name", list(S.SCENES))
def test_brute_knn_equals_oracle_kdtree(oracle, name):
    sc = S.SCENES[name]()
    pts, ids = _finite_map(sc)
    om = oracle.OracleMap(pts)
    for rs in BOUNDS:
        q = sc.queries
        if sc.queries_far is not None and np.isfinite(rs):
            q = np.concatenate([q, sc.queries_far])
        qfin = np.isfinite(q).all(axis=1)
        b5 = S.scene_knn(sc, 5, rs) if q is sc.queries else brute_knn(q, sc.pts, 5, rs)
        assert (b5[0][~qfin] == -1).all() and np.isinf(b5[1][~qfin]).all()
        for k in (1, 3, 5):
            bi, bd = (b5[0][:, :k], b5[1][:, :k]) if k < 5 else b5
            if k == 3:  # the prefix of the 5-list is the 3-list: checked against a direct call once
                di, dd = brute_knn(q[:200], sc.pts, 3, rs)
                np.testing.assert_array_equal(di, bi[:200])
                np.testing.assert_array_equal(dd, bd[:200])
            oi, od = om.knn(q[qfin], k, rs)
            oi = np.where(oi >= 0, ids[np.maximum(oi, 0)], -1)
            np.testing.assert_array_equal(bi[qfin], oi)
            np.testing.assert_array_equal(bd[qfin], od)


def test_brute_knn_equals_oracle_dynmap_after_add_and_delete(oracle):
    sc = S.grown()
    om = oracle.OracleDynMap(sc.pts)
    om.add(sc.info["add"], False, 0.5)
    om.delete_boxes([[2.0, 2.0, 2.0, 5.0, 5.0, 5.0]])
    xyz, alive = om.by_id()
    assert alive.sum() < len(alive) and len(xyz) == len(sc.pts) + len(sc.info["add"])
    pts = np.where(alive[:, None], xyz, np.float32(np.nan))  # deleted ids: never candidates, ids unchanged
    for k, rs in ((5, S.RANGE_SQ), (3, np.inf), (1, S.RANGE_SQ)):
        bi, bd = brute_knn(sc.queries, pts, k, rs)
        oi, od = om.knn(sc.queries, k, rs)
        np.testing.assert_array_equal(bi, oi)
        np.testing.assert_array_equal(bd, od)


# ------------------------------------------------------------------ teeth
FACE_SCENES = [k for k in S.SCENES if k.split("-")[0] in ("faces", "far", "extent")]


@pytest.mark.parametrize("name", FACE_SCENES)
def test_teeth_faces_and_ties(name):
    sc = S.SCENES[name]()
    ids, _ = S.scene_knn(sc, 5, S.RANGE_SQ)
    assert S.shared_face_teeth(sc, ids).sum() >= 200
    assert S.tie_teeth(sc).sum() >= 50
    # the points on the faces: on one, two and three axes at once, the face itself and one float either side
    o, cs = sc.origin, sc.cell_eff
    kb = sc.info["kbase"]
    onface = np.zeros(len(sc.pts), int)
    for a in range(3):
        f = S.face(o[a], np.arange(int(kb[a]) + 2, int(kb[a]) + S.NC), cs)
        near = np.concatenate([f, np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))])
        onface += np.isin(sc.pts[:, a], near)
    assert all((onface == n).sum() >= 100 for n in (1, 2, 3))


@pytest.mark.parametrize("name", [k for k in S.SCENES if k.startswith("far") or k.startswith("extent")])
def test_teeth_stop_rules_at_far_offsets(name):
    sc = S.SCENES[name]()
    if name in S.TRAPPED:
        assert sc.info["n_combos"] > 0
        drops = S.early_stop_drops(sc, bound=S.TRAPPED[name])
        assert drops.sum() >= 50
        assert (~drops.any(axis=0)).sum() > 1000  # and most queries are no traps
        m = grid_margin(sc.origin, sc.cell_eff, sc.dims)  # the slack that grows with the geometry holds them
        assert m > sc.margin and S.early_stop_drops(sc, margin=m, bound=S.TRAPPED[name]).sum() == 0
    else:
        assert sc.info["n_combos"] == 0  # no face of this scene over-reaches (module docstring)
        for rs in BOUNDS:
            assert S.early_stop_drops(sc, bound=rs).sum() == 0
    big = float(np.abs(sc.centre).max()) >= 3e4 or name.startswith("extent")
    dyadic = sc.cell == 1.0
    assert not (name in S.TRAPPED and (dyadic or not big))


def test_every_far_scene_is_judged():
    far = [k for k in S.SCENES if k.startswith("far")]
    assert len(far) == len(S.CELLS) * len(S.OFFSETS) and set(S.TRAPPED) <= set(S.SCENES)


@pytest.mark.parametrize("cell", S.CELLS)
def test_teeth_cell_populations(cell):
    sc = S.populations(cell)
    own = sc.info["own_pop"]
    x0, ry, rz = sc.info["row"]
    cp = cell_of(sc.pts, sc.origin, sc.cell_eff)
    for j in range(S.NPOP):  # cell j of the row holds exactly j points
        assert ((cp == [x0 + j, ry, rz]).all(axis=1)).sum() == j
    cq = cell_of(sc.queries, sc.origin, sc.cell_eff)
    row_q = (cq[:, 1] == ry) & (cq[:, 2] == rz)
    assert set(own[row_q]) == set(range(S.NPOP)) and (own[row_q] == cq[row_q, 0] - x0).all()
    assert set(S.table_sizes(sc).tolist()) >= set(range(1, 71))
    out = own < 0  # the same row from just outside the grid on the +y side
    assert out.sum() == 3 * S.NPOP and (cq[out, 1] == sc.dims[1]).all()
    ids, _ = S.scene_knn(sc, 5, S.RANGE_SQ)
    if cell < 2.0:  # within the range of the row: the far pass has points to find
        assert (ids[out, 0] >= 0).all()


@pytest.mark.parametrize("cell", S.CELLS)
def test_teeth_thin_grids(cell):
    plane, line = S.thin(cell, "plane"), S.thin(cell, "line")
    assert plane.dims[2] == 3 and min(plane.dims[:2]) > 3
    assert line.dims[1] == 3 and line.dims[2] == 3 and line.dims[0] > 3
    assert len(S.thin(cell, "one").pts) == 1 and len(S.thin(cell, "five").pts) == 5
    for kind in ("plane", "line", "one", "five"):
        sc = S.thin(cell, kind)
        cq = cell_of(sc.queries, sc.origin, sc.cell_eff)
        inside = ((cq >= 0) & (cq < sc.dims)).all(axis=1)
        away = np.abs(cq - np.clip(cq, 0, sc.dims - 1)).max(axis=1)
        assert inside.sum() >= 50 and (~inside).sum() >= 100 and 40 <= away.max() <= 60
        ids, _ = S.scene_knn(sc, 5, S.RANGE_SQ)
        assert (ids[:, 0] >= 0).any() and (ids[:, 0] < 0).any()


def test_teeth_grown_cell():
    sc = S.grown()
    o1 = np.floor(sc.pts.min(0).astype(np.float64)) - 1.0
    n1 = np.floor(sc.pts.max(0).astype(np.float64) - o1) + 2
    assert n1.prod() > 2 ** 29 and sc.cell_eff == 2.0
    assert np.array_equal(sc.dims, np.floor((sc.pts.max(0).astype(np.float64) - sc.origin) / 2.0) + 2)
    assert sc.dims.prod() < 2 ** 29 and (np.abs(sc.dims - n1 / 2) <= 1).all()


@pytest.mark.parametrize("where", ["scan", "map"])
def test_teeth_nonfinite_rows(where):
    sc = S.nonfinite(0.6, where)
    arr = sc.queries if where == "scan" else sc.pts
    bad = np.nonzero(~np.isfinite(arr).all(axis=1))[0]
    assert np.array_equal(bad, sc.info["bad"])
    assert {0, 7, 8, 63, 64, len(arr) - 1} <= set(bad) and len(bad) >= len(arr) // 97
    vals = arr[bad]
    assert np.isnan(vals).any() and (vals == np.inf).any() and (vals == -np.inf).any()
    assert np.array_equal(grid_geom(sc.pts, 0.6)[0], S.faces(0.6).origin)
