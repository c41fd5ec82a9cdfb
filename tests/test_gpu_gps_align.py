"""GPU checks of the GPS alignment (lio_gpsalign.hip: lio_gps_align, lio_similarity2d_fit, lio_georeference_xy)
against the contract restated in numpy (tests/gps_align_ref.py; tests/test_gps_align_ref.py holds that
restatement against recorded runs of the reference).  Every output is compared bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import gps_align_ref as GR
from lio_gpu import _capi
from lio_gpu import formats
from lio_gpu import georef as G

pytestmark = pytest.mark.gpu
f64 = np.float64
dp = C.POINTER(C.c_double)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (n, m): below, at and above one TREE block; more targets than one LDS tile; the recorded 50-iteration shape;
# and one with three target chunks (2048, 2048, 3) whose last tile is ragged, run for 3 iterations
SHAPES = [(3, 2), (255, 257), (256, 256), (257, 1025), (700, 500), (5000, 4099)]
BIG = (5000, 4099)


@pytest.fixture(scope="module")
def al():
    return G.GpsAligner()


_cache = {}


def reference(key, gps, slam, iters, tol=1e-4):
    """the restatement's result, computed once per scene"""
    if key not in _cache:
        _cache[key] = GR.gps_align(gps, slam, iters, tol)
    return _cache[key]


def bits(a):
    return np.ascontiguousarray(a, f64).view(np.uint64)


def check(al, gps, slam, exp, iters, tol=1e-4):
    al.max_iterations, al.tolerance = iters, tol
    r = al.align(gps, slam)
    msg = f"n={len(slam)} m={len(gps)} iters={iters}"
    assert r.iterations == exp.iterations and int(r.converged) == exp.converged, msg
    np.testing.assert_array_equal(r.nn, exp.nn, err_msg=msg)
    np.testing.assert_array_equal(bits(r.out), bits(exp.out), err_msg=msg)
    np.testing.assert_array_equal(bits(r.aligned), bits(exp.aligned + exp.cB), err_msg=msg)
    assert r.mean_error == exp.mean_error and r.total.scale == exp.out[20] and r.reference_return.scale == exp.out[15]
    np.testing.assert_array_equal(r.total.R, [[exp.out[21], -exp.out[22]], [exp.out[22], exp.out[21]]])
    np.testing.assert_array_equal(r.reference_return.t, exp.out[18:20])
    return r


def golden(name):
    return (np.load(os.path.join(GOLD, f"gps_align_{name}_gps.npy")), np.load(os.path.join(GOLD, f"gps_align_{name}_slam.npy")))


# ----------------------------------------------------------------------- lio_gps_align
@pytest.mark.parametrize("n,m", SHAPES)
def test_shapes_at_national_grid_offsets(al, n, m):
    """scenes at HK1980 offsets (+836 000, +818 000) with 0.4 m of noise"""
    gps, slam = GR.scene(n, m, seed=n + m)
    assert gps[:, 0].min() > 8.3e5 and gps[:, 1].min() > 8.1e5
    iters = 3 if (n, m) == BIG else 50
    check(al, gps, slam, reference(("scene", n, m, iters), gps, slam, iters), iters)


@pytest.mark.parametrize("n,m", [(255, 257), (700, 500)])
def test_one_iteration(al, n, m):
    gps, slam = GR.scene(n, m, seed=n + m)
    r = check(al, gps, slam, reference(("scene", n, m, 1), gps, slam, 1), 1)
    assert r.iterations == 1 and not r.converged  # prev starts at +inf
    # with one iteration the reference's return triple has the total's scale and rotation (s0 sc, R) to the bit;
    # its translation follows the script's own closing formula and is not the total's even then
    assert r.total.scale == r.reference_return.scale and np.array_equal(r.total.R, r.reference_return.R)


def test_recorded_scenes_stop_where_the_reference_stopped(al):
    """the early-converging scene and the one that runs all 50 iterations (tests/golden)"""
    import json
    runs = json.load(open(os.path.join(GOLD, "gps_align_reference_runs.json")))
    for name in ("early", "full", "tiny"):
        gps, slam = golden(name)
        r = check(al, gps, slam, reference(("golden", name), gps, slam, 50), 50)
        assert r.iterations == runs[name]["iterations"] and r.converged == runs[name]["converged"]
    assert runs["early"]["iterations"] < 50 and runs["full"]["iterations"] == 50


def test_duplicate_targets_across_tile_and_chunk_boundaries(al):
    """Exact duplicates of a target on both sides of an LDS tile boundary inside a chunk (1023 | 1024), of a chunk
    boundary (2047 | 2048), two chunks apart (10 | 4097, the last in the ragged tile) and inside one tile
    (500 | 501): the lowest index wins every time."""
    n, m = BIG
    assert GR.TILE == 1024 and GR.CHUNK_MIN == 2048
    gps, slam = GR.scene(n, m, seed=n + m)
    pairs = [(1023, 1024), (2047, 2048), (10, 4097), (500, 501)]
    # each pair goes where a much-matched target of the plain scene stands (that target moves to the pair's old
    # place), so that the tie is somebody's nearest neighbour
    cnt = np.bincount(reference(("scene", n, m, 3), gps, slam, 3).nn, minlength=m)
    popular = [int(p) for p in np.argsort(-cnt, kind="stable") if all(abs(p - x) > 5 for pr in pairs for x in pr)][:4]
    gps = gps.copy()
    for (lo, hi), p in zip(pairs, popular):
        spot = gps[p].copy()
        gps[p] = gps[lo]
        gps[lo] = gps[hi] = spot
    exp = reference(("dup", n, m), gps, slam, 3)
    for lo, hi in pairs:  # of the inputs: the duplicated target is somebody's nearest
        assert (exp.nn == lo).any() and not (exp.nn == hi).any(), (lo, hi)
    r = check(al, gps, slam, exp, 3)
    for lo, hi in pairs:
        assert (r.nn == lo).any() and not (r.nn == hi).any()
    # the same, first iteration only: all equal targets, every source takes index 0
    gps1 = np.repeat(gps[:1], m, axis=0)
    gps1[-1] += 1.0  # one other point, or the set has zero variance
    exp1 = reference(("dup1", n, m), gps1, slam[:300], 1)
    r1 = check(al, gps1, slam[:300], exp1, 1)
    assert set(np.unique(r1.nn)) <= {0, m - 1} and (r1.nn == 0).any()


def test_degenerate_inputs_are_errors(al):
    L = _capi.lib()
    gps, slam = GR.scene(40, 30, seed=1)
    al.max_iterations, al.tolerance = 50, 1e-4

    def code(g, s, iters=50):
        al.max_iterations = iters
        with pytest.raises(_capi.LioError) as e:
            al.align(g, s)
        al.max_iterations = 50
        return e.value.code

    # zero variance, as the reference raises (counts and values whose TREE mean is exact: the centred set is 0)
    assert code(gps, np.tile([3.0, -5.0], (64, 1))) == _capi.LIO_ERR_ARG
    assert code(np.tile([836000.0, 818000.0], (32, 1)), slam) == _capi.LIO_ERR_ARG
    assert code(gps, slam[:1]) == _capi.LIO_ERR_ARG  # one source point has zero variance too
    assert GR.gps_align(gps, slam[:1]) is None
    assert code(gps, slam, iters=0) == _capi.LIO_ERR_ARG
    assert code(gps, np.zeros((0, 2))) == _capi.LIO_ERR_ARG and code(np.zeros((0, 2)), slam) == _capi.LIO_ERR_ARG
    for bad in (np.nan, np.inf, -np.inf):
        g2, s2 = gps.copy(), slam.copy()
        g2[29, 1] = bad
        s2[0, 0] = bad
        assert code(g2, slam) == _capi.LIO_ERR_ARG and code(gps, s2) == _capi.LIO_ERR_ARG
    out = np.zeros(_capi.LIO_GPSALIGN_LEN)
    a = np.zeros((40, 2))
    args = (gps.ctypes.data_as(dp), 30, slam.ctypes.data_as(dp), 40, 50, 1e-4)
    assert L.lio_gps_align(al._h, *args, None, None, out.ctypes.data_as(dp)) == _capi.LIO_ERR_ARG
    assert L.lio_gps_align(al._h, *args, a.ctypes.data_as(dp), None, None) == _capi.LIO_ERR_ARG
    assert L.lio_gps_align(al._h, None, 30, slam.ctypes.data_as(dp), 40, 50, 1e-4, a.ctypes.data_as(dp), None,
                           out.ctypes.data_as(dp)) == _capi.LIO_ERR_ARG
    assert L.lio_gps_align(al._h, *args, a.ctypes.data_as(dp), None, out.ctypes.data_as(dp)) == 0  # nn is optional
    # every source equally near both targets: all take index 0, the matched set has no extent, the scale is 0,
    # the sources collapse, and the second iteration has saa == 0
    g3, s3 = np.array([[-1.0, 0.0], [1.0, 0.0]]), np.array([[0.0, 1.0], [0.0, -1.0], [0.0, 3.0]])
    assert GR.gps_align(g3, s3) == "state"
    assert code(g3, s3) == _capi.LIO_ERR_STATE
    # the handle still works
    check(al, gps, slam, reference(("scene", 40, 30, 50), gps, slam, 50), 50)


def test_sizes_change_on_one_handle(al):
    a = GR.scene(255, 257, seed=255 + 257)
    b = GR.scene(700, 500, seed=700 + 500)
    first = check(al, *a, reference(("scene", 255, 257, 50), *a, 50), 50)
    check(al, *b, reference(("scene", 700, 500, 50), *b, 50), 50)
    again = check(al, *a, reference(("scene", 255, 257, 50), *a, 50), 50)
    np.testing.assert_array_equal(bits(first.out), bits(again.out))
    np.testing.assert_array_equal(bits(first.aligned), bits(again.aligned))
    np.testing.assert_array_equal(first.nn, again.nn)
    before = _capi.lib().lio_alloc_count()
    check(al, *b, reference(("scene", 700, 500, 50), *b, 50), 50)
    assert _capi.lib().lio_alloc_count() == before  # no allocation at a size seen before


def test_total_similarity_reproduces_the_aligned_points(al):
    """`total` applied to slam_xy against `aligned`.  Measured with the restatement on the CPU, as
    total.scale * (slam @ total.R.T) + total.t against aligned + cB: 1.17e-10 m on each of the three scenes below
    (3 x 2 after 3 iterations, 255 x 257 and 700 x 500 after 50), which is one spacing of doubles at the
    coordinates' 8.4e5 m.  The bound is 8 times that."""
    bound = 8 * 1.17e-10
    for n, m in [(3, 2), (255, 257), (700, 500)]:
        gps, slam = GR.scene(n, m, seed=n + m)
        exp = reference(("scene", n, m, 50), gps, slam, 50)
        r = check(al, gps, slam, exp, 50)
        err = np.abs(r.total.apply(slam) - r.aligned).max()
        print(f"total vs aligned, n={n} m={m}: {err:.3g} m")
        assert err <= bound


# ----------------------------------------------------------------------- lio_similarity2d_fit
@pytest.mark.parametrize("n", [2, 256, 257])
def test_fit_pairs(al, n):
    rng = np.random.default_rng(n)
    src = GR.trajectory(n, n)
    c, s = np.cos(-0.9), np.sin(-0.9)
    dst = 0.97 * (src @ np.array([[c, -s], [s, c]]).T) + [836000.0, 818000.0] + rng.normal(0, 0.4, (n, 2))
    exp = GR.fit_pairs(src, dst)
    got = G.fit_pairs(src, dst, handle=al)
    np.testing.assert_array_equal(bits([got.scale, got.R[0, 0], got.R[1, 0], got.t[0], got.t[1]]), bits(exp))
    assert got.R[0, 1] == -got.R[1, 0] and got.R[1, 1] == got.R[0, 0]
    assert abs(got.scale - 0.97) < 0.05 and abs(got.R[1, 0] - s) < 0.05


def test_fit_pairs_errors(al):
    one = np.array([[1.0, 2.0]])
    assert GR.fit_pairs(one, one) is None
    with pytest.raises(_capi.LioError) as e:
        G.fit_pairs(one, one, handle=al)  # one pair fixes no similarity: saa == 0
    assert e.value.code == _capi.LIO_ERR_STATE
    with pytest.raises(_capi.LioError) as e:
        G.fit_pairs(np.zeros((0, 2)), np.zeros((0, 2)), handle=al)
    assert e.value.code == _capi.LIO_ERR_ARG
    with pytest.raises(_capi.LioError) as e:
        G.fit_pairs(np.array([[0.0, np.nan], [1.0, 1.0]]), np.zeros((2, 2)), handle=al)
    assert e.value.code == _capi.LIO_ERR_ARG


# ----------------------------------------------------------------------- lio_georeference_xy
SIM = (1.0200000000000002, np.array([[np.cos(0.6), -np.sin(0.6)], [np.sin(0.6), np.cos(0.6)]]), np.array([836012.25, 818007.5]))


def records(n, stride, seed):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 2**32, (n, stride), dtype=np.uint64).astype(np.uint32)  # any bit pattern, NaNs among them
    pts = raw.view(np.float32).copy()
    pts[:, 0] = rng.uniform(-500, 500, n).astype(np.float32)
    pts[:, 1] = rng.uniform(-500, 500, n).astype(np.float32)
    return pts


@pytest.mark.parametrize("stride", [3, 4, 8])
@pytest.mark.parametrize("n", [0, 1, 255, 257])
def test_georeference(al, n, stride):
    pts = records(n, stride, 10 * n + stride)
    for origin in ((0.0, 0.0), (836000.0, 818000.0)):
        exp, exp_xy = GR.georeference(pts, *SIM, origin=origin)
        out, xy = G.georeference(pts, *SIM, origin=origin, return_f64=True, handle=al)
        assert out.shape == (n, stride) and xy.shape == (n, 2)
        np.testing.assert_array_equal(out.view(np.uint32), exp.view(np.uint32))  # the other fields bit for bit
        np.testing.assert_array_equal(bits(xy), bits(exp_xy))
        only = G.georeference(pts, *SIM, origin=origin, handle=al)
        np.testing.assert_array_equal(only.view(np.uint32), exp.view(np.uint32))
    if n:
        far, _ = GR.georeference(pts, *SIM)
        near, near_xy = GR.georeference(pts, *SIM, origin=(836000.0, 818000.0))
        _, far_xy = GR.georeference(pts, *SIM)
        # at 8e5 m a float32 step is 6.25 cm; with the origin the records keep the doubles to well under a millimetre
        assert np.abs(far[:, :2] - far_xy).max() <= 0.0625 / 2
        assert np.abs(near[:, :2] - near_xy).max() <= 2.0 ** -14


def test_georeference_argument_errors(al):
    L = _capi.lib()
    pts = records(4, 4, 0)
    R, t = SIM[1].ravel().copy(), SIM[2].copy()
    out = np.zeros_like(pts)
    fp = _capi.fp
    call = lambda p, n, stride, Rp, tp, o: L.lio_georeference_xy(al._h, p, n, stride, 1.0, Rp, tp, None, o, None)  # noqa: E731
    ok = (pts.ctypes.data_as(fp), 4, 4, R.ctypes.data_as(dp), t.ctypes.data_as(dp), out.ctypes.data_as(fp))
    assert call(*ok) == 0
    assert call(ok[0], 4, 2, *ok[3:]) == _capi.LIO_ERR_ARG and call(ok[0], 4, 9, *ok[3:]) == _capi.LIO_ERR_ARG
    assert call(ok[0], -1, 4, *ok[3:]) == _capi.LIO_ERR_ARG
    assert call(None, 4, 4, *ok[3:]) == _capi.LIO_ERR_ARG and call(*ok[:5], None) == _capi.LIO_ERR_ARG
    assert call(*ok[:3], None, ok[4], ok[5]) == _capi.LIO_ERR_ARG and call(*ok[:4], None, ok[5]) == _capi.LIO_ERR_ARG


def test_pcd_round_trip(al, tmp_path):
    pts = records(257, 4, 77)
    pts[:, 2:] = np.random.default_rng(1).uniform(-50, 50, (257, 2)).astype(np.float32)
    src, par, dst = (str(tmp_path / k) for k in ("map.pcd", "georef_params.txt", "map_geo.pcd"))
    formats.write_pcd_binary(src, pts)
    G.write_georef_params(par, *SIM)
    assert G.georeference_pcd(src, par, dst) == 257
    got = formats.CloudCodec().read_pcd(dst)
    exp, _ = GR.georeference(pts, *G.read_georef_params(par))
    np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32))
    exp0, _ = GR.georeference(pts, *SIM)
    np.testing.assert_array_equal(exp.view(np.uint32), exp0.view(np.uint32))  # the file keeps every bit of the doubles
    assert G.georeference_pcd(src, par, dst, origin=(836000.0, 818000.0)) == 257
    near, _ = GR.georeference(pts, *SIM, origin=(836000.0, 818000.0))
    np.testing.assert_array_equal(formats.CloudCodec().read_pcd(dst).view(np.uint32), near.view(np.uint32))
