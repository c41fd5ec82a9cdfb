"""CPU checks of tests/normals_ref.py, the numpy restatement of lio_estimate_normals' contract that the GPU tests
compare against bit for bit: its eigenvector against numpy.linalg.eigh, its normals on a noisy plane, the index
rule at tied distances, the strict radius test and the degenerate neighbourhoods."""
import numpy as np
import pytest

import normals_ref as NR


def plane_cloud():
    """the noisy plane of the normal tests: default_rng(1), n = 600, xy uniform in +-2, z ~ N(0, 0.01), offset
    (100, -50, 3)"""
    rng = np.random.default_rng(1)
    p = np.stack([rng.uniform(-2, 2, 600), rng.uniform(-2, 2, 600), rng.normal(0, 0.01, 600)], axis=1)
    return (p + np.array([100.0, -50.0, 3.0])).astype(np.float32)


def lattice_cloud():
    """8 x 8 x 3 lattice of spacing 0.25: every distance is tied many times over"""
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3)
    return (0.25 * g).astype(np.float32)


MODES = (dict(radius=0.5, k=0), dict(radius=0.0, k=16), dict(radius=0.3, k=16))


def _moment_matrices(pts, **mode):
    xyz = np.ascontiguousarray(pts[:, :3])
    first, cols, d2 = NR.neighbours(xyz, **mode)
    S, SS, m, B = NR.moments(xyz, first, cols, d2, mode["radius"])
    sel = m >= 3
    M, T = NR.covariance(S[sel], SS[sel], m[sel])
    return M, T, sel


def test_eigenvector_matches_eigh():
    """where lambda_1 - lambda_0 > 1e-3 T: 1 - |n . n_eigh| <= 1e-9 (the eigenvector's perturbation is about
    eps ||M|| / gap, 1e-13 here); the gap condition excludes no point of the noisy plane"""
    pts = plane_cloud()
    worst = 0.0
    for mode in MODES:
        M, T, sel = _moment_matrices(pts, **mode)
        lam, V = NR.jacobi(M)
        w, U = np.linalg.eigh(M)
        gap_ok = (w[:, 1] - w[:, 0]) > 1e-3 * T
        assert gap_ok.all(), (mode, (~gap_ok).sum())
        pick = np.argmin(lam, axis=1)
        n = V[np.arange(len(M)), :, pick]
        err = 1.0 - np.abs(np.einsum("ij,ij->i", n, U[:, :, 0]))
        worst = max(worst, float(err.max()))
        assert np.allclose(np.sort(lam, axis=1), w, rtol=0, atol=1e-9 * np.abs(w).max())
    print("worst 1 - |n . n_eigh| =", worst)
    assert worst <= 1e-9


@pytest.mark.parametrize("mode", MODES, ids=("radius", "knn", "hybrid"))
def test_noisy_plane_normals_point_up(mode):
    r = NR.estimate_normals(plane_cloud(), **mode)
    dense = r["counts"] >= 10
    assert dense.sum() > 300
    nz = np.abs(r["normals"][dense, 2])
    print(mode, "min |n_z| =", nz.min())
    assert (nz > 0.99).all()
    # no viewpoint: the sign rule makes n_z positive; a viewpoint below the plane turns every normal down
    assert (r["normals"][dense, 2] > 0).all()
    down = NR.estimate_normals(plane_cloud(), viewpoint=np.array([100, -50, -10], np.float32), **mode)
    assert np.array_equal(down["normals"][dense], -r["normals"][dense])
    assert np.array_equal(down["curvature"], r["curvature"], equal_nan=True)
    assert (r["curvature"][dense] >= 0).all() and (r["curvature"][dense] < 0.05).all()
    s = r["stats"]
    assert s[0] == 600 and s[1] + s[2] + s[3] == 600 and s[4] == r["counts"].max() and s[5] == r["counts"].sum()


def test_lattice_ties_exercise_the_index_rule():
    pts = lattice_cloud()
    k = 10
    d2 = NR.sqdist3(pts[:, None, :], pts[None, :, :])
    srt = np.sort(d2, axis=1)
    tied = srt[:, k - 1] == srt[:, k]  # the k-th and the (k + 1)-th candidate are equally far
    assert tied.sum() >= 96, tied.sum()
    first, cols, dd = NR.neighbours(pts, 0.0, k)
    assert (np.diff(first) == k).all()
    for i in np.flatnonzero(tied)[:40]:  # among the candidates at the k-th distance the lowest indices are taken
        mine = cols[first[i]:first[i + 1]]
        kth = srt[i, k - 1]
        at = np.flatnonzero(d2[i] == kth)
        taken = np.intersect1d(mine, at)
        assert np.array_equal(taken, at[:len(taken)])
        assert set(np.flatnonzero(d2[i] < kth)) <= set(mine)


def test_lattice_radius_is_strict():
    pts = lattice_cloud()
    r = NR.estimate_normals(pts, radius=0.25)
    assert (r["counts"] == 1).all() and np.isnan(r["normals"]).all() and np.isnan(r["curvature"]).all()
    assert list(r["stats"]) == [192, 0, 192, 0, 1, 192]
    r = NR.estimate_normals(pts, radius=0.5)
    assert r["counts"].min() == 8 and r["counts"].max() == 27


def test_coincident_points_are_degenerate():
    pts = np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (5, 1))
    for mode in (dict(k=5), dict(k=3), dict(radius=0.5), dict(radius=0.5, k=4)):
        r = NR.estimate_normals(pts, **mode)
        want = mode.get("k") or 5
        assert (r["counts"] == want).all() and np.isnan(r["normals"]).all(), mode
        assert list(r["stats"]) == [5, 0, 0, 5, want, 5 * want]


def test_collinear_points_give_a_normal_across_the_line():
    t = np.linspace(-1, 1, 21)
    line = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    pts = (t[:, None] * line[None, :] + np.array([3.0, 4.0, 5.0])).astype(np.float32)
    for mode in (dict(k=7), dict(radius=0.45)):
        r = NR.estimate_normals(pts, **mode)
        ok = r["counts"] >= 3
        n = r["normals"][ok].astype(np.float64)
        assert ok.sum() >= 19 and not np.isnan(n).any()
        assert np.all(np.abs(np.linalg.norm(n, axis=1) - 1.0) < 1e-6)
        assert np.all(np.abs(n @ line) < 1e-3)


def test_non_finite_points_are_nobodys_neighbour():
    pts = plane_cloud()[:64].copy()
    pts[0, 1] = np.nan
    pts[63, 2] = np.inf
    r = NR.estimate_normals(pts, k=200)  # k > n: every finite point
    assert r["counts"][0] == 0 and r["counts"][63] == 0 and (r["counts"][1:63] == 62).all()
    assert np.isnan(r["normals"][[0, 63]]).all() and not np.isnan(r["normals"][1:63]).any()
    assert list(r["stats"]) == [62, 62, 0, 0, 62, 62 * 62]
    e = NR.estimate_normals(np.zeros((0, 3), np.float32), k=5)
    assert e["normals"].shape == (0, 3) and list(e["stats"]) == [0] * 6
