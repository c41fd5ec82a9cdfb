"""Plain numpy reference of the grid searches: a brute-force kNN and the float32 cell arithmetic.

Test infrastructure only.  brute_knn uses no grid and no tree, so the HIP searches (csrc/lio_dev.hpp) and the
oracle's kd-tree can both be held against it: float32 d2 = (dx*dx + dy*dy) + dz*dz as sqdist3 computes it (one
rounding per operation, no FMA), the k smallest under the total order (d2, id), restricted to d2 <= range_sq.
cell_of / face / base_margin / grid_geom restate the grid's own float arithmetic (cell_coord, the face formula
o + k * cell, grid_view's slack, grid_rebuild's geometry) so a scene can place points by it.
"""
import numpy as np

F32 = np.float32


def brute_knn(q, pts, k=5, range_sq=np.inf, chunk=256):
    """(ids[n, k] int32, d2[n, k] float32): missing slots id -1 / d2 inf.  Rows of pts that are not finite are
    never candidates; rows of q that are not finite return all -1."""
    q = np.asarray(q, np.float32).reshape(-1, 3)
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    rs = F32(range_sq)
    ids = np.full((len(q), k), -1, np.int32)
    d2 = np.full((len(q), k), np.inf, np.float32)
    pok = np.isfinite(pts).all(axis=1)
    qok = np.isfinite(q).all(axis=1)
    if not len(pts):
        return ids, d2
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, len(q), chunk):
            qq = q[s:s + chunk]
            dx = qq[:, None, 0] - pts[None, :, 0]
            dy = qq[:, None, 1] - pts[None, :, 1]
            dz = qq[:, None, 2] - pts[None, :, 2]
            d = (dx * dx + dy * dy) + dz * dz  # float32 throughout, no FMA
            avail = pok[None, :] & qok[s:s + chunk, None] & (d <= rs)
            rows = np.arange(len(qq))
            for j in range(k):
                dm = np.where(avail, d, F32(np.inf))
                a = np.argmin(dm, axis=1)  # first index of the minimum = lowest id among ties
                got = avail[rows, a]
                ids[s:s + chunk, j] = np.where(got, a, -1)
                d2[s:s + chunk, j] = np.where(got, d[rows, a], F32(np.inf))
                avail[rows, a] = False
    return ids, d2


def cell_of(v, origin, cell):
    """cell_coord / cell_key_of (unclamped to the grid): floor((v - o) * (1 / cell)) in float32"""
    v = np.asarray(v, np.float32)
    o = np.asarray(origin, np.float32)
    inv = F32(1.0) / F32(cell)
    with np.errstate(invalid="ignore"):
        f = np.floor((v - o) * inv)
        f = np.fmin(np.fmax(f, F32(-1.0e9)), F32(1.0e9))  # fmaxf / fminf: NaN -> -1e9
    return f.astype(np.int64)


def face(origin, k, cell):
    """lower face k of an axis as the searches compute it: o + float32(k) * cell in float32"""
    return np.asarray(origin, np.float32) + np.asarray(k).astype(np.float32) * F32(cell)


def base_margin(cell):
    """the fixed slack of the cell faces: 1e-3f + 1e-4f * cell"""
    return F32(1e-3) + F32(1e-4) * F32(cell)


def grid_margin(origin, cell, dims):
    """csrc/lio_grid_margin.hpp: the fixed slack up to a few km, then 3 * 2^-23 * max|coordinate| + 3e-7 * extent"""
    o = np.asarray(origin, np.float32).astype(np.float64)
    e = np.asarray(dims, np.float64) * float(F32(cell))
    amax = max(np.abs(o).max(), np.abs(o + e).max())
    return max(base_margin(cell), F32(3.0 * np.ldexp(amax, -23) + 3e-7 * e.max()))


def grid_geom(pts, cell):
    """grid_rebuild's geometry for a Build of pts (no slack): (origin float32[3], cell float32, dims int[3]);
    the cell doubles while the table would exceed 2^29 cells.  Rows that are not finite are no part of the
    map (Build stores them as deleted ids)."""
    p = np.asarray(pts, np.float32).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)]
    lo = p.min(axis=0).astype(np.float64)
    hi = p.max(axis=0).astype(np.float64)
    c = F32(cell)
    while True:
        cd = float(c)
        o = np.floor(lo / cd) * cd - cd
        n = np.floor((hi - o) / cd) + 2
        if n[0] * n[1] * n[2] <= float(1 << 29):
            return o.astype(np.float32), c, n.astype(np.int64)
        c = F32(c * F32(2))


def first_float_of_cell(origin1, k, cell):
    """the smallest float32 v with cell_of(v) == k on one axis (origin1: that axis' origin)"""
    o = F32(origin1)
    v = F32(face(o, k, cell))
    while cell_of(v, o, cell) >= k:
        v = np.nextafter(v, F32(-np.inf))
    while cell_of(v, o, cell) < k:
        v = np.nextafter(v, F32(np.inf))
    return F32(v)
