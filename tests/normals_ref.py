"""The contract of lio_estimate_normals (include/lio_gpu.h) restated in vectorised numpy: the test oracle of the
normal estimation.  Candidates come from a cKDTree with slack; distances and ties are decided again in float32
by the written rule ((dx*dx + dy*dy) + dz*dz, then the index), and the slack is widened while its last distance
does not exceed the k-th strictly.  Everything behind the search is integer or IEEE double arithmetic in the
written order, so a conforming implementation matches bit for bit."""
import numpy as np
from scipy.spatial import cKDTree

NAN32 = np.float32(np.nan)


def sqdist3(a, b):
    """float32 ((dx*dx + dy*dy) + dz*dz) of rows a - b"""
    d = a.astype(np.float32) - b.astype(np.float32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def radius_sq(radius):
    return np.float32(np.float64(np.float32(radius)) * np.float64(np.float32(radius)))


def _candidates(xyz, fin, radius, k):
    """(row, col) pairs of input indices: for every finite point a superset of its neighbourhood N_i"""
    idx = np.flatnonzero(fin)
    nf = len(idx)
    P = xyz[idx].astype(np.float64)
    tree = cKDTree(P)
    if radius > 0:  # float32 d2 < r2 implies a double distance below radius (1 + 1e-6)
        lists = tree.query_ball_point(P, float(np.float32(radius)) * (1.0 + 1e-5) + 1e-300)
        rows = np.repeat(np.arange(nf), [len(l) for l in lists])
        cols = np.concatenate([np.asarray(l, np.int64) for l in lists]) if nf else np.zeros(0, np.int64)
        return idx[rows], idx[cols]
    kq = min(nf, k + 16)
    while True:
        _, nb = tree.query(P, kq)
        nb = nb.reshape(nf, kq)
        if kq == nf:
            break
        d2 = sqdist3(xyz[idx][:, None, :], xyz[idx[nb]])
        srt = np.sort(d2, axis=1)
        # the candidates hold every point up to their largest double distance; a point outside has a float32 d2
        # within 1e-6 (relative) of at least that
        if np.all(srt[:, -1].astype(np.float64) * (1.0 - 1e-6) > srt[:, k - 1]):
            break
        kq = min(nf, 2 * kq)
    return np.repeat(idx, kq), idx[nb.reshape(-1)]


def neighbours(pts, radius=0.0, k=0):
    """N_i as CSR over the input points: (start (n + 1), cols, d2 per entry), each row in (d2, index) order"""
    xyz = np.ascontiguousarray(np.asarray(pts, np.float32)[:, :3])
    n = len(xyz)
    fin = np.isfinite(xyz).all(axis=1)
    if not fin.any():
        return np.zeros(n + 1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    rows, cols = _candidates(xyz, fin, radius, k)
    d2 = sqdist3(xyz[rows], xyz[cols])
    if radius > 0:
        keep = d2 < radius_sq(radius)  # strict
        rows, cols, d2 = rows[keep], cols[keep], d2[keep]
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | cols.astype(np.uint64)
    order = np.lexsort((key, rows))
    rows, cols, d2 = rows[order], cols[order], d2[order]
    first = np.searchsorted(rows, np.arange(n + 1))
    if k > 0:
        keep = np.arange(len(rows)) - first[rows] < k
        rows, cols, d2 = rows[keep], cols[keep], d2[keep]
        first = np.searchsorted(rows, np.arange(n + 1))
    return first.astype(np.int64), cols, d2


def scale_of(B):
    """s = 2^(15 - h), h = ceil(e / 2), (mant, e) = frexp((double)B)"""
    _, e = np.frexp(np.asarray(B, np.float32).astype(np.float64))
    h = (e.astype(np.int64) + 1) >> 1
    return np.ldexp(1.0, (15 - h).astype(np.int32))


def covariance(S, SS, m):
    """M (n, 3, 3) float64 and T from the integer sums S (n, 3), SS (n, 6: xx xy xz yy yz zz), m (n)"""
    S, SS = np.asarray(S, np.int64), np.asarray(SS, np.int64)
    s = S.astype(np.float64)
    dm = np.asarray(m, np.int64).astype(np.float64)
    M = np.zeros((len(S), 3, 3))
    with np.errstate(all="ignore"):
        for t, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            M[:, a, b] = M[:, b, a] = SS[:, t].astype(np.float64) - (s[:, a] * s[:, b]) / dm
    T = (M[:, 0, 0] + M[:, 1, 1]) + M[:, 2, 2]
    return M, T


def jacobi(M):
    """cyclic Jacobi, at most 10 sweeps -> (lambda (n, 3), V (n, 3, 3)); a pair with A_pq = 0 is skipped, so a
    matrix whose off-diagonal is exactly zero stays as it is (the written stop)"""
    A = np.array(M, np.float64)
    V = np.broadcast_to(np.eye(3), A.shape).copy()
    with np.errstate(all="ignore"):
        for _ in range(10):
            if not ((A[:, 0, 1] != 0) | (A[:, 0, 2] != 0) | (A[:, 1, 2] != 0)).any():
                break
            for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
                apq = A[:, p, q].copy()
                do = apq != 0
                theta = (A[:, q, q] - A[:, p, p]) / (2.0 * apq)
                t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(theta < 0, -t, t)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                app, aqq = A[:, p, p] - t * apq, A[:, q, q] + t * apq
                arp, arq = A[:, r, p].copy(), A[:, r, q].copy()
                nrp, nrq = c * arp - s * arq, s * arp + c * arq
                A[:, p, p] = np.where(do, app, A[:, p, p])
                A[:, q, q] = np.where(do, aqq, A[:, q, q])
                A[:, p, q] = A[:, q, p] = np.where(do, 0.0, apq)
                A[:, r, p] = A[:, p, r] = np.where(do, nrp, arp)
                A[:, r, q] = A[:, q, r] = np.where(do, nrq, arq)
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p] = np.where(do[:, None], c[:, None] * vp - s[:, None] * vq, vp)
                V[:, :, q] = np.where(do[:, None], s[:, None] * vp + c[:, None] * vq, vq)
    return np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], axis=1), V


def solve(S, SS, m, B, xyz, viewpoints=None):
    """normals (n, 3) float32, curvature (n) float32, ok (n) from the moments of neighbourhoods with m >= 3;
    viewpoints: None or (n, 3) float32 rows"""
    m = np.asarray(m, np.int64)
    B = np.asarray(B, np.float32)
    xyz = np.asarray(xyz, np.float32).astype(np.float64)
    M, T = covariance(S, SS, m)
    with np.errstate(all="ignore"):
        ok = (B != 0) & (T > 0)
    lam, V = jacobi(np.where(ok[:, None, None], M, 0.0))
    pick = np.zeros(len(m), np.int64)
    pick = np.where(lam[:, 1] < lam[:, 0], 1, pick)
    pick = np.where(lam[:, 2] < lam[np.arange(len(m)), pick], 2, pick)
    nrm = V[np.arange(len(m)), :, pick]
    l0 = lam[np.arange(len(m)), pick]
    if viewpoints is not None:
        v = np.asarray(viewpoints, np.float32).astype(np.float64)
        with np.errstate(all="ignore"):
            s = ((v[:, 0] - xyz[:, 0]) * nrm[:, 0] + (v[:, 1] - xyz[:, 1]) * nrm[:, 1]) + (v[:, 2] - xyz[:, 2]) * nrm[:, 2]
            flip = s < 0
    else:
        flip = (nrm[:, 2] < 0) | ((nrm[:, 2] == 0) & ((nrm[:, 1] < 0) | ((nrm[:, 1] == 0) & (nrm[:, 0] < 0))))
    nrm = np.where(flip[:, None], -nrm, nrm)
    with np.errstate(all="ignore"):
        curv = np.abs(l0) / T
    normals = np.where(ok[:, None], nrm, np.nan).astype(np.float32)
    curvature = np.where(ok, curv, np.nan).astype(np.float32)
    return normals, curvature, ok


def moments(xyz, first, cols, d2, radius):
    """S (n, 3), SS (n, 6), m (n), B (n) of the CSR neighbourhoods"""
    n = len(xyz)
    m = np.diff(first)
    rows = np.repeat(np.arange(n), m)
    if radius > 0:
        B = np.full(n, radius_sq(radius), np.float32)
    else:
        B = np.zeros(n, np.float32)
        B[m > 0] = d2[first[1:][m > 0] - 1]  # rows are in ascending d2
    s = scale_of(B)
    o = xyz[cols] - xyz[rows]  # float32
    q = np.rint(o.astype(np.float64) * s[rows][:, None]).astype(np.int64)

    def rowsum(v):
        cs = np.concatenate([np.zeros(1, np.int64), np.cumsum(v, dtype=np.int64)])
        return cs[first[1:]] - cs[first[:-1]]

    S = np.stack([rowsum(q[:, a]) for a in range(3)], axis=1)
    SS = np.stack([rowsum(q[:, a] * q[:, b]) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], axis=1)
    return S, SS, m, B


def estimate_normals(pts, radius=0.0, k=0, viewpoint=None):
    """dict(normals (n, 3) float32, curvature (n) float32, counts (n) int32, stats (6) int64); viewpoint: None,
    (3,) or (n, 3)"""
    pts = np.asarray(pts, np.float32)
    pts = pts.reshape(len(pts), -1) if pts.size else pts.reshape(0, 3)
    xyz = np.ascontiguousarray(pts[:, :3])
    n = len(xyz)
    normals = np.full((n, 3), np.nan, np.float32)
    curvature = np.full(n, np.nan, np.float32)
    counts = np.zeros(n, np.int32)
    stats = np.zeros(6, np.int64)
    if n == 0:
        return dict(normals=normals, curvature=curvature, counts=counts, stats=stats)
    fin = np.isfinite(xyz).all(axis=1)
    first, cols, d2 = neighbours(xyz, radius, k)
    S, SS, m, B = moments(xyz, first, cols, d2, radius)
    counts[:] = m
    sel = np.flatnonzero(m >= 3)
    vp = None
    if viewpoint is not None:
        vp = np.asarray(viewpoint, np.float32)
        vp = np.broadcast_to(vp[:3], (n, 3)) if vp.ndim == 1 else vp[:, :3]
        vp = vp[sel]
    if len(sel):
        nr, cu, ok = solve(S[sel], SS[sel], m[sel], B[sel], xyz[sel], vp)
        normals[sel], curvature[sel] = nr, cu
    else:
        ok = np.zeros(0, bool)
    stats[:] = (fin.sum(), ok.sum(), (fin & (m < 3)).sum(), len(sel) - ok.sum(), m.max(), m.sum())
    return dict(normals=normals, curvature=curvature, counts=counts, stats=stats)
