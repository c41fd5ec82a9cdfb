"""The contract of lio_gps_align / lio_similarity2d_fit / lio_georeference_xy (include/lio_gpu.h) restated in
numpy, operation for operation: IEEE double + - x / sqrt in the written order (numpy evaluates every elementwise
operation on its own, so nothing is fused), every sum by TREE.  Written from the contract, not from the
reference's script; tests/test_gps_align_ref.py holds it against recorded runs of the reference's icp_alignment.
"""
from types import SimpleNamespace

import numpy as np

f64 = np.float64
TILE, CHUNK_MIN = 1024, 2048  # the library's LDS tile and smallest target chunk (lio_gpsalign.hpp): tests place
# duplicates on both sides of these boundaries; no result depends on them


def tree(v):
    """TREE(v): blocks of 256 (the last padded with +0.0), halving inside a block, block sums added in ascending
    order into a scalar that starts at 0.0."""
    v = np.asarray(v, f64)
    nb = (len(v) + 255) // 256
    a = np.zeros(nb * 256, f64)
    a[: len(v)] = v
    a = a.reshape(nb, 256)
    w = 128
    while w >= 1:
        a = a[:, :w] + a[:, w:2 * w]
        w //= 2
    t = f64(0.0)
    for b in a[:, 0]:
        t = t + b
    return t


def nearest(S, D, rows=256):
    """per source the target with the smallest d2 = (dx dx) + (dy dy), the lowest index on an equal d2; (k, d2)"""
    n = len(S)
    k = np.zeros(n, np.int64)
    d2 = np.zeros(n, f64)
    for a in range(0, n, rows):
        dx = S[a:a + rows, 0][:, None] - D[None, :, 0]
        dy = S[a:a + rows, 1][:, None] - D[None, :, 1]
        q = dx * dx + dy * dy
        kk = q.argmin(axis=1)  # the first of equal minima
        k[a:a + rows] = kk
        d2[a:a + rows] = q[np.arange(len(kk)), kk]
    return k, d2


def rotation(h00, h01, h10, h11):
    """step 4: the proper rotation (c, s) that maximises tr(R H)"""
    p = h00 + h11
    q = h01 - h10
    r = np.sqrt(p * p + q * q)
    if r == 0:
        return f64(1.0), f64(0.0)
    return p / r, q / r


def fit_step(S, M):
    """steps 2-5 on the pairs (S[j], M[j]); None when saa == 0 or the scale is not finite (LIO_ERR_STATE)"""
    n = f64(len(S))
    cs = np.array([tree(S[:, 0]) / n, tree(S[:, 1]) / n])
    cd = np.array([tree(M[:, 0]) / n, tree(M[:, 1]) / n])
    ax, ay = S[:, 0] - cs[0], S[:, 1] - cs[1]
    bx, by = M[:, 0] - cd[0], M[:, 1] - cd[1]
    h00, h01, h10, h11 = tree(ax * bx), tree(ax * by), tree(ay * bx), tree(ay * by)
    saa, sbb = tree(ax * ax + ay * ay), tree(bx * bx + by * by)
    c, s = rotation(h00, h01, h10, h11)
    with np.errstate(all="ignore"):
        sc = np.sqrt(sbb) / np.sqrt(saa)
    if saa == 0 or not np.isfinite(sc):
        return None
    t = np.array([cd[0] - sc * (c * cs[0] - s * cs[1]), cd[1] - sc * (s * cs[0] + c * cs[1])])
    return SimpleNamespace(cs=cs, cd=cd, sc=sc, c=c, s=s, t=t, H=np.array([[h00, h01], [h10, h11]]), saa=saa, sbb=sbb)


def gps_align(gps_xy, slam_xy, max_iterations=50, tolerance=1e-4, nearest_fn=nearest):
    """lio_gps_align.  Returns None for a zero-variance set (LIO_ERR_ARG), the string "state" for LIO_ERR_STATE,
    else every output plus, per iteration, mean_error, |prev - mean_error| - tolerance (`margins`) and the smallest
    gap between a source's best and second-best rooted distance (`gaps`; inf with one target)."""
    A = np.ascontiguousarray(slam_xy, f64).reshape(-1, 2)
    B = np.ascontiguousarray(gps_xy, f64).reshape(-1, 2)
    n, m = len(A), len(B)
    cA = np.array([tree(A[:, 0]) / f64(n), tree(A[:, 1]) / f64(n)])
    cB = np.array([tree(B[:, 0]) / f64(m), tree(B[:, 1]) / f64(m)])
    Ac, D = A - cA, B - cB
    sA = np.sqrt(tree(Ac[:, 0] * Ac[:, 0] + Ac[:, 1] * Ac[:, 1]))
    sB = np.sqrt(tree(D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]))
    if sA == 0 or sB == 0:
        return None
    s0 = sB / sA if sA > 1e-8 else f64(1.0)
    S = s0 * Ac
    tS, tC, tSn = s0, f64(1.0), f64(0.0)
    tT = np.array([-(s0 * cA[0]), -(s0 * cA[1])])
    prev = f64(np.inf)
    errors, margins, gaps = [], [], []
    converged = 0
    for i in range(max_iterations):
        k, d2 = nearest_fn(S, D)
        dist = np.sqrt(d2)
        st = fit_step(S, D[k])
        if st is None:
            return "state"
        S = np.stack([st.sc * (st.c * S[:, 0] - st.s * S[:, 1]) + st.t[0],
                      st.sc * (st.s * S[:, 0] + st.c * S[:, 1]) + st.t[1]], axis=1)
        tS = st.sc * tS
        tC, tSn = st.c * tC - st.s * tSn, st.s * tC + st.c * tSn
        tT = np.array([st.sc * (st.c * tT[0] - st.s * tT[1]) + st.t[0], st.sc * (st.s * tT[0] + st.c * tT[1]) + st.t[1]])
        mean_error = tree(dist) / f64(n)
        errors.append(float(mean_error))
        margins.append(float(abs(prev - mean_error) - tolerance))
        if abs(prev - mean_error) < tolerance:
            converged = 1
            break
        prev = mean_error
    u = cB - st.t
    r = np.array([st.c * u[0] + st.s * u[1], st.c * u[1] - st.s * u[0]])
    v = np.array([st.cd[0] - s0 * r[0], st.cd[1] - s0 * r[1]])
    ref_T = np.array([cB[0] + st.sc * (st.c * v[0] - st.s * v[1]), cB[1] + st.sc * (st.s * v[0] + st.c * v[1])])
    out = np.zeros(25, f64)
    out[0:4] = len(errors), converged, errors[-1], s0
    out[4:6], out[6:8] = cA, cB
    out[8:11] = st.sc, st.c, st.s
    out[11:13], out[13:15] = st.t, st.cd
    out[15:18] = s0 * st.sc, st.c, st.s
    out[18:20] = ref_T
    out[20:23] = tS, tC, tSn
    out[23:25] = tT + cB
    return SimpleNamespace(aligned=S, nn=k.astype(np.int32), out=out, iterations=len(errors), converged=converged,
                           mean_error=errors[-1], errors=errors, margins=margins, s0=s0, cA=cA, cB=cB, last=st)


def best_gaps(S, D):
    """per source the gap between the best and the second-best rooted distance"""
    out = np.full(len(S), np.inf)
    if len(D) < 2:
        return out
    for a in range(0, len(S), 256):
        d = np.sqrt((S[a:a + 256, 0][:, None] - D[None, :, 0]) ** 2 + (S[a:a + 256, 1][:, None] - D[None, :, 1]) ** 2)
        d.partition(1, axis=1)
        out[a:a + 256] = d[:, 1] - d[:, 0]
    return out


def fit_pairs(src, dst):
    """lio_similarity2d_fit: (scale, c, s, tx, ty), or None for LIO_ERR_STATE"""
    st = fit_step(np.ascontiguousarray(src, f64).reshape(-1, 2), np.ascontiguousarray(dst, f64).reshape(-1, 2))
    return None if st is None else np.array([st.sc, st.c, st.s, st.t[0], st.t[1]])


def georeference(pts, scale, R, t, origin=(0.0, 0.0)):
    """lio_georeference_xy: (records, n x 2 doubles)"""
    pts = np.ascontiguousarray(pts, np.float32)
    R = np.asarray(R, f64).reshape(2, 2)
    x, y = pts[:, 0].astype(f64), pts[:, 1].astype(f64)
    gx = ((x * R[0, 0] + y * R[0, 1]) * f64(scale) + f64(t[0])) - f64(origin[0])
    gy = ((x * R[1, 0] + y * R[1, 1]) * f64(scale) + f64(t[1])) - f64(origin[1])
    out = pts.copy()
    out[:, 0], out[:, 1] = gx.astype(np.float32), gy.astype(np.float32)
    return out, np.stack([gx, gy], axis=1)


def trajectory(n, seed, length=400.0):
    """a wandering 2-D path of n poses (a SLAM trajectory in its own frame)"""
    rng = np.random.default_rng(seed)
    u = np.linspace(0.0, 1.0, n)
    a, b = rng.uniform(0.5, 1.5, 2)
    x = length * u + 30.0 * np.sin(2 * np.pi * a * u)
    y = 0.35 * length * np.sin(np.pi * b * u) + 20.0 * np.cos(3 * np.pi * u)
    return np.stack([x, y], axis=1)


def scene(n, m, seed, noise=0.4, offset=(836000.0, 818000.0), angle=0.6, scale=1.02):
    """(gps_xy m x 2, slam_xy n x 2): the GPS track is the same path sampled at m other instants, moved by a
    similarity to national-grid offsets, with `noise` metres of Gaussian error"""
    rng = np.random.default_rng(seed + 1000)
    dense = trajectory(8 * max(n, m), seed)
    slam = dense[np.linspace(0, len(dense) - 1, n).round().astype(int)]
    g = dense[np.linspace(0, len(dense) - 1, m).round().astype(int)]
    c, s = np.cos(angle), np.sin(angle)
    gps = scale * (g @ np.array([[c, -s], [s, c]]).T) + np.asarray(offset) + rng.normal(0.0, noise, (m, 2))
    return gps, slam
