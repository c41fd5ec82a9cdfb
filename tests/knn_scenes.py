"""Constructed scenes for the grid kNN (front end, seeded pass, batch search) and the loop ICP's 1-NN.

Test infrastructure only, shared by tests/test_knn_ref.py (CPU: the brute-force reference against the oracle's
kd-tree, and every scene's "teeth" counted by the reference alone) and tests/test_gpu_knn_faces.py.  Points are
placed by the grid's own float32 arithmetic (knn_ref.cell_of / face / grid_geom), so they sit exactly on cell
faces, one float either side of them, and - at large offsets - where a rounded face disagrees with the cell
assignment.  Every scene is deterministic; the map has at most 30 000 points, the queries at most 4 000.

A scene's queries are reached through the front end with the pose (identity rotation, t_LI = synth.T_LI,
t = centre - t_LI) and the scan body = queries - centre: the body is exact in float32 (Scene.body checks it: the
queries lie within about 100 m of the centre, or the centre is 0) and world = float((body + t_LI) + t) gives the
queries back bit for bit (the GPU test checks that too).
"""
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from knn_ref import F32, base_margin, brute_knn, cell_of, face, first_float_of_cell, grid_geom  # noqa: F401

CELLS = (1.0, 0.6, 2.3)
OFFSETS = ((1e4, -1e4, 50.0), (3e4, 3e4, 100.0), (1e5, -2e5, 100.0), (1e6, 1e6, 0.0))
RANGE_SQ = 5.0


@dataclass
class Scene:
    name: str
    cell: float              # the cell size asked for
    pts: np.ndarray          # the map, float32 (n, 3); ids = rows
    queries: np.ndarray      # float32 (m, 3)
    centre: np.ndarray       # float64 (3): the pose translation that keeps the scan body small
    origin: np.ndarray = None   # grid_geom of pts
    cell_eff: float = None
    dims: np.ndarray = None
    info: dict = field(default_factory=dict)
    queries_far: np.ndarray = None  # queries for range-bounded searches only (an unbounded walk would be long)

    def __post_init__(self):
        self.pts = np.ascontiguousarray(self.pts, np.float32)
        self.queries = np.ascontiguousarray(self.queries, np.float32)
        self.origin, self.cell_eff, self.dims = grid_geom(self.pts, self.cell)
        assert len(self.pts) <= 30000 and len(self.queries) <= 4000

    @property
    def margin(self):
        return base_margin(self.cell_eff)

    def body(self, q=None):
        q = self.queries if q is None else q
        b = (np.asarray(q, np.float64) - self.centre).astype(np.float32)
        fin = np.isfinite(b).all(axis=1)
        assert np.array_equal(b[fin].astype(np.float64) + self.centre, np.asarray(q, np.float64)[fin])
        return b


def pose24(scene, shift=(0.0, 0.0, 0.0)):
    """identity rotation, t_LI = synth.T_LI, t = centre - t_LI (+ shift)"""
    from lio_gpu import synth

    p = np.zeros(24)
    p[0:9] = np.eye(3).ravel()
    p[12:21] = np.eye(3).ravel()
    p[21:24] = synth.T_LI
    p[9:12] = scene.centre - synth.T_LI + np.asarray(shift, np.float64)
    return p


def _step(v, n):
    """v moved by n floats"""
    v = np.asarray(v, np.float32).copy()
    for _ in range(abs(int(n))):
        v = np.nextafter(v, F32(np.inf if n > 0 else -np.inf))
    return v


# ------------------------------------------------------------------ restated stop rule (teeth of scene b)
def own_radius(q, origin, cell, margin):
    """`own` of group_knn_near: the distance from q to the nearest face of its own cell, from the computed
    faces lo = o + c * cell and lo + cell, minus the margin (float32 throughout)"""
    q = np.asarray(q, np.float32)
    o = np.asarray(origin, np.float32)
    cs, m = F32(cell), F32(margin)
    lo = o + cell_of(q, o, cs).astype(np.float32) * cs
    a = np.minimum(q - lo, (lo + cs) - q)
    return np.minimum(np.minimum(a[..., 0], a[..., 1]), a[..., 2]) - m


def early_stop_drops(scene, margin=None, bound=RANGE_SQ):
    """Queries for which a stop rule of the shell walk fires although the true 5-NN holds a point the walk has
    not scanned: after the own cell (own > 0 and d5 < own * own * 0.999999f, d5 the 5th best of the own cell)
    or after the 3x3x3 block (gr = own + cell, d5 the block's).  The search then returns without that point.
    Restated in numpy from the reference's lists; margin: the face slack to judge.  Returns (stage 0, stage 1)."""
    o, cs = scene.origin, scene.cell_eff
    m = scene.margin if margin is None else F32(margin)
    q = scene.queries
    fin = np.isfinite(scene.pts).all(axis=1)
    cq = cell_of(q, o, cs)
    cp = cell_of(scene.pts, o, cs)
    inside = ((cq >= 0) & (cq < scene.dims)).all(axis=1)
    own = own_radius(q, o, cs, m)
    ids, _ = scene_knn(scene, 5, bound)
    out = np.zeros((2, len(q)), bool)
    for i in np.nonzero(inside & (own > 0))[0]:
        dc = np.abs(cp - cq[i]).max(axis=1)
        true_ids = ids[i][ids[i] >= 0]
        for stage in (0, 1):
            seen = np.nonzero((dc <= stage) & fin)[0]
            if len(seen) < 5:
                continue
            od = brute_knn(q[i:i + 1], scene.pts[seen], 5, bound)[1]
            reach = own[i] if stage == 0 else F32(own[i] + cs)
            if od[0, 4] < reach * reach * F32(0.999999):  # a full list inside the reach: the walk stops here
                out[stage, i] = bool((dc[true_ids] > stage).any())
                break
    return out


@lru_cache(maxsize=None)
def _scene_knn_cached(key, k, range_sq):
    sc = _REGISTRY[key]
    return brute_knn(sc.queries, sc.pts, k, range_sq)


_REGISTRY = {}


def scene_knn(scene, k=5, range_sq=RANGE_SQ):
    """brute_knn(scene.queries, scene.pts) computed once per (scene, k, range) and shared (read-only)"""
    _REGISTRY[scene.name] = scene
    ids, d2 = _scene_knn_cached(scene.name, k, float(range_sq))
    ids.setflags(write=False)
    d2.setflags(write=False)
    return ids, d2


# ------------------------------------------------------------------ a / b: faces, at any offset
NC = 12   # cells per horizontal axis that hold the background, the face and the tie points
NCH = 24  # cells per horizontal axis in all: the far-offset traps use every face of them
NCZ = 42  # and in z: cells [0, 7) background, faces and ties, [8, 42) the far-offset traps on 8 levels


def _trap_combos(o, cs, m, kbase, axes, spacing):
    """(axis, k, dir, stage) for which a restated stop rule of the shell walk reaches past the nearest point it
    has not scanned.  stage 0: `own` after the own cell; stage 1: `own + cell` after the 3x3x3 block.
    dir +1: the query in cell k - 1 below face k, p the first float of cell k + stage;
    dir -1: the query in cell k above face k, p the last float of cell k - 1 - stage."""
    out = []
    for a in axes:
        for k in range(int(kbase[a]) + 2, int(kbase[a]) + NCH - 1):
            for d in (1, -1):
                for stage in (0, 1):
                    vmin = first_float_of_cell(o[a], k + stage if d > 0 else k - stage, cs)
                    p = vmin if d > 0 else np.nextafter(vmin, F32(-np.inf))
                    edge = first_float_of_cell(o[a], k, cs)  # the query's distance g from its own face
                    edge = edge if d > 0 else np.nextafter(edge, F32(-np.inf))
                    g = max(F32(0.3 if stage == 0 else 0.2) * cs, (4 if stage == 0 else 2) * spacing[a])
                    qx = F32(edge - F32(d) * g)
                    lo = face(o[a], k - 1 if d > 0 else k, cs)
                    own = (F32(F32(lo + cs) - qx) if d > 0 else F32(qx - lo)) - m
                    reach = own if stage == 0 else F32(own + cs)
                    dp = F32(qx - p)
                    if (cell_of(qx, o[a], cs) == (k - 1 if d > 0 else k) and own > 0
                            and dp * dp < reach * reach * F32(0.999999)):
                        out.append((a, k, d, stage, F32(p), F32(qx), F32(reach), F32(dp * dp)))
    return out


def _ring(rng, q, a, d, lo_r, hi_r, n=1500):
    """candidate neighbours of q at radii inside (lo_r, hi_r): along axis a away from the face, across the
    other horizontal axis on its float lattice, and z (the fine lattice) solved for the radius"""
    tr = 1 - a
    rt = rng.uniform(lo_r, hi_r, n)
    c = np.tile(q, (n, 1)).astype(np.float32)
    c[:, a] = (q[a] - d * rng.uniform(0, 0.25, n) * rt).astype(np.float32)
    c[:, tr] = (q[tr] + rng.uniform(-0.8, 0.8, n) * rt).astype(np.float32)
    ea = c[:, a].astype(np.float64) - float(q[a])
    et = c[:, tr].astype(np.float64) - float(q[tr])
    ez2 = rt * rt - ea * ea - et * et
    ez = np.sqrt(np.maximum(ez2, 0.0)) * rng.choice([-1.0, 1.0], n)
    c[:, 2] = (q[2] + ez).astype(np.float32)
    return c[ez2 > 0]


def _faces_build(name, cell, offset, seed, cluster_a=None, centre=None):
    rng = np.random.default_rng(seed)
    c = np.asarray(offset, np.float64)
    csd = float(F32(cell))
    lo = (c + 0.25 * csd).astype(np.float32)
    hi = (c + (np.array([NCH, NCH, NCZ]) - 0.25) * csd).astype(np.float32)
    anchors = [lo, hi]
    if cluster_a is not None:
        anchors += list(cluster_a)
    o, cs, dims = grid_geom(np.array(anchors, np.float32), cell)
    assert cs == F32(cell)
    m = base_margin(cs)
    kbase = cell_of(lo, o, cs)  # the box holds cells kbase .. kbase + NC - 1
    inlo, inhi = np.nextafter(lo, F32(np.inf)), np.nextafter(hi, F32(-np.inf))
    spacing = np.spacing(np.maximum(np.abs(lo), np.abs(hi))).astype(np.float32)
    zsplit = 7

    def fc(a, k):
        return F32(face(o[a], k, cs))

    def clip(p):
        return np.minimum(np.maximum(np.asarray(p, np.float32), inlo), inhi)

    pts, qs = [lo[None], hi[None]], []
    if cluster_a is not None:
        pts.append(np.asarray(cluster_a, np.float32))
    # sparse uniform background
    zb_hi = fc(2, kbase[2] + zsplit)
    hb = np.array([fc(0, kbase[0] + NC), fc(1, kbase[1] + NC), zb_hi], np.float32)
    bg = rng.uniform(lo, hb, (3000, 3))
    pts.append(clip(bg))

    def zone_a():
        return rng.uniform(lo + cs, hb - cs)

    # points exactly on faces, one float below / above, on one, two and three axes
    deltas = [("ulp", 0), ("ulp", -1), ("ulp", 1)] + [("m", s * d) for d in (0.5, 1.0, 2.0) for s in (-1.0, 1.0)]
    for i in range(150):
        axes = rng.permutation(3)[: 1 + i % 3]
        base = zone_a()
        ks = {a: int(kbase[a]) + int(rng.integers(2, zsplit - 1 if a == 2 else NC - 1)) for a in axes}
        for var in (-1, 0, 1):
            p = (base + rng.uniform(-0.05, 0.05, 3) * csd).astype(np.float32)
            for a in axes:
                p[a] = _step(fc(a, ks[a]), var)
            pts.append(p[None])
        for kind, d in deltas:
            q = (base + rng.uniform(-0.05, 0.05, 3) * csd).astype(np.float32)
            for a in axes:
                f = fc(a, ks[a])
                q[a] = _step(f, d) if kind == "ulp" else F32(f + F32(d) * m)
            qs.append(q[None])
    # ties: a pair at equal distance either side of a face (different cells), four closer points
    for i in range(90):
        a = i % 3
        b, e = (a + 1) % 3, (a + 2) % 3
        q = zone_a().astype(np.float32)
        q[a] = fc(a, int(kbase[a]) + int(rng.integers(2, zsplit - 1 if a == 2 else NC - 1)))
        dlt = max(F32(0.125), 4 * spacing.max())
        w = F32(dlt / 4)
        unit = np.eye(3, dtype=np.float32)
        pair = [q + dlt * unit[a], q - dlt * unit[a]]
        if rng.integers(0, 2):
            pair.reverse()
        near = [q + w * unit[b], q - 2 * w * unit[b], q + 3 * w * unit[e], q + 2 * w * unit[b] + 2 * w * unit[e]]
        pts.append(np.array(near + pair, np.float32))
        qs.append(q[None])
    # cell centres, uniform queries
    kc = kbase + rng.integers(0, NC, (200, 3))
    qs.append((o + (kc.astype(np.float32) + F32(0.5)) * cs).astype(np.float32))
    qs.append(rng.uniform(lo, hi, (300, 3)).astype(np.float32))
    if cluster_a is not None:
        qs.append((np.asarray(cluster_a[:100], np.float64) + rng.uniform(-0.3, 0.3, (100, 3))).astype(np.float32))
    # traps (far offsets): five neighbours of the query, all inside what the walk has scanned when its stop
    # rule is tested, between the nearest point p it has not scanned and the radius the rounded faces claim
    combos = _trap_combos(o, cs, m, kbase, (0, 1), spacing) if np.abs(c).max() >= 1e3 or cluster_a is not None else []
    n_traps = [0, 0]
    if combos:
        # one trap per (axis, level, row, half of the row): three or more cells apart each way, so the
        # points of one trap (within 1.3 cells of its query) are farther from another's query than its own
        slots = [(a, lev, t, r) for lev in range(8) for t in range(1, NCH - 1, 3) for r in range(4) for a in (0, 1)]
        for si, (a_want, lev, t, r) in enumerate(slots):
            sel = [cb for cb in combos if cb[0] == a_want and 2 + 6 * r <= cb[1] - int(kbase[a_want]) <= 4 + 6 * r]
            if not sel or sum(n_traps) >= 160:
                continue
            a, k, d, stage, p1, qx, reach, d2p = sel[si % len(sel)]
            tr = 1 - a  # the other horizontal axis
            q = np.empty(3, np.float32)
            q[a] = qx
            q[tr] = F32(o[tr] + (F32(kbase[tr] + t) + F32(0.5)) * cs)
            q[2] = F32(o[2] + (F32(kbase[2] + 10 + 4 * lev) + F32(0.5)) * cs)
            p = q.copy()
            p[a] = p1
            cnd = _ring(rng, q, a, d, np.sqrt(float(d2p)), float(reach) * np.sqrt(0.999999))
            dd = q - cnd
            d2 = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
            dc = np.abs(cell_of(cnd, o, cs) - cell_of(q, o, cs)).max(axis=1)
            ok = (d2 > d2p) & (d2 < reach * reach * F32(0.999999)) & (dc <= stage)
            cnd = np.unique(cnd[ok], axis=0)
            if len(cnd) < 5:
                continue
            pts.append(np.concatenate([cnd[rng.permutation(len(cnd))[:5]], p[None]]))
            qs.append(q[None])
            n_traps[stage] += 1
    pts = np.concatenate(pts)
    qs = np.concatenate(qs)
    sc = Scene(name, cell, pts, qs, c if centre is None else np.asarray(centre, np.float64),
               info=dict(kbase=kbase, n_traps=n_traps, n_combos=len(combos)))
    assert np.array_equal(sc.origin, o) and np.array_equal(sc.dims, dims)
    return sc


@lru_cache(maxsize=None)
def faces(cell, offset=(0.0, 0.0, 0.0)):
    """scene (a) at offset 0, scene (b) at the far offsets (rebuilt there, not translated)"""
    tag = "faces" if not any(offset) else "far"
    return _faces_build(f"{tag}-{cell}-{offset}", cell, offset, seed=11)


@lru_cache(maxsize=None)
def extent():
    """origin near 0, two clusters 20 km apart along x, cell 2.3: the faces near x = 20 km are computed from an
    origin near 0 (o + k * cell with k ~ 8700).  The table is 8700 x 14 x 14 cells."""
    rng = np.random.default_rng(5)
    a = rng.uniform(0.6, 27.0, (500, 3)).astype(np.float32)
    return _faces_build("extent-2.3", 2.3, (20000.0, 0.0, 0.0), seed=12, cluster_a=a, centre=(0.0, 0.0, 0.0))


def shared_face_teeth(scene, ids):
    """queries whose 5-NN (ids) holds a point of another cell within 2 * margin of the face the cells share"""
    o, cs, m = scene.origin, scene.cell_eff, scene.margin
    cq = cell_of(scene.queries, o, cs)
    cp = cell_of(scene.pts, o, cs)
    hit = np.zeros(len(ids), bool)
    for j in range(ids.shape[1]):
        i = ids[:, j]
        ok = i >= 0
        c = cp[np.maximum(i, 0)]
        p = scene.pts[np.maximum(i, 0)]
        for a in range(3):
            adj = ok & (np.abs(c[:, a] - cq[:, a]) == 1)
            f = face(o[a], np.maximum(c[:, a], cq[:, a]), cs)
            hit |= adj & (np.abs(p[:, a].astype(np.float64) - f) <= 2.0 * float(m))
    return hit


def tie_teeth(scene):
    """queries with two equal d2 among their six nearest whose points lie in different cells"""
    ids, d2 = scene_knn(scene, 6, RANGE_SQ)
    cp = cell_of(scene.pts, scene.origin, scene.cell_eff)
    hit = np.zeros(len(ids), bool)
    for j in range(5):
        both = (ids[:, j] >= 0) & (ids[:, j + 1] >= 0) & (d2[:, j] == d2[:, j + 1])
        diff = (cp[np.maximum(ids[:, j], 0)] != cp[np.maximum(ids[:, j + 1], 0)]).any(axis=1)
        hit |= both & diff
    return hit


# ------------------------------------------------------------------ c: cell populations
NPOP = 71


@lru_cache(maxsize=None)
def populations(cell, seed=20):
    """Cell j of one x row holds exactly j points (j = 0..70); the rows beside it hold 0-4 points per cell.
    The row is the last one before the +y pad, so queries just outside the grid on that side reach it."""
    rng = np.random.default_rng(seed)
    cs = F32(cell)
    csd = float(cs)
    lo = np.array([0.5, 0.5, 0.5], np.float32) * cs
    hi = np.array([(NPOP + 5.5) * csd, 4.5 * csd, 6.5 * csd], np.float32)
    o, ce, dims = grid_geom(np.array([lo, hi]), cell)
    k0 = cell_of(lo, o, cs)
    row_y, row_z, x0 = int(k0[1]) + 4, int(k0[2]) + 3, int(k0[0]) + 3
    assert row_y == dims[1] - 2

    def inside(cx, cy, cz, n):
        c = np.array([cx, cy, cz], np.float32)
        p = (o + (c + rng.uniform(0.08, 0.92, (n, 3)).astype(np.float32)) * cs).astype(np.float32)
        assert (cell_of(p, o, cs) == [cx, cy, cz]).all()
        return p

    pts = [lo[None], hi[None]]
    beside = {}
    for j in range(NPOP):
        pts.append(inside(x0 + j, row_y, row_z, j))
        for dy, dz in ((-1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1)):
            n = int(rng.integers(1, 5)) if rng.random() < (0.12 if j < 12 else 0.5) else 0
            if n:
                pts.append(inside(x0 + j, row_y + dy, row_z + dz, n))
            beside[(j, dy, dz)] = n
    qs, own_cell = [], []
    yc = F32(o[1] + (F32(row_y) + F32(0.5)) * cs)
    zc = F32(o[2] + (F32(row_z) + F32(0.5)) * cs)
    ytop = first_float_of_cell(o[1], int(dims[1]), cs)  # first y outside the grid
    for j in range(NPOP):
        xl = first_float_of_cell(o[0], x0 + j, cs)
        xh = np.nextafter(first_float_of_cell(o[0], x0 + j + 1, cs), F32(-np.inf))
        xm = F32(o[0] + (F32(x0 + j) + F32(0.5)) * cs)
        for x in (xm, xl, xh):
            qs.append([x, yc, zc])
            own_cell.append(j)
            qs.append([x, _step(ytop, int(rng.integers(0, 3))), zc])
            own_cell.append(-1)
        if j < 16:  # from the sparse row beside it: an own cell of 0-4 points, the row in the table
            qs.append([xm, F32(yc - cs), zc])
            own_cell.append(beside[(j, -1, 0)])
    # the small tables by construction: an empty own cell whose only neighbour holds T points, T = 1..20
    for t in range(1, 21):
        cx, cy, cz = x0 + 3 * (t - 1), row_y - 3, row_z + 3
        pts.append(inside(cx + 1, cy, cz, t))
        qs.append(list((o + (np.array([cx, cy, cz], np.float32) + F32(0.5)) * cs).astype(np.float32)))
        own_cell.append(0)
    sc = Scene(f"pop-{cell}", cell, np.concatenate(pts), np.array(qs, np.float32), np.zeros(3),
               info=dict(own_pop=np.array(own_cell), row=(x0, row_y, row_z)))
    assert np.array_equal(sc.origin, o) and np.array_equal(sc.dims, dims)
    return sc


def table_sizes(scene):
    """Restated near pass of every in-row query: T = points of the shell-1 cells (3x3x3 block minus the own
    cell) left after the axis_gap prune against the own cell's 5th best (the range when it holds fewer)."""
    o, cs, m = scene.origin, scene.cell_eff, scene.margin
    w = F32(cs + F32(2) * m)
    cp = cell_of(scene.pts, o, cs)
    counts = {}
    for c in map(tuple, cp):
        counts[c] = counts.get(c, 0) + 1
    T = np.full(len(scene.queries), -1)

    def gap(q, lo_, hi_):
        g = np.maximum(np.maximum(lo_ - q, q - hi_), F32(0))
        return g * g

    for i, q in enumerate(scene.queries):
        if scene.info["own_pop"][i] < 0:
            continue
        c = cell_of(q, o, cs)
        mine = np.nonzero((cp == c).all(axis=1))[0]
        bound = F32(RANGE_SQ)
        if len(mine) >= 5:
            bound = brute_knn(q[None], scene.pts[mine], 5, RANGE_SQ)[1][0, 4]
        lo = o + c.astype(np.float32) * cs
        t = 0
        for k in range(27):
            if k == 13:
                continue
            d = np.array([k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1])
            l = lo + d.astype(np.float32) * cs - m
            bd = (gap(q[0], l[0], l[0] + w) + gap(q[1], l[1], l[1] + w)) + gap(q[2], l[2], l[2] + w)
            if not bd * F32(0.999999) > bound:
                t += counts.get(tuple(c + d), 0)
        T[i] = t
    return T


# ------------------------------------------------------------------ d: flat and thin grids
@lru_cache(maxsize=None)
def thin(cell, kind):
    """kind: plane (nz == 3), line (ny == nz == 3), one, five"""
    rng = np.random.default_rng({"plane": 31, "line": 32, "one": 33, "five": 34}[kind])
    cs = float(F32(cell))
    if kind == "plane":
        m = np.stack([rng.uniform(0, 10, 2000), rng.uniform(0, 10, 2000), np.full(2000, 1.25)], 1)
    elif kind == "line":
        m = np.stack([rng.uniform(0, 20, 300), np.full(300, -2.5), np.full(300, 1.25)], 1)
    elif kind == "one":
        m = np.array([[3.0, -1.0, 2.0]])
    else:
        m = rng.uniform(-0.4, 0.4, (5, 3)) * cs + [3.0, -1.0, 2.0]
    m = m.astype(np.float32)
    lo, hi = m.min(0).astype(np.float64), m.max(0).astype(np.float64)
    n = 120
    q_in = rng.uniform(lo - cs, hi + cs, (n, 3))
    q_out = rng.uniform(lo, hi + 1e-9, (n, 3))
    ax = rng.integers(0, 3, n)
    side = rng.integers(0, 2, n)
    off = rng.uniform(0.01, 2.5, n) + cs  # beyond the one-cell pad: up to 2.5 m outside the grid
    q_out[np.arange(n), ax] = np.where(side == 1, hi[ax] + off, lo[ax] - off)
    # up to 60 cells away (the unbounded walk visits whole shells until five are found)
    q_away = rng.uniform(lo, hi + 1e-9, (60, 3))
    ax = rng.integers(0, 3, 60)
    far = rng.uniform(3, 58, 60) * cs
    far[:6] = 58 * cs
    q_away[np.arange(60), ax] = np.where(rng.integers(0, 2, 60) == 1, hi[ax] + far, lo[ax] - far)
    q_far = np.array([[500.0, 0, 0], [-1e4, 3, 2], [0, 0, 3e5], [lo[0], 1e6, lo[2]]])
    sc = Scene(f"thin-{kind}-{cell}", cell, m, np.concatenate([q_in, q_out, q_away]), np.zeros(3),
               queries_far=q_far.astype(np.float32))
    return sc


# ------------------------------------------------------------------ e: grown cell
@lru_cache(maxsize=None)
def grown():
    """two clusters whose 1.0 m table would hold 5.46e8 cells (> 2^29): the build doubles the cell to 2.0"""
    rng = np.random.default_rng(41)
    a = rng.uniform(0, 10, (5000, 3))
    b = rng.uniform(0, 10, (5000, 3)) + [1000.0, 800.0, 650.0]
    m = np.concatenate([a, b]).astype(np.float32)
    qa = rng.uniform(-3, 13, (600, 3))
    qb = rng.uniform(-3, 13, (600, 3)) + [1000.0, 800.0, 650.0]
    add = (rng.uniform(0, 10, (800, 3)) + [1000.0, 800.0, 650.0]).astype(np.float32)
    sc = Scene("grown", 1.0, m, np.concatenate([qa, qb]), np.zeros(3), info=dict(add=add))
    return sc


# ------------------------------------------------------------------ f: non-finite rows
def _bad_rows(n, rng):
    pos = sorted({0, 7, 8, 63, 64, n - 1} | {b + int(rng.integers(0, min(97, n - b))) for b in range(0, n, 97)})
    vals = [np.nan, np.inf, -np.inf]
    return [(p, vals[i % 3], (i // 3) % 3) for i, p in enumerate(pos)]  # (row, value, column)


@lru_cache(maxsize=None)
def nonfinite(cell, where):
    """scene (a) with NaN / +inf / -inf rows at 0, 7, 8, 63, 64, the last row and one in every 97;
    where: 'scan' (the queries) or 'map' (the points given to Build)"""
    base = faces(cell)
    rng = np.random.default_rng(51)
    pts, qs = base.pts.copy(), base.queries.copy()
    if where == "map":  # copies of the two AABB anchors (rows 0, 1) stay finite, so the grid is scene (a)'s
        pts = np.concatenate([pts, pts[0:2], pts[2:3]])
    tgt = qs if where == "scan" else pts
    rows = [r for r in _bad_rows(len(tgt), rng) if where == "scan" or r[0] not in (len(pts) - 3, len(pts) - 2)]
    for i, (r, v, col) in enumerate(rows):
        tgt[r, col] = v
        if i % 4 == 3:
            tgt[r, :] = v
    bad = np.array([r for r, _, _ in rows])
    sc = Scene(f"nonfinite-{where}-{cell}", cell, pts, qs, base.centre, info=dict(bad=bad))
    return sc


# ------------------------------------------------------------------ the catalogue
def _catalogue():
    cat = {}
    for cell in CELLS:
        cat[f"faces-{cell}"] = (lambda c=cell: faces(c))
        for off in OFFSETS:
            cat[f"far-{cell}-{off[0]:g}"] = (lambda c=cell, o=off: faces(c, o))
        cat[f"pop-{cell}"] = (lambda c=cell: populations(c))
        for kind in ("plane", "line", "one", "five"):
            cat[f"thin-{kind}-{cell}"] = (lambda c=cell, k=kind: thin(c, k))
        for where in ("scan", "map"):
            cat[f"nonfinite-{where}-{cell}"] = (lambda c=cell, w=where: nonfinite(c, w))
    cat["extent-2.3"] = extent
    cat["grown"] = grown
    return cat


SCENES = _catalogue()
ICP_SCENES = [k for k in SCENES if k.split("-")[0] in ("faces", "far", "extent", "thin", "grown")]
# scene (b): where the float arithmetic lets a restated stop rule (own, own + cell) reach past an unscanned
# point at all, and within which range the trapped neighbour lies (5.0: the front end's, inf: the batch search)
TRAPPED = {"far-0.6-1e+06": RANGE_SQ, "far-2.3-100000": np.inf, "extent-2.3": RANGE_SQ}
