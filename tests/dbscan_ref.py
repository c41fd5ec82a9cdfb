"""Plain numpy / scipy references of DBSCAN by the contract of lio_dbscan (include/lio_gpu.h), written from the
contract alone.  Test infrastructure only.

neighbour_graph  brute-force float32 ((dx*dx + dy*dy) + dz*dz) over all pairs of finite points in row chunks of
                 512; i and j (j = i included) are neighbours where d2 <= float32(float64(float32(eps)) ** 2):
                 the inclusive test.
dbscan_sets      the contract as sets: core by row sums, scipy's connected_components on the core sub-graph, a
                 border point's cluster by the minimum over its core neighbours, labels by the rank of the
                 lowest core index.
dbscan_sequential  the literal procedure: clusters opened in index order at unlabelled core points, each expanded
                 fully with a stack over the same neighbour lists; a border point keeps the first cluster that
                 reaches it and spreads nothing.
Both return (labels int32[n], core bool[n]); non-finite rows are label -1, not core, nobody's neighbour.
Expected(pts, labels, core) turns that into everything lio_dbscan returns.
"""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

f32, f64 = np.float32, np.float64


def eps2(eps):
    e = f32(eps)
    return f32(f64(e) * f64(e))


def sqdist3(a, b):
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def neighbour_graph(pts, eps):
    """(fin, g): the input indices of the finite points, ascending, and their neighbour graph as a CSR matrix
    (m x m, diagonal included, column indices ascending in every row)"""
    xyz = np.asarray(pts, f32)[:, :3]
    fin = np.flatnonzero(np.isfinite(xyz).all(1))
    q = xyz[fin]
    e2 = eps2(eps)
    rows, cols = [np.zeros(0, np.int32)], [np.zeros(0, np.int32)]
    for i0 in range(0, len(q), 512):
        a, b = np.nonzero(sqdist3(q[i0:i0 + 512], q) <= e2)
        rows.append((a + i0).astype(np.int32))
        cols.append(b.astype(np.int32))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    g = csr_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(len(q), len(q)))
    g.sort_indices()
    return fin, g


def dbscan_sets(n, fin, g, min_samples, details=None):
    m = len(fin)
    deg = np.diff(g.indptr)
    is_core = deg >= min_samples
    key = np.full(m, n, np.int64)  # per finite point the lowest core index of its cluster; n: noise
    contested = 0
    if is_core.any():
        cidx = np.flatnonzero(is_core)
        sub = g[cidx][:, cidx]
        ncomp, comp = connected_components(sub, directed=False)
        low = np.full(ncomp, n, np.int64)
        np.minimum.at(low, comp, fin[cidx])
        key[cidx] = low[comp]
        for i in np.flatnonzero(~is_core):
            nb = g.indices[g.indptr[i]:g.indptr[i + 1]]
            nb = nb[is_core[nb]]
            if len(nb):
                ks = np.unique(key[nb])
                key[i] = ks[0]
                contested += len(ks) > 1
    labels = np.full(n, -1, np.int32)
    core = np.zeros(n, bool)
    core[fin] = is_core
    order = np.unique(key[key < n])  # ascending lowest core index = cluster number
    inside = key < n
    labels[fin[inside]] = np.searchsorted(order, key[inside]).astype(np.int32)
    if details is not None:
        details["contested"] = int(contested)
    return labels, core


def dbscan_sequential(n, fin, g, min_samples):
    m = len(fin)
    indptr, indices = g.indptr, g.indices
    is_core = np.diff(indptr) >= min_samples
    lab = np.full(m, -1, np.int64)
    nxt = 0
    for i in range(m):
        if lab[i] != -1 or not is_core[i]:
            continue
        lab[i] = nxt
        stack = [i]
        while stack:
            a = stack.pop()
            if not is_core[a]:
                continue
            nb = indices[indptr[a]:indptr[a + 1]]
            new = nb[lab[nb] == -1]
            lab[new] = nxt
            stack.extend(new.tolist())
        nxt += 1
    labels = np.full(n, -1, np.int32)
    core = np.zeros(n, bool)
    labels[fin] = lab
    core[fin] = is_core
    return labels, core


class Expected:
    """what lio_dbscan returns for these labels and core flags"""

    def __init__(self, pts, labels, core):
        xyz = np.asarray(pts, f32)[:, :3]
        self.labels = labels
        self.core = core
        self.core_indices = np.flatnonzero(core).astype(np.int64)
        k = int(labels.max()) + 1 if len(labels) else 0
        sizes = np.bincount(labels[labels >= 0], minlength=k)
        self.offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        by_label = np.argsort(labels, kind="stable")  # indices ascending inside a cluster
        self.indices = by_label[labels[by_label] >= 0].astype(np.int32)
        self.clusters = [self.indices[self.offsets[t]:self.offsets[t + 1]] for t in range(k)]
        self.aabb = np.array([np.concatenate([xyz[c].min(0), xyz[c].max(0)]) for c in self.clusters], f32).reshape(-1, 6)
        finite = int(np.isfinite(xyz).all(1).sum())
        self.stats = np.array([finite, core.sum(), k, (labels >= 0).sum()], np.int64)
        self.n_core, self.n_border = int(core.sum()), int((labels >= 0).sum() - core.sum())
        self.n_noise = finite - int((labels >= 0).sum())  # among the finite points
