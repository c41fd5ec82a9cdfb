#!/usr/bin/env python3
"""Timing of the GPU DBSCAN against the Euclidean cluster extraction of the same run and a CPU DBSCAN (not a test,
not bench.py).

    python scripts/dbscan_timing.py [--out profiles/dbscan_timing.json] [--skip-cpu] [--skip-gpu]

The step: lio_dbscan on the 2 M-point scene of scripts/denoise_timing.py at the offline pipeline's parameters
(eps 0.5, min_samples 10: post_process/clustering.py:30-36) — the whole Python call, the C call alone into
preallocated outputs, and lio_euclidean_clusters (0.5, 10, 25000) IN THE SAME PROCESS as the yardstick — with the
cluster / core / border / noise counts.  The CPU figure is sklearn.cluster.DBSCAN(n_jobs=16) on the float64 copy
where scikit-learn imports, else the cKDTree formulation of scripts/cluster_timing.py extended by the core rule;
the result names which.  The GPU step runs in a child process of its own under a time limit (`timeout`), so that
trouble in it ends it; a step that fails ends the run.  Times are host wall times of the whole call (upload,
kernels, download), the best of three after one warm-up call.

    rocprofv3 --kernel-trace --stats -- python scripts/dbscan_timing.py --child scene

gives the per-kernel table of that step (profiles/dbscan_kernel_stats.md holds one).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fast-lio-sam_gps_amd"), os.path.join(ROOT, "scripts")]

import numpy as np  # noqa: E402

from denoise_timing import best_of, slam_scene  # noqa: E402

PARAMS = dict(eps=0.5, min_samples=10)  # post_process/clustering.py:30-36
EUCLIDEAN = dict(tolerance=0.5, min_size=10, max_size=25000)  # the yardstick: scripts/cluster_timing.py


def gpu_step(name):
    import ctypes as C

    from lio_gpu import _capi
    from lio_gpu import filters as FL

    assert name == "scene"
    pts = slam_scene()
    n = len(pts)
    db = FL.DBSCAN(PARAMS["eps"], PARAMS["min_samples"])
    ms, clusters = best_of(lambda: db.fit(pts))
    # the C calls alone into preallocated outputs (the wrapper adds the allocation and the per-cluster slices)
    labels, idx, off = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n + 1, np.int64)
    core, box, stats, m = np.empty(n, np.uint8), np.empty((n, 6), np.float32), np.zeros(4, np.int64), C.c_int64(0)
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    call_ms, _ = best_of(lambda: _capi.check(_capi.lib().lio_dbscan(
        db._h, pts.ctypes.data_as(_capi.fp), n, pts.shape[1], PARAMS["eps"], PARAMS["min_samples"],
        labels.ctypes.data_as(i32p), core.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(m), n, off.ctypes.data_as(i64p),
        idx.ctypes.data_as(i32p), box.ctypes.data_as(_capi.fp), stats.ctypes.data_as(i64p))))
    sizes = np.diff(off[: m.value + 1])
    res = dict(step=name, n=n, ms=ms, c_call_ms=call_ms, bytes_up=pts.nbytes, bytes_down=int(5 * n + 4 * stats[3]),
               stats=[int(s) for s in stats], n_clusters=len(clusters), core=int(stats[1]),
               border=int(stats[3] - stats[1]), noise=int(stats[0] - stats[3]),
               largest=[int(s) for s in np.sort(sizes)[::-1][:5]])
    estats, em = np.zeros(4, np.int64), C.c_int64(0)
    res["euclidean_c_call_ms"], _ = best_of(lambda: _capi.check(_capi.lib().lio_euclidean_clusters(
        db._h, pts.ctypes.data_as(_capi.fp), n, pts.shape[1], EUCLIDEAN["tolerance"], EUCLIDEAN["min_size"],
        EUCLIDEAN["max_size"], labels.ctypes.data_as(i32p), C.byref(em), n, off.ctypes.data_as(i64p),
        idx.ctypes.data_as(i32p), box.ctypes.data_as(_capi.fp), estats.ctypes.data_as(i64p))))
    res["euclidean_stats"] = [int(s) for s in estats]
    res["ratio_to_euclidean"] = call_ms / res["euclidean_c_call_ms"]
    return res


def cpu_dbscan(pts, workers=16):
    """(method, clusters, core, border, noise)"""
    xyz = pts[:, :3].astype(np.float64)
    try:
        from sklearn.cluster import DBSCAN
    except ImportError:
        DBSCAN = None
    if DBSCAN is not None:
        sk = DBSCAN(eps=PARAMS["eps"], min_samples=PARAMS["min_samples"], n_jobs=workers).fit(xyz)
        k, ncore, nin = int(sk.labels_.max()) + 1, len(sk.core_sample_indices_), int((sk.labels_ >= 0).sum())
        return f"sklearn.cluster.DBSCAN(n_jobs={workers})", k, ncore, nin - ncore, len(xyz) - nin
    return cpu_dbscan_ckdtree(xyz, workers)


def cpu_dbscan_ckdtree(xyz, workers=16):
    """the cKDTree formulation of scripts/cluster_timing.py with the core rule: components of the core graph"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree

    n, chunk = len(xyz), 50_000
    tree = cKDTree(xyz)
    deg = tree.query_ball_point(xyz, PARAMS["eps"], workers=workers, return_length=True)
    is_core = deg >= PARAMS["min_samples"]
    label = np.arange(n)  # components of the core graph; a border point records one core neighbour's component
    reached = is_core.copy()
    for i0 in range(0, n, chunk):
        hits = tree.query_ball_point(xyz[i0:i0 + chunk], PARAMS["eps"], workers=workers)
        lens = np.fromiter((len(h) for h in hits), np.int64, len(hits))
        rows = np.repeat(np.arange(i0, i0 + len(hits)), lens)
        cols = np.fromiter((j for h in hits for j in h), np.int64, int(lens.sum()))
        both = is_core[rows] & is_core[cols]
        near_core = np.zeros(n, bool)
        near_core[rows[is_core[cols]]] = True
        reached |= near_core
        rows, cols = np.concatenate([rows[both], np.arange(n)]), np.concatenate([cols[both], label])
        g = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n, n))
        _, comp = connected_components(g, directed=False)
        _, first = np.unique(comp, return_index=True)
        label = first[comp]
    k = len(np.unique(label[is_core]))
    return ("cKDTree.query_ball_point + csgraph.connected_components", k, int(is_core.sum()),
            int(reached.sum() - is_core.sum()), int(n - reached.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbscan_timing.json"))
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--skip-gpu", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--limit", type=int, default=240, help="time limit of the GPU step [s]")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(gpu_step(a.child)))
        return 0
    res = dict(params=PARAMS, euclidean_params=EUCLIDEAN, gpu=[], cpu=[])
    if os.path.exists(a.out):  # a run with --skip-gpu or --skip-cpu keeps the other half of an earlier run
        with open(a.out) as f:
            old = json.load(f)
        res["gpu"], res["cpu"] = old.get("gpu", []), old.get("cpu", [])
    if not a.skip_gpu:
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "scene"],
                           capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"scene: failed (exit {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            return 1  # nothing more is started on the GPU
        res["gpu"] = [json.loads(line[0][7:])]
        print(res["gpu"][-1], flush=True)
    if not a.skip_cpu:
        pts = slam_scene()
        t0 = time.perf_counter()
        method, k, ncore, nborder, nnoise = cpu_dbscan(pts)
        res["cpu"] = [dict(step="scene", n=len(pts), ms=(time.perf_counter() - t0) * 1e3, n_clusters=k, core=ncore,
                           border=nborder, noise=nnoise, workers=16, cpus=os.cpu_count(), method=method)]
        print(res["cpu"][-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
