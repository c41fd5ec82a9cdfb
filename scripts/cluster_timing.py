#!/usr/bin/env python3
"""Timing of the Euclidean cluster extraction against scipy's cKDTree on the host (not a test, not bench.py).

    python scripts/cluster_timing.py [--out profiles/cluster_timing.json] [--skip-cpu] [--skip-gpu]

Steps: lio_euclidean_clusters on the 2 M-point scene of scripts/denoise_timing.py and on that scene's denoised
output, at the reference's commented parameters (tolerance 0.5, min 10, max 25000: fast_lio_sam.cpp:343-363),
and the same work with scipy.spatial.cKDTree — query_ball_point(workers=16) in chunks of points, the hits
folded into the components chunk by chunk with scipy.sparse.csgraph.connected_components — as the only CPU
reference available here.  It is NOT PCL's serial breadth-first search (one radiusSearch per queue element on
one thread); it uses 16 workers for the neighbour queries and float64 distances.  Every GPU step runs in a child
process of its own under a time limit (`timeout`), so that trouble in one ends it; a step that fails ends the
run.  Times are host wall times of the whole call (upload, kernels, download), the best of three after one
warm-up call.
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

from denoise_timing import CFG, best_of, slam_scene  # noqa: E402

PARAMS = dict(tolerance=0.5, min_size=10, max_size=25000)  # fast_lio_sam.cpp:343-363


def step_cloud(name):
    """the scene, or its denoised output (lio_denoise_slam_map at the shipped configuration)"""
    pts = slam_scene()
    if name == "scene":
        return pts
    from lio_gpu import filters as FL

    out, _ = FL.denoise_slam_map(pts, **CFG)
    return out


def gpu_step(name):
    import ctypes as C

    from lio_gpu import _capi
    from lio_gpu import filters as FL

    pts = step_cloud(name)
    ec = FL.EuclideanClusterExtraction(PARAMS["tolerance"], PARAMS["min_size"], PARAMS["max_size"])
    ms, clusters = best_of(lambda: ec.extract(pts))
    # the C call alone into preallocated outputs (the wrapper adds the allocation and the per-cluster slices)
    n = len(pts)
    labels, idx, off = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n + 1, np.int64)
    box, stats, m = np.empty((n, 6), np.float32), np.zeros(4, np.int64), C.c_int64(0)
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    call_ms, _ = best_of(lambda: _capi.check(_capi.lib().lio_euclidean_clusters(
        ec._h, pts.ctypes.data_as(_capi.fp), n, pts.shape[1], PARAMS["tolerance"], PARAMS["min_size"], PARAMS["max_size"],
        labels.ctypes.data_as(i32p), C.byref(m), n, off.ctypes.data_as(i64p), idx.ctypes.data_as(i32p),
        box.ctypes.data_as(_capi.fp), stats.ctypes.data_as(i64p))))
    sizes = np.diff(off[: m.value + 1])
    return dict(step=name, n=n, ms=ms, c_call_ms=call_ms, bytes_up=pts.nbytes, bytes_down=int(4 * n + 4 * stats[3]),
                stats=[int(s) for s in stats], largest=[int(s) for s in sizes[:5]], n_clusters=len(clusters))


def cpu_clusters(pts, workers=16, chunk=50_000):
    """components of the radius graph: label[i] = a representative of i's component, refined chunk by chunk
    (the edges of one chunk's queries plus a star edge i -> label[i] per point keep what earlier chunks joined)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree

    xyz = pts[:, :3].astype(np.float64)
    n = len(xyz)
    tree = cKDTree(xyz)
    label = np.arange(n)
    for i0 in range(0, n, chunk):
        hits = tree.query_ball_point(xyz[i0:i0 + chunk], PARAMS["tolerance"], workers=workers)
        lens = np.fromiter((len(h) for h in hits), np.int64, len(hits))
        rows = np.repeat(np.arange(i0, i0 + len(hits)), lens)
        cols = np.fromiter((j for h in hits for j in h), np.int64, int(lens.sum()))
        rows, cols = np.concatenate([rows, np.arange(n)]), np.concatenate([cols, label])
        g = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n, n))
        _, comp = connected_components(g, directed=False)
        _, first = np.unique(comp, return_index=True)
        label = first[comp]  # a point of the component stands for it
        if (i0 // chunk) % 8 == 7:
            print(f"cpu: {i0 + chunk} of {n} points", file=sys.stderr, flush=True)
    sizes = np.unique(label, return_counts=True)[1]
    ok = (sizes >= PARAMS["min_size"]) & (sizes <= PARAMS["max_size"])
    return len(sizes), int(ok.sum()), int(sizes[ok].sum()), np.sort(sizes[ok])[::-1][:5]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_timing.json"))
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--skip-gpu", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--limit", type=int, default=240, help="time limit of one GPU step [s]")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(gpu_step(a.child)))
        return 0
    res = dict(params=PARAMS, gpu=[], cpu=[])
    for step in () if a.skip_gpu else ("scene", "denoised"):
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", step],
                           capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{step}: failed (exit {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            return 1  # nothing more is started on the GPU
        res["gpu"].append(json.loads(line[0][7:]))
        print(res["gpu"][-1], flush=True)
    if not a.skip_cpu:
        pts = slam_scene()
        t0 = time.perf_counter()
        ncomp, nacc, npts, top = cpu_clusters(pts)
        res["cpu"].append(dict(step="scene", n=len(pts), ms=(time.perf_counter() - t0) * 1e3, components=ncomp,
                               n_clusters=nacc, clustered_points=npts, largest=[int(s) for s in top], workers=16,
                               cpus=os.cpu_count(), method="cKDTree.query_ball_point + csgraph.connected_components"))
        print(res["cpu"][-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
