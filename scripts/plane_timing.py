#!/usr/bin/env python3
"""Timing of the RANSAC plane segmentation against a dense float32 formulation on the host (not a test, not
bench.py).

    python scripts/plane_timing.py [--out profiles/plane_timing.json] [--skip-cpu] [--skip-gpu]

Steps: lio_segment_plane on the 2 M-point scene of scripts/denoise_timing.py at the reference's parameters
(distance_threshold 0.2, ransac_n 3, num_iterations 1000: post_process/clustering.py:21-28); the clustering of
that scene before and after ground removal (tolerance 0.5, min 10, max 25000: the parameters of DESIGN §4b); the
chain of clustering.py's main block (SOR 20 / 2.0 -> plane -> clusters 0.5 / 10 / 10000), every stage timed.
The CPU comparison scores the same 1000 planes (lio_plane_sample_triples' triples, the contract's float plane
of each) against all points as `pts @ normals.T + d` in float32, chunk by chunk, then |.| < thr and the column
sums, with 16 threads (torch on the CPU when it is importable, else numpy).  It is NOT Open3D's serial loop
over the hypotheses with its early exit; it is the strongest dense formulation available without Open3D, it
counts inliers only (no squared-error sum), and its sums may contract to FMA, so its counts can differ from
the library's in a few hypotheses.  Every GPU step runs in a child process of its own under a time limit
(`timeout`), so that trouble in one ends it; a step that fails ends the run.  Times are host wall times, the
best of three after one warm-up call.
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

PARAMS = dict(distance_threshold=0.2, num_iterations=1000, seed=0)  # post_process/clustering.py:21-28
CLUSTER_4B = dict(tolerance=0.5, min_size=10, max_size=25000)
CHAIN = dict(nb_neighbors=20, std_ratio=2.0, tolerance=0.5, min_size=10, max_size=10000)  # clustering.py:77-118


def cluster_summary(ec, pts):
    ec.extract(pts)
    sizes = np.diff(ec.offsets)
    return dict(n=len(pts), finite=int(ec.stats[0]), components=int(ec.stats[1]), clusters=int(ec.stats[2]),
                clustered_points=int(ec.stats[3]), largest=[int(s) for s in sizes[:5]])


def gpu_step(name):
    import ctypes as C

    from lio_gpu import _capi
    from lio_gpu import filters as FL

    pts = slam_scene()
    n = len(pts)
    seg = FL.PlaneSegmentation()
    thr, k, seed = PARAMS["distance_threshold"], PARAMS["num_iterations"], PARAMS["seed"]
    if name == "once":  # one warm call and one measured call: the profiler's target
        seg.segment_plane(pts, thr, 3, k, seed)
        plane, inl = seg.segment_plane(pts, thr, 3, k, seed)
        return dict(step=name, n=n, n_inliers=len(inl))
    if name == "plane":
        ms, (plane, inl) = best_of(lambda: seg.segment_plane(pts, thr, 3, k, seed))
        # the C call alone into preallocated outputs (the wrapper adds the allocation of its result arrays)
        p4, idx, best, m = np.zeros(4, np.float32), np.empty(n, np.int32), C.c_int64(0), C.c_int64(0)
        refit = np.zeros(4)
        call_ms, _ = best_of(lambda: _capi.check(_capi.lib().lio_segment_plane(
            seg._h, pts.ctypes.data_as(_capi.fp), n, pts.shape[1], thr, 3, k, seed, None, p4.ctypes.data_as(_capi.fp),
            C.byref(best), idx.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(m), None, None, None, None,
            refit.ctypes.data_as(C.POINTER(C.c_double)))))
        return dict(step=name, n=n, ms=ms, c_call_ms=call_ms, bytes_up=pts.nbytes, bytes_down=int(4 * m.value),
                    best_iteration=int(seg.best_iteration), n_inliers=len(inl), plane=[float(v) for v in plane],
                    refit=[float(v) for v in seg.refit], top_count_ties=int((seg.counts == seg.counts.max()).sum()),
                    degenerate=int(seg.degenerate.sum()))
    if name == "ground":  # DESIGN §4b's clustering of the scene, before and after ground removal
        ec = FL.EuclideanClusterExtraction(**CLUSTER_4B)
        before = cluster_summary(ec, pts)
        plane, inl = seg.segment_plane(pts, thr, 3, k, seed)
        after = cluster_summary(ec, pts[seg.mask == 0])
        return dict(step=name, params=CLUSTER_4B, n_ground=len(inl), before=before, after=after)
    if name == "chain":
        sor = FL.StatisticalOutlierRemoval(CHAIN["nb_neighbors"], CHAIN["std_ratio"])
        sor_ms, filtered = best_of(lambda: sor.filter(pts))
        plane_ms, (plane, inl) = best_of(lambda: seg.segment_plane(filtered, thr, 3, k, seed))
        rest = filtered[seg.mask == 0]
        ec = FL.EuclideanClusterExtraction(CHAIN["tolerance"], CHAIN["min_size"], CHAIN["max_size"])
        cl_ms, _ = best_of(lambda: ec.extract(rest))
        whole_ms, out = best_of(lambda: FL.cluster_objects(pts, seed=seed), reps=1)
        return dict(step=name, params=CHAIN, n=n, sor_ms=sor_ms, n_after_sor=len(filtered), plane_ms=plane_ms,
                    n_ground=len(inl), cluster_ms=cl_ms, clusters=cluster_summary(ec, rest), cluster_objects_ms=whole_ms,
                    cluster_objects_clusters=len(out["clusters"]))
    raise ValueError(name)


def contract_planes(pts, k, seed):
    """the K planes of the sampler's triples in the contract's float order (numpy, no device)"""
    import ctypes as C

    from lio_gpu import _capi

    tr = np.zeros((k, 3), np.int32)
    _capi.check(_capi.lib().lio_plane_sample_triples(seed, len(pts), k, tr.ctypes.data_as(C.POINTER(C.c_int32))))
    xyz = pts[:, :3]
    p0, p1, p2 = xyz[tr[:, 0]], xyz[tr[:, 1]], xyz[tr[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    nrm = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                    e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    with np.errstate(all="ignore"):
        nrm = nrm / np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])[:, None]
        d = -((nrm[:, 0] * p0[:, 0] + nrm[:, 1] * p0[:, 1]) + nrm[:, 2] * p0[:, 2])
    return np.nan_to_num(nrm.astype(np.float32)), np.nan_to_num(d.astype(np.float32), nan=np.float32(1e30))


def cpu_counts(pts, nrm, d, thr, threads=16, chunk=32768):
    """inliers per plane: float32 pts @ normals.T + d, |.| < thr, column sums; chunks of points"""
    xyz = np.ascontiguousarray(pts[:, :3])
    try:
        import torch

        torch.set_num_threads(threads)
        X, N, D = torch.from_numpy(xyz), torch.from_numpy(np.ascontiguousarray(nrm.T)), torch.from_numpy(d)
        cnt = torch.zeros(len(d), dtype=torch.int64)
        for i0 in range(0, len(X), chunk):
            cnt += ((X[i0:i0 + chunk] @ N + D).abs_() < thr).sum(0)
        return cnt.numpy(), f"torch {torch.__version__} on the CPU, {threads} threads"
    except ImportError:
        cnt = np.zeros(len(d), np.int64)
        NT = np.ascontiguousarray(nrm.T)
        for i0 in range(0, len(xyz), chunk):
            cnt += (np.abs(xyz[i0:i0 + chunk] @ NT + d) < np.float32(thr)).sum(0)
        return cnt, "numpy (BLAS threads as OMP_NUM_THREADS sets them)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_timing.json"))
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--skip-gpu", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--limit", type=int, default=240, help="time limit of one GPU step [s]")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(gpu_step(a.child)))
        return 0
    res = dict(params=PARAMS, gpu=[], cpu=[])
    for step in () if a.skip_gpu else ("plane", "ground", "chain"):
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
        nrm, d = contract_planes(pts, PARAMS["num_iterations"], PARAMS["seed"])
        cpu_counts(pts[:200_000], nrm, d, PARAMS["distance_threshold"])  # warm-up
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            cnt, how = cpu_counts(pts, nrm, d, PARAMS["distance_threshold"])
            ts.append((time.perf_counter() - t0) * 1e3)
        res["cpu"].append(dict(step="plane", n=len(pts), ms=min(ts), best_count=int(cnt.max()), best_iteration=int(cnt.argmax()),
                               threads=16, cpus=os.cpu_count(), method="float32 pts @ normals.T + d, abs < thr, column sums; " + how,
                               note="counts only (no squared-error sum), not Open3D's serial loop"))
        print(res["cpu"][-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
