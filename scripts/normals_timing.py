#!/usr/bin/env python3
"""Timing of lio_estimate_normals (not a test, not bench.py).

    python scripts/normals_timing.py [--out profiles/normals_timing.json] [--skip-cpu] [--skip-gpu] [--no-kernels]

Cloud (lio_gpu.synth): the 2 000 000-point surface sample of the street scene the other timing scripts use, 3
floats per point.  Three settings: k = 20; radius 0.5; the hybrid search (radius 0.5, k 30).  Per setting:
  whole_ms     NormalEstimation.compute: upload, grid build, search and eigen-step, the counts, download of the
               normals, curvature and counts
  sor_ms       lio_sor_filter at mean_k = k - 1 (so k candidates per query, as here) in the same process on the same
               cloud: the parent's nearest equivalent of the search (the radius setting has no k: it is compared
               with mean_k = 19 too, and is another search)
  kernels      per kernel the calls, average and total microseconds over TWO calls (a warm one, then one more) from a
               run of those alone under `rocprofv3 --kernel-trace --stats` (a child process of its own)
  stats        the six counts of the call
The CPU figure is scipy's cKDTree (query with workers=16 / query_ball_point with workers=16) plus numpy's batched
linalg.eigh on float64 covariances, on the same host: another formulation (no integer moments, no tie rule).
PCL and Open3D are not installed here: neither was timed.
Every GPU step runs in a child process of its own under a time limit (`timeout`), so that trouble in one ends it;
a step that fails ends the run.  Times are host wall times around calls that end in a device synchronise, the best
of five after one warm-up call of the same shape.
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fast-lio-sam_gps_amd")]

import numpy as np  # noqa: E402

SETTINGS = {"k20": dict(k=20, radius=0.0), "r0.5": dict(k=0, radius=0.5), "hybrid": dict(k=30, radius=0.5)}
N = 2_000_000


def cloud(n=N):
    from lio_gpu import synth

    return np.ascontiguousarray(synth.sample_surface(synth.make_scene(), n)[:, :3], dtype=np.float32)


def best_of(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), r


def gpu_step(name, n):
    from lio_gpu import filters as FL

    once = name.startswith("once-")
    s = SETTINGS[name[5:] if once else name]
    pts = cloud(n)
    ne = FL.NormalEstimation(s["k"], s["radius"])
    if once:  # one warm call and one measured call: the profiler's target
        ne.compute(pts)
        ne.compute(pts)
        return dict(step=name, n=len(pts))
    whole_ms, _ = best_of(lambda: ne.compute(pts))
    sor = FL.StatisticalOutlierRemoval((s["k"] or 20) - 1, 1.0)
    sor_ms, _ = best_of(lambda: sor.filter(pts))
    return dict(step=name, n=len(pts), k=s["k"], radius=s["radius"], whole_ms=whole_ms, sor_mean_k=sor.mean_k, sor_ms=sor_ms,
                ratio_to_sor=whole_ms / sor_ms, stats=[int(v) for v in ne.stats], mean_neighbours=float(ne.stats[5]) / max(int(ne.stats[0]), 1),
                bytes_up=pts.nbytes, bytes_down=20 * len(pts))


def kernel_stats(name, n, limit):
    """per-kernel rows of a child that makes the call twice (a warm call, then one more) under rocprofv3: calls and
    totals are over the two, the averages per launch"""
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run",
                            "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--child", "once-" + name,
                            "--n", str(n)], capture_output=True, text=True)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return None, r
        rows = []
        for x in csv.DictReader(open(files[0])):
            m = re.search(r"(\w+_kernel)", x["Name"])
            short = m.group(1) if m else ("rocprim:" + (re.search(r"detail::(\w+)", x["Name"]) or [0, x["Name"][:40]])[1])
            rows.append(dict(kernel=short, calls=int(x["Calls"]), avg_us=float(x["AverageNs"]) / 1e3,
                             total_us=float(x["TotalDurationNs"]) / 1e3))
        return rows, r


def cpu_step(name, n, threads=16):
    from scipy.spatial import cKDTree

    s = SETTINGS[name]
    pts = cloud(n).astype(np.float64)
    t0 = time.perf_counter()
    tree = cKDTree(pts)
    if s["k"]:  # a fixed number of columns; the hybrid search leaves the columns beyond the radius empty
        kw = dict(distance_upper_bound=s["radius"]) if s["radius"] > 0 else {}
        _, nb = tree.query(pts, s["k"], workers=threads, **kw)
        valid = nb < len(pts)
        o = np.where(valid[..., None], pts[np.minimum(nb, len(pts) - 1)] - pts[:, None, :], 0.0)
        m = valid.sum(1)
        S = o.sum(1)
        SS = np.einsum("nka,nkb->nab", o, o)
    else:  # neighbourhoods of varying size: the sums over the pair list, 50 000 queries at a time
        m, S, SS = np.zeros(len(pts), np.int64), np.zeros((len(pts), 3)), np.zeros((len(pts), 3, 3))
        for c0 in range(0, len(pts), 50_000):
            q = pts[c0:c0 + 50_000]
            lists = tree.query_ball_point(q, s["radius"], workers=threads, return_sorted=False)
            mc = np.fromiter((len(v) for v in lists), np.int64, len(lists))
            cols = np.concatenate([np.asarray(v, np.int64) for v in lists])
            o = pts[cols] - np.repeat(q, mc, axis=0)
            first = np.concatenate([[0], np.cumsum(mc)])[:-1]  # every query finds itself: no empty row
            m[c0:c0 + len(q)] = mc
            S[c0:c0 + len(q)] = np.add.reduceat(o, first, axis=0)
            SS[c0:c0 + len(q)] = np.add.reduceat(o[:, :, None] * o[:, None, :], first, axis=0)
    search_ms = (time.perf_counter() - t0) * 1e3
    dm = np.maximum(m, 1)[:, None, None]
    M = SS - S[:, :, None] * S[:, None, :] / dm
    w, V = np.linalg.eigh(M)
    normals = V[:, :, 0]
    total_ms = (time.perf_counter() - t0) * 1e3
    import scipy

    return dict(step=name, n=len(pts), ms=total_ms, tree_search_moments_ms=search_ms, eigh_ms=total_ms - search_ms,
                threads=threads, cpus=os.cpu_count(), finite_normals=int(np.isfinite(normals).all(1).sum()),
                method=f"scipy {scipy.__version__} cKDTree (workers={threads}) + numpy {np.__version__} linalg.eigh, float64, "
                       "one run")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_timing.json"))
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--skip-gpu", action="store_true")
    ap.add_argument("--no-kernels", action="store_true", help="no rocprofv3 runs")
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--limit", type=int, default=240, help="time limit of one GPU step [s]")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(gpu_step(a.child, a.n)))
        return 0
    res = dict(n=a.n, settings=SETTINGS, gpu=[], kernels={}, cpu=[],
               note="PCL and Open3D are not installed on this host: neither was timed")
    for step in () if a.skip_gpu else SETTINGS:
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", step,
                            "--n", str(a.n)], capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{step}: failed (exit {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            return 1  # nothing more is started on the GPU
        res["gpu"].append(json.loads(line[0][7:]))
        print(res["gpu"][-1], flush=True)
        if not a.no_kernels:
            rows, r = kernel_stats(step, a.n, a.limit)
            if rows is None:
                print(f"{step}: the kernel trace failed (exit {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                return 1
            res["kernels"][step] = rows
            print(rows, flush=True)
    if not a.skip_cpu:
        for step in SETTINGS:
            res["cpu"].append(cpu_step(step, a.n))
            print(res["cpu"][-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
