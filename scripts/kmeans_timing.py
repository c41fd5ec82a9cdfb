#!/usr/bin/env python3
"""Timing of lio_kmeans against scikit-learn's KMeans on the host (not a test, not bench.py).

    python scripts/kmeans_timing.py [--out profiles/kmeans_timing.json] [--skip-cpu] [--skip-gpu]

Clouds (lio_gpu.synth): a 131 072-point scan (ouster64 pattern in the street scene, 3 floats per point) and a
2 000 000-point surface sample of that scene.  Per cloud and K in (5, 64), at the reference call's parameters
(post_process/lidar_projection/src/lidar_projection.cpp:82-92: TermCriteria(EPS + MAX_ITER, 100, 0.1), 3
attempts, k-means++ centres):
  whole_ms        KMeans.fit: upload, counting pass, 3 x (seeding, Lloyd, compactness), boxes, download
  iterations      per attempt, and the assign passes they ran (it - 1 each)
  seeding_ms      one attempt stopped after its first iteration, seeded, minus the same from given centres
  lloyd_iter_ms   one attempt from given centres (attempt 0's seeds), run to its stop, minus the same stopped after
                  its first iteration, over the further assign passes: one assign-and-accumulate launch, the K x 4
                  integers read back and the host's centre arithmetic
  assign_gbs      n x stride x 4 bytes over lloyd_iter_ms: the algorithmic bytes of an iteration over its WALL time
                  (launch, read-back and wait included), not the kernel's own rate
The CPU figure is sklearn.cluster.KMeans(5, init="k-means++", n_init=3, max_iter=100, algorithm="lloyd") on the
same host with 16 threads: SCIKIT-LEARN, NOT OpenCV — another seeding (one trial set per centre of 2 + log K
candidates from numpy's generator) and another stop rule (tol relative to the variance), in double precision.
Every GPU step runs in a child process of its own under a time limit (`timeout`), so that trouble in one ends it;
a step that fails ends the run.  Times are host wall times around calls that end in a device synchronise, the
best of five after one warm-up call of the same shape.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fast-lio-sam_gps_amd")]

import numpy as np  # noqa: E402

PARAMS = dict(max_iter=100, eps=0.1, attempts=3, seed=0)  # lidar_projection.cpp:82-92
KS = (5, 64)
CLOUDS = ("scan131k", "map2m")


def cloud(name):
    from lio_gpu import synth

    scene = synth.make_scene()
    if name == "scan131k":
        return synth.make_scan(scene, 131072, "ouster64", (0.0, 0.0, 1.0)).body
    return np.ascontiguousarray(synth.sample_surface(scene, 2_000_000)[:, :3], dtype=np.float32)


def best_of(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), r


def gpu_step(name):
    from lio_gpu import filters as FL

    which, k = name.split(":")
    k = int(k)
    once = which.startswith("once-")
    pts = cloud(which[5:] if once else which)
    n, stride = pts.shape
    km = FL.KMeans(k, PARAMS["max_iter"], PARAMS["eps"], PARAMS["attempts"], PARAMS["seed"])
    if once:  # "once-map2m:5": one warm call and one measured call, the profiler's target
        km.fit(pts)
        km.fit(pts)
        return dict(step=name, n=n)
    whole_ms, _ = best_of(lambda: km.fit(pts))
    res = dict(step=name, n=n, stride=stride, K=k, whole_ms=whole_ms, iterations=[int(v) for v in km.attempt_iters],
               assign_passes=int((km.attempt_iters - 1).sum()), best_attempt=km.best_attempt, inertia=km.inertia_,
               counts=[int(v) for v in km.counts], repairs=int(km.stats[3]), bytes_up=pts.nbytes, bytes_down=4 * n)
    init = pts[km.seeds[:1], :3].copy()  # attempt 0's centres
    km.attempts = 1
    km.max_iter = 1
    seeded_ms, _ = best_of(lambda: km.fit(pts))
    first_ms, _ = best_of(lambda: km.fit(pts, init))
    km.max_iter = PARAMS["max_iter"]
    full_ms, _ = best_of(lambda: km.fit(pts, init))
    passes = int(km.attempt_iters[0]) - 1
    res.update(seeding_ms=seeded_ms - first_ms, one_attempt_ms=full_ms, one_attempt_passes=passes,
               one_pass_call_ms=first_ms)
    if passes > 1:
        it_ms = (full_ms - first_ms) / (passes - 1)
        res.update(lloyd_iter_ms=it_ms, assign_gbs=n * stride * 4 / (it_ms * 1e-3) / 1e9)
    return res


def cpu_step(which, threads=16):
    from sklearn.cluster import KMeans
    from threadpoolctl import threadpool_limits

    pts = cloud(which).astype(np.float64)
    with threadpool_limits(limits=threads):
        KMeans(5, init="k-means++", n_init=1, max_iter=5, algorithm="lloyd", random_state=0).fit(pts[:100_000])  # warm-up
        ts = []
        for _ in range(2):
            t0 = time.perf_counter()
            km = KMeans(5, init="k-means++", n_init=3, max_iter=100, algorithm="lloyd", random_state=0).fit(pts)
            ts.append((time.perf_counter() - t0) * 1e3)
    import sklearn

    return dict(step=which + ":5", n=len(pts), ms=min(ts), n_iter_of_best=int(km.n_iter_), inertia=float(km.inertia_),
                threads=threads, cpus=os.cpu_count(),
                method=f"scikit-learn {sklearn.__version__} KMeans(5, init='k-means++', n_init=3, max_iter=100, "
                       "algorithm='lloyd'), float64",
                note="scikit-learn, not OpenCV: another seeding and another stop rule (tol = 1e-4 of the variance)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_timing.json"))
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--skip-gpu", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--limit", type=int, default=240, help="time limit of one GPU step [s]")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(gpu_step(a.child)))
        return 0
    res = dict(params=PARAMS, gpu=[], cpu=[])
    for step in () if a.skip_gpu else [f"{c}:{k}" for c in CLOUDS for k in KS]:
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", step],
                           capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{step}: failed (exit {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            return 1  # nothing more is started on the GPU
        res["gpu"].append(json.loads(line[0][7:]))
        print(res["gpu"][-1], flush=True)
    if not a.skip_cpu:
        for which in CLOUDS:
            res["cpu"].append(cpu_step(which))
            print(res["cpu"][-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
