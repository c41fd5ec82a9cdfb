#!/usr/bin/env python3
"""Timing of the GPU GPS-to-SLAM alignment against a CPU k-d tree formulation (not a test, not bench.py).

    python scripts/gps_align_timing.py [--out profiles/gps_align_timing.json] [--skip-cpu] [--skip-gpu]

The step: lio_gps_align at the reference's defaults (50 iterations, tolerance 1e-4:
post_process/align_slam_gps_icp.py:81) on two scenes at national-grid offsets with 0.4 m of GPS noise — 36 000
poses against 36 000 fixes (one hour at 10 Hz with keyframe_threshold 0) and 131 072 against 131 072 — the whole
Python call and the C call alone into preallocated outputs.  The CPU yardstick is the numpy restatement of the
contract (tests/gps_align_ref.py) with its nearest-neighbour step replaced by scipy.spatial.cKDTree in double with
16 workers, its two nearest candidates re-ranked by the contract's (d2, index) rule; the result says whether its
iteration count and final indices equal the GPU's.  The reference's own dense formulation is not run: at 36 000 x
36 000 it needs a 10 GB distance matrix and a 20 GB intermediate per iteration.  Each GPU step runs in a child
process of its own under a time limit (`timeout`), so that trouble in it ends it; a step that fails ends the run.
Times are host wall times of the whole call (upload, kernels, the host's scalar steps, download), the best of
three after one warm-up call.

    rocprofv3 --kernel-trace --stats -- python scripts/gps_align_timing.py --child 36000

gives the per-kernel table of that step.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fast-lio-sam_gps_amd"), os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import gps_align_ref as GR  # noqa: E402
from denoise_timing import best_of  # noqa: E402

PARAMS = dict(max_iterations=50, tolerance=1e-4)  # align_slam_gps_icp.py:81
SCENES = {"36000": (36000, 36000), "131072": (131072, 131072)}


def scene(name):
    n, m = SCENES[name]
    return GR.scene(n, m, seed=n % 1000, noise=0.4)


def digest(nn, out):
    return hashlib.sha1(np.ascontiguousarray(nn, np.int32).tobytes() + np.ascontiguousarray(out, np.float64).tobytes()).hexdigest()


def gpu_step(name):
    import ctypes as C

    from lio_gpu import _capi
    from lio_gpu import georef as G

    gps, slam = scene(name)
    n, m = len(slam), len(gps)
    al = G.GpsAligner(**PARAMS)
    ms, r = best_of(lambda: al.align(gps, slam))
    dp = C.POINTER(C.c_double)
    aligned, nn, out = np.empty((n, 2)), np.empty(n, np.int32), np.zeros(_capi.LIO_GPSALIGN_LEN)
    call_ms, _ = best_of(lambda: _capi.check(_capi.lib().lio_gps_align(
        al._h, gps.ctypes.data_as(dp), m, slam.ctypes.data_as(dp), n, PARAMS["max_iterations"], PARAMS["tolerance"],
        aligned.ctypes.data_as(dp), nn.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(dp))))
    iters = int(out[_capi.GPSALIGN_ITERATIONS])
    return dict(step=name, n=n, m=m, ms=ms, c_call_ms=call_ms, iterations=iters, converged=bool(out[_capi.GPSALIGN_CONVERGED]),
                mean_error=float(out[_capi.GPSALIGN_MEAN_ERROR]), ms_per_iteration=call_ms / iters,
                pair_tests_per_iteration=n * m, total_scale=r.total.scale, digest=digest(nn, out))


def kdtree_nearest(workers):
    from scipy.spatial import cKDTree

    def nearest(S, D):
        tree = cKDTree(D)
        _, k = tree.query(S, k=min(2, len(D)), workers=workers)
        k = k.reshape(len(S), -1)
        dx, dy = S[:, 0][:, None] - D[k, 0], S[:, 1][:, None] - D[k, 1]
        d2 = dx * dx + dy * dy  # the contract's d2 of both candidates, ranked by (d2, index)
        if k.shape[1] == 2:
            second = (d2[:, 1] < d2[:, 0]) | ((d2[:, 1] == d2[:, 0]) & (k[:, 1] < k[:, 0]))
            pick = second.astype(np.int64)
        else:
            pick = np.zeros(len(S), np.int64)
        rows = np.arange(len(S))
        return k[rows, pick], d2[rows, pick]

    return nearest


def cpu_step(name, workers=16):
    gps, slam = scene(name)
    fn = kdtree_nearest(workers)
    t0 = time.perf_counter()
    r = GR.gps_align(gps, slam, PARAMS["max_iterations"], PARAMS["tolerance"], nearest_fn=fn)
    ms = (time.perf_counter() - t0) * 1e3
    return dict(step=name, n=len(slam), m=len(gps), ms=ms, iterations=r.iterations, converged=bool(r.converged),
                mean_error=r.mean_error, workers=workers, cpus=os.cpu_count(), digest=digest(r.nn, r.out),
                method=f"tests/gps_align_ref.py with scipy.spatial.cKDTree.query(k=2, workers={workers}) as the nearest-neighbour step",
                reference_dense="not run: a 36000 x 36000 float64 distance matrix is 10 GB and its N x M x 2 intermediate 20 GB, "
                                "per iteration")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gps_align_timing.json"))
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--skip-gpu", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--limit", type=int, default=240, help="time limit of one GPU step [s]")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(gpu_step(a.child)))
        return 0
    res = dict(params=PARAMS, gpu=[], cpu=[])
    if os.path.exists(a.out):  # a run with --skip-gpu or --skip-cpu keeps the other half of an earlier run
        with open(a.out) as f:
            old = json.load(f)
        res["gpu"], res["cpu"] = old.get("gpu", []), old.get("cpu", [])
    if not a.skip_gpu:
        res["gpu"] = []
        for name in SCENES:
            r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", name],
                               capture_output=True, text=True)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                print(f"{name}: failed (exit {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                return 1  # nothing more is started on the GPU
            res["gpu"].append(json.loads(line[0][7:]))
            print(res["gpu"][-1], flush=True)
    if not a.skip_cpu:
        res["cpu"] = []
        for name in SCENES:
            res["cpu"].append(cpu_step(name))
            print(res["cpu"][-1], flush=True)
    same = {g["step"]: g["digest"] == c["digest"] for g in res["gpu"] for c in res["cpu"] if g["step"] == c["step"]}
    res["cpu_equals_gpu_bit_for_bit"] = same
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
