#!/usr/bin/env python3
"""Timing of the denoise entry points against scipy's cKDTree on the host (not a test, not bench.py).

    python scripts/denoise_timing.py [--out profiles/denoise_timing.json] [--skip-cpu]

Steps: lio_sor_filter at 1 M points with mean_k 50 and 200, lio_denoise_slam_map on a 2 M-point scene, and
the same work with scipy.spatial.cKDTree (workers=16) as the only CPU reference available here.  Every GPU
step runs in a child process of its own under a time limit (`timeout`), so that trouble in one ends it; a
step that fails ends the run.  Times are host wall times of the whole call (upload, kernels, the host
threshold loop, download), the best of three after one warm-up call.
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

CFG = dict(seed_thres=2800.0, cluster_seed_radius=0.1, denoise_radius=0.5, noise_thres=2700.0, mean_k=200,
           stddev_mul=0.2)  # the shipped configuration


def sor_cloud(n=1_000_000, seed=0):
    """a street-like slab: ground, two walls, 1 % far outliers"""
    rng = np.random.default_rng(seed)
    k = n // 100
    g = np.column_stack([rng.uniform(-60, 60, n - 3 * k), rng.uniform(-15, 15, n - 3 * k), rng.normal(0, 0.03, n - 3 * k)])
    w = np.column_stack([rng.uniform(-60, 60, 2 * k), np.repeat([-15.0, 15.0], k) + rng.normal(0, 0.03, 2 * k),
                         rng.uniform(0, 6, 2 * k)])
    o = rng.uniform(-60, 60, (k, 3))
    p = np.concatenate([g, w, o])
    return np.column_stack([p, rng.uniform(0, 255, len(p))]).astype(np.float32)


def slam_scene(n=2_000_000, seed=1, boards=40):
    """ground + walls at intensity 500-2000, `boards` 1 m signboards above 2800 (0.5 % of the points each way)
    with a 2000-2700 halo, 1 % of the points at intensity 0"""
    rng = np.random.default_rng(seed)
    nb = n // 400
    base = sor_cloud(n - 2 * boards * (nb // boards) - n // 100, seed)[:, :3]
    parts = [np.column_stack([base, rng.uniform(500, 2000, len(base))])]
    per = nb // boards
    for b in range(boards):
        cx, cy = rng.uniform(-55, 55), rng.uniform(-14, 14)
        parts.append(np.column_stack([cx + rng.uniform(-0.5, 0.5, per), cy + rng.normal(0, 0.005, per),
                                      rng.uniform(1, 2, per), rng.uniform(2801, 3500, per)]))
        parts.append(np.column_stack([cx + rng.uniform(-0.7, 0.7, per), cy + rng.normal(0, 0.06, per),
                                      rng.uniform(0.8, 2.2, per), rng.uniform(2000, 2700, per)]))
    nz = n // 100
    parts.append(np.column_stack([rng.uniform(-60, 60, nz), rng.uniform(-15, 15, nz), rng.uniform(0, 3, nz), np.zeros(nz)]))
    pts = np.concatenate(parts).astype(np.float32)
    return pts[rng.permutation(len(pts))]


def best_of(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), r


def gpu_step(name):
    from lio_gpu import filters as FL

    if name.startswith("sor"):
        k = int(name[3:])
        pts = sor_cloud()
        f = FL.StatisticalOutlierRemoval(k, 1.0)
        ms, out = best_of(lambda: f.filter(pts))
        return dict(step=name, n=len(pts), mean_k=k, ms=ms, kept=len(out), threshold=float(f.stats[2]))
    pts = slam_scene()
    h = FL._Handle()
    ms, (out, counts) = best_of(lambda: FL.denoise_slam_map(pts, handle=h, **CFG))
    # the parts of that figure: the C call alone (upload, kernels, five counts read back, download) into a
    # preallocated output, and the wrapper's allocation + copy of the result
    import ctypes as C

    from lio_gpu import _capi

    buf, cnt, m = np.empty_like(pts), np.zeros(5, np.int64), C.c_int64(0)
    p = _capi.DenoiseParams(CFG["seed_thres"], CFG["cluster_seed_radius"], CFG["denoise_radius"], CFG["noise_thres"],
                            CFG["mean_k"], CFG["stddev_mul"])
    fp = C.POINTER(C.c_float)
    call_ms, _ = best_of(lambda: _capi.check(_capi.lib().lio_denoise_slam_map(
        h._h, pts.ctypes.data_as(fp), len(pts), C.byref(p), buf.ctypes.data_as(fp), C.byref(m),
        cnt.ctypes.data_as(C.POINTER(C.c_int64)))))
    copy_ms, _ = best_of(lambda: np.empty_like(pts)[: m.value].copy())
    return dict(step=name, n=len(pts), ms=ms, c_call_ms=call_ms, wrapper_alloc_copy_ms=copy_ms, bytes_up=pts.nbytes,
                bytes_down=int(m.value) * 16, n_out=len(out), counts=[int(c) for c in counts])


def cpu_sor(pts, k, mul, workers=16):
    from scipy.spatial import cKDTree

    xyz = pts[:, :3].astype(np.float64)
    d, _ = cKDTree(xyz).query(xyz, k + 1, workers=workers)
    m = d[:, 1:].mean(1)
    return pts[m <= m.mean() + mul * m.std(ddof=1)]


def cpu_denoise(pts, workers=16):
    from scipy.spatial import cKDTree

    inten = pts[:, 3]
    seeds = pts[inten > CFG["seed_thres"], :3].astype(np.float64)
    st = cKDTree(seeds)
    d, _ = st.query(pts[:, :3].astype(np.float64), 1, distance_upper_bound=CFG["cluster_seed_radius"], workers=workers)
    seg = pts[(inten != 0) & np.isfinite(d)]
    rem = pts[(inten != 0) & ~np.isfinite(d)]
    sor = cpu_sor(seg, CFG["mean_k"], CFG["stddev_mul"], workers)
    d, _ = st.query(sor[:, :3].astype(np.float64), 1, distance_upper_bound=CFG["denoise_radius"], workers=workers)
    den = sor[~((sor[:, 3] < CFG["noise_thres"]) & np.isfinite(d))]
    return np.concatenate([den, rem])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_timing.json"))
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--limit", type=int, default=240, help="time limit of one GPU step [s]")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(gpu_step(a.child)))
        return 0
    res = dict(gpu=[], cpu=[])
    for step in ("sor50", "sor200", "slam"):
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", step],
                           capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{step}: failed (exit {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            return 1  # nothing more is started on the GPU
        res["gpu"].append(json.loads(line[0][7:]))
        print(res["gpu"][-1], flush=True)
    if not a.skip_cpu:
        pts = sor_cloud()
        for k in (50, 200):
            t0 = time.perf_counter()
            out = cpu_sor(pts, k, 1.0)
            res["cpu"].append(dict(step=f"sor{k}", n=len(pts), ms=(time.perf_counter() - t0) * 1e3, kept=len(out), workers=16))
            print(res["cpu"][-1], flush=True)
        pts = slam_scene()
        t0 = time.perf_counter()
        out = cpu_denoise(pts)
        res["cpu"].append(dict(step="slam", n=len(pts), ms=(time.perf_counter() - t0) * 1e3, n_out=len(out), workers=16))
        print(res["cpu"][-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
