#!/usr/bin/env python3
"""Timing of the GPU image undistortion against its numpy restatement (not a test, not bench.py).

    python scripts/undistort_timing.py [--out profiles/undistort_timing.json] [--skip-cpu] [--skip-gpu]

The workload: one 4096 x 2464 x 3 frame (the rig's: post_process/undistort_image.py) with the rig's 8-parameter
calibration (K8 / DIST8 of tests/colorize_ref.py), rectified to the same intrinsics — the scripts' call.  Reported:
the host wall time of set_camera (the map kernel, with the first call's allocation apart); per frame the median over
the frames of the host wall time of one call and of the device times of its stages from stream events (the upload
with its pinned staging copy, the gather kernel, the download); the kernel's bytes per second against its
algorithmic bytes (per output pixel 3 read, 3 written, 8 of map) and that as a fraction of the HBM peak.  The one-
channel frame is timed the same way.  The CPU baseline is the numpy restatement of one frame (tests/undistort_ref.py,
one thread) on the same host, map and gather apart; its output is compared with the GPU's (sha1).  There is no OpenCV
on these machines, so no cv2.undistort timing.  The GPU part runs in one child process under a time limit
(`timeout`), so that trouble in it ends it.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fast-lio-sam_gps_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import undistort_ref as UR  # noqa: E402

WIDTH, HEIGHT = 4096, 2464
FRAMES = 12
HBM_PEAK = 8.0e12  # bytes per second (the MI355X's specification)


def scene(channels):
    cam = UR.Cam(*UR.K8, WIDTH, HEIGHT, UR.DIST8)
    shape = (HEIGHT, WIDTH, 3) if channels == 3 else (HEIGHT, WIDTH)
    img = np.random.default_rng(2025).integers(0, 256, shape, dtype=np.uint8)
    return cam, img


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a, np.uint8).tobytes()).hexdigest()


def gpu_part():
    from lio_gpu import camera as CAM

    out = []
    for channels in (3, 1):
        cam, img = scene(channels)
        model = CAM.CameraModel(cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, cam.dist)
        ud = CAM.Undistorter()
        set_ms = []
        for _ in range(4):  # the first call allocates the map
            t0 = time.perf_counter()
            ud.set_camera(model, None, channels=channels)
            set_ms.append((time.perf_counter() - t0) * 1e3)
        res = np.empty_like(img)
        t0 = time.perf_counter()
        ud(img, out=res)
        first_wall = (time.perf_counter() - t0) * 1e3
        first_digest = digest(res)
        rows = []
        for _ in range(FRAMES):
            t0 = time.perf_counter()
            ud(img, out=res)
            rows.append(dict(ud.timing(), wall_ms=(time.perf_counter() - t0) * 1e3))
        med = {k: statistics.median(r[k] for r in rows) for k in ("wall_ms", "upload_ms", "kernel_ms", "download_ms")}
        pixels = cam.width * cam.height
        algo = pixels * (2 * channels + 8)
        rate = algo / (med["kernel_ms"] * 1e-3)
        out.append(dict(channels=channels, set_camera_first_ms=set_ms[0], set_camera_ms=statistics.median(set_ms[1:]),
                        first_frame_wall_ms=first_wall, per_frame_median=med, frames=rows, kernel_algorithmic_bytes=algo,
                        kernel_bytes_per_s=rate, kernel_fraction_of_hbm_peak=rate / HBM_PEAK,
                        copies_fraction_of_device_time=(med["upload_ms"] + med["download_ms"]) /
                        (med["upload_ms"] + med["kernel_ms"] + med["download_ms"]),
                        same_bits_on_repeat=digest(res) == first_digest, digest=first_digest))
        ud.close()
    return dict(image=[WIDTH, HEIGHT], frame_mb=WIDTH * HEIGHT * 3 / 1e6, frames=FRAMES, hbm_peak_bytes_per_s=HBM_PEAK, runs=out)


def cpu_part():
    out = []
    for channels in (3, 1):
        cam, img = scene(channels)
        t0 = time.perf_counter()
        m = UR.undistort_map(cam)
        map_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        res = UR.remap(img, m, cam)
        remap_ms = (time.perf_counter() - t0) * 1e3
        out.append(dict(channels=channels, map_ms=map_ms, remap_ms=remap_ms, digest=digest(res), classes=UR.classes(m, cam),
                        method="tests/undistort_ref.py undistort_map + remap (numpy, one thread)", cpus=os.cpu_count()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort_timing.json"))
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--skip-gpu", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--limit", type=int, default=240, help="time limit of the GPU part [s]")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(gpu_part()))
        return 0
    res = dict(gpu=None, cpu=[])
    if os.path.exists(a.out):  # a run with --skip-gpu or --skip-cpu keeps the other half of an earlier run
        with open(a.out) as f:
            old = json.load(f)
        res["gpu"], res["cpu"] = old.get("gpu"), old.get("cpu", [])
    if not a.skip_gpu:
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child"],
                           capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"GPU part failed (exit {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            return 1
        res["gpu"] = json.loads(line[0][7:])
        for c in res["gpu"]["runs"]:
            print(c["channels"], "channel(s)", c["per_frame_median"], "set_camera", c["set_camera_ms"],
                  "kernel B/s", c["kernel_bytes_per_s"], flush=True)
    if not a.skip_cpu:
        res["cpu"] = cpu_part()
        for c in res["cpu"]:
            print(c["channels"], "channel(s) numpy: map", c["map_ms"], "remap", c["remap_ms"], flush=True)
    if res["gpu"] and res["cpu"]:
        g = {c["channels"]: c["digest"] for c in res["gpu"]["runs"]}
        res["cpu_equals_gpu_bit_for_bit"] = {str(c["channels"]): g.get(c["channels"]) == c["digest"] for c in res["cpu"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
