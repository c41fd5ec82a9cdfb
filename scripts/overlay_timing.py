#!/usr/bin/env python3
"""Timing of the GPU point overlay against its numpy restatement (not a test, not bench.py).

    python scripts/overlay_timing.py [--out profiles/overlay_timing.json] [--skip-cpu] [--skip-gpu] [--ab-lib PATH]

The workload is that of scripts/colorize_timing.py: the 2 000 000-point street scene and the 4096 x 2464 x 3 frame
over keyframes two metres apart.  Per radius in 0, 3, 7, 15 and per order, the median over the warm frames of the
host wall time of lio_overlay_draw and of the device times of its stages from stream events (upload with its pinned
staging copy, fill, stamp, compose, download).  In the same run: lio_overlay_draw_undistorted against
lio_undistorter_run + lio_overlay_draw on the rig's 8-parameter camera (alternating, frame by frame), and the
colorizer's splat at radius 3, the nearest existing kernel (49 pixels per point and 32-bit atomics against 29 and
64-bit here).  The CPU baseline is the numpy restatement of one frame (tests/overlay_ref.py) on the same host; the
frame's owner image, image and n_drawn are compared with the GPU's (sha1).
--ab-lib: another build of the library (loaded through LIO_GPU_LIB), e.g. one whose lio_overlay.hip was compiled
with -DLIO_OV_READ_FIRST=0; the stamp times of both builds are then taken in alternating child processes.
Each GPU part runs in a child process under a time limit (`timeout`), so that trouble in it ends it.
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
sys.path[:0] = [os.path.join(ROOT, "fast-lio-sam_gps_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

import numpy as np  # noqa: E402

import colorize_ref as CR  # noqa: E402
import overlay_ref as OR  # noqa: E402
from colorize_timing import scene  # noqa: E402

RADII = (0, 3, 7, 15)
ORDERS = (("draw", OR.DRAW_ORDER), ("nearest", OR.NEAREST))
STAGES = ("upload_ms", "fill_ms", "stamp_ms", "compose_ms", "download_ms")


def digest(out, owner, n_drawn):
    h = hashlib.sha1()
    h.update(np.ascontiguousarray(owner, np.int32).tobytes())
    h.update(np.ascontiguousarray(out, np.uint8).tobytes())
    h.update(str(int(n_drawn)).encode())
    return h.hexdigest()


def median_rows(rows, keys):
    return {k: statistics.median(r[k] for r in rows) for k in keys}


def stamp_part():
    """the A/B's child: the stamp stage alone, every radius and order"""
    from lio_gpu import camera as CAM

    pts, cam, img, poses = scene()
    model = CAM.CameraModel(cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height)
    out = {}
    for r in RADII:
        for name, _ in ORDERS:
            ov = CAM.PointOverlay(r, name)
            ov.set_cloud(pts)
            buf = np.empty_like(img)
            rows = []
            for rep in range(2):  # the second pass over the same frames is the warm one
                rows = []
                for Rt in poses:
                    ov.draw(model, Rt, img, out=buf)
                    rows.append(ov.timing())
            out[f"r={r} {name}"] = statistics.median(x["stamp_ms"] for x in rows)
            ov.close()
    return out


def gpu_part():
    from lio_gpu import camera as CAM

    pts, cam, img, poses = scene()
    model = CAM.CameraModel(cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height)
    configs = []
    buf = np.empty_like(img)
    for r in RADII:
        for name, _ in ORDERS:
            ov = CAM.PointOverlay(r, name)
            t0 = time.perf_counter()
            ov.set_cloud(pts)
            set_cloud_ms = (time.perf_counter() - t0) * 1e3
            out, owner = ov.draw(model, poses[0], img, owner=True)
            first = digest(out, owner, ov.n_drawn)
            owned = int(np.count_nonzero(owner >= 0))
            rows = []
            for rep in range(2):  # the second pass over the same frames is the warm one
                rows = []
                for Rt in poses:
                    t0 = time.perf_counter()
                    ov.draw(model, Rt, img, out=buf)
                    wall = (time.perf_counter() - t0) * 1e3
                    rows.append(dict(ov.timing(), wall_ms=wall, n_drawn=ov.n_drawn))
            configs.append(dict(config=f"r={r} {name}", radius=r, order=name, set_cloud_ms=set_cloud_ms,
                                per_frame_median=median_rows(rows, ("wall_ms",) + STAGES), frames=rows,
                                first_frame_digest=first, first_frame_owned_pixels=owned))
            ov.close()

    # the colorizer's splat at radius 3 on the same cloud, frames and image
    cz = CAM.Colorizer(occlusion=True, splat_radius=3, depth_rel=0.02, depth_abs=0.05)
    cz.set_cloud(pts)
    rows = []
    for rep in range(2):
        cz.reset()
        rows = []
        for Rt in poses:
            cz.add_frame(model, Rt, img)
            rows.append(cz.timing())
    splat = median_rows(rows, ("upload_ms", "fill_ms", "splat_ms", "resolve_ms"))
    cz.close()

    # the chained call against the two calls, on the rig's 8-parameter camera, alternating frame by frame
    raw_cam = CAM.CameraModel(*CR.K8, cam.width, cam.height, CR.DIST8)
    rect = raw_cam.rectified()
    ud = CAM.Undistorter()
    ud.set_camera(raw_cam)
    ov = CAM.PointOverlay(3, "draw")
    ov.set_cloud(pts)
    rectified = np.empty_like(img)
    chained_rows, two_rows, equal = [], [], True
    for rep in range(2):
        chained_rows, two_rows = [], []
        for Rt in poses:
            t0 = time.perf_counter()
            ud(img, out=rectified)
            mid = time.perf_counter()
            two = ov.draw(rect, Rt, rectified)
            t1 = time.perf_counter()
            two_rows.append(dict(wall_ms=(t1 - t0) * 1e3, undistort_wall_ms=(mid - t0) * 1e3, draw_wall_ms=(t1 - mid) * 1e3))
            t0 = time.perf_counter()
            chained = ov.draw_undistorted(ud, rect, Rt, img)
            chained_rows.append(dict(ov.timing(), wall_ms=(time.perf_counter() - t0) * 1e3))
            equal = equal and bool(np.array_equal(two, chained))
    undistorted = dict(chained=median_rows(chained_rows, ("wall_ms",) + STAGES),
                       two_calls=median_rows(two_rows, ("wall_ms", "undistort_wall_ms", "draw_wall_ms")),
                       chained_equals_two_calls_bit_for_bit=equal)
    ud.close()
    ov.close()
    return dict(n_points=len(pts), image=[cam.width, cam.height], image_mb=img.nbytes / 1e6, frames=len(poses), configs=configs,
                colorizer_splat_r3=splat, undistorted=undistorted)


def cpu_part():
    pts, cam, img, poses = scene()
    out = []
    for name, order in ORDERS:
        t0 = time.perf_counter()
        res = OR.draw(pts, cam, poses[0], img, 3, order)
        ms = (time.perf_counter() - t0) * 1e3
        out.append(dict(config=f"r=3 {name}", one_frame_ms=ms, first_frame_digest=digest(*res),
                        method="tests/overlay_ref.py draw (numpy, one thread)", cpus=os.cpu_count()))
    return out


def child(mode, limit, lib=None):
    env = dict(os.environ)
    if lib:
        env["LIO_GPU_LIB"] = os.path.abspath(lib)
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", mode],
                       capture_output=True, text=True, env=env)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        print(f"GPU part '{mode}' failed (exit {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        return None
    return json.loads(line[0][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_timing.json"))
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--skip-gpu", action="store_true")
    ap.add_argument("--ab-lib", help="another build of the library for the stamp A/B")
    ap.add_argument("--ab-name", default="without read-before-atomic", help="what --ab-lib is")
    ap.add_argument("--child", choices=("gpu", "stamp"), help=argparse.SUPPRESS)
    ap.add_argument("--limit", type=int, default=300, help="time limit of each GPU part [s]")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(gpu_part() if a.child == "gpu" else stamp_part()))
        return 0
    res = dict(gpu=None, cpu=[], stamp_ab=None)
    if os.path.exists(a.out):  # a run that skips a part keeps that part of an earlier run
        with open(a.out) as f:
            old = json.load(f)
        res.update({k: old.get(k, res[k]) for k in res})
    if not a.skip_gpu:
        res["gpu"] = child("gpu", a.limit)
        if res["gpu"] is None:
            return 1  # nothing more is started on the device
        for c in res["gpu"]["configs"]:
            print(c["config"], c["per_frame_median"], flush=True)
        print("colorizer splat r=3", res["gpu"]["colorizer_splat_r3"], flush=True)
        print("undistorted", res["gpu"]["undistorted"], flush=True)
        if a.ab_lib:
            runs = []
            for k in range(4):  # this build, the other, this build, the other
                runs.append(child("stamp", a.limit, a.ab_lib if k % 2 else None))
                if runs[-1] is None:
                    return 1
            res["stamp_ab"] = {"this build": runs[0::2], a.ab_name: runs[1::2]}
            print("stamp A/B", json.dumps(res["stamp_ab"]), flush=True)
    if not a.skip_cpu:
        res["cpu"] = cpu_part()
        for c in res["cpu"]:
            print(c["config"], c["one_frame_ms"], flush=True)
    if res["gpu"] and res["cpu"]:
        g = {c["config"]: c["first_frame_digest"] for c in res["gpu"]["configs"]}
        res["cpu_equals_gpu_bit_for_bit"] = {c["config"]: g.get(c["config"]) == c["first_frame_digest"] for c in res["cpu"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
