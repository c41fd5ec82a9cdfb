#!/usr/bin/env python3
"""Timing of the GPU colorizer against its numpy restatement (not a test, not bench.py).

    python scripts/colorize_timing.py [--out profiles/colorize_timing.json] [--skip-cpu] [--skip-gpu]

The workload: a 2 000 000-point street scene (ground, two facades, clutter) in the LiDAR frame and a 4096 x 2464
image (the rig's: post_process/colorize_pcd.py) over several keyframes two metres apart, with the script's extrinsic
and intrinsics.  Per configuration — occlusion off, and on at splat radius 0, 1 and 3 — the median over the frames
of: the host wall time of lio_colorizer_add_frame, and the device times of its stages from stream events (the
upload with its pinned staging copy; the depth fill, the splat and the resolve, or the one fused kernel).  The
first frame of a configuration, which allocates, is reported apart.  The CPU baseline is the numpy restatement of
one frame (tests/colorize_ref.py) on the same host; the state after that frame is compared with the GPU's (sha1).
The GPU part runs in one child process under a time limit (`timeout`), so that trouble in it ends it.
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

import colorize_ref as CR  # noqa: E402

N_POINTS = 2_000_000
FRAMES = 6
CONFIGS = [dict(name="no occlusion", occlusion=False, splat_radius=0),
           dict(name="occlusion r=0", occlusion=True, splat_radius=0, depth_rel=0.02, depth_abs=0.05),
           dict(name="occlusion r=1", occlusion=True, splat_radius=1, depth_rel=0.02, depth_abs=0.05),
           dict(name="occlusion r=3", occlusion=True, splat_radius=3, depth_rel=0.02, depth_abs=0.05)]


def scene():
    """points (float32 x y z intensity) along a 100 m street, the image, and the keyframes' Rt"""
    from lio_gpu import camera as CAM

    rng = np.random.default_rng(2024)
    n = N_POINTS
    kind = rng.random(n)
    x = rng.uniform(-20.0, 80.0, n)
    y = rng.uniform(-15.0, 15.0, n)
    z = np.full(n, -1.8)
    wall = (kind > 0.45) & (kind <= 0.85)
    y[wall] = np.where(rng.random(wall.sum()) < 0.5, -15.0, 15.0) + rng.normal(0, 0.02, wall.sum())
    z[wall] = rng.uniform(-1.8, 12.0, wall.sum())
    clutter = kind > 0.85
    z[clutter] = rng.uniform(-1.8, 4.0, clutter.sum())
    # the street runs along the camera's optical axis (the third row of the script's R, levelled)
    ax, ay = CR.SCRIPT_R[2, :2] / np.linalg.norm(CR.SCRIPT_R[2, :2])
    pts = np.stack([x * ax - y * ay, x * ay + y * ax, z, rng.uniform(0, 255, n)], 1).astype(np.float32)
    cam = CR.script_cam()
    img = rng.integers(0, 256, (cam.height, cam.width, 3), dtype=np.uint8)
    T_cam_lidar = np.eye(4)
    T_cam_lidar[:3, :3], T_cam_lidar[:3, 3] = CR.SCRIPT_R, CR.SCRIPT_T
    poses = []
    for k in range(FRAMES):
        Tw = np.eye(4)
        Tw[:3, 3] = [2.0 * k * ax, 2.0 * k * ay, 0.0]
        poses.append(CAM.world_to_camera(Tw, T_cam_lidar))
    return pts, cam, img, poses


def digest(rgb, frame, depth):
    h = hashlib.sha1()
    for a, t in ((rgb, np.uint8), (frame, np.int32), (depth, np.float64)):
        h.update(np.ascontiguousarray(a, t).tobytes())
    return h.hexdigest()


def gpu_part():
    from lio_gpu import camera as CAM

    pts, cam, img, poses = scene()
    model = CAM.CameraModel(cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height)
    out = []
    for cfg in CONFIGS:
        params = {k: v for k, v in cfg.items() if k != "name"}
        cz = CAM.Colorizer(**params)
        t0 = time.perf_counter()
        cz.set_cloud(pts)
        set_cloud_ms = (time.perf_counter() - t0) * 1e3
        rows, first_digest = [], None
        for rep in range(2):  # the second pass over the same frames is the warm one
            cz.reset()
            rows = []
            for k, Rt in enumerate(poses):
                t0 = time.perf_counter()
                updated = cz.add_frame(model, Rt, img)
                wall = (time.perf_counter() - t0) * 1e3
                rows.append(dict(cz.timing(), wall_ms=wall, n_updated=updated))
                if rep == 0 and k == 0:
                    first_digest, first_wall = digest(*cz.state()), wall
        med = {k: statistics.median(r[k] for r in rows) for k in ("wall_ms", "upload_ms", "fill_ms", "splat_ms", "resolve_ms")}
        coloured = int(np.count_nonzero(cz.frame >= 0))
        out.append(dict(config=cfg["name"], params=params, set_cloud_ms=set_cloud_ms, first_frame_wall_ms=first_wall,
                        per_frame_median=med, frames=rows, coloured_points=coloured, first_frame_digest=first_digest))
        cz.close()
    return dict(n_points=len(pts), image=[cam.width, cam.height], image_mb=img.nbytes / 1e6, frames=FRAMES, configs=out)


def cpu_part():
    pts, cam, img, poses = scene()
    out = []
    for cfg in (CONFIGS[0], CONFIGS[2]):
        st = CR.State(len(pts))
        t0 = time.perf_counter()
        st.add_frame(pts, cam, poses[0], img, occlusion=cfg["occlusion"], radius=cfg["splat_radius"],
                     depth_rel=cfg.get("depth_rel", 0.0), depth_abs=cfg.get("depth_abs", 0.0))
        ms = (time.perf_counter() - t0) * 1e3
        out.append(dict(config=cfg["name"], one_frame_ms=ms, first_frame_digest=digest(st.rgb, st.frame, st.best_z),
                        method="tests/colorize_ref.py State.add_frame (numpy, one thread)", cpus=os.cpu_count()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colorize_timing.json"))
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--skip-gpu", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--limit", type=int, default=300, help="time limit of the GPU part [s]")
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
        for c in res["gpu"]["configs"]:
            print(c["config"], c["per_frame_median"], flush=True)
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
