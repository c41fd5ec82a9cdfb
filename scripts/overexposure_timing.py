#!/usr/bin/env python3
"""Timing of the GPU overexposure recovery and 8-bit Gaussian blur against their numpy restatement (not a test, not
bench.py).

    python scripts/overexposure_timing.py [--out profiles/overexposure_timing.json] [--skip-cpu] [--skip-gpu]

The workload: scripts/exposure_timing.py's 4096 x 2464 x 3 frame, medians over 12 warm frames, everything in one
process on one GPU.  Reported: `recover` (the script's 200 / 5 / 15 / 0) as host wall time per frame and the three
device stage times from stream events; `gaussian_blur` (15, 0) likewise; the chained call (recover_undistorted, K8 /
DIST8 of tests/colorize_ref.py) beside the undistorter alone and beside the two calls one after the other; `clahe` and
its apply-kernel time for comparison; the stencil kernel's algorithmic bytes (one read and one write of the frame) per
second.  Two conditions are evaluated and written out, not tuned: the stencil kernel stage stays below the upload
stage of the same call, and the chained call costs less than the two calls.  The CPU baseline is the numpy restatement
(tests/overexposure_ref.py, one thread) on the same host; the sha1 of its output is compared with the GPU's.  The GPU
part runs in one child process under a time limit (`timeout`), so that trouble in it ends it.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fast-lio-sam_gps_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

import numpy as np  # noqa: E402

import exposure_timing as ET  # noqa: E402
import overexposure_ref as OR  # noqa: E402
import undistort_ref as UR  # noqa: E402

WIDTH, HEIGHT, HBM_PEAK = ET.WIDTH, ET.HEIGHT, ET.HBM_PEAK


def gpu_part():
    from lio_gpu import camera as CAM
    from lio_gpu import exposure as EX

    img = ET.frame()
    res = np.empty_like(img)
    frame_bytes = WIDTH * HEIGHT * 3
    out = dict(image=[WIDTH, HEIGHT, 3], frames=ET.FRAMES, hbm_peak_bytes_per_s=HBM_PEAK,
               parameters=dict(threshold=200, dilate=5, ksize=15, sigma=0.0))
    ex = EX.Exposure()
    t0 = time.perf_counter()
    ex.recover(img, out=res)
    first = (time.perf_counter() - t0) * 1e3
    d = ET.digest(res)
    med, rows = ET.timed(lambda: ex.recover(img, out=res), ex.stencil_timing)
    rate = 2 * frame_bytes / (med["kernel_ms"] * 1e-3)
    out["recover"] = dict(first_frame_wall_ms=first, per_frame_median=med, frames=rows, digest=d,
                          same_bits_on_repeat=ET.digest(res) == d, masked_fraction=float((img.max(-1) > 200).mean()),
                          kernel_algorithmic_bytes=2 * frame_bytes, kernel_bytes_per_s=rate,
                          kernel_fraction_of_hbm_peak=rate / HBM_PEAK,
                          kernel_below_upload=med["kernel_ms"] < med["upload_ms"])
    ex.gaussian_blur(img, 15, out=res)
    d = ET.digest(res)
    med_blur, _ = ET.timed(lambda: ex.gaussian_blur(img, 15, out=res), ex.stencil_timing)
    rate = 2 * frame_bytes / (med_blur["kernel_ms"] * 1e-3)
    out["gaussian_blur"] = dict(per_frame_median=med_blur, digest=d, kernel_bytes_per_s=rate,
                                kernel_fraction_of_hbm_peak=rate / HBM_PEAK)
    ex.gaussian_blur(img, 31, 10.0, out=res)
    med31, _ = ET.timed(lambda: ex.gaussian_blur(img, 31, 10.0, out=res), ex.stencil_timing)
    ex.recover(img, 200, 15, 31, 10.0, out=res)
    med_r31, _ = ET.timed(lambda: ex.recover(img, 200, 15, 31, 10.0, out=res), ex.stencil_timing)
    out["largest_kernel"] = dict(gaussian_blur_31_per_frame_median=med31, recover_15_31_per_frame_median=med_r31)
    # clahe and its apply kernel, for comparison
    ex.clahe(img, out=res)
    med_clahe, _ = ET.timed(lambda: ex.clahe(img, out=res), ex.timing)
    out["clahe"] = dict(per_frame_median=med_clahe)
    # the chained call beside the undistorter alone and beside the two calls
    cam = UR.Cam(*UR.K8, WIDTH, HEIGHT, UR.DIST8)
    model = CAM.CameraModel(cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, cam.dist)
    ud = CAM.Undistorter()
    ud.set_camera(model, None, channels=3)
    rect = ud(img)
    two = ex.recover(rect)
    ex.recover_undistorted(ud, img, out=res)
    same = bool(np.array_equal(res, two))
    med_chain, _ = ET.timed(lambda: ex.recover_undistorted(ud, img, out=res), ex.stencil_timing)
    med_ud, _ = ET.timed(lambda: ud(img, out=rect), ud.timing)
    med_two, _ = ET.timed(lambda: ex.recover(ud(img, out=rect), out=res))
    out["chained"] = dict(per_frame_median=med_chain, undistorter_alone_per_frame_median=med_ud,
                          two_calls_wall_ms=med_two["wall_ms"], equals_the_two_calls=same, digest=ET.digest(res),
                          added_over_undistorter_alone_ms=med_chain["wall_ms"] - med_ud["wall_ms"],
                          ratio_to_undistorter_alone=med_chain["wall_ms"] / med_ud["wall_ms"],
                          chained_below_two_calls=med_chain["wall_ms"] < med_two["wall_ms"])
    ud.close()
    ex.close()
    return out


def cpu_part():
    img = ET.frame()
    t0 = time.perf_counter()
    r = OR.recover(img)
    recover_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    b = OR.gaussian_blur(img, 15)
    blur_ms = (time.perf_counter() - t0) * 1e3
    return dict(recover_ms=recover_ms, gaussian_blur_ms=blur_ms, recover_digest=ET.digest(r), gaussian_blur_digest=ET.digest(b),
                method="tests/overexposure_ref.py recover / gaussian_blur (numpy, one thread)", cpus=os.cpu_count())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overexposure_timing.json"))
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--skip-gpu", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--limit", type=int, default=300, help="time limit of the GPU part [s]")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(gpu_part()))
        return 0
    res = dict(gpu=None, cpu=None)
    if os.path.exists(a.out):  # a run with --skip-gpu or --skip-cpu keeps the other half of an earlier run
        with open(a.out) as f:
            old = json.load(f)
        res["gpu"], res["cpu"] = old.get("gpu"), old.get("cpu")
    if not a.skip_gpu:
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child"],
                           capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"GPU part failed (exit {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            return 1
        g = res["gpu"] = json.loads(line[0][7:])
        print("recover", g["recover"]["per_frame_median"], flush=True)
        print("gaussian_blur", g["gaussian_blur"]["per_frame_median"], flush=True)
        print("largest kernel", g["largest_kernel"], flush=True)
        print("clahe", g["clahe"]["per_frame_median"], flush=True)
        print("chained", g["chained"]["per_frame_median"], "undistorter alone", g["chained"]["undistorter_alone_per_frame_median"],
              "two calls", g["chained"]["two_calls_wall_ms"], flush=True)
        print("kernel below upload:", g["recover"]["kernel_below_upload"], " chained below two calls:",
              g["chained"]["chained_below_two_calls"], flush=True)
    if not a.skip_cpu:
        c = res["cpu"] = cpu_part()
        print("numpy: recover", c["recover_ms"], "gaussian_blur", c["gaussian_blur_ms"], flush=True)
    if res["gpu"] and res["cpu"]:
        g, c = res["gpu"], res["cpu"]
        res["cpu_equals_gpu_bit_for_bit"] = dict(recover=g["recover"]["digest"] == c["recover_digest"],
                                                 gaussian_blur=g["gaussian_blur"]["digest"] == c["gaussian_blur_digest"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
