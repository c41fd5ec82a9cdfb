#!/usr/bin/env python3
"""Timing of the GPU exposure adaption against its numpy restatement (not a test, not bench.py).

    python scripts/exposure_timing.py [--out profiles/exposure_timing.json] [--skip-cpu] [--skip-gpu]

The workload: one 4096 x 2464 x 3 frame (the rig's), medians over 12 warm frames.  Reported: `clahe` (adapt_exposure:
clip 2.0, 8 x 8 tiles) as host wall time per frame and the five device stage times from stream events; `remap` (lut_v
and lut_all) and `histograms` per frame; the chained call
(clahe_undistorted, K8 / DIST8 of tests/colorize_ref.py) beside the undistorter alone as scripts/undistort_timing.py
measures it in the same process, and beside the two calls one after the other; the kernels' algorithmic bytes per
second.  The CPU baseline is the numpy restatement (tests/exposure_ref.py, one thread) on the same host; its outputs
are compared with the GPU's (sha1).  There is no OpenCV on these machines, so there is no cv2 timing.  The GPU part
runs in one child process under a time limit (`timeout`), so that trouble in it ends it.
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

import exposure_ref as ER  # noqa: E402
import undistort_ref as UR  # noqa: E402

WIDTH, HEIGHT = 4096, 2464
FRAMES = 12
HBM_PEAK = 8.0e12  # bytes per second (the MI355X's specification)
STAGES = ("upload_ms", "hist_ms", "lut_ms", "apply_ms", "download_ms")


def frame():
    """a frame with structure (a bright sky over a darker ground, noise on both), so that tiles differ and clip"""
    rng = np.random.default_rng(2025)
    img = rng.integers(0, 90, (HEIGHT, WIDTH, 3), dtype=np.uint8)
    img[:HEIGHT // 3] = rng.integers(200, 256, (HEIGHT // 3, WIDTH, 3), dtype=np.uint8)
    img[HEIGHT // 3:HEIGHT // 2] += np.uint8(80)
    return img


def tables():
    rng = np.random.default_rng(7)
    return np.sort(rng.integers(0, 256, 256, dtype=np.uint8)), np.sort(rng.integers(0, 256, 256, dtype=np.uint8))


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a, np.uint8).tobytes()).hexdigest()


def timed(fn, timing=None):
    rows = []
    for _ in range(FRAMES):
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        rows.append(dict(timing() if timing else {}, wall_ms=wall))
    return {k: statistics.median(r[k] for r in rows) for k in rows[0]}, rows


def gpu_part():
    import undistort_timing as UT
    from lio_gpu import camera as CAM
    from lio_gpu import exposure as EX

    img = frame()
    lut_v, lut_all = tables()
    res = np.empty_like(img)
    pixels = WIDTH * HEIGHT
    out = dict(image=[WIDTH, HEIGHT, 3], frames=FRAMES, hbm_peak_bytes_per_s=HBM_PEAK)
    ex = EX.Exposure()
    t0 = time.perf_counter()
    ex.clahe(img, out=res)
    first = (time.perf_counter() - t0) * 1e3
    d = digest(res)
    med, rows = timed(lambda: ex.clahe(img, out=res), ex.timing)
    # algorithmic bytes: the histogram reads the frame once; the apply reads and writes it and gathers 4 table bytes a pixel
    hist_rate = pixels * 3 / (med["hist_ms"] * 1e-3)
    apply_rate = pixels * (3 + 3 + 4) / (med["apply_ms"] * 1e-3)
    out["clahe"] = dict(first_frame_wall_ms=first, per_frame_median=med, frames=rows, digest=d,
                        same_bits_on_repeat=digest(res) == d, hist_algorithmic_bytes=pixels * 3,
                        hist_bytes_per_s=hist_rate, hist_fraction_of_hbm_peak=hist_rate / HBM_PEAK,
                        hist_pixels_per_s=pixels / (med["hist_ms"] * 1e-3),
                        apply_algorithmic_bytes=pixels * 10, apply_bytes_per_s=apply_rate,
                        apply_fraction_of_hbm_peak=apply_rate / HBM_PEAK,
                        copies_fraction_of_device_time=(med["upload_ms"] + med["download_ms"]) / sum(med[k] for k in STAGES))
    # the histogram kernel's worst case: every pixel in bin 255
    full = np.full_like(img, 255)
    ex.clahe(full, out=res)
    med_full, _ = timed(lambda: ex.clahe(full, out=res), ex.timing)
    out["clahe_saturated_frame"] = dict(per_frame_median=med_full, one_value=bool((res == res.flat[0]).all()))
    ex.remap(img, lut_v, lut_all, out=res)
    d = digest(res)
    med, _ = timed(lambda: ex.remap(img, lut_v, lut_all, out=res), ex.timing)
    out["remap"] = dict(per_frame_median=med, digest=d)
    hv, hg = ex.histograms(img)
    med, _ = timed(lambda: ex.histograms(img), ex.timing)
    out["histograms"] = dict(per_frame_median=med, digest=digest(np.concatenate([hv, hg]).view(np.uint8)))
    # the chained call beside the undistorter alone and beside the two calls
    cam = UR.Cam(*UR.K8, WIDTH, HEIGHT, UR.DIST8)
    model = CAM.CameraModel(cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, cam.dist)
    ud = CAM.Undistorter()
    ud.set_camera(model, None, channels=3)
    rect = ud(img)
    two = ex.clahe(rect)
    ex.clahe_undistorted(ud, img, out=res)
    same = bool(np.array_equal(res, two))
    med_chain, _ = timed(lambda: ex.clahe_undistorted(ud, img, out=res), ex.timing)
    med_ud, _ = timed(lambda: ud(img, out=rect), ud.timing)
    med_two, _ = timed(lambda: ex.clahe(ud(img, out=rect), out=res))
    out["chained"] = dict(per_frame_median=med_chain, undistorter_alone_per_frame_median=med_ud,
                          two_calls_wall_ms=med_two["wall_ms"], equals_the_two_calls=same, digest=digest(res),
                          added_over_undistorter_alone_ms=med_chain["wall_ms"] - med_ud["wall_ms"],
                          ratio_to_undistorter_alone=med_chain["wall_ms"] / med_ud["wall_ms"])
    ud.close()
    ex.close()
    ut = UT.gpu_part()["runs"][0]  # scripts/undistort_timing.py's own measurement, in this process
    out["undistort_timing_py"] = dict(per_frame_median=ut["per_frame_median"], channels=ut["channels"])
    return out


def cpu_part():
    img = frame()
    lut_v, lut_all = tables()
    t0 = time.perf_counter()
    c = ER.clahe(img, 2.0, (8, 8))
    clahe_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    r = ER.remap(img, lut_v, lut_all)
    remap_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    hv, hg = ER.histograms(img)
    hist_ms = (time.perf_counter() - t0) * 1e3
    return dict(clahe_ms=clahe_ms, remap_ms=remap_ms, histograms_ms=hist_ms, clahe_digest=digest(c), remap_digest=digest(r),
                histograms_digest=digest(np.concatenate([hv, hg]).view(np.uint8)),
                method="tests/exposure_ref.py clahe / remap / histograms (numpy, one thread)", cpus=os.cpu_count())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exposure_timing.json"))
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
        print("clahe", g["clahe"]["per_frame_median"], flush=True)
        print("clahe, saturated frame", g["clahe_saturated_frame"]["per_frame_median"], flush=True)
        print("remap", g["remap"]["per_frame_median"], flush=True)
        print("chained", g["chained"]["per_frame_median"], "undistorter alone", g["chained"]["undistorter_alone_per_frame_median"],
              "two calls", g["chained"]["two_calls_wall_ms"], flush=True)
    if not a.skip_cpu:
        c = res["cpu"] = cpu_part()
        print("numpy: clahe", c["clahe_ms"], "remap", c["remap_ms"], "histograms", c["histograms_ms"], flush=True)
    if res["gpu"] and res["cpu"]:
        g, c = res["gpu"], res["cpu"]
        res["cpu_equals_gpu_bit_for_bit"] = dict(
            clahe=g["clahe"]["digest"] == c["clahe_digest"],
            remap=g["remap"]["digest"] == c["remap_digest"], histograms=g["histograms"]["digest"] == c["histograms_digest"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
