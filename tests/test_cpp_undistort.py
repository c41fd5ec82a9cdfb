"""The undistortion part of the C++ mirror (include/lio_gpu.hpp: Undistorter, undistort_map):
tests/cpp/undistort_api.cpp compiles and links with g++ against liblio_gpu.so here (CPU) and runs on the GPU on the
scenes of tests/test_gpu_undistort.py, where its output buffer and map are compared byte for byte with Python's."""
import os
import subprocess

import numpy as np
import pytest

import undistort_ref as UR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "fast-lio-sam_gps_amd", "lio_gpu", "_lib")
SRC = os.path.join(ROOT, "tests", "cpp", "undistort_api.cpp")
BORDER = (7, 200, 31)
FILL = 0xA5


def _build(tmp_path):
    exe = str(tmp_path / "undistort_api")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
           "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
           "-L", LIBDIR, "-llio_gpu", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("undistort_api"))


def test_cpp_undistort_compiles_and_links(exe):
    assert os.path.exists(os.path.join(LIBDIR, "liblio_gpu.so")), "build the library first (make -C fast-lio-sam_gps_amd)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stdout  # no scene: nothing touches the device


def test_makefile_builds_the_driver():
    """`all` reaches the driver's rule (g++ with -Werror on tests/cpp/undistort_api.cpp) and the kernels' object, and
    `clean` removes the driver: read from make's own dry run, whatever way the Makefile spells its rules"""
    def dry(goal):
        r = subprocess.run(["make", "-n", "-B", "-C", os.path.join(ROOT, "fast-lio-sam_gps_amd"), goal], capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout
    built = dry("all")
    rule = [line for line in built.splitlines() if "../tests/cpp/undistort_api.cpp" in line]
    assert len(rule) == 1 and rule[0].startswith("g++ ") and "-Werror" in rule[0] and "-o lio_gpu/_lib/undistort_api" in rule[0]
    assert "csrc/lio_undistort.hip" in built
    assert "lio_gpu/_lib/undistort_api" in dry("clean")


def write_scene(path, scene, channels, border, img_rows, pitch, out_pitch):
    src, dst = scene.src, scene.dst
    d = np.zeros(32, np.float64)
    d[0:4] = src.fx, src.fy, src.cx, src.cy
    d[4:12] = src.dist
    d[12:14] = src.width, src.height
    if dst is not None:
        d[14] = 1.0
        d[15:19] = dst.fx, dst.fy, dst.cx, dst.cy
        d[19:21] = dst.width, dst.height
    d[21] = channels
    d[22:25] = border
    d[25:28] = pitch, out_pitch, FILL
    with open(path, "wb") as f:
        f.write(d.tobytes())
        f.write(img_rows.tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("scene", UR.scenes(), ids=lambda s: s.name)
def test_cpp_undistort_equals_python_on_gpu(exe, tmp_path, scene):
    from lio_gpu import camera as CAM

    def model(cam):
        return CAM.CameraModel(cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, cam.dist)

    src, out_cam = scene.src, scene.out_cam
    new = model(scene.dst) if scene.dst is not None else None
    _, sxy, axy = CAM.undistort_map(model(src), new)
    ud = CAM.Undistorter()
    try:
        for channels in (3, 1):
            pitch, out_pitch = channels * src.width + 7, channels * out_cam.width + 5
            rows = np.random.default_rng(11 + channels).integers(0, 256, (src.height, pitch), dtype=np.uint8)
            shape, strides = ((src.height, src.width), (pitch, 1)) if channels == 1 else ((src.height, src.width, 3), (pitch, 3, 1))
            img = np.lib.stride_tricks.as_strided(rows, shape, strides)
            write_scene(tmp_path / "scene.bin", scene, channels, BORDER, rows, pitch, out_pitch)
            r = subprocess.run([exe, str(tmp_path / "scene.bin"), str(tmp_path / "result.bin")], capture_output=True, text=True,
                               timeout=120)
            print(r.stdout[-2000:])
            assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
            raw = np.fromfile(tmp_path / "result.bin", np.uint8)
            n_out, n_map = out_cam.height * out_pitch, 2 * out_cam.height * out_cam.width
            assert len(raw) == n_out + 5 * n_map
            got = raw[:n_out].reshape(out_cam.height, out_pitch)
            ud.set_camera(model(src), new, channels=channels, border=BORDER)
            py = ud(img)
            np.testing.assert_array_equal(got[:, :channels * out_cam.width], py.reshape(out_cam.height, channels * out_cam.width))
            np.testing.assert_array_equal(py, UR.remap(img, UR.undistort_map(scene.src, scene.dst), src, BORDER))
            assert (got[:, channels * out_cam.width:] == FILL).all(), "the C++ output's padding was written"
            np.testing.assert_array_equal(raw[n_out:n_out + 4 * n_map].view(np.int32), sxy.ravel())
            np.testing.assert_array_equal(raw[n_out + 4 * n_map:], axy.ravel())
    finally:
        ud.close()
