"""The stencil part of the C++ mirror (include/lio_gpu.hpp: Exposure::recover, Exposure::gaussian_blur,
lio_gpu::gaussian_weights): tests/cpp/overexposure_api.cpp compiles and links with g++ against liblio_gpu.so here
(CPU), where its weights are compared with the restatement's, and runs on the GPU, where the hashes of its output
buffers are compared with those of the numpy restatement's outputs (tests/overexposure_ref.py) for the same frame."""
import os
import subprocess

import numpy as np
import pytest

import exposure_ref as ER
import overexposure_ref as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "fast-lio-sam_gps_amd", "lio_gpu", "_lib")
SRC = os.path.join(ROOT, "tests", "cpp", "overexposure_api.cpp")
FILL = 0xA5


def _build(tmp_path):
    exe = str(tmp_path / "overexposure_api")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
           "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
           "-L", LIBDIR, "-llio_gpu", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("overexposure_api"))


def fnv1a(data: bytes) -> int:
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_overexposure_compiles_and_links(exe):
    assert os.path.exists(os.path.join(LIBDIR, "liblio_gpu.so")), "build the library first (make -C fast-lio-sam_gps_amd)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stdout  # no scene: nothing touches the device


def test_cpp_weights_equal_the_restatement(exe):
    for k, sigma in ((15, 0.0), (7, 0.0), (1, 0.0), (31, 10.0), (9, 0.5), (15, 2.6)):
        r = subprocess.run([exe, "--weights", str(k), repr(sigma)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        np.testing.assert_array_equal(np.array(r.stdout.split(), np.int64), OR.gaussian_weights(k, sigma))
    r = subprocess.run([exe, "--weights", "4", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "ksize must be odd" in r.stdout


def test_makefile_builds_the_driver():
    """`all` reaches the driver's rule (g++ with -Werror on tests/cpp/overexposure_api.cpp) and the kernels' object, and
    `clean` removes the driver: read from make's own dry run"""
    def dry(goal):
        r = subprocess.run(["make", "-n", "-B", "-C", os.path.join(ROOT, "fast-lio-sam_gps_amd"), goal], capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout
    built = dry("all")
    rule = [line for line in built.splitlines() if "../tests/cpp/overexposure_api.cpp" in line]
    assert len(rule) == 1 and rule[0].startswith("g++ ") and "-Werror" in rule[0] and "-o lio_gpu/_lib/overexposure_api" in rule[0]
    assert "csrc/lio_overexposure.hip" in built
    assert "lio_gpu/_lib/overexposure_api" in dry("clean")


# width height channels order threshold dilate ksize sigma
CASES = [(67, 38, 3, 0, 200, 5, 15, 0.0), (67, 38, 1, 0, 200, 5, 15, 0.0), (67, 38, 3, 1, 120, 15, 31, 2.6)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_cpp_overexposure_hashes_equal_the_restatement_on_gpu(exe, tmp_path, case):
    width, height, channels, order, thr, dilate, ksize, sigma = case
    pitch, out_pitch = channels * width + 7, channels * width + 5
    rng = np.random.default_rng(width + channels)
    rows = rng.integers(0, 256, (height, pitch), dtype=np.uint8)
    img = ER.strided(rows, width, height, channels)
    head = np.zeros(16, np.float64)
    head[:11] = width, height, channels, order, pitch, out_pitch, FILL, thr, dilate, ksize, sigma
    with open(tmp_path / "scene.bin", "wb") as f:
        f.write(head.tobytes() + rows.tobytes())
    r = subprocess.run([exe, str(tmp_path / "scene.bin"), str(tmp_path / "result.bin")], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    got = dict(line.split() for line in r.stdout.splitlines() if line.startswith(("recover ", "gaussian_blur ")))
    row = channels * width
    for name, want in (("recover", OR.recover(img, thr, dilate, ksize, sigma, order)), ("gaussian_blur", OR.gaussian_blur(img, ksize, sigma))):
        buf = np.full((height, out_pitch), FILL, np.uint8)  # the output buffer as the driver holds it, padding included
        buf[:, :row] = want.reshape(height, row)
        assert int(got[name], 16) == fnv1a(buf.tobytes()), name
    raw = np.fromfile(tmp_path / "result.bin", np.uint8)
    assert len(raw) == 2 * height * out_pitch
    np.testing.assert_array_equal(raw[:height * out_pitch].reshape(height, out_pitch)[:, :row].reshape(img.shape),
                                  OR.recover(img, thr, dilate, ksize, sigma, order))
