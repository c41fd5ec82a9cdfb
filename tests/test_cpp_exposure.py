"""The exposure part of the C++ mirror (include/lio_gpu.hpp: Exposure and the table helpers):
tests/cpp/exposure_api.cpp compiles and links with g++ against liblio_gpu.so here (CPU), where its gamma tables are
compared with numpy's, and runs on the GPU, where its output buffers, histograms and tables are compared byte for
byte with the numpy restatement (tests/exposure_ref.py) and lio_gpu.exposure."""
import os
import subprocess

import numpy as np
import pytest

import exposure_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "fast-lio-sam_gps_amd", "lio_gpu", "_lib")
SRC = os.path.join(ROOT, "tests", "cpp", "exposure_api.cpp")
FILL = 0xA5


def _build(tmp_path):
    exe = str(tmp_path / "exposure_api")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
           "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
           "-L", LIBDIR, "-llio_gpu", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("exposure_api"))


def test_cpp_exposure_compiles_and_links(exe):
    assert os.path.exists(os.path.join(LIBDIR, "liblio_gpu.so")), "build the library first (make -C fast-lio-sam_gps_amd)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stdout  # no scene: nothing touches the device


def test_cpp_gamma_tables_equal_numpy(exe):
    """libm's pow against numpy's, byte for byte"""
    from lio_gpu import exposure as EX

    r = subprocess.run([exe, "--luts"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2
    for line, g in zip(lines, (0.8, 1.2)):
        got = np.array(line.split(), np.int64)
        x = np.arange(256)
        np.testing.assert_array_equal(got, np.clip(((x / 255.0) ** g) * 255.0, 0, 255).astype(np.uint8))
        np.testing.assert_array_equal(got, EX.gamma_lut(g))


def test_makefile_builds_the_driver():
    """`all` reaches the driver's rule (g++ with -Werror on tests/cpp/exposure_api.cpp) and the kernels' object, and
    `clean` removes the driver: read from make's own dry run, whatever way the Makefile spells its rules"""
    def dry(goal):
        r = subprocess.run(["make", "-n", "-B", "-C", os.path.join(ROOT, "fast-lio-sam_gps_amd"), goal], capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout
    built = dry("all")
    rule = [line for line in built.splitlines() if "../tests/cpp/exposure_api.cpp" in line]
    assert len(rule) == 1 and rule[0].startswith("g++ ") and "-Werror" in rule[0] and "-o lio_gpu/_lib/exposure_api" in rule[0]
    assert "csrc/lio_exposure.hip" in built
    assert "lio_gpu/_lib/exposure_api" in dry("clean")


CASES = [(67, 38, 3, 0, 2.0, 8, 8), (67, 38, 1, 0, 2.0, 8, 8), (64, 48, 3, 1, 40.0, 3, 5), (9, 7, 1, 0, 0.0, 8, 6)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_cpp_exposure_equals_the_restatement_on_gpu(exe, tmp_path, case):
    from lio_gpu import exposure as EX

    width, height, channels, order, clip, tx, ty = case
    pitch, out_pitch = channels * width + 7, channels * width + 5
    rng = np.random.default_rng(width + channels)
    rows = rng.integers(0, 256, (height, pitch), dtype=np.uint8)
    img = ER.strided(rows, width, height, channels)
    lut_v, lut_all = rng.integers(0, 256, 256, dtype=np.uint8), rng.integers(0, 256, 256, dtype=np.uint8)
    head = np.zeros(16, np.float64)
    head[:10] = width, height, channels, order, pitch, out_pitch, FILL, clip, tx, ty
    with open(tmp_path / "scene.bin", "wb") as f:
        f.write(head.tobytes() + rows.tobytes() + lut_v.tobytes() + lut_all.tobytes())
    r = subprocess.run([exe, str(tmp_path / "scene.bin"), str(tmp_path / "result.bin")], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    raw = np.fromfile(tmp_path / "result.bin", np.uint8)
    n_out = height * out_pitch
    assert len(raw) == 2 * n_out + 2 * 256 * 8 + 4 * 256
    row = channels * width
    shape = (height, width) if channels == 1 else (height, width, 3)
    for k, want in enumerate((ER.clahe(img, clip, (tx, ty), order), ER.remap(img, lut_v, lut_all, order))):
        got = raw[k * n_out:(k + 1) * n_out].reshape(height, out_pitch)
        np.testing.assert_array_equal(got[:, :row].reshape(shape), want, err_msg=("clahe", "remap")[k])
        assert (got[:, row:] == FILL).all(), "the C++ output's padding was written"
    hv, hg = ER.histograms(img, order)
    hists = raw[2 * n_out:2 * n_out + 4096].view(np.int64)
    np.testing.assert_array_equal(hists[:256], hv)
    np.testing.assert_array_equal(hists[256:], hg)
    luts = raw[2 * n_out + 4096:].reshape(4, 256)
    np.testing.assert_array_equal(luts[0], EX.gamma_lut(0.8))
    np.testing.assert_array_equal(luts[1], EX.gamma_lut(1.2))
    np.testing.assert_array_equal(luts[2], EX.equalize_lut(hv))
    np.testing.assert_array_equal(luts[3], EX.stretch_lut(hv))
