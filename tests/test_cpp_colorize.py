"""The camera part of the C++ mirror (include/lio_gpu.hpp: CameraModel, project_points, Colorizer):
tests/cpp/colorize_api.cpp compiles and links with g++ against liblio_gpu.so here (CPU) and runs on the GPU, where
it checks the projection and the colorizer's state bit for bit against the contract written out in C++."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "fast-lio-sam_gps_amd", "lio_gpu", "_lib")
SRC = os.path.join(ROOT, "tests", "cpp", "colorize_api.cpp")


def _build(tmp_path):
    exe = str(tmp_path / "colorize_api")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
           "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
           "-L", LIBDIR, "-llio_gpu", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_cpp_colorize_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(LIBDIR, "liblio_gpu.so")), "build the library first (make -C fast-lio-sam_gps_amd)"
    _build(tmp_path)


def test_makefile_builds_the_driver():
    """`all` reaches the driver's rule (g++ with -Werror on tests/cpp/colorize_api.cpp) and the kernels' object, and
    `clean` removes the driver: read from make's own dry run, whatever way the Makefile spells its rules"""
    def dry(goal):
        r = subprocess.run(["make", "-n", "-B", "-C", os.path.join(ROOT, "fast-lio-sam_gps_amd"), goal], capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout
    built = dry("all")
    rule = [line for line in built.splitlines() if "../tests/cpp/colorize_api.cpp" in line]
    assert len(rule) == 1 and rule[0].startswith("g++ ") and "-Werror" in rule[0] and "-o lio_gpu/_lib/colorize_api" in rule[0]
    assert "csrc/lio_colorize.hip" in built
    assert "lio_gpu/_lib/colorize_api" in dry("clean")


@pytest.mark.gpu
def test_cpp_colorize_runs_on_gpu(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
