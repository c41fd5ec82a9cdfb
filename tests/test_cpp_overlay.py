"""The overlay part of the C++ mirror (include/lio_gpu.hpp: PointOverlay): tests/cpp/overlay.cpp compiles and links
with g++ against liblio_gpu.so here (CPU) and runs on the GPU, where it draws one seeded frame and prints digests
that are compared with the contract restated in numpy (tests/overlay_ref.py) on the same scene."""
import os
import re
import subprocess

import numpy as np
import pytest

import overlay_ref as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "fast-lio-sam_gps_amd", "lio_gpu", "_lib")
SRC = os.path.join(ROOT, "tests", "cpp", "overlay.cpp")


def _build(tmp_path):
    exe = str(tmp_path / "overlay")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
           "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
           "-L", LIBDIR, "-llio_gpu", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_cpp_overlay_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(LIBDIR, "liblio_gpu.so")), "build the library first (make -C fast-lio-sam_gps_amd)"
    _build(tmp_path)


def test_makefile_builds_the_driver():
    """`all` reaches the driver's rule (g++ with -Werror on tests/cpp/overlay.cpp) and the kernels' object, and `clean`
    removes the driver: read from make's own dry run"""
    def dry(goal):
        r = subprocess.run(["make", "-n", "-B", "-C", os.path.join(ROOT, "fast-lio-sam_gps_amd"), goal], capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout
    built = dry("all")
    rule = [line for line in built.splitlines() if "../tests/cpp/overlay.cpp" in line]
    assert len(rule) == 1 and rule[0].startswith("g++ ") and "-Werror" in rule[0] and "-o lio_gpu/_lib/overlay" in rule[0]
    assert "csrc/lio_overlay.hip" in built
    assert "lio_gpu/_lib/overlay" in dry("clean")


def expected(radius, order, **src):
    """the digests the driver prints for one draw: the owner image, the whole padded buffer, n_drawn"""
    img, rec, labels = OR.cpp_scene()
    if "labels" in src:
        src["labels"] = labels
    out, owner, n = OR.draw(rec, OR.cpp_cam(), OR.CPP_RT, img, radius, order, **src)
    buf = np.lib.stride_tricks.as_strided(img, (64, OR.CPP_PITCH), (OR.CPP_PITCH, 1)).copy()  # the rows with their padding
    np.lib.stride_tricks.as_strided(buf, (64, 96, 3), (OR.CPP_PITCH, 3, 1))[:] = out
    return f"owner={OR.fnv1a(owner):016x} image={OR.fnv1a(buf):016x} n_drawn={n}"


@pytest.mark.gpu
def test_cpp_overlay_runs_on_gpu(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    got = dict(re.findall(r"^(\w+): (owner=\w+ image=\w+ n_drawn=\d+)$", r.stdout, re.M))
    assert got["nearest"] == expected(3, OR.NEAREST, labels=True, palette=OR.CPP_PALETTE)
    assert got["tool"] == expected(3, OR.DRAW_ORDER)
