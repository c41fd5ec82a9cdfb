"""The slack of the computed cell faces (csrc/lio_grid_margin.hpp grid_margin), host only: tests/cpp/grid_margin.cpp
restates cell_coord and the face formula, sweeps cells {0.3, 0.6, 0.7, 1.0, 2.3}, origins {-3.1, 2e4, 1e5, 1e6} and
extents up to 5e4 m, finds at every face the first float assigned to the cell above it and checks that the face,
the upper face derived from the cell below and both box faces stay within the margin of it.  The former constant
1e-3 + 1e-4 * cell fails the same sweep.  Built with the address and undefined-behaviour sanitizers (a stand-alone
program: nothing is preloaded)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "grid_margin.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("grid_margin") / "grid_margin")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", SRC, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_grid_margin_covers_the_face_rounding(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]


def test_former_constant_does_not(exe):
    r = subprocess.run([exe, "old"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "MARGIN EXCEEDED" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr  # the sanitizers stay quiet
