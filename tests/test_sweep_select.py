"""The row selection of a sweep upload (csrc/lio_sweep_select.hpp), host only: tests/cpp/sweep_select.cpp packs
sweeps of 0 to 1000 rows, record widths 4 to 8, point_filter_num 1, 3 and 4, in 1, 2 and 8 pieces (rising and
random times, a step down at a piece boundary, NaN coordinates, points at exactly the blind radius, a first half
that is dropped) and compares the pieces' concatenation, the row count and the sorted flag with a sequential
restatement, built with the address and undefined-behaviour sanitizers (a stand-alone program: nothing is
preloaded)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sweep_select.cpp")


def test_sweep_select(tmp_path):
    exe = str(tmp_path / "sweep_select")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-g", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
