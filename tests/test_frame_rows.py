"""The byte arithmetic of csrc/lio_frame.hpp, host only: tests/cpp/frame_rows.cpp checks the span of a pitched image
(one row, and 32767 rows of a padded pitch, past 2^31), the device pitch, and copy_rows over widths 1, 3, 4, 5 and 67,
1 and 3 channels, 1, 2 and 5 rows and every pair of packed, rounded-to-4 and + 7 pitches: every pixel byte arrives,
every padding byte of the destination keeps its sentinel, and both blocks are exactly their span, built with the
address and undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "frame_rows.cpp")


def test_frame_rows(tmp_path):
    exe = str(tmp_path / "frame_rows")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-g", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
