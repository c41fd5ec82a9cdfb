"""The arena carver of csrc/lio_scratch.hpp, host only: tests/cpp/scratch_layout.cpp carves a struct of mixed
element types for counts 0, 1, 255, 257 and 4097 and checks sizes, 256-byte alignment, no overlap, zero-count
fields and the first / last element of every field, by hand and through carve_arena (the measure / assign helper
every reserve runs), built with the address and undefined-behaviour sanitizers
(a stand-alone program: nothing is preloaded)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "scratch_layout.cpp")


def test_scratch_layout(tmp_path):
    exe = str(tmp_path / "scratch_layout")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-g", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
