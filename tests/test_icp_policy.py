"""The loop ICP's HIP-free decisions (csrc/lio_icp_policy.hpp), host only: tests/cpp/icp_policy.cpp checks the
re-pass policy at every rule's boundary (pass counts 3 and 4, re-exchanges 1 and 2, lists equal to and one above
the slot capacity, each hard flag alone, the one-rank use), the event slot (floor, cap, steps of 256, never
shrinking) and the polled mailbox (0 skipped at the wrap-around; a stale word equal to the next sequence number
does not count as arrived), built with the address and undefined-behaviour sanitizers (a stand-alone program:
nothing is preloaded)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "icp_policy.cpp")


def test_icp_policy(tmp_path):
    exe = str(tmp_path / "icp_policy")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-g", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
