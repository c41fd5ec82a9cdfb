"""The arithmetic of lio_estimate_normals behind the search, host build: tests/cpp/normals_math.cpp compiles
csrc/lio_normals_math.hpp — the text the device compiles — with g++, -ffp-contract=off and the address and
undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded) and prints, for 1208 generated moment
sets (random, near-planar, near-linear, exactly planar, exactly linear, zero, and sums near the int64 range), the
bits of the normal and the curvature, and 400 quantisations.  They are compared exactly with tests/normals_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import normals_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "normals_math.cpp")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("normals_math") / "normals_math")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-g", "-I", os.path.join(ROOT, "fast-lio-sam_gps_amd", "csrc"), SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.splitlines()


def _f32(words):
    return np.array([int(w, 16) for w in words], np.uint32).view(np.float32)


def test_moment_sets_match_the_restatement_bit_for_bit(lines):
    rows = [ln.split() for ln in lines if ln and ln[0] in "-0123456789"]
    assert len(rows) >= 1000
    S = np.array([[int(v) for v in r[0:3]] for r in rows], np.int64)
    SS = np.array([[int(v) for v in r[3:9]] for r in rows], np.int64)
    m = np.array([int(r[9]) for r in rows], np.int64)
    B = _f32([r[10] for r in rows])
    xyz = np.stack([_f32([r[11 + d] for r in rows]) for d in range(3)], axis=1)
    has_vp = np.array([int(r[14]) for r in rows], bool)
    vp = np.stack([_f32([r[15 + d] for r in rows]) for d in range(3)], axis=1)
    ok = np.array([int(r[18]) for r in rows], bool)
    got = np.stack([_f32([r[19 + d] for r in rows]) for d in range(4)], axis=1)
    want = np.zeros_like(got)
    want_ok = np.zeros(len(rows), bool)
    for sel, v in ((has_vp, vp[has_vp]), (~has_vp, None)):
        nr, cu, k = NR.solve(S[sel], SS[sel], m[sel], B[sel], xyz[sel], v)
        want[sel, :3], want[sel, 3], want_ok[sel] = nr, cu, k
    assert np.array_equal(ok, want_ok)
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    # every kind is there: normals, degenerate sets (zero ones among them) and flipped and unflipped signs
    assert ok.sum() >= 800 and (~ok).sum() >= 200
    assert (got[ok & ~has_vp, 2] >= 0).all() and (got[ok & has_vp, 2] < 0).any()
    assert np.all(np.abs(np.linalg.norm(got[ok, :3].astype(np.float64), axis=1) - 1.0) < 1e-6)


def test_quantisation_matches_the_restatement(lines):
    rows = [ln.split() for ln in lines if ln.startswith("Q ")]
    assert len(rows) == 400
    B, o = _f32([r[1] for r in rows]), _f32([r[2] for r in rows])
    q = np.array([int(r[3]) for r in rows], np.int64)
    want = np.rint(o.astype(np.float64) * NR.scale_of(B)).astype(np.int64)
    assert np.array_equal(q, want)
    assert np.abs(q).max() <= 2**15 and np.abs(q).max() > 2**13
