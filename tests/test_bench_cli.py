"""bench.py's command line: a plain run measures the headline only (--full adds the rest), --steps sets the
number of timed steps, and --dump-outputs writes the last timed step's results, which equal the same update
made through the Python mirror in this process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
SECONDARY = ("upload_inclusive", "roofline", "cpu_baseline", "loop_icp", "multi_stream", "pipeline", "loop_sequence")


def test_bench_options(monkeypatch):
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    from lio_gpu import frontend as F
    from lio_gpu import synth

    d = str(tmp_path / "out")
    # C1 (200k-pt static map, 16k-pt scans), 2 resident scans, 3 timed steps: the last one uses scan 0
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--prewarm-s", "0",
                        "--config", "C1", "--scans", "2", "--dump-outputs", d],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["full"] is False and all(line[k] is None for k in SECONDARY)
    assert line["steps"] == 3 and len(line["step_ms"]) == 3
    assert line["unit"] == "scans/s" and line["higher_is_better"] is True and line["dtype"] == "f32/f64"
    # one rank: value = steps / elapsed and ms_per_step = elapsed / steps; the line rounds ms_per_step to 1e-4 ms
    # (half a unit = 5e-5 ms, under 0.5 % of any step of 0.01 ms or more) and value to 1e-3 scans/s
    assert line["ms_per_step"] >= 0.01
    assert line["value"] * line["ms_per_step"] == pytest.approx(1e3, rel=5e-3)

    got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert sorted(got) == ["cov", "knn_idx", "point_selected", "state", "stats"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 2**20

    # the same update in this process: bench.py's inputs for rank 0 are make_config's
    _, m, scans = synth.make_config("C1", n_scans=1)
    sc = scans[0]
    tree = F.IkdTreeGPU()
    tree.Build(m)
    hm = F.HShareModelGPU(tree)
    hm.set_scan(sc.body)
    kf = F.EsekfGPU(hm, laser_point_cov=0.001, max_iteration=3, epsi=0.001)
    x, P, st = kf.update_iterated_dyn_share_modified(synth.initial_state(sc.pos_init, sc.rot_init),
                                                     synth.initial_cov())
    keys = ("pos", "rot", "offset_R_L_I", "offset_T_L_I", "vel", "bg", "ba", "grav")
    assert np.array_equal(got["state"], np.concatenate([x[k] for k in keys]))
    assert np.array_equal(got["cov"], P)
    assert np.array_equal(got["stats"], [st["h_evals"], st["knn_calls"], st["converged"], st["n_eff"], st["res_mean"]])
    assert line["h_evals_per_scan"] >= 1 and st["n_eff"] > 0
    idx, _ = hm.nearest_points()
    _, sel = hm.normvec()
    assert got["knn_idx"].shape == (len(sc.body), 5) and np.array_equal(got["knn_idx"], idx)
    assert np.array_equal(got["point_selected"], sel)
    hm.close()
    tree.close()
