"""Loop-closure ICP correspondence search on the GPU (icp_tile_kernel) vs brute force.

Every source point's 1-NN in the final (getFitnessScore) pass must be the exact
(d2, id)-minimum over the target, d2 = float ((dx*dx + dy*dy) + dz*dz) — the
kd-tree NN of PCL's KdTreeFLANN restated with the reference's total order
(oracle header, tests/oracle_py.py).  The aligned cloud the pass searched from
is `getFinalAlignedCloud()`, so the check needs no transform restatement.
Cases: the C4 shape at a small size, a source far outside the target (empty
surroundings: the geometric growth), a target of 1-3 points, exact ties, and
a multi-iteration alignment (later passes start from the previous
correspondence).
"""
import numpy as np
import pytest

from icp_stats_ref import brute_nn
from lio_gpu import loop_closure as LC
from lio_gpu import synth

pytestmark = pytest.mark.gpu


def run(src, dst, cell=1.0, guess=None):
    lc = LC.LoopClosure(LC.LoopClosureConfig(), cell_size=cell)
    lc.setInputSource(src)
    lc.setInputTarget(dst)
    r = lc.align(guess=guess)
    ids, d2 = lc.correspondences()
    return lc, r, ids, d2


def check_nn(lc, ids, d2, dst):
    q = lc.getFinalAlignedCloud()
    bi, bd = brute_nn(q, dst)
    np.testing.assert_array_equal(d2, bd)
    np.testing.assert_array_equal(ids, bi)


@pytest.mark.parametrize("cell", [0.5, 1.0, 2.0])
def test_icp_nn_exact_c4_shape(cell):
    src, dst, _ = synth.make_icp_pair(n_points=20_000, seed=5)
    lc, r, ids, d2 = run(src, dst, cell)
    check_nn(lc, ids, d2, dst)


def test_icp_nn_source_far_outside_target():
    rng = np.random.default_rng(3)
    dst = rng.uniform(-5, 5, (4000, 3)).astype(np.float32)
    src = np.concatenate([rng.uniform(-5, 5, (3000, 3)),               # overlapping
                          rng.uniform(40, 60, (500, 3)),               # 40+ m away, one side
                          rng.uniform(-200, -150, (300, 3))]).astype(np.float32)
    lc, r, ids, d2 = run(src, dst, 1.0)
    check_nn(lc, ids, d2, dst)


@pytest.mark.parametrize("nt", [1, 3])
def test_icp_nn_tiny_target(nt):
    rng = np.random.default_rng(nt)
    dst = rng.uniform(-1, 1, (nt, 3)).astype(np.float32)
    src = rng.uniform(-30, 30, (5000, 3)).astype(np.float32)
    lc, r, ids, d2 = run(src, dst, 1.0)
    check_nn(lc, ids, d2, dst)


def test_icp_nn_ties_lowest_id():
    # target on an integer lattice, duplicated points: equal distances everywhere
    g = np.stack(np.meshgrid(np.arange(-4, 5), np.arange(-4, 5), np.arange(0, 3), indexing="ij"), -1).reshape(-1, 3)
    dst = np.concatenate([g, g[::-1]]).astype(np.float32)  # every point twice, different ids
    rng = np.random.default_rng(7)
    src = (rng.integers(-8, 9, (4000, 3)) * 0.5).astype(np.float32)  # half-integer: many exact ties
    lc, r, ids, d2 = run(src, dst, 1.0, guess=np.eye(4, dtype=np.float32))
    check_nn(lc, ids, d2, dst)


def test_icp_nn_zero_distance_ties():
    """Source points ON duplicated target points: d2 = 0 exactly, so the (d2, id) key the tile kernel
    minimises as an f64 is a denormal (just the id) — the lowest id must still win."""
    g = np.stack(np.meshgrid(np.arange(1, 9), np.arange(1, 9), np.arange(1, 4), indexing="ij"), -1).reshape(-1, 3)
    g = g.astype(np.float32) * np.float32(0.75) + np.float32(3.0)
    dst = np.concatenate([g, g[::-1], g]).astype(np.float32)  # every point three times, different ids
    src = np.ascontiguousarray(g[np.random.default_rng(2).permutation(len(g))])
    lc, r, ids, d2 = run(src, dst, 1.0, guess=np.eye(4, dtype=np.float32))
    check_nn(lc, ids, d2, dst)
    assert np.count_nonzero(d2 == 0) > len(src) // 2


def test_icp_nn_multi_iteration_prior():
    # a larger displacement: several ICP iterations, later passes seeded with the previous NN
    src, dst, _ = synth.make_icp_pair(n_points=20_000, seed=9, disp=(1.0, 4.0))
    lc, r, ids, d2 = run(src, dst, 1.0)
    assert r.iterations >= 2
    check_nn(lc, ids, d2, dst)


@pytest.mark.parametrize("mode", [LC.FIDELITY_ORDER, LC.DOUBLE_STATS])
@pytest.mark.parametrize("n", [2, 4])
def test_icp_group_bit_identical_to_one_handle(n, mode):
    """lio_icp_group (single-process multi-GPU): n ranks — all on device 0 on a one-GPU
    box, so the records (and in the default PCL float mode the float chains' messages) travel through host memory;
    distinct devices use RCCL — give the one-handle transform, score, iterations and aligned cloud bit for
    bit, in the default mode and in the opt-in double statistics."""
    src, dst, _ = synth.make_icp_pair(n_points=60_000, seed=12, disp=(1.0, 3.0))
    grp = LC.LoopClosureGroup(LC.LoopClosureConfig(), n, devices=[0] * n, umeyama_float=mode)
    assert not grp.uses_rccl
    grp.setInputSource(src)
    grp.setInputTarget(dst)
    rg = grp.align()
    one = LC.LoopClosure(LC.LoopClosureConfig(), umeyama_float=mode)
    one.setInputSource(src)
    one.setInputTarget(dst)
    r1 = one.align()
    assert rg.iterations == r1.iterations >= 2 and rg.score == r1.score and rg.state == r1.state
    np.testing.assert_array_equal(np.array(list(rg.T)), np.array(list(r1.T)))
    np.testing.assert_array_equal(grp.aligned_, one.aligned_)


def test_icp_group_failure_is_reported_and_sticky():
    """A rank that fails mid-alignment (here: every rank, no target) releases the others (ADVICE r2:
    the communicators / barrier are torn down once), the group reports the rank's error, refuses later
    alignments, and is destroyed cleanly afterwards."""
    src, dst, _ = synth.make_icp_pair(n_points=20_000, seed=12, disp=(1.0, 3.0))
    grp = LC.LoopClosureGroup(LC.LoopClosureConfig(), 3, devices=[0, 0, 0])
    grp.setInputSource(src)
    with pytest.raises(LC._capi.LioError, match="rank"):
        grp.align()
    grp.setInputTarget(dst)
    with pytest.raises(LC._capi.LioError, match="failed earlier"):
        grp.align()
    grp.close()
    ok = LC.LoopClosureGroup(LC.LoopClosureConfig(), 3, devices=[0, 0, 0])  # a new group works
    ok.setInputSource(src)
    ok.setInputTarget(dst)
    assert ok.align().iterations >= 1
    ok.close()


@pytest.mark.skipif(LC._capi.lib().lio_device_count() < 2, reason="RCCL exchange needs two distinct devices")
def test_icp_group_rccl_bit_identical():
    src, dst, _ = synth.make_icp_pair(n_points=60_000, seed=12, disp=(1.0, 3.0))
    grp = LC.LoopClosureGroup(LC.LoopClosureConfig(), 2)
    assert grp.uses_rccl
    grp.setInputSource(src)
    grp.setInputTarget(dst)
    rg = grp.align()
    one = LC.LoopClosure(LC.LoopClosureConfig())
    one.setInputSource(src)
    one.setInputTarget(dst)
    r1 = one.align()
    assert rg.iterations == r1.iterations and rg.score == r1.score
    np.testing.assert_array_equal(np.array(list(rg.T)), np.array(list(r1.T)))


def _float_params(oracle, order=1):
    p = oracle.default_icp_params()
    p.umeyama_float = order
    return p


_FID_CASES = [(30_000, (1.0, 3.0)), (500_000, (0.3, 1.5)), (500_000, (2.5, 4.0))]


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("n,disp", _FID_CASES)
def test_icp_float_fidelity_matches_oracle(oracle, n, disp, order):
    """Float fidelity orders (lio_icp_params.umeyama_float; oracle UmeyamaOrder): pcl::umeyama's float means
    and sigma in the order of a given Eigen build — 1 sequential, 2 / 3 Eigen 3.3 GEMM blocking (32 / 48 KiB
    L1) — with the sequential float chains computed in parallel by seqsum (verified on the device) and
    the float JacobiSVD on the host: the transform bit-identical to the restatement (asserted, beside the 1e-5 bar),
    iterations / state identical, no serial fallback.  At 500 k (BASELINE configs[3], pairs A and B) this is
    the reference's float arithmetic at full size."""
    src, dst, _ = synth.make_icp_pair(n_points=n, seed=4321 if n > 100_000 else 12, disp=disp)
    lc = LC.LoopClosure(LC.LoopClosureConfig(), umeyama_float=order)
    lc.setInputSource(src)
    lc.setInputTarget(dst)
    r = lc.align(keep_aligned=False)
    o = oracle.icp_align(src, dst, params=_float_params(oracle, order))
    T = np.array(list(r.T), np.float32).reshape(4, 4)
    fs = lc.fidelity_stats()
    print(f"order {order} n={n} disp={disp}: iters {r.iterations} |dT|max {np.abs(T - o['T']).max():.3g} "
          f"bit-exact {np.array_equal(T, o['T'])} {fs}")
    assert r.iterations == o["iterations"] and r.state == o["state"]
    np.testing.assert_allclose(T, o["T"], atol=1e-5)
    assert np.array_equal(T, o["T"])
    np.testing.assert_allclose(r.score, o["fitness"], rtol=1e-5)
    assert fs["serial"] == 0 and fs["passes"] >= r.iterations


def test_icp_fidelity_recovery_paths(oracle):
    """The seqsum re-pass (a first pass that skips the grid-coarsening rule: verification fails, pass 2
    repairs), the serial fallback (event lists capped at 8) and a compaction look-back time-out (test hook:
    the pass re-compacts on the serial kernels) give the same transform bits as the normal path."""
    src, dst, _ = synth.make_icp_pair(n_points=60_000, seed=12, disp=(1.0, 3.0))
    out = {}
    for name, flags, evcap in (("normal", 0, 0), ("repass", 1, 0), ("serial", 0, 8), ("timeout", 4, 0)):
        lc = LC.LoopClosure(LC.LoopClosureConfig(), umeyama_float=2)
        lc.set_fidelity_debug(flags, evcap)
        lc.setInputSource(src)
        lc.setInputTarget(dst)
        r = lc.align(keep_aligned=False)
        out[name] = (np.array(list(r.T), np.float32), r.iterations, lc.fidelity_stats())
    assert out["repass"][2]["repasses"] > 0 and out["repass"][2]["serial"] == 0
    assert out["serial"][2]["serial"] > 0 and out["timeout"][2]["serial"] > 0
    for k in ("repass", "serial", "timeout"):
        np.testing.assert_array_equal(out[k][0], out["normal"][0])
        assert out[k][1] == out["normal"][1]


_POISON_REF = {}  # order -> (src, dst, the oracle's transform), computed once


def _poison_ref(oracle, order):
    if order not in _POISON_REF:
        src, dst, _ = synth.make_icp_pair(n_points=30_000, seed=12, disp=(1.0, 3.0))
        _POISON_REF[order] = (src, dst, oracle.icp_align(src, dst, params=_float_params(oracle, order))["T"])
    return _POISON_REF[order]


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("hook", [(4, 0), (0, 8)], ids=["timeout", "listcap"])
def test_icp_lookback_timeout_does_not_poison_the_handle(oracle, hook, order):
    """a compaction look-back time-out on one alignment (test hook) is cleared, so the next
    alignment on the same handle takes the parallel path again with the same transform bits.  ADVICE r06: so
    does an alignment after one whose event lists overflowed (capped at 8).  Either way the first alignment
    ends in the serial kernels, whose copy into the block the host polls must not be taken for the next pass's
    statistics (orders 2 / 3 copy the pack's output: lio_icp_policy.hpp Mailbox)."""
    src, dst, T_ref = _poison_ref(oracle, order)
    lc = LC.LoopClosure(LC.LoopClosureConfig(), umeyama_float=order)
    lc.setInputSource(src)
    lc.setInputTarget(dst)
    lc.set_fidelity_debug(*hook)
    r0 = lc.align(keep_aligned=False)
    s0 = lc.fidelity_stats()
    lc.set_fidelity_debug(0, 0)
    r1 = lc.align(keep_aligned=False)
    s1 = lc.fidelity_stats()
    print(f"hook {hook} order {order}: {s0} -> {s1}")
    assert s0["serial"] > 0  # the hook took the first alignment to the serial kernels
    assert s1["serial"] == s0["serial"]  # the second alignment never fell back
    np.testing.assert_array_equal(np.array(list(r0.T), np.float32), np.array(list(r1.T), np.float32))
    np.testing.assert_allclose(np.array(list(r1.T), np.float32).reshape(4, 4), T_ref, atol=1e-5)


@pytest.mark.parametrize("disp", [(0.3, 1.5), (2.5, 4.0)])
def test_icp_double_statistics_opt_in_bound_at_c4(oracle, disp):
    """The OPT-IN double statistics (LIO_ICP_UMEYAMA_DOUBLE; not the default, not parity-bearing) against the
    restated PCL float arithmetic at C4 (500 k vs 500 k).  The Eigen 3.3 float orders agree with each other to
    3.2e-6 (pair A) / 3.8e-5 (pair B) (tests/test_oracle.py, scripts/umeyama_spread.py); the double statistics
    sit 1.86e-4 / 1.2e-4 from them — outside the 1e-5 bar, which is why the default is float order 2
    (DESIGN §2).  Asserted: same iterations and state, and the documented bound of this opt-in mode (1e-3),
    which is NOT the parity bar (every default-path ICP test asserts 1e-5 against float order 2)."""
    src, dst, _ = synth.make_icp_pair(n_points=500_000, seed=4321, disp=disp)
    lc = LC.LoopClosure(LC.LoopClosureConfig(), umeyama_float=LC.DOUBLE_STATS)
    lc.setInputSource(src)
    lc.setInputTarget(dst)
    r = lc.align(keep_aligned=False)
    T = np.array(list(r.T), np.float32).reshape(4, 4)
    for order in (1, 2, 3):
        o = oracle.icp_align(src, dst, params=_float_params(oracle, order))
        gap = float(np.abs(T - o["T"]).max())
        print(f"C4 disp={disp}: double-mode vs float order {order} |dT|max {gap:.3g} "
              f"(rot {np.abs(T[:3, :3] - o['T'][:3, :3]).max():.3g}, trans {np.abs(T[:3, 3] - o['T'][:3, 3]).max():.3g})")
        assert r.iterations == o["iterations"] and r.state == o["state"]
        assert gap < 1e-3


@pytest.mark.parametrize("mode,world,debug", [(LC.FIDELITY_ORDER, 2, None), (LC.DOUBLE_STATS, 2, None),
                                               (LC.FIDELITY_ORDER, 3, None), (LC.DOUBLE_STATS, 3, None),
                                               (1, 2, None), (3, 3, None),
                                               (LC.FIDELITY_ORDER, 2, ("repass", 1, 0)),
                                               (LC.FIDELITY_ORDER, 3, ("serial", 0, 8)),
                                               (LC.FIDELITY_ORDER, 2, ("timeout", 4, 0))])
def test_icp_device_exchange_emulated_ranks(world, mode, debug):
    """The device-side exchange (lio_icp_set_shard_device + caller-owned exchange buffers, the form the
    RCCL paths use): `world` ranks as threads on the one GPU, the all-gather emulated with device copies
    between the ranks' torch buffers on each handle's own stream; the record-order sum runs on the
    device.  Every rank's transform, score and iterations equal the one-rank alignment bit for bit — in the
    sharded float orders 1-3 (the chains split over the ranks' windows) and through their
    recovery paths on every rank: re-passes after a failed verification, the serial fallback over the gathered
    pairs (event lists capped at 8), a compaction look-back time-out."""
    import threading

    import torch

    from lio_gpu import _capi, dist as ld

    src, dst, _ = synth.make_icp_pair(n_points=60_000, seed=12, disp=(1.0, 3.0))
    n = ld.exchange_len(len(src), world)
    dev = torch.device("cuda", 0)
    sends = [torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(world)]
    recvs = [torch.zeros(n * world, dtype=torch.float64, device=dev) for _ in range(world)]
    evs = [None] * world
    bar = threading.Barrier(world)

    def make_cb(rank):
        def cb(send_p, nn, recv_p, stream, user):
            try:
                # a pass's messages (records, block sums, event lists, depth blocks): nn <= the capacity
                assert send_p == sends[rank].data_ptr() and recv_p == recvs[rank].data_ptr() and 0 < nn <= n
                s = torch.cuda.ExternalStream(stream, device=dev)
                e = torch.cuda.Event()
                e.record(s)
                evs[rank] = e
                bar.wait()
                with torch.cuda.stream(s):
                    for k in range(world):
                        s.wait_event(evs[k])
                        recvs[rank][k * nn:(k + 1) * nn].copy_(sends[k][:nn])
                s.synchronize()  # emulation only: no rank's next pass overwrites a send being copied
                bar.wait()
                return 0
            except Exception:
                import traceback

                traceback.print_exc()
                return -1

        return _capi.ALLGATHER_DEV_FN(cb)

    cbs = [make_cb(r) for r in range(world)]
    lcs = [LC.LoopClosure(LC.LoopClosureConfig(), umeyama_float=mode) for _ in range(world)]
    results = [None] * world
    if debug:
        for lc in lcs:
            lc.set_fidelity_debug(debug[1], debug[2])

    def run(rank):
        h = lcs[rank]._h
        _capi.check(_capi.lib().lio_icp_set_shard_device(h, rank, world, cbs[rank], None))
        lcs[rank].setInputSource(src)
        _capi.check(_capi.lib().lio_icp_set_exchange_buffers(h, sends[rank].data_ptr(), recvs[rank].data_ptr(), n))
        lcs[rank].setInputTarget(dst)
        results[rank] = lcs[rank].align(keep_aligned=False)

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=300) for t in th]
    one = LC.LoopClosure(LC.LoopClosureConfig(), umeyama_float=mode)
    one.setInputSource(src)
    one.setInputTarget(dst)
    r1 = one.align(keep_aligned=False)
    assert r1.iterations >= 2
    for r in results:
        assert r is not None
        np.testing.assert_array_equal(np.array(list(r.T), np.float32), np.array(list(r1.T), np.float32))
        assert r.score == r1.score and r.iterations == r1.iterations and r.state == r1.state
    if debug:
        fs = [lc.fidelity_stats() for lc in lcs]
        print(debug[0], fs)
        key = "repasses" if debug[0] == "repass" else "serial"
        assert all(f[key] > 0 for f in fs) and len({f[key] for f in fs}) == 1  # every rank took the same path


@pytest.mark.parametrize("mode", [LC.DOUBLE_STATS, LC.FIDELITY_ORDER], ids=["records", "sharded-float"])
def test_icp_failing_host_allgather_is_reported(mode):
    """A host all-gather callback that returns non-zero and leaves no message of its own: the alignment fails
    with "allgather callback failed" (the text callers match; a callee's own message would follow it), through
    both host forms of the exchange: the records alone (double statistics) and the staged device buffers (the
    sharded float orders).  Two ranks as threads, both callbacks failing in their first call, so no rank waits
    for a peer."""
    import threading

    from lio_gpu import _capi

    src, dst, _ = synth.make_icp_pair(n_points=8_000, seed=3)
    world = 2
    calls = [0] * world
    errors = [None] * world

    def make_cb(rank):
        def cb(send_p, n, recv_p, user):
            calls[rank] += 1
            return -1

        return _capi.ALLGATHER_FN(cb)

    cbs = [make_cb(r) for r in range(world)]
    lcs = [LC.LoopClosure(LC.LoopClosureConfig(), umeyama_float=mode) for _ in range(world)]

    def run(rank):
        lcs[rank].set_shard(rank, world, cbs[rank])
        lcs[rank].setInputSource(src)
        lcs[rank].setInputTarget(dst)
        try:
            lcs[rank].align(keep_aligned=False)
        except _capi.LioError as e:
            errors[rank] = e

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=120) for t in th]
    for r in range(world):
        assert calls[r] == 1 and errors[r] is not None, (r, calls[r], errors[r])
        assert errors[r].code == _capi.LIO_ERR_STATE
        assert "allgather callback failed" in str(errors[r])
        assert str(errors[r]).endswith("allgather callback failed")  # nothing appended: the callee said nothing
