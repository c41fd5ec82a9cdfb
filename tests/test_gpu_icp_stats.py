"""The loop ICP's float statistics (pcl::umeyama's means and sigma, orders 1-3) with rejected pairs and small counts.

Every case here has correspondences that are REJECTED (max_corr_dist 2 m against far points 40 m away), so the
compaction of the accepted pairs in source order (icp_stats_kernel: 1024-point slab counts, the look-back over
the 4096-point records) sees empty, partial and full slabs and records, and pair counts at every threshold the
statistics branch on: fewer than 3 pairs (state 5), the lazy product below 14 pairs, one depth block up to
kc, the change of kc just above max_kc, a `% 8` tail, and more depth blocks than one staging window of
pcl_pack.  Sharded, the windows hold zero, two or thousands of accepted pairs, a rank may own no source
point at all, and a depth block may start two ranks before the one it ends in.

The references are independent of the library: tests/icp_stats_ref.py (numpy only: brute-force 1-NN, the
acceptance rule, the 16 floats of a pass) and the oracle (umeyama_float on the brute-force pairs, and
icp_align with its own kd-tree).  Everything is compared bit for bit (as uint32) except the double MSE
(any-order sum of fewer than 1e6 positive terms: rtol 1e-9) and the fitness score (the suite's rtol 1e-5).
Every case asserts its own precondition from the reference mask before it looks at the GPU.

One pass per alignment (identity guess, max_iter = 1): the statistics are those of the raw source and T is the
one incremental transform.  test_partial_acceptance_many_iterations runs the default 50.
"""
import functools

import numpy as np
import pytest

import icp_stats_ref as R
from lio_gpu import dist as ld
from lio_gpu import loop_closure as LC
from lio_gpu import synth

pytestmark = pytest.mark.gpu

REC = 4096  # points per record; a slab is 1024 of them
MAX_CORR = 2.0
IDENTITY = np.eye(4, dtype=np.float32)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def _target():
    rng = np.random.default_rng(11)
    cube = rng.uniform(-6, 6, (3000, 3))
    return _frozen(np.concatenate([cube, [[100.0, 0.0, 0.0]]]).astype(np.float32))[0]


def _make_source(near, rng):
    """near[i]: a random cube point + uniform(-0.3, 0.3)^3 (its NN within 0.52 m); else that + (40, 0, 0) (its NN
    beyond 28 m)"""
    tgt = _target()
    n = len(near)
    src = tgt[rng.integers(0, 3000, n)].astype(np.float64) + rng.uniform(-0.3, 0.3, (n, 3))
    src[~near, 0] += 40.0
    return src.astype(np.float32)


def _reference(src, tgt, max_corr):
    ids, d2 = R.brute_nn(src, tgt)
    return ids, d2, R.accepted(d2, max_corr)


@functools.lru_cache(maxsize=None)
def _case_a():
    """5 records + a 777-point tail: all far | all near | near with p = 0.5 | near at the first and last point |
    slabs 0 and 2 near, 1 and 3 far | tail near with p = 0.3, with the two boundary points in it"""
    rng = np.random.default_rng(11)
    n = 5 * REC + 777
    near = np.zeros(n, bool)
    near[1 * REC:2 * REC] = True
    near[2 * REC:3 * REC] = rng.random(REC) < 0.5
    near[3 * REC] = near[4 * REC - 1] = True
    near[4 * REC:4 * REC + 1024] = True
    near[4 * REC + 2048:4 * REC + 3072] = True
    near[5 * REC:] = rng.random(777) < 0.3
    src = _make_source(near, rng)
    ia, ir = 5 * REC + 300, 5 * REC + 301
    src[ia] = (102.0, 0.0, 0.0)  # d2 = 4.0 = max_d2 from the lone target point: accepted
    src[ir] = (100.0, 0.0, np.nextafter(np.float32(2), np.float32(3)))  # one ulp beyond: rejected
    near[ia], near[ir] = True, False
    ids, d2, acc = _reference(src, _target(), MAX_CORR)
    return _frozen(src, near, ids, d2, acc) + (ia, ir)


def _small_source(m, layout):
    """3 records + 5 points with exactly m near points.  spread: for m >= 2 one at index 0 and one in the tail
    record, the rest anywhere; last: all of them in the last two records (world 3's last window)"""
    rng = np.random.default_rng(7000 + m + (100_000 if layout == "last" else 0))
    n = 3 * REC + 5
    near = np.zeros(n, bool)
    if layout == "last":
        near[2 * REC + rng.choice(n - 2 * REC, m, replace=False)] = True
    elif m == 1:
        near[rng.integers(0, n)] = True
    elif m >= 2:
        near[0] = True
        near[3 * REC + rng.integers(0, 5)] = True
        free = np.flatnonzero(~near)
        near[rng.choice(free, m - 2, replace=False)] = True
    return _make_source(near, rng), near


@functools.lru_cache(maxsize=None)
def _small_case(m, layout):
    src, near = _small_source(m, layout)
    ids, d2, acc = _reference(src, _target(), MAX_CORR)
    return _frozen(src, near, ids, d2, acc)


def _config(max_corr=MAX_CORR):
    cfg = LC.LoopClosureConfig()
    cfg.icp_max_corr_dist_ = max_corr
    return cfg


def _oracle_params(oracle, order, max_corr, max_iter):
    p = oracle.default_icp_params()
    p.umeyama_float = order
    p.max_corr_dist = max_corr
    p.max_iter = max_iter
    return p


def _T(res):
    return np.array(list(res.T), np.float32).reshape(4, 4)


def _align(lc, src, tgt):
    lc.setInputSource(src)
    lc.setInputTarget(tgt)
    return lc.align(guess=IDENTITY)


def _check_one_pass(oracle, lc, res, src, tgt, ids, d2, acc, order, max_corr=MAX_CORR):
    """a one-pass alignment (identity guess, max_iter 1) against the numpy statistics and both oracle references"""
    m = int(acc.sum())
    ps, qs = src[acc], tgt[ids[acc]]
    o = oracle.icp_align(src, tgt, params=_oracle_params(oracle, order, max_corr, 1))
    np.testing.assert_array_equal(_u32(lc.umeyama_stats()), _u32(R.stats16(ps, qs, order)))
    T = _T(res)
    assert res.last_corr == m
    assert res.iterations == o["iterations"] and res.state == o["state"]
    if m < 3:
        assert res.state == 5 and res.iterations == 0 and not res.is_converged and not res.is_valid
        np.testing.assert_array_equal(_u32(T), _u32(IDENTITY))
        np.testing.assert_array_equal(_u32(o["T"]), _u32(IDENTITY))
    else:
        assert res.iterations == 1 and res.state == 1 and res.is_converged
        np.testing.assert_array_equal(_u32(T), _u32(oracle.umeyama_float(ps, qs, order)))
        np.testing.assert_array_equal(_u32(T), _u32(o["T"]))
        assert o["trace"][0][0] == m
        np.testing.assert_allclose(res.last_mse, d2[acc].astype(np.float64).sum() / m, rtol=1e-9)
    np.testing.assert_allclose(res.score, o["fitness"], rtol=1e-5)
    assert lc.fidelity_stats()["serial"] == 0


def _assert_group_equals_one(rg, grp, r1, one):
    assert rg.iterations == r1.iterations and rg.state == r1.state and rg.score == r1.score
    assert rg.last_corr == r1.last_corr and rg.is_converged == r1.is_converged and rg.is_valid == r1.is_valid
    np.testing.assert_array_equal(_u32(_T(rg)), _u32(_T(r1)))
    np.testing.assert_array_equal(_u32(grp.aligned_), _u32(one.aligned_))


# ------------------------------------------------------------------ a. rejected pairs, one rank
def _per_record(acc):
    return [int(acc[k:k + REC].sum()) for k in range(0, len(acc), REC)]


def _assert_case_a_precondition():
    src, near, ids, d2, acc, ia, ir = _case_a()
    np.testing.assert_array_equal(acc, near)
    c = _per_record(acc)
    assert len(c) == 6 and c[0] == 0 and c[1] == REC and 0 < c[2] < REC and c[3] == 2 and c[4] == 2048
    assert 0 < c[5] < 777
    for k in range(4):  # record 4: slabs 0 and 2 full, 1 and 3 empty; record 1: every slab count exactly 1024
        assert int(acc[4 * REC + 1024 * k:4 * REC + 1024 * (k + 1)].sum()) == (1024 if k % 2 == 0 else 0)
        assert int(acc[REC + 1024 * k:REC + 1024 * (k + 1)].sum()) == 1024
    assert acc[3 * REC] and acc[4 * REC - 1]
    assert acc[ia] and d2[ia] == np.float32(4.0) and ids[ia] == 3000  # equality is accepted
    assert not acc[ir] and d2[ir] > np.float32(4.0) and ids[ir] == 3000


@pytest.mark.parametrize("order", [1, 2, 3])
def test_rejected_pairs_one_rank(oracle, order):
    """Empty, full, half-full, two-pair and alternating-slab records in one source; d2 == max_d2 kept, one ulp
    more dropped."""
    _assert_case_a_precondition()
    src, near, ids, d2, acc, _, _ = _case_a()
    lc = LC.LoopClosure(_config(), umeyama_float=order, max_iter=1)
    res = _align(lc, src, _target())
    _check_one_pass(oracle, lc, res, src, _target(), ids, d2, acc, order)
    lc.close()


# ------------------------------------------------------------------ b. small counts, one handle per order
_SMALL_M = [0, 1, 2, 3, 4, 13, 14, 15, 47, 48, 49, 679, 680, 681, 1016, 1017, 1361]
# (order, m, id) in running order: each order's handle sees its counts ascending, then 14 once more after the largest
_SMALL_RUNS = [(1, m, f"o1-m{m}") for m in (3, 13, 14, 681)] + [(1, 14, "o1-m14-after-681")]
for _o in (2, 3):
    _SMALL_RUNS += [(_o, m, f"o{_o}-m{m}") for m in _SMALL_M] + [(_o, 14, f"o{_o}-m14-after-1361")]


@pytest.fixture(scope="module")
def handle_of_order():
    made = {}

    def get(order):
        if order not in made:
            made[order] = LC.LoopClosure(_config(), umeyama_float=order, max_iter=1)
        return made[order]

    yield get
    for lc in made.values():
        lc.close()


@pytest.mark.parametrize("order,m", [(o, m) for o, m, _ in _SMALL_RUNS], ids=[i for _, _, i in _SMALL_RUNS])
def test_small_counts(oracle, handle_of_order, order, m):
    """Exactly m accepted pairs among 12 293 source points, on ONE handle per order reused through the whole
    list (a stale depth block, count or ticket of a larger pass must not leak into a smaller one): state 5
    below 3 pairs, the lazy product up to 13, one depth block up to max_kc (680 / 1016), the smaller kc just
    above it, block tails that are no multiple of 8."""
    src, near, ids, d2, acc = _small_case(m, "spread")
    np.testing.assert_array_equal(acc, near)
    assert int(acc.sum()) == m
    if m >= 2:
        assert acc[0] and acc[3 * REC:].sum() >= 1
    if order != 1 and m + 6 >= 20:
        kc, max_kc = R.eigen_gemm_kc(m, R.L1_OF_ORDER[order]), (680 if order == 2 else 1016)
        assert (kc == m) == (m <= max_kc) and (m <= max_kc or kc < max_kc)
    lc = handle_of_order(order)
    res = _align(lc, src, _target())
    _check_one_pass(oracle, lc, res, src, _target(), ids, d2, acc, order)


# ------------------------------------------------------------------ c. more depth blocks than one pack window
@functools.lru_cache(maxsize=None)
def _case_c():
    rng = np.random.default_rng(11)
    g = np.arange(4) * 2.0 - 3.0
    tgt = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    n = 696_999
    src = (tgt[rng.integers(0, 64, n)].astype(np.float64) + rng.uniform(-0.3, 0.3, (n, 3))).astype(np.float32)
    ids, d2, acc = _reference(src, tgt, 52.5)
    return _frozen(src, tgt, ids, d2, acc)


@pytest.mark.parametrize("order", [2, 3])
def test_pack_second_window(oracle, order):
    """696 999 accepted pairs: 1025 depth blocks at order 2 — one more than pcl_pack stages per window (1024) —
    and 687 at order 3 (the control on the same input).  Also the suite's only source above 129 records
    (528 384 points), the floor of the pinned record buffer: its capacity has to follow the source."""
    src, tgt, ids, d2, acc = _case_c()
    assert acc.all()
    assert R.n_blocks(len(src), 2) == 1025 > 1024 and R.n_blocks(len(src), 3) == 687
    lc = LC.LoopClosure(LC.LoopClosureConfig(), umeyama_float=order, max_iter=1)
    res = _align(lc, src, tgt)
    _check_one_pass(oracle, lc, res, src, tgt, ids, d2, acc, order, max_corr=52.5)
    lc.close()


# ------------------------------------------------------------------ d. rejected pairs, sharded
def _windows(ns, world, acc):
    """per rank: (first source index, source points, accepted pairs, accepted pairs before the window)"""
    out, before = [], 0
    for r in range(world):
        b, n = ld.shard_range(ns, r, world)
        c = int(acc[b:b + n].sum())
        out.append((b, n, c, before))
        before += c
    return out


def _block_spans_three_ranks(win, total, kc):
    """a depth block [q kc, (q + 1) kc) that holds a middle rank's whole (non-empty) accepted range and pairs of
    ranks on both sides of it"""
    for r in range(1, len(win) - 1):
        _, _, c, gb = win[r]
        if c == 0:
            continue
        q = gb // kc
        if q * kc < gb and gb + c < min((q + 1) * kc, total):
            return True
    return False


@pytest.mark.parametrize("world,order", [(2, 2), (3, 2), (4, 2), (8, 2), (4, 1), (4, 3)])
def test_rejected_pairs_group(oracle, world, order):
    """Case a's source over `world` ranks (threads on one device, the exchange through host memory): windows
    with 0 and 2 accepted pairs, a depth block spanning three ranks, ranks without source points."""
    _assert_case_a_precondition()
    src, near, ids, d2, acc, _, _ = _case_a()
    win = _windows(len(src), world, acc)
    assert sum(n for _, n, _, _ in win) == len(src)
    if world == 4:
        counts = [c for _, _, c, _ in win]
        assert 0 in counts and 2 in counts
        if order != 1:
            total = int(acc.sum())
            assert _block_spans_three_ranks(win, total, R.eigen_gemm_kc(total, R.L1_OF_ORDER[order]))
    if world == 8:
        assert any(n == 0 for _, n, _, _ in win)
    one = LC.LoopClosure(_config(), umeyama_float=order, max_iter=1)
    r1 = _align(one, src, _target())
    _check_one_pass(oracle, one, r1, src, _target(), ids, d2, acc, order)
    grp = LC.LoopClosureGroup(_config(), world, devices=[0] * world, umeyama_float=order, max_iter=1)
    assert not grp.uses_rccl
    grp.setInputSource(src)
    grp.setInputTarget(_target())
    rg = grp.align(guess=IDENTITY)
    _assert_group_equals_one(rg, grp, r1, one)
    grp.close()
    one.close()


@pytest.mark.parametrize("layout", ["spread", "last"])
@pytest.mark.parametrize("m", [2, 13, 14, 700])
def test_small_counts_group(oracle, m, layout):
    """Small counts over 3 ranks at order 2: too few pairs, the lazy product across ranks (from the gathered
    heads), one depth block and two — with the pairs spread over the windows, and all in the last one."""
    src, near, ids, d2, acc = _small_case(m, layout)
    np.testing.assert_array_equal(acc, near)
    assert int(acc.sum()) == m
    counts = [c for _, _, c, _ in _windows(len(src), 3, acc)]
    if layout == "last":
        assert counts == [0, 0, m]
    elif m == 2:
        assert counts == [1, 0, 1]
    else:
        assert min(counts) >= 1
    one = LC.LoopClosure(_config(), umeyama_float=2, max_iter=1)
    r1 = _align(one, src, _target())
    _check_one_pass(oracle, one, r1, src, _target(), ids, d2, acc, 2)
    grp = LC.LoopClosureGroup(_config(), 3, devices=[0, 0, 0], umeyama_float=2, max_iter=1)
    grp.setInputSource(src)
    grp.setInputTarget(_target())
    rg = grp.align(guess=IDENTITY)
    _assert_group_equals_one(rg, grp, r1, one)
    grp.close()
    one.close()


# ------------------------------------------------------------------ e. partial acceptance over several iterations
def _xform(T, p):
    """the restatement's point transform in float32: a + (b + (c + t)) per row"""
    T = np.asarray(T, np.float32).reshape(4, 4)
    p = np.asarray(p, np.float32)
    cols = []
    for r in range(3):
        a, b, c = T[r, 0] * p[:, 0], T[r, 1] * p[:, 1], T[r, 2] * p[:, 2]
        cols.append(a + (b + (c + T[r, 3])))
    return np.stack(cols, 1)


@pytest.mark.parametrize("order", [1, 2, 3])
def test_partial_acceptance_many_iterations(oracle, order):
    """Two samples of one street 1 m / 3 deg apart with max_corr_dist 0.6 m: a different subset of the source is
    accepted in every iteration.  The last pass's statistics are rebuilt from the oracle's trace (its incremental
    transforms applied to the source in float32, brute-force 1-NN, the acceptance rule)."""
    src, dst, _ = synth.make_icp_pair(20_000, seed=5, disp=(1.0, 3.0))
    o = oracle.icp_align(src, dst, params=_oracle_params(oracle, order, 0.6, 50))
    counts = [int(t[0]) for t in o["trace"]]
    assert o["iterations"] == len(counts) >= 2 and len(set(counts)) > 1 and max(counts) < len(src)
    cur = np.ascontiguousarray(src, dtype=np.float32)
    for t in o["trace"][:-1]:
        cur = _xform(t[2:18], cur)
    ids, d2 = R.brute_nn(cur, dst)
    acc = R.accepted(d2, 0.6)
    assert int(acc.sum()) == counts[-1]
    lc = LC.LoopClosure(_config(0.6), umeyama_float=order)
    lc.setInputSource(src)
    lc.setInputTarget(dst)
    res = lc.align()
    assert res.iterations == o["iterations"] and res.state == o["state"]
    np.testing.assert_array_equal(_u32(_T(res)), _u32(o["T"]))
    assert res.last_corr == counts[-1]
    np.testing.assert_array_equal(_u32(lc.umeyama_stats()), _u32(R.stats16(cur[acc], dst[ids[acc]], order)))
    np.testing.assert_allclose(res.score, o["fitness"], rtol=1e-5)
    assert lc.fidelity_stats()["serial"] == 0
    grp = LC.LoopClosureGroup(_config(0.6), 3, devices=[0, 0, 0], umeyama_float=order)
    grp.setInputSource(src)
    grp.setInputTarget(dst)
    rg = grp.align()
    _assert_group_equals_one(rg, grp, res, lc)
    grp.close()
    lc.close()
