"""Plain numpy restatement of the loop ICP's float statistics (pcl::umeyama's means and sigma).

Test infrastructure only.  It calls neither the oracle nor the library, so a test can hold both against
it: the exact float32 1-NN, the acceptance rule, Eigen 3.3's GEMM depth blocking and the 16 floats a
correspondence pass hands to the host Umeyama (include/lio_gpu.h lio_icp_get_umeyama_stats).  numpy's
float32 arithmetic is one rounding per operation (no FMA) and np.cumsum(dtype=float32) is a sequential
chain from the first element, which is what Eigen's redux and gebp's 1 x 1 path do.
"""
import numpy as np

F32 = np.float32


def brute_nn(q, t):
    """exact 1-NN under (d2, id), float32 d2 in the reference's operation order."""
    q = np.asarray(q, np.float32)
    t = np.asarray(t, np.float32)
    ids = np.empty(len(q), np.int32)
    d2 = np.empty(len(q), np.float32)
    for s in range(0, len(q), 2048):
        qq = q[s:s + 2048]
        dx = qq[:, None, 0] - t[None, :, 0]
        dy = qq[:, None, 1] - t[None, :, 1]
        dz = qq[:, None, 2] - t[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz  # float32 throughout, no FMA
        j = np.argmin(d, axis=1)  # first index of the minimum = lowest id among ties
        ids[s:s + 2048] = j
        d2[s:s + 2048] = d[np.arange(len(qq)), j]
    return ids, d2


def accepted(d2, max_corr_dist):
    """the correspondence rejection: a pair is dropped when (double) d2 > max_corr_dist^2 — equality stays"""
    return ~(np.asarray(d2).astype(np.float64) > float(max_corr_dist) * float(max_corr_dist))


L1_OF_ORDER = {2: 32 * 1024, 3: 48 * 1024}


def eigen_gemm_kc(k, l1):
    """Eigen 3.3 evaluateProductBlockingSizesHeuristic for a 3 x k by k x 3 float GEMM, one thread, SSE2
    (mr 8, nr 4, no FMA): the depth block.  Depths below 48 are not blocked."""
    k = int(k)
    mr, nr, k_peeling = 8, 4, 8
    k_div, k_sub = mr * 4 + nr * 4, mr * nr * 4
    if max(k, 3) < 48:
        return k
    max_kc = max(((int(l1) - k_sub) // k_div) & ~(k_peeling - 1), 1)
    if k > max_kc:
        if k % max_kc == 0:
            return max_kc
        return max_kc - k_peeling * ((max_kc - 1 - (k % max_kc)) // (k_peeling * (k // max_kc + 1)))
    return k


def n_blocks(n, order):
    kc = eigen_gemm_kc(n, L1_OF_ORDER[order])
    return -(-int(n) // kc)


def _chain(x):
    """sequential float32 sum of the rows of x, from the first row"""
    return np.cumsum(x, axis=0, dtype=np.float32)[-1]


def stats16(src_acc, tgt_acc, order):
    """[sum src xyz, sum tgt xyz, count (uint32 bits), sigma 9 row-major target x source]: order 1 the raw
    sequential accumulator, orders 2 / 3 scaled by 1/n as Eigen's product leaves it"""
    src = np.ascontiguousarray(src_acc, dtype=np.float32).reshape(-1, 3)
    tgt = np.ascontiguousarray(tgt_acc, dtype=np.float32).reshape(-1, 3)
    n = len(src)
    assert len(tgt) == n and order in (1, 2, 3)
    out = np.zeros(16, np.float32)
    out[6:7] = np.array([n], np.uint32).view(np.float32)
    if n == 0:
        return out
    out[0:3] = _chain(src)
    out[3:6] = _chain(tgt)
    oon = F32(1) / F32(n)
    sm = out[0:3] * oon
    dm = out[3:6] * oon
    dt = tgt - dm  # float32 (n, 3)
    ds = src - sm
    if order == 1:
        out[7:16] = _chain((dt[:, :, None] * ds[:, None, :]).reshape(n, 9))
    elif n + 6 < 20:  # the lazy coefficient-based product: (alpha * dst_demean).row(r) . src_demean.row(c)
        out[7:16] = _chain(((oon * dt)[:, :, None] * ds[:, None, :]).reshape(n, 9))
    else:
        kc = eigen_gemm_kc(n, L1_OF_ORDER[order])
        prod = (dt[:, :, None] * ds[:, None, :]).reshape(n, 9)
        res = np.zeros(9, np.float32)
        zero = np.zeros((1, 9), np.float32)
        for k0 in range(0, n, kc):
            cb = _chain(np.concatenate([zero, prod[k0:k0 + kc]]))  # C0 = 0; C0 += a * b
            res = res + oon * cb
        out[7:16] = res
    return out
