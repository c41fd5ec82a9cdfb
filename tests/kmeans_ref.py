"""The contract of lio_kmeans (include/lio_gpu.h) restated in numpy and Python integers: the two scales, the
counter-based draws, the k-means++ seeding with three trials, Lloyd with the empty-cluster repair, the best
attempt.  Float32 arithmetic is numpy's float32 in the written order (numpy does not contract); every sum is an
integer sum.  tests/test_kmeans_ref.py checks this file against its own properties and scikit-learn,
tests/test_gpu_kmeans.py checks the library against it bit for bit."""
import math

import numpy as np

M64 = 2**64 - 1
F32 = np.float32


def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, c):
    return _mix((seed + (c + 1) * 0x9E3779B97F4A7C15) & M64)


def uniform_cloud(n, seed=12345, half=40.0, stride=3):
    """n x stride float32, every coordinate uniform in [-half, half) on a 2^-24 grid from the draws above (no
    library generator: the recorded figures of the tests depend on nothing else); z is scaled by 0.1"""
    c = np.arange(1, 3 * n + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + c * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(np.float64) / 2.0**24
    xyz = ((u * 2.0 - 1.0) * half).reshape(n, 3) * np.array([1.0, 1.0, 0.1])
    out = np.zeros((n, stride), F32)
    out[:, :3] = xyz
    for d in range(3, stride):
        out[:, d] = np.arange(n) % 97 + d
    return out


def blobs(n=4097, k=5, sigma=1.0, seed=1, stride=3, origin=(0.0, 0.0, 0.0)):
    """k Gaussian blobs of n points in all: centres uniform in +-40 m (z x 0.1) about `origin`, float32"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-40.0, 40.0, (k, 3)) * np.array([1.0, 1.0, 0.1])
    who = rng.integers(0, k, n)
    out = np.zeros((n, stride), F32)
    out[:, :3] = centres[who] + sigma * rng.normal(size=(n, 3)) + np.asarray(origin)
    for d in range(3, stride):
        out[:, d] = np.arange(n) % 97 + d
    return out


def ord_of(v):
    """float32 -> uint32 keys whose unsigned order is the float order (-0 below +0)"""
    b = np.ascontiguousarray(v, F32).view(np.uint32)
    return np.where(b >> 31 != 0, b ^ np.uint32(0xFFFFFFFF), b ^ np.uint32(0x80000000)).astype(np.uint32)


def ord_to(k):
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31 != 0, k ^ np.uint32(0x80000000), k ^ np.uint32(0xFFFFFFFF)).astype(np.uint32).view(F32)


def box_of(P):
    """float min x, y, z, max x, y, z through the order-preserving map (so -0 < +0, as the device's atomics see it)"""
    k = ord_of(P)
    return np.concatenate([ord_to(k.min(0)), ord_to(k.max(0))])


def scales(P):
    """(ec, ed) of the finite points P (m x 3 float32)"""
    box = box_of(P)
    lo, hi = box[:3], box[3:]
    A = float(max(np.abs(lo).max(), np.abs(hi).max()))
    ec = math.frexp(A)[1] if A != 0.0 else 0
    with np.errstate(over="ignore"):
        e = hi - lo
        D2 = F32(F32(e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    if not np.isfinite(D2):
        raise ValueError("the squared diagonal of the box is not a finite float")
    ed = math.frexp(float(D2))[1] if D2 != 0 else 0
    return ec, ed


def quant_x(P, ec):
    return np.rint(P.astype(np.float64) * math.ldexp(1.0, 31 - ec)).astype(np.int64)


def quant_d(d, ed):
    return np.floor(np.asarray(d, F32).astype(np.float64) * math.ldexp(1.0, 31 - ed)).astype(np.uint64)


def d2(P, c):
    """float32 ((dx dx + dy dy) + dz dz) of the rows of P to c"""
    c = np.asarray(c, F32)
    with np.errstate(over="ignore"):
        dx, dy, dz = P[:, 0] - c[0], P[:, 1] - c[1], P[:, 2] - c[2]
        return (dx * dx + dy * dy) + dz * dz


def assign(P, C):
    """strict < over ascending k: the lowest k wins a tie (argmin returns the first minimum)"""
    D = np.stack([d2(P, c) for c in C])
    return np.argmin(D, axis=0).astype(np.int32)


def mean_of(S, cnt, ec):
    return np.array([F32((float(int(s)) / float(int(cnt))) * math.ldexp(1.0, ec - 31)) for s in S], F32)


def seed_attempt(P, seed, a, K, ed):
    """the k-means++ indices (into the finite points P) of attempt a"""
    nf = len(P)
    out = [draw(seed, (a * K) * 3) % nf]
    w = quant_d(d2(P, P[out[0]]), ed)
    for k in range(1, K):
        sum0 = int(w.sum(dtype=np.uint64))
        best = None
        for j in range(3):
            u = draw(seed, (a * K + k) * 3 + j) >> 11
            t = (u * sum0) >> 53
            if sum0 == 0:
                ci = 0
            else:
                ci = int(np.searchsorted(np.cumsum(w, dtype=np.uint64), np.uint64(t), side="right"))
            w2 = np.minimum(quant_d(d2(P, P[ci]), ed), w)
            s = int(w2.sum(dtype=np.uint64))
            if best is None or s < best[0]:
                best = (s, ci, w2)
        out.append(best[1])
        w = best[2]
    return out


def lloyd(P, Q, C, max_iter, eps, ec, ed):
    """One attempt from the centres C (K x 3 float32) -> labels, centres, counts, cq, it, repairs"""
    K = len(C)
    C = np.array(C, F32)
    eps2 = float(F32(eps)) * float(F32(eps))
    labels = assign(P, C)
    it, repairs = 1, 0
    while True:
        cnt = np.bincount(labels, minlength=K).astype(np.int64)
        S = np.zeros((K, 3), np.int64)
        for d in range(3):
            # exact: |q| <= 2^31 and fewer than 2^31 points; add.at keeps int64
            np.add.at(S[:, d], labels, Q[:, d])
        for k in range(K):
            if cnt[k]:
                continue
            mk = int(np.argmax(cnt))  # the first maximum: the lowest index among equals
            members = np.flatnonzero(labels == mk)
            i = int(members[np.argmax(d2(P[members], mean_of(S[mk], cnt[mk], ec)))])  # the lowest index among equals
            labels[i] = k
            S[mk] -= Q[i]
            S[k] = Q[i]
            cnt[mk] -= 1
            cnt[k] = 1
            repairs += 1
        new = np.stack([mean_of(S[k], cnt[k], ec) for k in range(K)])
        t = (new - C).astype(np.float64)
        shift = float(((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]).max())
        C = new
        it += 1
        if it == max(max_iter, 2) or shift <= eps2:
            break
        labels = assign(P, C)
    cq = 0
    for k in range(K):
        cq += int(quant_d(d2(P[labels == k], C[k]), ed).sum(dtype=np.uint64))
    return labels, C, cnt, cq, it, repairs


def kmeans(pts, K=5, max_iter=100, eps=0.1, attempts=3, seed=0, init_centers=None):
    """dict of everything lio_kmeans returns, plus ``per_attempt`` (labels and centres of every attempt)."""
    pts = np.ascontiguousarray(pts, F32)
    pts = pts.reshape(len(pts), -1)
    n = len(pts)
    fin = np.isfinite(pts[:, :3]).all(1)
    idx = np.flatnonzero(fin)
    nf = len(idx)
    if nf < K:
        raise ValueError("fewer finite points than clusters")
    P = np.ascontiguousarray(pts[idx, :3])
    ec, ed = scales(P)
    Q = quant_x(P, ec)
    seeds = np.full((attempts, K), -1, np.int32)
    attempt_q, attempt_iters, per_attempt = [], [], []
    best, repairs = None, 0
    for a in range(attempts):
        if init_centers is not None:
            C0 = np.asarray(init_centers, F32).reshape(attempts, K, 3)[a]
        else:
            s = seed_attempt(P, seed & M64, a, K, ed)
            seeds[a] = idx[s]
            C0 = P[s]
        lab, C, cnt, cq, it, rep = lloyd(P, Q, C0, max_iter, eps, ec, ed)
        repairs += rep
        attempt_q.append(cq)
        attempt_iters.append(it)
        full = np.full(n, -1, np.int32)
        full[idx] = lab
        per_attempt.append((full, C))
        if best is None or cq < best[0]:
            best = (cq, a, full, C, cnt, it)
    cq, a, labels, C, cnt, it = best
    aabb = np.stack([box_of(pts[labels == k, :3]) for k in range(K)]).astype(F32)
    return dict(labels=labels, centers=C, compactness=math.ldexp(float(cq), ed - 31), counts=cnt.astype(np.int64),
                aabb=aabb, seeds=seeds, attempt_q=np.array(attempt_q, np.uint64),
                attempt_iters=np.array(attempt_iters, np.int32),
                stats=np.array([nf, a, it, repairs, ec, ed], np.int64), per_attempt=per_attempt)
