// lio_normals_math.hpp — the arithmetic of lio_estimate_normals (include/lio_gpu.h) after the neighbour search:
// the quantisation scale, one neighbour's contribution to the ten integer sums, the covariance M, the Jacobi
// eigen-iteration, the pick of the smallest eigenvalue and the orientation.  ONE text for the device
// (lio_normals.hip) and a host build (tests/cpp/normals_math.cpp compiles it with g++): every operation is an
// IEEE + - * / sqrt, rint, frexp or ldexp in the written order, so both give the same bits without contraction
// (-ffp-contract=off on either side).  No HIP header is needed.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LIO_NM_HD __host__ __device__ __forceinline__
#else
#define LIO_NM_HD inline
#endif

namespace lio {

// the integer moments of one neighbourhood: S_a = sum q_a, S_ab = sum q_a q_b (xx, xy, xz, yy, yz, zz), exact
// in int64 for every n < 2^31 (|q_a| <= 2^15)
struct NmSums {
    int64_t s[3] = {0, 0, 0};
    int64_t ss[6] = {0, 0, 0, 0, 0, 0};
};

struct NmResult {
    float n[3];
    float curvature;
    bool ok;  // false: degenerate (n and curvature are NaN)
};

LIO_NM_HD float nm_nan() { return __builtin_nanf(""); }

// s = 2^(15 - h), h = ceil(e / 2), (mant, e) = frexp((double)B): |o_a| <= sqrt(B) < 2^h, so |o_a s| < 2^15
LIO_NM_HD double nm_scale(float B) {
    int e = 0;
    (void)frexp((double)B, &e);
    const int h = (e + 1) >> 1;  // ceil(e / 2) for either sign (arithmetic shift)
    return ldexp(1.0, 15 - h);
}

// one neighbour: o = p_j - p_i in float, q_a = (int64) rint((double)o_a * s)
LIO_NM_HD void nm_add(NmSums& a, float ox, float oy, float oz, double s) {
    const int64_t qx = (int64_t)rint((double)ox * s), qy = (int64_t)rint((double)oy * s), qz = (int64_t)rint((double)oz * s);
    a.s[0] += qx, a.s[1] += qy, a.s[2] += qz;
    a.ss[0] += qx * qx, a.ss[1] += qx * qy, a.ss[2] += qx * qz;
    a.ss[3] += qy * qy, a.ss[4] += qy * qz, a.ss[5] += qz * qz;
}

template <int P, int Q>
LIO_NM_HD void nm_rotate_row(double (&v)[3], double c, double s) {
    const double vp = v[P], vq = v[Q];
    v[P] = c * vp - s * vq;
    v[Q] = s * vp + c * vq;
}

// one Jacobi rotation of the pair (P, Q), R the third index; skipped when A_pq = 0
template <int P, int Q, int R>
LIO_NM_HD void nm_rotate(double (&A)[3][3], double (&V)[3][3]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    A[P][P] -= t * apq;
    A[Q][Q] += t * apq;
    A[P][Q] = A[Q][P] = 0.0;
    const double arp = A[R][P], arq = A[R][Q];
    A[R][P] = A[P][R] = c * arp - s * arq;
    A[R][Q] = A[Q][R] = s * arp + c * arq;
    nm_rotate_row<P, Q>(V[0], c, s);
    nm_rotate_row<P, Q>(V[1], c, s);
    nm_rotate_row<P, Q>(V[2], c, s);
}

// the normal and curvature of a neighbourhood of m >= 3 points with bound B (the scale's), at the point
// (x, y, z); vp: the viewpoint's 3 floats or null
LIO_NM_HD NmResult nm_solve(const NmSums& a, int64_t m, float B, float x, float y, float z, const float* vp) {
    NmResult out;
    out.n[0] = out.n[1] = out.n[2] = out.curvature = nm_nan();
    out.ok = false;
    const double dm = (double)m;
    const double s0 = (double)a.s[0], s1 = (double)a.s[1], s2 = (double)a.s[2];
    double A[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    A[0][0] = (double)a.ss[0] - (s0 * s0) / dm;
    A[0][1] = A[1][0] = (double)a.ss[1] - (s0 * s1) / dm;
    A[0][2] = A[2][0] = (double)a.ss[2] - (s0 * s2) / dm;
    A[1][1] = (double)a.ss[3] - (s1 * s1) / dm;
    A[1][2] = A[2][1] = (double)a.ss[4] - (s1 * s2) / dm;
    A[2][2] = (double)a.ss[5] - (s2 * s2) / dm;
    const double T = (A[0][0] + A[1][1]) + A[2][2];
    if (B == 0.f || !(T > 0.0)) return out;
    for (int sweep = 0; sweep < 10; ++sweep) {
        if (A[0][1] == 0.0 && A[0][2] == 0.0 && A[1][2] == 0.0) break;
        nm_rotate<0, 1, 2>(A, V);
        nm_rotate<0, 2, 1>(A, V);
        nm_rotate<1, 2, 0>(A, V);
    }
    // the smallest eigenvalue, the lowest index among equals; its column of V
    // (selects on a flag, not an index into V: a run-time column index would put V in scratch memory on the device)
    const bool p1 = A[1][1] < A[0][0];
    double lam = p1 ? A[1][1] : A[0][0];
    double n0 = p1 ? V[0][1] : V[0][0], n1 = p1 ? V[1][1] : V[1][0], n2 = p1 ? V[2][1] : V[2][0];
    const bool p2 = A[2][2] < lam;
    lam = p2 ? A[2][2] : lam;
    n0 = p2 ? V[0][2] : n0, n1 = p2 ? V[1][2] : n1, n2 = p2 ? V[2][2] : n2;
    bool flip;
    if (vp) {
        const double s = (((double)vp[0] - (double)x) * n0 + ((double)vp[1] - (double)y) * n1) + ((double)vp[2] - (double)z) * n2;
        flip = s < 0.0;  // a NaN s flips nothing
    } else {
        flip = n2 < 0.0 || (n2 == 0.0 && (n1 < 0.0 || (n1 == 0.0 && n0 < 0.0)));
    }
    if (flip) n0 = -n0, n1 = -n1, n2 = -n2;
    out.n[0] = (float)n0, out.n[1] = (float)n1, out.n[2] = (float)n2;
    out.curvature = (float)(fabs(lam) / T);
    out.ok = true;
    return out;
}

}  // namespace lio
