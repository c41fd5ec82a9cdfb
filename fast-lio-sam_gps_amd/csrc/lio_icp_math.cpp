// lio_icp_math.cpp — the loop ICP's host arithmetic (lio_icp_math.hpp).  Built with the library's flags
// (-ffp-contract=off): every float expression below is evaluated as written.
#include "lio_icp_math.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

namespace {

// ---- 3x3 SVD by one-sided Jacobi (Hestenes) on the columns of A: A = U S V^T
void svd3(const double A[9], double U[9], double S[3], double V[9]) {
    double W[9];
    std::memcpy(W, A, sizeof(W));
    for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double al = 0, be = 0, ga = 0;
                for (int r = 0; r < 3; ++r) {
                    al += W[3 * r + p] * W[3 * r + p];
                    be += W[3 * r + q] * W[3 * r + q];
                    ga += W[3 * r + p] * W[3 * r + q];
                }
                if (ga == 0.0) continue;
                off = std::max(off, std::fabs(ga) / std::sqrt(al * be + 1e-300));
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                for (int r = 0; r < 3; ++r) {
                    const double wp = W[3 * r + p], wq = W[3 * r + q];
                    W[3 * r + p] = c * wp - s * wq;
                    W[3 * r + q] = s * wp + c * wq;
                    const double vp = V[3 * r + p], vq = V[3 * r + q];
                    V[3 * r + p] = c * vp - s * vq;
                    V[3 * r + q] = s * vp + c * vq;
                }
            }
        if (off < 1e-15) break;
    }
    double sv[3];
    for (int c = 0; c < 3; ++c) sv[c] = std::sqrt(W[c] * W[c] + W[3 + c] * W[3 + c] + W[6 + c] * W[6 + c]);
    int ord[3] = {0, 1, 2};
    std::sort(ord, ord + 3, [&](int a, int b) { return sv[a] > sv[b]; });
    double Vs[9], Us[9];
    for (int k = 0; k < 3; ++k) {
        const int c = ord[k];
        S[k] = sv[c];
        for (int r = 0; r < 3; ++r) {
            Vs[3 * r + k] = V[3 * r + c];
            Us[3 * r + k] = sv[c] > 0 ? W[3 * r + c] / sv[c] : 0.0;
        }
    }
    // complete U to an orthonormal basis where sigma vanished
    if (!(S[2] > 1e-300 * S[0])) {
        Us[2] = Us[3] * Us[7] - Us[6] * Us[4];
        Us[5] = Us[6] * Us[1] - Us[0] * Us[7];
        Us[8] = Us[0] * Us[4] - Us[3] * Us[1];
    }
    std::memcpy(U, Us, sizeof(Us));
    std::memcpy(V, Vs, sizeof(Vs));
}
double det3(const double* M) {
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// ---- PCL-order fidelity mode (lio_icp_params.umeyama_float): the host half of pcl::umeyama(src, dst,
// false) in float [U] (Eigen 3.3 Umeyama.h / JacobiSVD.h / Jacobi.h as PCL 1.10 instantiates them for
// Scalar = float, no FMA).  The GPU returns the sequential float sums (means) and the sequential
// sigma accumulator (lio_icp.hip icp_pcl_*); here: sigma = one_over_n * acc, the two-sided Jacobi SVD
// of the 3x3, R = U S V^T (S(2) = -1 when det U det V < 0), t = dst_mean - R src_mean.
struct Rot2 {
    float c, s;
};

// JacobiRotation::makeJacobi(x, y, z) for real scalars
Rot2 make_jacobi_f(float x, float y, float z) {
    const float deno = 2.f * std::fabs(y);
    if (deno < FLT_MIN) return {1.f, 0.f};
    const float tau = (x - z) / deno;
    const float w = std::sqrt(tau * tau + 1.f);
    const float t = tau > 0.f ? 1.f / (tau + w) : 1.f / (tau - w);
    const float sign_t = t > 0.f ? 1.f : -1.f;
    const float n = 1.f / std::sqrt(t * t + 1.f);
    return {n, ((-sign_t) * (y / std::fabs(y))) * std::fabs(t) * n};
}

// apply_rotation_in_the_plane(x, y, j) over 3 elements with stride `inc` (a no-op for the identity)
void plane_rot(float* x, float* y, int inc, Rot2 j) {
    if (j.c == 1.f && j.s == 0.f) return;
    for (int i = 0; i < 3; ++i) {
        const float xi = x[i * inc], yi = y[i * inc];
        x[i * inc] = j.c * xi + j.s * yi;
        y[i * inc] = -j.s * xi + j.c * yi;
    }
}

// JacobiSVD<Matrix3f>(A, ComputeFullU | ComputeFullV), column-major storage M[3 * col + row]
void jacobi_svd3_f(const float* A, float* U, float* V, float* sv) {
    float scale = 0.f;
    for (int i = 0; i < 9; ++i) scale = std::max(scale, std::fabs(A[i]));
    if (scale == 0.f) scale = 1.f;
    float W[9];
    for (int i = 0; i < 9; ++i) {
        W[i] = A[i] / scale;
        U[i] = V[i] = (i % 4 == 0) ? 1.f : 0.f;
    }
    auto at = [&](int r, int c) -> float& { return W[3 * c + r]; };
    const float precision = 2.f * FLT_EPSILON;
    float max_diag = std::max(std::max(std::fabs(at(0, 0)), std::fabs(at(1, 1))), std::fabs(at(2, 2)));
    for (bool finished = false; !finished;) {
        finished = true;
        for (int p = 1; p < 3; ++p)
            for (int q = 0; q < p; ++q) {
                const float thr = std::max(FLT_MIN, precision * max_diag);
                if (!(std::fabs(at(p, q)) > thr || std::fabs(at(q, p)) > thr)) continue;
                finished = false;
                // real_2x2_jacobi_svd: rot1 makes the 2x2 block symmetric, then makeJacobi on it
                float m00 = at(p, p), m01 = at(p, q), m10 = at(q, p), m11 = at(q, q);
                Rot2 rot1{1.f, 0.f};
                const float t = m00 + m11, d = m10 - m01;
                if (!(std::fabs(d) < FLT_MIN)) {
                    const float u = t / d;
                    const float tmp = std::sqrt(1.f + u * u);
                    rot1 = {u / tmp, 1.f / tmp};
                }
                if (!(rot1.c == 1.f && rot1.s == 0.f)) {  // m.applyOnTheLeft(0, 1, rot1)
                    const float a0 = m00, b0 = m10, a1 = m01, b1 = m11;
                    m00 = rot1.c * a0 + rot1.s * b0;
                    m10 = -rot1.s * a0 + rot1.c * b0;
                    m01 = rot1.c * a1 + rot1.s * b1;
                    m11 = -rot1.s * a1 + rot1.c * b1;
                }
                const Rot2 jr = make_jacobi_f(m00, m01, m11);
                const Rot2 jrt{jr.c, -jr.s};
                const Rot2 jl{rot1.c * jrt.c - rot1.s * jrt.s, rot1.c * jrt.s + rot1.s * jrt.c};  // rot1 * j_right^T
                plane_rot(W + p, W + q, 3, jl);            // W.applyOnTheLeft(p, q, j_left): rows
                // U.applyOnTheRight(p, q, j_left^T): columns, and applyOnTheRight rotates by the transpose of
                // its argument, so the plane rotation is j_left itself
                plane_rot(U + 3 * p, U + 3 * q, 1, jl);
                plane_rot(W + 3 * p, W + 3 * q, 1, {jr.c, -jr.s});  // W.applyOnTheRight(p, q, j_right)
                plane_rot(V + 3 * p, V + 3 * q, 1, {jr.c, -jr.s});  // V.applyOnTheRight(p, q, j_right)
                max_diag = std::max(max_diag, std::max(std::fabs(at(p, p)), std::fabs(at(q, q))));
            }
    }
    for (int i = 0; i < 3; ++i) {
        const float a = at(i, i);
        sv[i] = std::fabs(a);
        if (a < 0.f)
            for (int r = 0; r < 3; ++r) U[3 * i + r] = -U[3 * i + r];
    }
    for (int i = 0; i < 3; ++i) sv[i] *= scale;
    for (int i = 0; i < 3; ++i) {  // descending; maxCoeff keeps the first maximum
        int pos = i;
        for (int k = i + 1; k < 3; ++k)
            if (sv[k] > sv[pos]) pos = k;
        if (sv[pos] == 0.f) break;
        if (pos != i) {
            std::swap(sv[i], sv[pos]);
            for (int r = 0; r < 3; ++r) {
                std::swap(U[3 * i + r], U[3 * pos + r]);
                std::swap(V[3 * i + r], V[3 * pos + r]);
            }
        }
    }
}

float det3_f(const float* M) {  // column-major; Eigen determinant_impl<3>
    auto m = [&](int r, int c) { return M[3 * c + r]; };
    auto h = [&](int a, int b, int c) { return m(a, 0) * (m(b, 1) * m(c, 2) - m(b, 2) * m(c, 1)); };
    return h(0, 1, 2) - h(1, 0, 2) + h(2, 0, 1);
}

}  // namespace

namespace lio::icp {

// Umeyama without scaling (Eigen::umeyama(src, dst, false)) from statistics:
// st[0]=n, st[1..3]=sum p, st[4..6]=sum q, st[7..15]=sum q p^T, all about c0.
void umeyama(const double* st, const double c0[3], float Ti[16]) {
    const double inv_n = 1.0 / st[0];
    double pm[3], qm[3], Sg[9];
    for (int d = 0; d < 3; ++d) {
        pm[d] = st[1 + d] * inv_n;
        qm[d] = st[4 + d] * inv_n;
    }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Sg[3 * r + c] = st[7 + 3 * r + c] * inv_n - qm[r] * pm[c];
    double U[9], S[3], V[9];
    svd3(Sg, U, S, V);
    const double D = (det3(U) * det3(V) < 0) ? -1.0 : 1.0;
    double R[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1] + D * U[3 * r + 2] * V[3 * c + 2];
    std::memset(Ti, 0, 16 * sizeof(float));
    for (int r = 0; r < 3; ++r) {
        const double t = (qm[r] + c0[r]) -
                         (R[3 * r] * (pm[0] + c0[0]) + R[3 * r + 1] * (pm[1] + c0[1]) + R[3 * r + 2] * (pm[2] + c0[2]));
        for (int c = 0; c < 3; ++c) Ti[4 * r + c] = (float)R[3 * r + c];
        Ti[4 * r + 3] = (float)t;
    }
    Ti[15] = 1.f;
}

// out16 from the fidelity statistics -> the incremental transform (row-major 4x4 float); order 1 returns
// the raw sequential sigma accumulator (scaled here), orders 2 / 3 sigma as Eigen's GEMM leaves it
void umeyama_pcl_float(const float* out16, float Ti[16], int order) {
    const uint32_t n = [&] {
        uint32_t u;
        std::memcpy(&u, out16 + 6, sizeof(u));
        return u;
    }();
    const float one_over_n = 1.f / (float)n;
    float sm[3], dm[3];
    for (int d = 0; d < 3; ++d) {
        sm[d] = out16[d] * one_over_n;
        dm[d] = out16[3 + d] * one_over_n;
    }
    float sigma[9];  // column-major
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) sigma[3 * c + r] = order == 1 ? one_over_n * out16[7 + 3 * r + c] : out16[7 + 3 * r + c];
    float U[9], V[9], sv[3];
    jacobi_svd3_f(sigma, U, V, sv);
    const float S2 = det3_f(U) * det3_f(V) < 0.f ? -1.f : 1.f;
    std::memset(Ti, 0, 16 * sizeof(float));
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {  // (U S) V^T, each entry e0 + (e1 + e2)
            const float e0 = U[r] * V[c], e1 = U[3 + r] * V[3 + c], e2 = (U[6 + r] * S2) * V[6 + c];
            Ti[4 * r + c] = e0 + (e1 + e2);
        }
    }
    for (int r = 0; r < 3; ++r)
        Ti[4 * r + 3] = dm[r] - (Ti[4 * r] * sm[0] + (Ti[4 * r + 1] * sm[1] + Ti[4 * r + 2] * sm[2]));
    Ti[15] = 1.f;
}

void compose4f(const float Ti[16], float fin[16]) {
    float nf[16];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            float s = Ti[4 * r] * fin[c];
            s += Ti[4 * r + 1] * fin[4 + c];
            s += Ti[4 * r + 2] * fin[8 + c];
            s += Ti[4 * r + 3] * fin[12 + c];
            nf[4 * r + c] = s;
        }
    std::memcpy(fin, nf, sizeof(nf));
}

bool convergence_step(const float Ti[16], double mse, double prev_mse, int iters, const lio_icp_params& p, int* state) {
    if (iters >= p.max_iter) {
        *state = 1;
        return true;
    }
    const double rot_thr = p.rot_eps > 0 ? p.rot_eps : 1.0 - p.trans_eps;
    // PCL 1.10 DefaultConvergenceCriteria<float>: the coefficients of the Matrix4f are summed and
    // squared in float, then widened (0.5 * float -> double; float -> double translation_sqr)
    const float tr_f = Ti[0] + Ti[5] + Ti[10] - 1.f;
    const float tsq_f = Ti[3] * Ti[3] + Ti[7] * Ti[7] + Ti[11] * Ti[11];
    const double cosang = 0.5 * (double)tr_f;
    const double tsq = (double)tsq_f;
    if (cosang >= rot_thr && tsq <= p.trans_eps) {
        *state = 2;
        return true;
    }
    if (std::fabs(mse - prev_mse) < 1e-12) {
        *state = 3;
        return true;
    }
    if (std::fabs(mse - prev_mse) / prev_mse < p.fitness_eps) {
        *state = 4;
        return true;
    }
    return false;
}

}  // namespace lio::icp
