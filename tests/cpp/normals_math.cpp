// The arithmetic of lio_estimate_normals behind the search (csrc/lio_normals_math.hpp: scale, quantisation, covariance,
// Jacobi, pick, orientation) built for the host with g++ — the text the device compiles — over generated
// neighbourhoods: random, near-planar, near-linear, exactly planar, exactly linear and zero ones, each with a
// viewpoint of its own (the point itself among them) or none.  Prints, per set, the inputs (the integer sums, m, the bits of B, of
// the point and of the viewpoint) and the bits of the normal and the curvature; tests/test_normals_math.py
// compares them exactly with tests/normals_ref.py.  Stand-alone (address and UB sanitizers: nothing is preloaded).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lio_normals_math.hpp"

static uint64_t g_state = 0x1234567ull;
static uint64_t next() {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static float frand() { return (float)(next() >> 40) * (1.0f / 16777216.0f) * 2.f - 1.f; }  // [-1, 1)
static uint32_t bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}

int main() {
    int sets = 0;
    for (int kind = 0; kind < 6; ++kind)
        for (int rep = 0; rep < 200; ++rep) {
            const int m = 3 + (int)(next() % 60);
            const float scale = std::ldexp(1.f, (int)(next() % 24) - 12);
            const float p[3] = {100.f * frand(), 100.f * frand(), 10.f * frand()};
            float u[3] = {frand(), frand(), frand()}, v[3] = {frand(), frand(), frand()}, w[3] = {frand(), frand(), frand()};
            if (kind >= 3 && rep % 2) u[0] = 1.f, u[1] = u[2] = 0.f, v[0] = v[2] = 0.f, v[1] = 1.f;  // axis-aligned: exact zeros
            std::vector<float> o(3 * (size_t)m);
            float B = 0.f;
            for (int i = 0; i < m; ++i) {
                const float a = frand(), b = frand(), c = frand();
                for (int d = 0; d < 3; ++d) {
                    float x = 0.f;
                    if (kind == 0) x = (d == 0 ? a : d == 1 ? b : c);          // random
                    if (kind == 1) x = a * u[d] + b * v[d] + 1e-3f * c * w[d];  // near-planar
                    if (kind == 2) x = a * u[d] + 1e-3f * (b * v[d] + c * w[d]);  // near-linear
                    if (kind == 3) x = (float)(int)(8.f * a) * u[d] + (float)(int)(8.f * b) * v[d];  // planar
                    if (kind == 4) x = (float)(int)(8.f * a) * u[d];            // linear
                    o[3 * (size_t)i + d] = x * scale;                           // kind 5: zero
                }
                const float* q = &o[3 * (size_t)i];
                const float d2 = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
                if (d2 > B) B = d2;
            }
            if (rep % 3 == 1 && B > 0.f) B = B * 1.5f;  // a radius search's bound lies above every d2
            const double s = lio::nm_scale(B);
            lio::NmSums a;
            for (int i = 0; i < m; ++i) lio::nm_add(a, o[3 * (size_t)i], o[3 * (size_t)i + 1], o[3 * (size_t)i + 2], s);
            const int mode = rep % 4;  // 0: no viewpoint; else one
            float vp[3] = {p[0] + 50.f * frand(), p[1] + 50.f * frand(), p[2] + 50.f * frand()};
            if (mode == 3) vp[0] = p[0], vp[1] = p[1], vp[2] = p[2];  // s = 0: nothing flips
            const lio::NmResult r = lio::nm_solve(a, m, B, p[0], p[1], p[2], mode ? vp : nullptr);
            std::printf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %d %08x %08x %08x %08x %d %08x %08x %08x %d %08x %08x %08x %08x\n",
                        (long long)a.s[0], (long long)a.s[1], (long long)a.s[2], (long long)a.ss[0], (long long)a.ss[1],
                        (long long)a.ss[2], (long long)a.ss[3], (long long)a.ss[4], (long long)a.ss[5], m, bits(B), bits(p[0]),
                        bits(p[1]), bits(p[2]), mode ? 1 : 0, bits(vp[0]), bits(vp[1]), bits(vp[2]), r.ok ? 1 : 0, bits(r.n[0]),
                        bits(r.n[1]), bits(r.n[2]), bits(r.curvature));
            ++sets;
        }
    // sums as large as n < 2^31 neighbours allow (|q| <= 2^15): the int64 -> double conversions round
    for (int rep = 0; rep < 8; ++rep) {
        lio::NmSums a;
        const int64_t m = ((int64_t)1 << 31) - 1 - rep;
        const int64_t q[3] = {32768 - rep, -(32768 - 3 * rep), 12345 + rep};
        for (int d = 0; d < 3; ++d) a.s[d] = (m / 2) * q[d] + (m - m / 2) * (q[d] / 2);
        int t = 0;
        for (int x = 0; x < 3; ++x)
            for (int y = x; y < 3; ++y, ++t) a.ss[t] = (m / 2) * q[x] * q[y] + (m - m / 2) * (q[x] / 2) * (q[y] / 2);
        const float B = 4.f, p[3] = {1.f, 2.f, 3.f}, vp[3] = {0.f, 0.f, 10.f};
        const lio::NmResult r = lio::nm_solve(a, m, B, p[0], p[1], p[2], vp);
        std::printf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %08x %08x %08x %08x %d %08x %08x %08x %d %08x %08x %08x %08x\n",
                    (long long)a.s[0], (long long)a.s[1], (long long)a.s[2], (long long)a.ss[0], (long long)a.ss[1],
                    (long long)a.ss[2], (long long)a.ss[3], (long long)a.ss[4], (long long)a.ss[5], (long long)m, bits(B),
                    bits(p[0]), bits(p[1]), bits(p[2]), 1, bits(vp[0]), bits(vp[1]), bits(vp[2]), r.ok ? 1 : 0, bits(r.n[0]),
                    bits(r.n[1]), bits(r.n[2]), bits(r.curvature));
        ++sets;
    }
    // the quantisation alone: Q <bits of B> <bits of o> <q>, over bounds of every exponent parity and halfway cases
    for (int rep = 0; rep < 400; ++rep) {
        const float B = std::ldexp(0.5f + 0.5f * (float)(next() >> 40) * (1.0f / 16777216.0f), (int)(next() % 80) - 40);
        float o = std::sqrt(B) * frand();
        if (rep % 4 == 0) o = (float)(((double)(next() % 65536) - 32768.0 + 0.5) / lio::nm_scale(B));  // a tie of rint
        lio::NmSums a;
        lio::nm_add(a, o, 0.f, 0.f, lio::nm_scale(B));
        std::printf("Q %08x %08x %lld\n", bits(B), bits(o), (long long)a.s[0]);
    }
    std::printf("SETS %d\nALL OK\n", sets);
    return 0;
}
