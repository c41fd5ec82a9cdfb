// lio_exposure_dev.hpp — the per-pixel device half of the exposure contract (include/lio_gpu.h, lio_exposure_*): the
// 8-bit BGR -> HSV in integers, the HSV -> BGR in float32, V of a pixel and the load of 4 pixels at any alignment.
// It is the ONLY copy: lio_exposure.hip (CLAHE, the table remaps) and lio_overexposure.hip (the overexposure
// recovery) include it, so a pixel has the same h, s, v and the same round trip in both.  Files that include this
// are compiled with -ffp-contract=off: no multiply-add is fused.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lio {

// ---- the division tables of the 8-bit BGR -> HSV: sdiv[i] = rint((255 << 12) / i), hdiv[i] = rint((180 << 12) / (6 i)).
// The quotients are below 2^21 and an exact tie is a tie in double too, so the integer rounding below (ties to
// even) is the double rint of the contract.
struct ExDivTab {
    int32_t v[256];
};
constexpr int32_t ex_rdiv(int64_t a, int64_t b) {
    int64_t q = a / b;
    const int64_t r = a % b;
    if (2 * r > b || (2 * r == b && (q & 1))) ++q;
    return (int32_t)q;
}
constexpr ExDivTab ex_make_div(int64_t num, int64_t per) {
    ExDivTab t{};
    for (int i = 1; i < 256; ++i) t.v[i] = ex_rdiv(num, per * i);
    return t;
}
static_assert(ex_rdiv(255 << 12, 255) == 4096 && ex_rdiv(180 << 12, 6) == 122880 && ex_rdiv(5, 2) == 2 && ex_rdiv(7, 2) == 4,
              "rint of a quotient, ties to even");
// internal linkage: each file that includes this holds the two tables (2 KB) in its own code object
static __constant__ const ExDivTab ex_sdiv = ex_make_div(255 << 12, 1);
static __constant__ const ExDivTab ex_hdiv = ex_make_div(180 << 12, 6);

constexpr float kExHs = 0x1.111112p-5f;  // the float nearest 1/30
constexpr float kExK = 0x1.010102p-8f;   // the float nearest 1/255

__device__ __forceinline__ int ex_sat_rint(float x) { return min(max((int)rintf(x), 0), 255); }

__device__ __forceinline__ void ex_bgr2hsv(int b, int g, int r, int& h, int& s, int& v) {
    v = max(b, max(g, r));
    const int vmin = min(b, min(g, r));
    const int d = v - vmin;
    s = (d * ex_sdiv.v[v] + 2048) >> 12;
    const int h0 = v == r ? g - b : (v == g ? b - r + 2 * d : r - g + 4 * d);
    h = (h0 * ex_hdiv.v[d] + 2048) >> 12;
    if (h < 0) h += 180;
}

__device__ __forceinline__ void ex_hsv2bgr(int h, int s, int v, int& b, int& g, int& r) {
    const float vf = (float)v * kExK;
    if (s == 0) {
        b = g = r = ex_sat_rint(vf * 255.0f);
        return;
    }
    const float hf = (float)h * kExHs, sf = (float)s * kExK;
    int sec = (int)floorf(hf);
    float f = hf - (float)sec;
    if (sec >= 6) sec = 0, f = 0.f;
    const float t0 = vf, t1 = vf * (1.f - sf), t2 = vf * (1.f - sf * f), t3 = vf * (1.f - sf * (1.f - f));
    float fb, fg, fr;  // the sector table {1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}
    switch (sec) {
        case 0: fb = t1, fg = t3, fr = t0; break;
        case 1: fb = t1, fg = t0, fr = t2; break;
        case 2: fb = t3, fg = t0, fr = t1; break;
        case 3: fb = t0, fg = t2, fr = t1; break;
        case 4: fb = t0, fg = t1, fr = t3; break;
        default: fb = t2, fg = t1, fr = t0; break;
    }
    b = ex_sat_rint(fb * 255.0f), g = ex_sat_rint(fg * 255.0f), r = ex_sat_rint(fr * 255.0f);
}

__device__ __forceinline__ int ex_gray(int b, int g, int r) { return (3735 * b + 19235 * g + 9798 * r + 16384) >> 15; }

// the 4 * C bytes of 4 consecutive pixels at p, at any alignment, one value per byte
template <int C>
__device__ __forceinline__ void ex_load4(const uint8_t* __restrict__ p, uint32_t* v) {
    uint32_t w[C];
    __builtin_memcpy(w, p, 4 * C);
#pragma unroll
    for (int k = 0; k < 4 * C; ++k) v[k] = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
}

// V (gray != 0: gray) of the pixel whose C bytes are c
template <int C>
__device__ __forceinline__ int ex_value(const uint32_t* c, int order, int gray) {
    if constexpr (C == 1) {
        return (int)c[0];
    } else {
        const int b = (int)(order ? c[2] : c[0]), g = (int)c[1], r = (int)(order ? c[0] : c[2]);
        return gray ? ex_gray(b, g, r) : max(b, max(g, r));
    }
}

// the store of ex_load4's layout: 4 * C values as C dwords at o (4-byte aligned)
template <int C>
__device__ __forceinline__ void ex_store4(uint8_t* __restrict__ o, const uint32_t* v) {
    uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
    for (int k = 0; k < C; ++k) o4[k] = v[4 * k] | (v[4 * k + 1] << 8) | (v[4 * k + 2] << 16) | (v[4 * k + 3] << 24);
}

}  // namespace lio
