// lio_overexposure.hip — the stencil calls of the camera leg on gfx950 (lio_overexposure.hpp): the overexposure
// recovery of the reference's solve_overexposure script and the 8-bit Gaussian blur, as the integer contract of
// include/lio_gpu.h (lio_gaussian_weights, lio_exposure_recover, lio_exposure_gaussian_blur).  The only floats are
// those of the shared HSV -> BGR (lio_exposure_dev.hpp); the file is compiled with -ffp-contract=off.
//
//   ox_stencil_kernel  one 256-thread workgroup per 64 x 32 tile of the output, everything between the load and the
//                      store in LDS with a halo of R = max(r, rd) pixels (r = ksize / 2, rd = (dilate - 1) / 2):
//                        load    the plane value of every pixel of the (64 + 2R) x (32 + 2R) patch, REFLECT_101 at the
//                                image's edges, as bytes: V = max(b, g, r) from the pixel's bytes (MODE 0), or channel
//                                p (MODE 1, one pass per channel); beside it m0 = V > threshold, 0 outside the image
//                        rows    a thread takes 4 consecutive columns of a patch row from a sliding window of k + 3
//                                bytes: Hrow of the 64 centre columns into uint16 (at most 65 280), stored 4 at a
//                                time; the OR of m0 over |dx| <= rd into bytes, stored as one dword
//                        columns a thread owns two groups of 4 consecutive pixels: B from k Hrow rows (one 8-byte
//                                read per tap), M from the 2 rd + 1 mask rows (one dword each)
//                        store   MODE 0: the pixel's bytes once more (they are in the cache from the load), h and s
//                                from them, V' = M ? B : V, HSV -> BGR; MODE 1: the blurred channels.  Full groups
//                                as dwords into rows of frame_pitch bytes, the last partial group as bytes.
//                      The weights and all parameters are kernel arguments; no atomics, no intermediate plane in
//                      global memory.
#include <cmath>

#include "lio_exposure_dev.hpp"
#include "lio_overexposure.hpp"
#include "lio_scratch.hpp"

namespace lio {
namespace {

constexpr int kOxTW = 64, kOxTH = 32;                        // the tile of one workgroup
constexpr int kOxMaxR = kOxMaxKsize / 2;                     // 15 >= (kOxMaxDilate - 1) / 2
constexpr int kOxSW = kOxTW + 2 * kOxMaxR, kOxSH = kOxTH + 2 * kOxMaxR;  // the largest patch: 94 x 62
constexpr int kOxGroups = kOxTW * kOxTH / 4 / 256;           // groups of 4 pixels per thread: 2
static_assert(kOxTW == 64 && kOxGroups * 256 * 4 == kOxTW * kOxTH && (kOxMaxDilate - 1) / 2 <= kOxMaxR, "the index arithmetic below");

struct OxArg {
    int W, H, order;
    int threshold, rd;  // MODE 0
    int k;              // ksize; w[0 .. k - 1]
    uint16_t w[kOxMaxKsize + 1];
};

// REFLECT_101 applied until the index is in 0 .. n - 1
__device__ __forceinline__ int ox_refl(int p, int n) {
    if (p >= 0 && p < n) return p;
    if (n == 1) return 0;
    const int m = 2 * (n - 1);
    int q = p % m;
    if (q < 0) q += m;
    return q < n ? q : m - q;
}

// MODE 0: recovery; 1: Gaussian blur of every channel.  img rows of `pitch` bytes at any alignment; out rows out_pitch
// bytes, a multiple of 4 and this library's own buffer.  grid (ceil(W / 64), ceil(H / 32)).
template <int C, int MODE>
__global__ __launch_bounds__(256) void ox_stencil_kernel(const uint8_t* __restrict__ img, int64_t pitch, OxArg a,
                                                         uint8_t* __restrict__ out, int64_t out_pitch) {
    __shared__ uint8_t sv[kOxSH * kOxSW];                        // the plane's patch
    __shared__ uint8_t sm[MODE == 0 ? kOxSH * kOxSW : 1];        // m0 of the patch: V > threshold, inside the image
    __shared__ __attribute__((aligned(8))) uint16_t hrow[kOxSH * kOxTW];
    __shared__ __attribute__((aligned(4))) uint8_t mrow[MODE == 0 ? kOxSH * kOxTW : 4];
    const int tid = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * kOxTW, y0 = (int)blockIdx.y * kOxTH;
    const int r = a.k >> 1, rd = MODE == 0 ? a.rd : 0, R = max(r, rd);
    const int sw = kOxTW + 2 * R, sh = kOxTH + 2 * R;  // the patch: at most kOxSW x kOxSH
    // The tap loops below are unrolled to the largest kernel and leave at the real one, so that every weight is
    // indexed by a constant and stays in a scalar register; w[j] = 0 from j = ksize on (ox_arg).
    uint32_t w[kOxMaxKsize];
#pragma unroll
    for (int j = 0; j < kOxMaxKsize; ++j) w[j] = a.w[j];
    constexpr int NP = MODE == 1 ? C : 1;  // passes: one plane each
    uint32_t blur[kOxGroups][4 * NP];      // pixel q of the group, plane p: [q * NP + p]
    [[maybe_unused]] uint32_t mask[kOxGroups] = {};  // byte q: M of pixel q of the group
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        // (a second pass may write sv at once: every thread has left the row pass that read it)
#pragma unroll 4
        for (int i = tid; i < sh * sw; i += 256) {
            const int ly = i / sw, lx = i - ly * sw;
            const int py = y0 - R + ly, px = x0 - R + lx;
            const uint8_t* pix = img + (int64_t)ox_refl(py, a.H) * pitch + (int64_t)ox_refl(px, a.W) * C;
            int v;
            if constexpr (MODE == 1)
                v = pix[p];
            else if constexpr (C == 1)
                v = pix[0];
            else
                v = max((int)pix[0], max((int)pix[1], (int)pix[2]));
            sv[i] = (uint8_t)v;
            if constexpr (MODE == 0) sm[i] = (uint8_t)(py >= 0 && py < a.H && px >= 0 && px < a.W && v > a.threshold);
        }
        __syncthreads();
        // rows: a thread takes 4 consecutive columns of a patch row; column x of the tile is patch column x + R
        for (int i = tid; i < sh * (kOxTW / 4); i += 256) {
            const int ly = i >> 4, x4 = (i & 15) * 4;
            const uint8_t* s = sv + ly * sw + x4 + (R - r);  // the taps of column x4 + o are s[o .. o + k - 1]
            uint32_t acc[4] = {0, 0, 0, 0};
#pragma unroll
            for (int t = 0; t < kOxMaxKsize + 3; ++t) {
                if (t >= a.k + 3) break;
                const uint32_t b = s[t];
#pragma unroll
                for (int o = 0; o < 4; ++o)
                    if (t - o >= 0 && t - o < kOxMaxKsize) acc[o] += w[t - o] * b;
            }
            *reinterpret_cast<uint2*>(hrow + ly * kOxTW + x4) = make_uint2(acc[0] | (acc[1] << 16), acc[2] | (acc[3] << 16));
            if constexpr (MODE == 0) {
                const uint8_t* m = sm + ly * sw + x4 + (R - rd);  // the window of column x4 + o is m[o .. o + 2 rd]
                uint32_t bits = 0;  // bit t: m[t] (each byte is 0 or 1)
                for (int t = 0; t < 2 * rd + 4; ++t) bits |= (uint32_t)m[t] << t;
                const uint32_t window = (2u << (2 * rd)) - 1u;  // 2 rd + 1 ones
                uint32_t any = 0;
#pragma unroll
                for (int o = 0; o < 4; ++o) any |= ((bits >> o) & window) ? 1u << (8 * o) : 0u;
                *reinterpret_cast<uint32_t*>(mrow + ly * kOxTW + x4) = any;
            }
        }
        __syncthreads();
        // columns: a thread owns kOxGroups groups of 4 pixels; row ly of the tile is patch row ly + R
#pragma unroll
        for (int g = 0; g < kOxGroups; ++g) {
            const int item = tid + g * 256, ly = item >> 4, xg = (item & 15) * 4;
            const uint16_t* top = hrow + (ly + R - r) * kOxTW + xg;
            uint32_t acc[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < kOxMaxKsize; ++j) {
                if (j >= a.k) break;
                const uint2 h = *reinterpret_cast<const uint2*>(top + j * kOxTW);
                acc[0] += w[j] * (h.x & 0xffffu), acc[1] += w[j] * (h.x >> 16);
                acc[2] += w[j] * (h.y & 0xffffu), acc[3] += w[j] * (h.y >> 16);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) blur[g][q * NP + p] = (acc[q] + 32768u) >> 16;
            if constexpr (MODE == 0) {
                const uint8_t* mtop = mrow + (ly + R - rd) * kOxTW + xg;
                uint32_t any = 0;
#pragma unroll
                for (int j = 0; j < kOxMaxDilate; ++j) {
                    if (j > 2 * rd) break;
                    any |= *reinterpret_cast<const uint32_t*>(mtop + j * kOxTW);
                }
                mask[g] = any;
            }
        }
    }
#pragma unroll
    for (int g = 0; g < kOxGroups; ++g) {
        const int item = tid + g * 256;
        const int row = y0 + (item >> 4), x = x0 + (item & 15) * 4;
        if (row >= a.H || x >= a.W) continue;
        const int n = min(4, a.W - x);
        uint32_t v[4 * C];
        if constexpr (MODE == 1) {
#pragma unroll
            for (int k = 0; k < 4 * C; ++k) v[k] = blur[g][k];
        } else {
            const uint8_t* src = img + (int64_t)row * pitch + (int64_t)x * C;
            if (n == 4) {
                ex_load4<C>(src, v);
            } else {
#pragma unroll
                for (int k = 0; k < 3 * C; ++k) v[k] = k < n * C ? src[k] : 0u;
#pragma unroll
                for (int k = 3 * C; k < 4 * C; ++k) v[k] = 0u;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k >= n) break;
                uint32_t* c = v + k * C;
                if constexpr (C == 1) {
                    if ((mask[g] >> (8 * k)) & 0xffu) c[0] = blur[g][k];
                } else {
                    int b = (int)(a.order ? c[2] : c[0]), gg = (int)c[1], rr = (int)(a.order ? c[0] : c[2]);
                    int h, s, val;
                    ex_bgr2hsv(b, gg, rr, h, s, val);
                    ex_hsv2bgr(h, s, ((mask[g] >> (8 * k)) & 0xffu) ? (int)blur[g][k] : val, b, gg, rr);
                    c[0] = (uint32_t)(a.order ? rr : b), c[1] = (uint32_t)gg, c[2] = (uint32_t)(a.order ? b : rr);
                }
            }
        }
        uint8_t* o = out + (int64_t)row * out_pitch + (int64_t)x * C;
        if (n == 4) {
            ex_store4<C>(o, v);
        } else {
#pragma unroll
            for (int k = 0; k < 3 * C; ++k)
                if (k < n * C) o[k] = (uint8_t)v[k];
        }
    }
}

template <int MODE>
int ox_launch(const uint8_t* d_img, int64_t pitch, int channels, const OxArg& a, uint8_t* out, hipStream_t st) {
    const dim3 grid((unsigned)((a.W + kOxTW - 1) / kOxTW), (unsigned)((a.H + kOxTH - 1) / kOxTH));
    const int64_t out_pitch = frame_pitch(a.W, channels);
    if (channels == 3)
        ox_stencil_kernel<3, MODE><<<grid, 256, 0, st>>>(d_img, pitch, a, out, out_pitch);
    else
        ox_stencil_kernel<1, MODE><<<grid, 256, 0, st>>>(d_img, pitch, a, out, out_pitch);
    LIO_HIP(hipGetLastError());
    return kOk;
}

OxArg ox_arg(int width, int height, int order, int threshold, int dilate, int ksize, const uint16_t* w) {
    OxArg a{};
    a.W = width, a.H = height, a.order = order;
    a.threshold = threshold, a.rd = (dilate - 1) / 2, a.k = ksize;
    for (int i = 0; i < ksize; ++i) a.w[i] = w[i];
    return a;
}

// a frame from the host through one launch and back: the three stages of e.stencil_timer
template <int MODE>
int ox_run(ExposureBuf& e, const uint8_t* image, int channels, int64_t pitch, const OxArg& a, uint8_t* out, int64_t out_pitch,
           hipStream_t st) {
    const size_t in_bytes = frame_span(a.H, pitch, (size_t)a.W * (size_t)channels);
    int rc = reserve_frames({{&e.out, (size_t)frame_pitch(a.W, channels) * (size_t)a.H}, {&e.in, in_bytes}});
    if (rc) return rc;
    LIO_HIP(e.stencil_timer.mark(kOxUpload, st));
    LIO_HIP(e.in.upload(image, in_bytes, st));
    LIO_HIP(e.stencil_timer.mark(kOxKernel, st));
    if ((rc = ox_launch<MODE>(e.in.dev, pitch, channels, a, e.out.dev, st))) return rc;
    LIO_HIP(e.stencil_timer.mark(kOxDownload, st));
    return download_frame(e.out, e.stencil_timer, a.W, a.H, channels, out, out_pitch, st);
}

}  // namespace

void gaussian_weights(int ksize, double sigma, uint16_t* w) {
    static const double fixed[4][7] = {{1.0},
                                       {0.25, 0.5, 0.25},
                                       {0.0625, 0.25, 0.375, 0.25, 0.0625},
                                       {0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125}};
    double g[kOxMaxKsize];
    if (sigma <= 0.0 && ksize <= 7) {
        for (int i = 0; i < ksize; ++i) g[i] = fixed[ksize >> 1][i];
    } else {
        const double s = sigma > 0.0 ? sigma : ((ksize - 1) * 0.5 - 1.0) * 0.3 + 0.8;
        const double scale2 = -0.5 / (s * s);
        double sum = 0.0;
        for (int i = 0; i < ksize; ++i) {
            const double x = i - (ksize - 1) * 0.5;
            g[i] = std::exp(scale2 * x * x);
            sum += g[i];
        }
        const double inv = 1.0 / sum;
        for (int i = 0; i < ksize; ++i) g[i] = g[i] * inv;
    }
    double err = 0.0;
    int left = 0;
    for (int i = 0; i < ksize / 2; ++i) {  // error diffusion over the left half; rint: ties to even
        const double a = g[i] * 256.0 + err;
        const double wi = std::rint(a);
        w[i] = w[ksize - 1 - i] = (uint16_t)wi;
        err = a - wi;
        left += (int)wi;
    }
    w[ksize / 2] = (uint16_t)(256 - 2 * left);
}

int exposure_recover(ExposureBuf& e, const uint8_t* image, int width, int height, int channels, int64_t pitch, int order,
                     const OxRecover& p, uint8_t* out, int64_t out_pitch, hipStream_t st) {
    return ox_run<0>(e, image, channels, pitch, ox_arg(width, height, order, p.threshold, p.dilate, p.ksize, p.w), out, out_pitch, st);
}

int exposure_gaussian_blur(ExposureBuf& e, const uint8_t* image, int width, int height, int channels, int64_t pitch, int ksize,
                           const uint16_t* w, uint8_t* out, int64_t out_pitch, hipStream_t st) {
    return ox_run<1>(e, image, channels, pitch, ox_arg(width, height, 0, 0, 1, ksize, w), out, out_pitch, st);
}

int exposure_recover_undistorted(ExposureBuf& e, UndistortBuf& u, const uint8_t* raw, int64_t pitch, int order, const OxRecover& p,
                                 uint8_t* out, int64_t out_pitch, hipStream_t st) {
    int rc = reserve_frames({{&e.out, (size_t)frame_pitch(u.dw, u.channels) * (size_t)u.dh}});
    if (rc) return rc;
    // the upload stage here is the undistorter's upload and gather: the rectified frame stays in u.out.dev
    LIO_HIP(e.stencil_timer.mark(kOxUpload, st));
    if ((rc = undistorter_rectify(u, raw, pitch, st))) return rc;
    LIO_HIP(e.stencil_timer.mark(kOxKernel, st));
    const OxArg a = ox_arg(u.dw, u.dh, order, p.threshold, p.dilate, p.ksize, p.w);
    if ((rc = ox_launch<0>(u.out.dev, frame_pitch(u.dw, u.channels), u.channels, a, e.out.dev, st))) return rc;
    LIO_HIP(e.stencil_timer.mark(kOxDownload, st));
    return download_frame(e.out, e.stencil_timer, u.dw, u.dh, u.channels, out, out_pitch, st);
}

}  // namespace lio
