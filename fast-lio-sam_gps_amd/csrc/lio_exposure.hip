// lio_exposure.hip — exposure adaption on gfx950: the per-frame work of the reference's
// post_process/exposure_adaption scripts (lio_exposure.hpp), restated as our own contract (include/lio_gpu.h:
// lio_exposure_*): OpenCV's 8-bit BGR -> HSV in integers, CLAHE of one plane, HSV -> BGR in float32, table remaps.
// The file is compiled with -ffp-contract=off, host and device: no multiply-add is fused anywhere.
//
//   ex_hist_kernel   several workgroups per tile, each over a stripe of the tile's rows of the EXTENDED plane (the
//                    reflected border counts); a thread takes 4 consecutive pixels, loaded as ud_remap_kernel loads
//                    its taps, and adds V (or gray) into one of 16 copies of the 256 bins in LDS (copy = thread &
//                    15, copies 257 words apart): a saturated sky, every pixel in bin 255, meets 16 addresses on 16
//                    banks per wave instead of one.  The copies are summed and flushed with one global atomicAdd
//                    per non-empty bin into uint32 hist[tile][256], cleared by a memset on the stream.  Integer
//                    counts: the result does not depend on the order.
//   ex_lut_kernel    one 256-thread workgroup per tile, thread i owns bin i: the excess by a block reduction, the
//                    closed-form residual, an inclusive scan, the table byte.
//   ex_apply_kernel  4 pixels of a row per thread (block 64 x 4: a wave is 256 consecutive pixels of one row): the
//                    conversions, four table gathers per pixel and the float32 interpolation; 4 * channels bytes
//                    out as dwords into device rows that are a multiple of 4 bytes, the last partial group as bytes.
//                    The tables (16 KB at 8 x 8 tiles) are left to the cache: staging the few tables a block can
//                    reach in LDS gave the same bits and the same time (profiles/exposure_ab.md).  The same kernel
//                    with MODE 1 is the table remap of lio_exposure_remap.
#include <cstring>

#include "lio_exposure.hpp"
#include "lio_exposure_dev.hpp"
#include "lio_scratch.hpp"

namespace lio {
namespace {

constexpr int kExCopies = 16, kExCopyStride = 257;

// grid (tiles, stripes): the rows [blockIdx.y * rows_per, + rows_per) of tile blockIdx.x of the extended plane.
// x >= W reads 2 (W - 1) - x, rows likewise (the host has checked that the padding is at most the size - 1).
template <int C>
__global__ __launch_bounds__(256) void ex_hist_kernel(const uint8_t* __restrict__ img, int64_t pitch, int W, int H, int order,
                                                      int gray, int tiles_x, int tw, int th, int rows_per,
                                                      uint32_t* __restrict__ hist) {
    __shared__ uint32_t bins[kExCopies * kExCopyStride];
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < kExCopies * kExCopyStride; i += 256) bins[i] = 0;
    __syncthreads();
    const int tile = (int)blockIdx.x, ty = tile / tiles_x, tx = tile % tiles_x;
    const int r0 = (int)blockIdx.y * rows_per, r1 = min(th, r0 + rows_per);
    const int gpr = (tw + 3) >> 2;  // groups of 4 pixels per tile row
    const int items = max(r1 - r0, 0) * gpr;
    uint32_t* mine = bins + (tid & (kExCopies - 1)) * kExCopyStride;
    for (int it = tid; it < items; it += 256) {
        const int c0 = 4 * (it % gpr), n = min(4, tw - c0);
        const int ey = ty * th + r0 + it / gpr, ex = tx * tw + c0;
        const int sy = ey < H ? ey : max(2 * (H - 1) - ey, 0);
        const uint8_t* row = img + (int64_t)sy * pitch;
        if (n == 4 && ex + 3 < W) {
            uint32_t v[4 * C];
            ex_load4<C>(row + (int64_t)ex * C, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) atomicAdd(&mine[ex_value<C>(v + k * C, order, gray)], 1u);
        } else {
            for (int k = 0; k < n; ++k) {
                const int x = ex + k, sx = x < W ? x : max(2 * (W - 1) - x, 0);
                uint32_t v[C];
#pragma unroll
                for (int c = 0; c < C; ++c) v[c] = row[(int64_t)sx * C + c];
                atomicAdd(&mine[ex_value<C>(v, order, gray)], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < kExCopies; ++k) sum += bins[k * kExCopyStride + tid];
    if (sum) atomicAdd(&hist[(int64_t)tile * 256 + tid], sum);
}

// grid (tiles): hist[tile] -> lut[tile].  clip 0: no clipping.  scale = 255.0f / (float)area.
__global__ __launch_bounds__(256) void ex_lut_kernel(const uint32_t* __restrict__ hist, int clip, float scale,
                                                     uint8_t* __restrict__ lut) {
    __shared__ int sh[256];
    const int i = (int)threadIdx.x;
    const int64_t at = (int64_t)blockIdx.x * 256 + i;
    int h = (int)hist[at];
    if (clip > 0) {
        sh[i] = max(h - clip, 0);
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (i < s) sh[i] += sh[i + s];
            __syncthreads();
        }
        const int excess = sh[0];
        __syncthreads();
        h = min(h, clip);
        const int batch = excess / 256, res = excess - 256 * batch;
        h += batch;
        if (res > 0) {
            const int step = max(256 / res, 1);
            if (i % step == 0 && i / step < res) ++h;
        }
    }
    sh[i] = h;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {  // inclusive scan
        const int add = i >= off ? sh[i - off] : 0;
        __syncthreads();
        sh[i] += add;
        __syncthreads();
    }
    lut[at] = (uint8_t)ex_sat_rint((float)sh[i] * scale);
}

struct ExApplyArg {
    int W, H, order;
    int tiles_x, tiles_y;
    float inv_tw, inv_th;  // 1.0f / (float)tw, 1.0f / (float)th
    int has_v, has_all;    // MODE 1: lut holds lut_v (256) then lut_all (256)
};

// the tile pair and the weights of one coordinate: (float)x * inv - 0.5f, its floor and fraction
struct ExAxis {
    int t1, t2;
    float a, a1;
};
__device__ __forceinline__ ExAxis ex_axis(int x, float inv, int tiles) {
    const float f = (float)x * inv - 0.5f;
    const int t = (int)floorf(f);
    ExAxis o;
    o.a = f - (float)t;
    o.a1 = 1.f - o.a;
    o.t2 = min(t + 1, tiles - 1);
    o.t1 = min(max(t, 0), tiles - 1);  // t <= tiles - 1 for every x of the plane; the upper bound only guards memory
    return o;
}

// MODE 0: CLAHE; 1: table remap.  img rows of `pitch` bytes at any alignment; out rows out_pitch bytes, a multiple of
// 4 and this file's own buffer.
template <int C, int MODE>
__global__ __launch_bounds__(256) void ex_apply_kernel(const uint8_t* __restrict__ img, int64_t pitch, ExApplyArg a,
                                                       const uint8_t* __restrict__ lut, uint8_t* __restrict__ out,
                                                       int64_t out_pitch) {
    const int x = 4 * ((int)blockIdx.x * 64 + (int)threadIdx.x);
    const int row = (int)blockIdx.y * 4 + (int)threadIdx.y;
    if (row >= a.H || x >= a.W) return;
    const int n = min(4, a.W - x);
    const uint8_t* src = img + (int64_t)row * pitch + (int64_t)x * C;
    uint32_t v[4 * C];
    if (n == 4) {
        ex_load4<C>(src, v);
    } else {
#pragma unroll
        for (int k = 0; k < 3 * C; ++k) v[k] = k < n * C ? src[k] : 0u;
#pragma unroll
        for (int k = 3 * C; k < 4 * C; ++k) v[k] = 0u;
    }
    ExAxis ay{};
    if constexpr (MODE == 0) ay = ex_axis(row, a.inv_th, a.tiles_y);
    auto table = [&](int ty, int tx, int p) -> float { return (float)lut[((int64_t)ty * a.tiles_x + tx) * 256 + p]; };
    // the new value of plane value p at column xx
    auto adapt = [&](int p, int xx) -> int {
        if constexpr (MODE == 1) {
            return a.has_v ? (int)lut[p] : p;
        } else {
            const ExAxis ax = ex_axis(xx, a.inv_tw, a.tiles_x);
            const float top = table(ay.t1, ax.t1, p) * ax.a1 + table(ay.t1, ax.t2, p) * ax.a;
            const float bot = table(ay.t2, ax.t1, p) * ax.a1 + table(ay.t2, ax.t2, p) * ax.a;
            return ex_sat_rint(top * ay.a1 + bot * ay.a);
        }
    };
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k >= n) break;
        uint32_t* c = v + k * C;
        if constexpr (C == 1) {
            int p = adapt((int)c[0], x + k);
            if (MODE == 1 && a.has_all) p = lut[256 + p];
            c[0] = (uint32_t)p;
        } else {
            int b = (int)(a.order ? c[2] : c[0]), g = (int)c[1], r = (int)(a.order ? c[0] : c[2]);
            if (MODE == 0 || a.has_v) {
                int h, s, val;
                ex_bgr2hsv(b, g, r, h, s, val);
                ex_hsv2bgr(h, s, adapt(val, x + k), b, g, r);
            }
            if (MODE == 1 && a.has_all) b = lut[256 + b], g = lut[256 + g], r = lut[256 + r];
            c[0] = (uint32_t)(a.order ? r : b), c[1] = (uint32_t)g, c[2] = (uint32_t)(a.order ? b : r);
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

// everything a run of `tiles` tiles needs, reserved before anything is enqueued: the arena (hist, lut), the result
// of out_height rows (0: the run returns no image), then the input (in_bytes 0: the frame is on the device already)
int ex_reserve(ExposureBuf& e, int64_t tiles, size_t in_bytes, int width, int out_height, int channels, uint32_t** hist,
               uint8_t** lut) {
    auto fields = [&](Carver& c) {
        c(*hist, (size_t)tiles * 256);
        c(*lut, (size_t)std::max<int64_t>(tiles, 2) * 256);
    };
    int rc = reserve_arena(&e.arena, e.arena_bytes, fields);
    if (!rc) rc = reserve_frames({{&e.out, (size_t)frame_pitch(width, channels) * (size_t)out_height}});
    if (!rc) rc = reserve_frames({{&e.in, in_bytes}});
    return rc;
}

// the upload stage: the frame into e.in
int ex_upload(ExposureBuf& e, const uint8_t* image, size_t in_bytes, hipStream_t st) {
    LIO_HIP(e.timer.mark(kExUpload, st));
    LIO_HIP(e.in.upload(image, in_bytes, st));
    LIO_HIP(e.timer.mark(kExHist, st));
    return kOk;
}

// hist[tiles][256] of V (gray: of gray) of the device image, cleared first
int ex_launch_hist(const uint8_t* d_img, int64_t pitch, int width, int height, int channels, int order, int gray, int tiles_x,
                   int tiles_y, int tw, int th, uint32_t* hist, hipStream_t st) {
    const int tiles = tiles_x * tiles_y;
    LIO_HIP(hipMemsetAsync(hist, 0, (size_t)tiles * 256 * sizeof(uint32_t), st));
    const int rows_per = std::min(th, std::max(1, (8192 + tw - 1) / tw));  // about 8192 pixels per workgroup
    const dim3 grid((unsigned)tiles, (unsigned)((th + rows_per - 1) / rows_per));
    if (channels == 3)
        ex_hist_kernel<3><<<grid, 256, 0, st>>>(d_img, pitch, width, height, order, gray, tiles_x, tw, th, rows_per, hist);
    else
        ex_hist_kernel<1><<<grid, 256, 0, st>>>(d_img, pitch, width, height, order, gray, tiles_x, tw, th, rows_per, hist);
    LIO_HIP(hipGetLastError());
    return kOk;
}

template <int MODE>
int ex_launch_apply(const uint8_t* d_img, int64_t pitch, int channels, const ExApplyArg& a, const uint8_t* lut, uint8_t* out,
                    hipStream_t st) {
    const dim3 block(64, 4), grid((unsigned)((a.W + 255) / 256), (unsigned)((a.H + 3) / 4));
    const int64_t out_pitch = frame_pitch(a.W, channels);
    if (channels == 3)
        ex_apply_kernel<3, MODE><<<grid, block, 0, st>>>(d_img, pitch, a, lut, out, out_pitch);
    else
        ex_apply_kernel<1, MODE><<<grid, block, 0, st>>>(d_img, pitch, a, lut, out, out_pitch);
    LIO_HIP(hipGetLastError());
    return kOk;
}

// the stages kExHist .. kExApply: histograms, tables and the apply of the device image into e.out
int ex_clahe_device(ExposureBuf& e, const uint8_t* d_img, int64_t pitch, int width, int height, int channels, int order,
                    const ExTiling& t, uint32_t* hist, uint8_t* lut, hipStream_t st) {
    int rc = ex_launch_hist(d_img, pitch, width, height, channels, order, 0, t.tiles_x, t.tiles_y, t.tw, t.th, hist, st);
    if (rc) return rc;
    LIO_HIP(e.timer.mark(kExLut, st));
    const float scale = 255.0f / (float)(t.tw * t.th);
    ex_lut_kernel<<<t.tiles_x * t.tiles_y, 256, 0, st>>>(hist, t.clip, scale, lut);
    LIO_HIP(hipGetLastError());
    LIO_HIP(e.timer.mark(kExApply, st));
    ExApplyArg a{};
    a.W = width, a.H = height, a.order = order, a.tiles_x = t.tiles_x, a.tiles_y = t.tiles_y;
    a.inv_tw = 1.0f / (float)t.tw, a.inv_th = 1.0f / (float)t.th;
    if ((rc = ex_launch_apply<0>(d_img, pitch, channels, a, lut, e.out.dev, st))) return rc;
    LIO_HIP(e.timer.mark(kExDownload, st));
    return kOk;
}

}  // namespace

int exposure_tiling(int width, int height, double clip_limit, int tiles_x, int tiles_y, ExTiling* t, const char** why) {
    t->tiles_x = tiles_x, t->tiles_y = tiles_y;
    t->ext_w = width, t->ext_h = height;
    if (width % tiles_x != 0 || height % tiles_y != 0) {
        const int pad_w = tiles_x - width % tiles_x, pad_h = tiles_y - height % tiles_y;
        if (pad_w > width - 1 || pad_h > height - 1) {
            *why = "the reflected padding (tiles_x - width % tiles_x columns, tiles_y - height % tiles_y rows) must be at most "
                   "width - 1 and height - 1";
            return kArg;
        }
        t->ext_w = width + pad_w, t->ext_h = height + pad_h;
    }
    t->tw = t->ext_w / tiles_x, t->th = t->ext_h / tiles_y;
    t->clip = 0;
    if (!(clip_limit <= 0.0)) {
        const double c = clip_limit * (double)(t->tw * t->th) / 256.0;
        if (!(c < 2147483648.0)) {
            *why = "clip_limit x tile area / 256 must be below 2^31 and not NaN";
            return kArg;
        }
        t->clip = std::max((int)c, 1);
    }
    return kOk;
}

int exposure_init(ExposureBuf& e) {
    LIO_HIP(e.timer.init());
    LIO_HIP(e.stencil_timer.init());
    return grow_pinned(&e.h_small, e.h_small_bytes, 2 * 256 * sizeof(uint32_t), 0);
}

void exposure_free(ExposureBuf& e) {
    dev_free(&e.arena);
    host_free(&e.h_small);
    e.in.free();
    e.out.free();
    e.timer.free();
    e.stencil_timer.free();
    e = ExposureBuf{};
}

int exposure_histograms(ExposureBuf& e, const uint8_t* image, int width, int height, int channels, int64_t pitch, int order,
                        int64_t* hist_v_opt, int64_t* hist_gray_opt, hipStream_t st) {
    uint32_t* hist = nullptr;
    uint8_t* lut = nullptr;
    const size_t in_bytes = frame_span(height, pitch, (size_t)width * (size_t)channels);
    int rc = ex_reserve(e, 2, in_bytes, width, 0, channels, &hist, &lut);  // two 1 x 1 tilings: V, then gray
    if (rc) return rc;
    if ((rc = ex_upload(e, image, in_bytes, st))) return rc;
    if (hist_v_opt && (rc = ex_launch_hist(e.in.dev, pitch, width, height, channels, order, 0, 1, 1, width, height, hist, st)))
        return rc;
    if (hist_gray_opt &&
        (rc = ex_launch_hist(e.in.dev, pitch, width, height, channels, order, 1, 1, 1, width, height, hist + 256, st)))
        return rc;
    LIO_HIP(e.timer.mark(kExLut, kExDownload, st));  // no tables, no apply
    LIO_HIP(hipMemcpyAsync(e.h_small, hist, 2 * 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    LIO_HIP(e.timer.mark(kExStages, st));
    LIO_HIP(e.timer.finish(st));
    for (int i = 0; i < 256; ++i) {
        if (hist_v_opt) hist_v_opt[i] = (int64_t)e.h_small[i];
        if (hist_gray_opt) hist_gray_opt[i] = (int64_t)e.h_small[256 + i];
    }
    return kOk;
}

int exposure_clahe(ExposureBuf& e, const uint8_t* image, int width, int height, int channels, int64_t pitch, int order,
                   const ExTiling& t, uint8_t* out, int64_t out_pitch, hipStream_t st) {
    uint32_t* hist = nullptr;
    uint8_t* lut = nullptr;
    const size_t in_bytes = frame_span(height, pitch, (size_t)width * (size_t)channels);
    int rc = ex_reserve(e, (int64_t)t.tiles_x * t.tiles_y, in_bytes, width, height, channels, &hist, &lut);
    if (rc) return rc;
    if ((rc = ex_upload(e, image, in_bytes, st))) return rc;
    if ((rc = ex_clahe_device(e, e.in.dev, pitch, width, height, channels, order, t, hist, lut, st))) return rc;
    return download_frame(e.out, e.timer, width, height, channels, out, out_pitch, st);
}

int exposure_remap(ExposureBuf& e, const uint8_t* image, int width, int height, int channels, int64_t pitch, int order,
                   const uint8_t* lut_v_opt, const uint8_t* lut_all_opt, uint8_t* out, int64_t out_pitch, hipStream_t st) {
    uint32_t* hist = nullptr;
    uint8_t* lut = nullptr;
    const size_t in_bytes = frame_span(height, pitch, (size_t)width * (size_t)channels);
    int rc = ex_reserve(e, 1, in_bytes, width, height, channels, &hist, &lut);
    if (rc) return rc;
    if ((rc = ex_upload(e, image, in_bytes, st))) return rc;
    LIO_HIP(e.timer.mark(kExLut, st));
    uint8_t* h_lut = reinterpret_cast<uint8_t*>(e.h_small);
    std::memset(h_lut, 0, 512);
    if (lut_v_opt) std::memcpy(h_lut, lut_v_opt, 256);
    if (lut_all_opt) std::memcpy(h_lut + 256, lut_all_opt, 256);
    LIO_HIP(hipMemcpyAsync(lut, h_lut, 512, hipMemcpyHostToDevice, st));
    LIO_HIP(e.timer.mark(kExApply, st));
    ExApplyArg a{};
    a.W = width, a.H = height, a.order = order, a.tiles_x = 1, a.tiles_y = 1;
    a.has_v = lut_v_opt != nullptr, a.has_all = lut_all_opt != nullptr;
    if ((rc = ex_launch_apply<1>(e.in.dev, pitch, channels, a, lut, e.out.dev, st))) return rc;
    LIO_HIP(e.timer.mark(kExDownload, st));
    return download_frame(e.out, e.timer, width, height, channels, out, out_pitch, st);
}

int exposure_clahe_undistorted(ExposureBuf& e, UndistortBuf& u, const uint8_t* raw, int64_t pitch, int order, const ExTiling& t,
                               uint8_t* out, int64_t out_pitch, hipStream_t st) {
    uint32_t* hist = nullptr;
    uint8_t* lut = nullptr;
    int rc = ex_reserve(e, (int64_t)t.tiles_x * t.tiles_y, 0, u.dw, u.dh, u.channels, &hist, &lut);
    if (rc) return rc;
    // the upload stage here is the undistorter's upload and gather: the rectified frame stays in u.out.dev
    LIO_HIP(e.timer.mark(kExUpload, st));
    if ((rc = undistorter_rectify(u, raw, pitch, st))) return rc;
    LIO_HIP(e.timer.mark(kExHist, st));
    if ((rc = ex_clahe_device(e, u.out.dev, frame_pitch(u.dw, u.channels), u.dw, u.dh, u.channels, order, t, hist, lut, st)))
        return rc;
    return download_frame(e.out, e.timer, u.dw, u.dh, u.channels, out, out_pitch, st);
}

}  // namespace lio
