// lio_overlay.hip — point overlay drawing on gfx950: the camera image with every projected point drawn as a filled
// disc, the output of the reference's projection tool (post_process/lidar_projection/src/lidar_projection.cpp:113-125:
// cv::circle(image, pt, 3, colour, -1) per point, later points over earlier ones), by the contract of
// include/lio_gpu.h (lio_overlay_*).  The file is compiled with -ffp-contract=off, host and device.
//
// Each pixel has one 64-bit key, all ones where empty; a drawn point i offers (hi << 32) | (0xFFFFFFFF - i) to every
// pixel of its clipped disc and the minimum stays.  hi = 0: the highest index wins, which is the tool's sequential
// loop.  hi = bits((float)zc), zc > 0: the nearest point wins, the higher index on equal float depth.  One code path,
// and a minimum does not depend on the order in which the points arrive.
//   ov_fill_kernel     the key image to the empty pattern, 16 bytes per thread
//   ov_stamp_kernel    one thread per point: cz_project (the colorizer's, lio_camera_dev.hpp), the centre rounded to
//                      even, then the clipped spans of the host's half-width table with atomicMin.  A pixel is read
//                      before its atomic and the atomic skipped when the key there is already not larger: keys only
//                      decrease, so a skipped atomic would have changed nothing (a stale read only costs an atomic
//                      that changes nothing).
//   ov_compose_kernel  one thread per 4 pixels of a row: the keys, the owners' colours, the source pixel otherwise,
//                      stored as dwords at frame_pitch; the owner image if asked for
#include <algorithm>

#include "lio_camera_dev.hpp"
#include "lio_overlay.hpp"
#include "lio_scratch.hpp"

// 0: every pixel of a disc takes its atomic unread.  A timing diagnostic between two builds; the keys,
// and with them every output, are the same either way.
#ifndef LIO_OV_READ_FIRST
#define LIO_OV_READ_FIRST 1
#endif

namespace lio {

namespace {

__global__ __launch_bounds__(256) void ov_fill_kernel(uint4* __restrict__ d, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) d[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
}

// keys: cam.height rows of key_pitch keys (key_pitch: cam.width rounded up to 4).  Every thread of the workgroup
// reaches the count.
__global__ __launch_bounds__(256) void ov_stamp_kernel(const float* __restrict__ pts, int64_t n, int stride, CamArg cam,
                                                       OvDisc disc, int nearest, const int32_t* __restrict__ labels,
                                                       unsigned long long* keys, int key_pitch,
                                                       unsigned long long* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool drawn = false;
    if (i < n && (!labels || labels[i] >= 0)) {
        const Projected o = cz_project(pts + (size_t)i * stride, cam);
        if (o.valid) {
            drawn = true;
            // 0 <= u < width, so the centre is in 0 .. width (ties to even): the spans below are clipped, never wrapped
            const int cx = (int)rint(o.u), cy = (int)rint(o.v);
            const unsigned long long hi = nearest ? (unsigned long long)__float_as_uint((float)o.zc) : 0ull;
            const unsigned long long key = (hi << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
            const int y0 = max(cy - disc.r, 0), y1 = min(cy + disc.r, cam.height - 1);
            for (int qy = y0; qy <= y1; ++qy) {
                const int w = (int)disc.half[abs(qy - cy)];
                const int x0 = max(cx - w, 0), x1 = min(cx + w, cam.width - 1);
                unsigned long long* row = keys + (size_t)qy * (size_t)key_pitch;
                for (int qx = x0; qx <= x1; ++qx) {
#if LIO_OV_READ_FIRST
                    if (row[qx] > key) atomicMin(row + qx, key);
#else
                    atomicMin(row + qx, key);
#endif
                }
            }
        }
    }
    const int c = __syncthreads_count(drawn ? 1 : 0);
    if (threadIdx.x == 0 && c) atomicAdd(count, (unsigned long long)c);
}

// the three bytes of point idx: its own colour, else its label's palette row, else row 0 (an owner's label is >= 0)
__device__ __forceinline__ void ov_colour(uint32_t idx, const uint8_t* __restrict__ colors, const int32_t* __restrict__ labels,
                                          const uint8_t* __restrict__ palette, int palette_rows, uint32_t* c) {
    const uint8_t* q = colors ? colors + 3 * (size_t)idx : palette + 3 * (size_t)(labels ? labels[idx] % palette_rows : 0);
    c[0] = q[0], c[1] = q[1], c[2] = q[2];
}

// block 64 x 4: a wave is 256 consecutive pixels of one row.  src rows are src_pitch bytes at any alignment (the
// caller's), out rows out_pitch bytes (a multiple of 4, at least 3 * width: this file's own buffer), owner rows width
// values.
__global__ __launch_bounds__(256) void ov_compose_kernel(const uint8_t* __restrict__ src, int64_t src_pitch, int width, int height,
                                                         const unsigned long long* __restrict__ keys, int key_pitch,
                                                         const uint8_t* __restrict__ colors, const int32_t* __restrict__ labels,
                                                         const uint8_t* __restrict__ palette, int palette_rows,
                                                         uint8_t* __restrict__ out, int64_t out_pitch,
                                                         int32_t* __restrict__ owner) {
    const int x = 4 * ((int)blockIdx.x * 64 + (int)threadIdx.x);
    const int row = (int)blockIdx.y * 4 + (int)threadIdx.y;
    if (row >= height || x >= width) return;
    const ulonglong2* k2 = reinterpret_cast<const ulonglong2*>(keys + (size_t)row * (size_t)key_pitch + (size_t)x);
    const ulonglong2 k01 = k2[0], k23 = k2[1];
    const unsigned long long k[4] = {k01.x, k01.y, k23.x, k23.y};
    const int pixels = min(4, width - x);  // the keys of the row's padding are never stamped: they stay empty
    const uint8_t* s = src + (int64_t)row * src_pitch + (int64_t)x * 3;
    uint32_t v[12];
    if (pixels == 4) {
        uint32_t w[3];
        __builtin_memcpy(w, s, 12);
#pragma unroll
        for (int b = 0; b < 12; ++b) v[b] = (w[b >> 2] >> (8 * (b & 3))) & 0xffu;
    } else {
#pragma unroll
        for (int b = 0; b < 9; ++b) v[b] = b < 3 * pixels ? (uint32_t)s[b] : 0u;
        v[9] = v[10] = v[11] = 0u;
    }
    int32_t own[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        own[j] = -1;
        if (k[j] != kOvEmpty) {
            const uint32_t idx = 0xFFFFFFFFu - (uint32_t)k[j];
            own[j] = (int32_t)idx;
            ov_colour(idx, colors, labels, palette, palette_rows, v + 3 * j);
        }
    }
    uint8_t* o = out + (int64_t)row * out_pitch + (int64_t)x * 3;
    if (pixels == 4) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
        for (int q = 0; q < 3; ++q) o4[q] = v[4 * q] | (v[4 * q + 1] << 8) | (v[4 * q + 2] << 16) | (v[4 * q + 3] << 24);
    } else {
#pragma unroll
        for (int b = 0; b < 9; ++b)
            if (b < 3 * pixels) o[b] = (uint8_t)v[b];
    }
    if (owner) {
        int32_t* w = owner + (size_t)row * (size_t)width + (size_t)x;
        if (pixels == 4 && (width & 3) == 0) {
            *reinterpret_cast<int4*>(w) = make_int4(own[0], own[1], own[2], own[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < pixels) w[j] = own[j];
        }
    }
}

// `count` elements at `host` into *dev, grown to hold them (at least one, so the pointer is never null)
template <class T>
int ov_upload(T** dev, int64_t& cap, const T* host, int64_t count, hipStream_t st) {
    const int rc = grow_buf(dev, cap, std::max<int64_t>(count, 1));
    if (rc) return rc;
    if (count > 0) LIO_HIP(hipMemcpyAsync(*dev, host, (size_t)count * sizeof(T), hipMemcpyHostToDevice, st));
    LIO_HIP(hipStreamSynchronize(st));
    return kOk;
}

}  // namespace

OvDisc overlay_disc(int radius) {
    OvDisc d{};
    d.r = radius;
    // OpenCV's filled circle (drawing.cpp, Circle with fill): the rows cy +- dy take the half-width dx, the rows
    // cy +- dx the half-width dy; a row reached twice keeps the wider span
    int err = 0, dx = radius, dy = 0, plus = 1, minus = 2 * radius - 1;
    while (dx >= dy) {
        d.half[dy] = (uint8_t)std::max<int>(d.half[dy], dx);
        d.half[dx] = (uint8_t)std::max<int>(d.half[dx], dy);
        ++dy;
        err += plus;
        plus += 2;
        if (err > 0) {
            err -= minus;
            --dx;
            minus -= 2;
        }
    }
    return d;
}

int overlay_init(OverlayBuf& o, hipStream_t st) {
    count_alloc(2);
    if (hipMalloc(reinterpret_cast<void**>(&o.count), sizeof(unsigned long long)) != hipSuccess) return kNoMem;
    if (hipHostMalloc(reinterpret_cast<void**>(&o.h_count), sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess)
        return kNoMem;
    LIO_HIP(o.timer.init());
    const uint8_t green[3] = {0, 255, 0};
    return overlay_set_palette(o, green, 1, st);
}

void overlay_free(OverlayBuf& o) {
    dev_free(&o.pts, &o.labels, &o.colors, &o.palette, &o.keys, &o.owner, &o.count);
    host_free(&o.h_count);
    o.in.free();
    o.out.free();
    o.timer.free();
    o = OverlayBuf{};
}

int overlay_set_cloud(OverlayBuf& o, const float* pts, int64_t n, int stride, hipStream_t st) {
    o.have_cloud = o.have_labels = o.have_colors = false;
    o.n = 0;
    const int rc = ov_upload(&o.pts, o.pts_cap, pts, n * stride, st);
    if (rc) return rc;
    o.n = n;
    o.stride = stride;
    o.have_cloud = true;
    return kOk;
}

int overlay_set_labels(OverlayBuf& o, const int32_t* labels, hipStream_t st) {
    o.have_labels = false;
    if (!labels) return kOk;
    const int rc = ov_upload(&o.labels, o.labels_cap, labels, o.n, st);
    if (rc) return rc;
    o.have_labels = true;
    return kOk;
}

int overlay_set_colors(OverlayBuf& o, const uint8_t* colors, hipStream_t st) {
    o.have_colors = false;
    if (!colors) return kOk;
    const int rc = ov_upload(&o.colors, o.colors_cap, colors, 3 * o.n, st);
    if (rc) return rc;
    o.have_colors = true;
    return kOk;
}

int overlay_set_palette(OverlayBuf& o, const uint8_t* palette, int32_t rows, hipStream_t st) {
    o.palette_rows = 0;
    const int rc = ov_upload(&o.palette, o.palette_cap, palette, 3 * (int64_t)rows, st);
    if (rc) return rc;
    o.palette_rows = rows;
    return kOk;
}

int overlay_draw(OverlayBuf& o, UndistortBuf* u, const CamArg& cam, const OvDisc& disc, int order, const uint8_t* image,
                 int64_t pitch, uint8_t* out, int64_t out_pitch, int32_t* owner_opt, int64_t* n_drawn, hipStream_t st) {
    const int W = cam.width, H = cam.height;
    const int key_pitch = (W + 3) & ~3;
    const int64_t d_pitch = frame_pitch(W, 3);
    const size_t in_bytes = u ? 0 : frame_span(H, pitch, (size_t)W * 3);
    int rc = reserve_frames({{&o.in, in_bytes}, {&o.out, (size_t)d_pitch * (size_t)H}});
    if (!rc) rc = grow_buf(&o.keys, o.keys_cap, (int64_t)key_pitch * H);
    if (!rc && owner_opt) rc = grow_buf(&o.owner, o.owner_cap, (int64_t)W * H);
    if (rc) return rc;
    // the upload stage of the chained call is the undistorter's upload and gather: the rectified frame stays in u->out.dev
    LIO_HIP(o.timer.mark(kOvUpload, st));
    if (u) {
        if ((rc = undistorter_rectify(*u, image, pitch, st))) return rc;
    } else {
        LIO_HIP(o.in.upload(image, in_bytes, st));
    }
    const uint8_t* d_src = u ? u->out.dev : o.in.dev;
    const int64_t src_pitch = u ? d_pitch : pitch;
    LIO_HIP(hipMemsetAsync(o.count, 0, sizeof(unsigned long long), st));
    LIO_HIP(o.timer.mark(kOvFill, st));
    const int64_t n4 = (int64_t)key_pitch * H / 2;  // two keys per 16 bytes; key_pitch is a multiple of 4
    ov_fill_kernel<<<nblk(n4), 256, 0, st>>>(reinterpret_cast<uint4*>(o.keys), n4);
    LIO_HIP(o.timer.mark(kOvStamp, st));
    if (o.n > 0)
        ov_stamp_kernel<<<nblk(o.n), 256, 0, st>>>(o.pts, o.n, o.stride, cam, disc, order == kOvNearest ? 1 : 0,
                                                   (o.have_labels && !o.have_colors) ? o.labels : nullptr, o.keys, key_pitch,
                                                   o.count);
    LIO_HIP(o.timer.mark(kOvCompose, st));
    const dim3 block(64, 4), grid((unsigned)((W + 255) / 256), (unsigned)((H + 3) / 4));
    ov_compose_kernel<<<grid, block, 0, st>>>(d_src, src_pitch, W, H, o.keys, key_pitch, o.have_colors ? o.colors : nullptr,
                                              o.have_labels ? o.labels : nullptr, o.palette, o.palette_rows, o.out.dev, d_pitch,
                                              owner_opt ? o.owner : nullptr);
    LIO_HIP(hipGetLastError());
    LIO_HIP(o.timer.mark(kOvDownload, st));
    if (owner_opt) LIO_HIP(hipMemcpyAsync(owner_opt, o.owner, (size_t)W * (size_t)H * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    LIO_HIP(hipMemcpyAsync(o.h_count, o.count, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if ((rc = download_frame(o.out, o.timer, W, H, 3, out, out_pitch, st))) return rc;
    *n_drawn = (int64_t)*o.h_count;
    return kOk;
}

}  // namespace lio
