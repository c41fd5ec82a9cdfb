// lio_colorize.hip — camera projection and point cloud colorization from images on gfx950: the camera step of
// the reference's offline leg (post_process/colorize_pcd.py:31-65; the projection role of
// post_process/lidar_projection/src/lidar_projection.cpp:9-34; the 8-parameter rational model of
// post_process/undistort_image.py:95-97), restated as IEEE double operations in a written order
// (include/lio_gpu.h: lio_project_points, lio_colorizer_*).  The file is compiled with -ffp-contract=off, host
// and device: no multiply-add is fused anywhere.
//
// One thread per point everywhere.  cz_project (lio_camera_dev.hpp) is the ONLY projection: the project, fused,
// splat and resolve kernels all call it, so a point's pixel and depth are the same bits in every pass.
//   without occlusion  cz_fused_kernel: project, gather the pixel, replace the state where zc < best_z
//   with occlusion     cz_fill_kernel (the depth image to the bits of +inf) -> cz_splat_kernel (atomicMin of the
//                      float depth's bits over the clipped splat) -> cz_resolve_kernel (project again, the
//                      visibility test, gather, replace)
// A float depth that is >= 0 orders as its bits do, so the minimum — and with it every output — does not depend
// on the order in which the points arrive.  The splat reads a pixel before its atomic and skips the atomic when
// the pixel already holds a depth that is not larger: the depth image only ever decreases, so a skipped atomic
// would have changed nothing (a stale read only costs an atomic that changes nothing).
#include <algorithm>

#include "lio_camera_dev.hpp"
#include "lio_colorize.hpp"
#include "lio_scratch.hpp"

namespace lio {

namespace {

__global__ __launch_bounds__(256) void cz_project_kernel(const float* __restrict__ pts, int64_t n, int stride, CamArg cam,
                                                         double2* __restrict__ uv, double* __restrict__ zc,
                                                         int2* __restrict__ pix, uint8_t* __restrict__ valid) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Projected o = cz_project(pts + (size_t)i * stride, cam);
    if (uv) uv[i] = make_double2(o.u, o.v);
    if (zc) zc[i] = o.zc;
    if (pix) pix[i] = make_int2(o.px, o.py);
    valid[i] = o.valid ? 1 : 0;
}

__global__ __launch_bounds__(256) void cz_reset_kernel(double* __restrict__ best_z, uint8_t* __restrict__ rgb,
                                                       int32_t* __restrict__ frame, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    best_z[i] = __longlong_as_double(0x7ff0000000000000ll);
    rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = 0;
    frame[i] = -1;
}

// a candidate replaces the state iff zc < best_z (strict: on a tie the earlier frame stays); true when it did
__device__ __forceinline__ bool cz_update(int64_t i, const Projected& o, const uint8_t* __restrict__ img, int64_t pitch,
                                          bool bgr, int32_t frame_no, double* __restrict__ best_z, uint8_t* __restrict__ rgb,
                                          int32_t* __restrict__ frame) {
    if (!(o.zc < best_z[i])) return false;
    const uint8_t* q = img + (size_t)o.py * (size_t)pitch + (size_t)o.px * 3;
    const uint8_t c0 = q[0], c1 = q[1], c2 = q[2];
    best_z[i] = o.zc;
    rgb[3 * i] = bgr ? c2 : c0;
    rgb[3 * i + 1] = c1;
    rgb[3 * i + 2] = bgr ? c0 : c2;
    frame[i] = frame_no;
    return true;
}

// the frame's replacements: counted per workgroup, then one atomic per workgroup that has any (integer adds: the
// total does not depend on their order).  Every thread of the workgroup calls it.
__device__ __forceinline__ void cz_count(bool replaced, unsigned long long* __restrict__ count) {
    const int c = __syncthreads_count(replaced ? 1 : 0);
    if (threadIdx.x == 0 && c) atomicAdd(count, (unsigned long long)c);
}

__global__ __launch_bounds__(256) void cz_fused_kernel(const float* __restrict__ pts, int64_t n, int stride, CamArg cam,
                                                       const uint8_t* __restrict__ img, int64_t pitch, bool bgr,
                                                       int32_t frame_no, double* __restrict__ best_z,
                                                       uint8_t* __restrict__ rgb, int32_t* __restrict__ frame,
                                                       unsigned long long* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool replaced = false;
    if (i < n) {
        const Projected o = cz_project(pts + (size_t)i * stride, cam);
        if (o.valid) replaced = cz_update(i, o, img, pitch, bgr, frame_no, best_z, rgb, frame);
    }
    cz_count(replaced, count);
}

__global__ __launch_bounds__(256) void cz_fill_kernel(uint4* __restrict__ d, int64_t n4, uint32_t pattern) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) d[i] = make_uint4(pattern, pattern, pattern, pattern);
}

__global__ __launch_bounds__(256) void cz_splat_kernel(const float* __restrict__ pts, int64_t n, int stride, CamArg cam,
                                                       int radius, uint32_t* depth) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Projected o = cz_project(pts + (size_t)i * stride, cam);
    if (!o.valid) return;
    const uint32_t zb = __float_as_uint((float)o.zc);
    const int x0 = max(o.px - radius, 0), x1 = min(o.px + radius, cam.width - 1);
    const int y0 = max(o.py - radius, 0), y1 = min(o.py + radius, cam.height - 1);
    for (int qy = y0; qy <= y1; ++qy) {
        uint32_t* row = depth + (size_t)qy * (size_t)cam.width;
        for (int qx = x0; qx <= x1; ++qx)
            if (row[qx] > zb) atomicMin(row + qx, zb);
    }
}

__global__ __launch_bounds__(256) void cz_resolve_kernel(const float* __restrict__ pts, int64_t n, int stride, CamArg cam,
                                                         const uint32_t* __restrict__ depth, float depth_rel,
                                                         float depth_abs, const uint8_t* __restrict__ img, int64_t pitch,
                                                         bool bgr, int32_t frame_no, double* __restrict__ best_z,
                                                         uint8_t* __restrict__ rgb, int32_t* __restrict__ frame,
                                                         unsigned long long* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool replaced = false;
    if (i < n) {
        const Projected o = cz_project(pts + (size_t)i * stride, cam);
        if (o.valid) {
            const float zf = (float)o.zc;
            const float d = __uint_as_float(depth[(size_t)o.py * (size_t)cam.width + (size_t)o.px]);
            const float bound = (d * (1.0f + depth_rel)) + depth_abs;
            if (zf <= bound) replaced = cz_update(i, o, img, pitch, bgr, frame_no, best_z, rgb, frame);
        }
    }
    cz_count(replaced, count);
}

}  // namespace

void project_free(ProjectBuf& b) {
    dev_free(&b.arena);
    b = ProjectBuf{};
}

int project_points(ProjectBuf& b, const float* d_pts, int64_t n, int stride, const CamArg& cam, double* uv_opt,
                   double* zc_opt, int32_t* pix_opt, uint8_t* valid, hipStream_t st) {
    if (n <= 0) return kOk;
    double2* d_uv = nullptr;
    double* d_zc = nullptr;
    int2* d_pix = nullptr;
    uint8_t* d_valid = nullptr;
    auto fields = [&](Carver& c) {
        c(d_uv, uv_opt ? (size_t)n : 0);
        c(d_zc, zc_opt ? (size_t)n : 0);
        c(d_pix, pix_opt ? (size_t)n : 0);
        c(d_valid, (size_t)n);
    };
    const int rc = reserve_arena(&b.arena, b.arena_bytes, fields);
    if (rc) return rc;
    if (!uv_opt) d_uv = nullptr;
    if (!zc_opt) d_zc = nullptr;
    if (!pix_opt) d_pix = nullptr;
    cz_project_kernel<<<nblk(n), 256, 0, st>>>(d_pts, n, stride, cam, d_uv, d_zc, d_pix, d_valid);
    LIO_HIP(hipGetLastError());
    if (uv_opt) LIO_HIP(hipMemcpyAsync(uv_opt, d_uv, (size_t)n * sizeof(double2), hipMemcpyDeviceToHost, st));
    if (zc_opt) LIO_HIP(hipMemcpyAsync(zc_opt, d_zc, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (pix_opt) LIO_HIP(hipMemcpyAsync(pix_opt, d_pix, (size_t)n * sizeof(int2), hipMemcpyDeviceToHost, st));
    LIO_HIP(hipMemcpyAsync(valid, d_valid, (size_t)n, hipMemcpyDeviceToHost, st));
    LIO_HIP(hipStreamSynchronize(st));
    return kOk;
}

int colorizer_init(ColorizeBuf& c) {
    count_alloc(2);
    if (hipMalloc(reinterpret_cast<void**>(&c.count), sizeof(unsigned long long)) != hipSuccess) return kNoMem;
    if (hipHostMalloc(reinterpret_cast<void**>(&c.h_count), sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess)
        return kNoMem;
    LIO_HIP(c.timer.init());
    return kOk;
}

void colorizer_free(ColorizeBuf& c) {
    dev_free(&c.pts, &c.best_z, &c.rgb, &c.frame, &c.depth, &c.count);
    host_free(&c.h_count);
    c.in.free();
    c.timer.free();
    c = ColorizeBuf{};
}

int colorizer_reset(ColorizeBuf& c, hipStream_t st) {
    c.frames = 0;
    if (c.n > 0) {
        cz_reset_kernel<<<nblk(c.n), 256, 0, st>>>(c.best_z, c.rgb, c.frame, c.n);
        LIO_HIP(hipGetLastError());
    }
    LIO_HIP(hipStreamSynchronize(st));
    return kOk;
}

int colorizer_set_cloud(ColorizeBuf& c, const float* pts, int64_t n, int stride, hipStream_t st) {
    c.have_cloud = false;
    c.n = 0;
    int rc = grow_buf(&c.pts, c.pts_cap, std::max<int64_t>(n * stride, 1));
    if (rc) return rc;
    if (n > c.state_cap || !c.best_z) {
        const int64_t cap = grown(std::max<int64_t>(n, 1), c.state_cap);
        c.state_cap = 0;
        rc = dev_alloc_all({dev_req(c.best_z, (size_t)cap), dev_req(c.rgb, (size_t)cap * 3), dev_req(c.frame, (size_t)cap)});
        if (rc) return rc;
        c.state_cap = cap;
    }
    if (n > 0) LIO_HIP(hipMemcpyAsync(c.pts, pts, (size_t)n * stride * sizeof(float), hipMemcpyHostToDevice, st));
    c.n = n;
    c.stride = stride;
    rc = colorizer_reset(c, st);
    if (rc) return rc;
    c.have_cloud = true;
    return kOk;
}

int colorizer_add_frame(ColorizeBuf& c, const CamArg& cam, const uint8_t* image, int64_t pitch, bool bgr, bool occlusion,
                        int splat_radius, float depth_rel, float depth_abs, int64_t* n_updated, hipStream_t st) {
    const size_t bytes = frame_span(cam.height, pitch, (size_t)cam.width * 3);
    const int64_t pixels = (int64_t)cam.width * cam.height;
    const int64_t pixels4 = (pixels + 3) / 4;
    int rc = reserve_frames({{&c.in, bytes}});
    if (!rc && occlusion) rc = grow_buf(&c.depth, c.depth_cap, pixels4 * 4);
    if (rc) return rc;
    const int32_t frame_no = c.frames;
    LIO_HIP(c.timer.mark(kCzUpload, st));
    LIO_HIP(c.in.upload(image, bytes, st));
    LIO_HIP(hipMemsetAsync(c.count, 0, sizeof(unsigned long long), st));
    LIO_HIP(c.timer.mark(kCzFill, st));
    if (occlusion && c.n > 0) {
        cz_fill_kernel<<<nblk(pixels4), 256, 0, st>>>(reinterpret_cast<uint4*>(c.depth), pixels4, kCzInfBits);
        LIO_HIP(c.timer.mark(kCzSplat, st));
        cz_splat_kernel<<<nblk(c.n), 256, 0, st>>>(c.pts, c.n, c.stride, cam, splat_radius, c.depth);
        LIO_HIP(c.timer.mark(kCzResolve, st));
        cz_resolve_kernel<<<nblk(c.n), 256, 0, st>>>(c.pts, c.n, c.stride, cam, c.depth, depth_rel, depth_abs, c.in.dev, pitch,
                                                     bgr, frame_no, c.best_z, c.rgb, c.frame, c.count);
    } else {
        LIO_HIP(c.timer.mark(kCzSplat, kCzResolve, st));  // no fill, no splat
        if (c.n > 0)
            cz_fused_kernel<<<nblk(c.n), 256, 0, st>>>(c.pts, c.n, c.stride, cam, c.in.dev, pitch, bgr, frame_no, c.best_z,
                                                       c.rgb, c.frame, c.count);
    }
    LIO_HIP(hipGetLastError());
    LIO_HIP(c.timer.mark(kCzStages, st));
    LIO_HIP(hipMemcpyAsync(c.h_count, c.count, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    LIO_HIP(c.timer.finish(st));
    c.frames = frame_no + 1;
    *n_updated = (int64_t)*c.h_count;
    return kOk;
}

int colorizer_get(ColorizeBuf& c, uint8_t* rgb, int32_t* frame_opt, double* depth_opt, hipStream_t st) {
    if (c.n > 0) {
        LIO_HIP(hipMemcpyAsync(rgb, c.rgb, (size_t)c.n * 3, hipMemcpyDeviceToHost, st));
        if (frame_opt) LIO_HIP(hipMemcpyAsync(frame_opt, c.frame, (size_t)c.n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (depth_opt) LIO_HIP(hipMemcpyAsync(depth_opt, c.best_z, (size_t)c.n * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    LIO_HIP(hipStreamSynchronize(st));
    return kOk;
}

}  // namespace lio
