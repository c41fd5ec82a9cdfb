// lio_undistort.hip — image undistortion (rectification) on gfx950: the cv2.undistort(img, K, D, None, K) of the
// reference's camera scripts (post_process/undistort_image.py:21-27 and three more; lio_undistort.hpp), restated
// as our own contract (include/lio_gpu.h: lio_undistort_map, lio_undistorter_*): per output pixel the distortion
// stage of lio_project_points in IEEE double (lio_camera_dev.hpp, the function cz_project calls), a map in 1/32
// pixel rounded to nearest even, and a bilinear gather in integers with a constant border per tap.  The file is
// compiled with -ffp-contract=off, host and device: no multiply-add is fused anywhere.
//
//   ud_map_kernel    one thread per map record: the 8-byte record the gather reads, and for lio_undistort_map the
//                    unquantised u, v and the int32 / uint8 map.  It runs once per camera pair.
//   ud_remap_kernel  one thread per 4 consecutive output pixels of one row: 32 bytes of map in two 16-byte loads,
//                    the taps served by the cache (neighbouring output pixels read neighbouring source bytes): a
//                    pixel whose four taps are inside loads the 2 * channels bytes of each source row in one or two
//                    unaligned loads, any other pixel its inside taps byte by byte (profiles/undistort_ab.md: 2.5x
//                    over bytes everywhere); 4 * channels bytes out as dwords.  The device's own output rows are a
//                    multiple of 4 bytes, so every full group of a row is dword-aligned whatever pitch the caller's
//                    buffer has; only the last, partial group of a row goes out as bytes.  Nothing is staged in LDS.
#include "lio_camera_dev.hpp"
#include "lio_scratch.hpp"
#include "lio_undistort.hpp"

namespace lio {
namespace {

constexpr uint32_t kUdFarLo = 0x80008000u;  // sx = sy = -32768
constexpr uint32_t kUdFarHi = 0x00010000u;  // ax = ay = 0, the FAR flag

__device__ __forceinline__ int ud_sat16(int v) { return min(max(v, -32768), 32767); }

// map_pitch records per row; the records at columns >= dst.width pad a row to a multiple of 4 and are FAR
__global__ __launch_bounds__(256) void ud_map_kernel(CamArg src, UdDst dst, int map_pitch, uint2* __restrict__ rec,
                                                     double2* __restrict__ uv, int2* __restrict__ sxy,
                                                     uchar2* __restrict__ axy) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)map_pitch * dst.height) return;
    const int i = (int)(t / map_pitch), j = (int)(t % map_pitch);
    if (j >= dst.width) {
        if (rec) rec[t] = make_uint2(kUdFarLo, kUdFarHi);
        return;
    }
    const double xn = ((double)j - dst.cx) / dst.fx;
    const double yn = ((double)i - dst.cy) / dst.fy;
    const Distorted d = cam_distort(xn, yn, src);
    const double qu = rint(d.u * 32.0), qv = rint(d.v * 32.0);  // ties to even
    const bool is_near = fabs(qu) < 1073741824.0 && fabs(qv) < 1073741824.0;  // false on NaN
    int sx = INT32_MIN, sy = INT32_MIN, ax = 0, ay = 0;
    if (is_near) {
        const int iu = (int)qu, iv = (int)qv;
        sx = iu >> 5, ax = iu & 31;
        sy = iv >> 5, ay = iv & 31;
    }
    if (rec)
        rec[t] = is_near ? make_uint2((uint32_t)(ud_sat16(sx) & 0xffff) | ((uint32_t)(ud_sat16(sy) & 0xffff) << 16),
                                   (uint32_t)ax | ((uint32_t)ay << 8))
                      : make_uint2(kUdFarLo, kUdFarHi);
    const int64_t p = (int64_t)i * dst.width + j;
    if (uv) uv[p] = make_double2(d.u, d.v);
    if (sxy) sxy[p] = make_int2(sx, sy);
    if (axy) axy[p] = make_uchar2((unsigned char)ax, (unsigned char)ay);
}

// One output pixel: the four taps (sx, sy) (sx + 1, sy) (sx, sy + 1) (sx + 1, sy + 1) with the integer weights
// (32 - ax)(32 - ay), ax (32 - ay), (32 - ax) ay, ax ay; a tap outside the source is the border value and is not
// loaded, whatever its weight.  A saturated tap coordinate is outside: widths and heights are at most 32767.
template <int C>
__device__ __forceinline__ void ud_sample(uint2 r, const uint8_t* __restrict__ img, int64_t pitch, int sw, int sh,
                                          uint32_t border, uint32_t* o) {
    const int sx = (int)(int16_t)(r.x & 0xffffu), sy = (int)(int16_t)(r.x >> 16);
    const int ax = (int)(r.y & 0xffu), ay = (int)((r.y >> 8) & 0xffu);
    const bool is_far = (r.y >> 16) & 1u;
    const bool x0 = !is_far && (unsigned)sx < (unsigned)sw, x1 = !is_far && (unsigned)(sx + 1) < (unsigned)sw;
    const bool y0 = (unsigned)sy < (unsigned)sh, y1 = (unsigned)(sy + 1) < (unsigned)sh;
    const int w00 = (32 - ax) * (32 - ay), w10 = ax * (32 - ay), w01 = (32 - ax) * ay, w11 = ax * ay;
    const int64_t at = (int64_t)sy * pitch + (int64_t)sx * C;
    if (x0 && x1 && y0 && y1) {
        // all four taps inside, nearly every pixel: the 2 C bytes of each source row in one load (C = 1) or two
        // (C = 3), at any alignment, instead of 2 C byte loads
        uint64_t r0 = 0, r1 = 0;
        if constexpr (C == 1) {
            uint16_t a, b;
            __builtin_memcpy(&a, img + at, 2);
            __builtin_memcpy(&b, img + at + pitch, 2);
            r0 = a, r1 = b;
        } else {
            uint32_t a, b;
            uint16_t a2, b2;
            __builtin_memcpy(&a, img + at, 4);
            __builtin_memcpy(&a2, img + at + 4, 2);
            __builtin_memcpy(&b, img + at + pitch, 4);
            __builtin_memcpy(&b2, img + at + pitch + 4, 2);
            r0 = (uint64_t)a | ((uint64_t)a2 << 32), r1 = (uint64_t)b | ((uint64_t)b2 << 32);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int p00 = (int)((r0 >> (8 * c)) & 0xffu), p10 = (int)((r0 >> (8 * (C + c))) & 0xffu);
            const int p01 = (int)((r1 >> (8 * c)) & 0xffu), p11 = (int)((r1 >> (8 * (C + c))) & 0xffu);
            o[c] = (uint32_t)((w00 * p00 + w10 * p10 + w01 * p01 + w11 * p11 + 512) >> 10);
        }
        return;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int b = (int)((border >> (8 * c)) & 0xffu);
        const int p00 = (x0 && y0) ? (int)img[at + c] : b;
        const int p10 = (x1 && y0) ? (int)img[at + C + c] : b;
        const int p01 = (x0 && y1) ? (int)img[at + pitch + c] : b;
        const int p11 = (x1 && y1) ? (int)img[at + pitch + C + c] : b;
        o[c] = (uint32_t)((w00 * p00 + w10 * p10 + w01 * p01 + w11 * p11 + 512) >> 10);
    }
}

// block 64 x 4: a wave is 256 consecutive pixels of one row.  map rows are map_pitch records (a multiple of 4, the
// padding FAR), out rows out_pitch bytes (a multiple of 4, at least C * dw): both are this file's own buffers.
template <int C>
__global__ __launch_bounds__(256) void ud_remap_kernel(const uint8_t* __restrict__ img, int64_t pitch, int sw, int sh,
                                                       const uint2* __restrict__ map, int map_pitch, int dw, int dh,
                                                       uint8_t* __restrict__ out, int64_t out_pitch, uint32_t border) {
    const int x = 4 * ((int)blockIdx.x * 64 + (int)threadIdx.x);
    const int row = (int)blockIdx.y * 4 + (int)threadIdx.y;
    if (row >= dh || x >= dw) return;
    const uint4* m = reinterpret_cast<const uint4*>(map + (int64_t)row * map_pitch + x);
    const uint4 m01 = m[0], m23 = m[1];
    uint32_t v[4 * C];
    ud_sample<C>(make_uint2(m01.x, m01.y), img, pitch, sw, sh, border, v);
    ud_sample<C>(make_uint2(m01.z, m01.w), img, pitch, sw, sh, border, v + C);
    ud_sample<C>(make_uint2(m23.x, m23.y), img, pitch, sw, sh, border, v + 2 * C);
    ud_sample<C>(make_uint2(m23.z, m23.w), img, pitch, sw, sh, border, v + 3 * C);
    uint8_t* o = out + (int64_t)row * out_pitch + (int64_t)x * C;
    if (x + 4 <= dw) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
        for (int k = 0; k < C; ++k) o4[k] = v[4 * k] | (v[4 * k + 1] << 8) | (v[4 * k + 2] << 16) | (v[4 * k + 3] << 24);
    } else {
        const int n = (dw - x) * C;  // 1 .. 3 pixels
#pragma unroll
        for (int k = 0; k < 3 * C; ++k)
            if (k < n) o[k] = (uint8_t)v[k];
    }
}

int launch_map(const CamArg& src, const UdDst& dst, int map_pitch, uint2* rec, double2* uv, int2* sxy, uchar2* axy,
               hipStream_t st) {
    ud_map_kernel<<<nblk((int64_t)map_pitch * dst.height), 256, 0, st>>>(src, dst, map_pitch, rec, uv, sxy, axy);
    LIO_HIP(hipGetLastError());
    return kOk;
}

}  // namespace

int undistort_map(ProjectBuf& b, const CamArg& src, const UdDst& dst, double* uv_opt, int32_t* sxy_opt, uint8_t* axy_opt,
                  hipStream_t st) {
    if (!uv_opt && !sxy_opt && !axy_opt) return kOk;
    const size_t n = (size_t)dst.width * (size_t)dst.height;
    double2* d_uv = nullptr;
    int2* d_sxy = nullptr;
    uchar2* d_axy = nullptr;
    auto fields = [&](Carver& c) {
        c(d_uv, uv_opt ? n : 0);
        c(d_sxy, sxy_opt ? n : 0);
        c(d_axy, axy_opt ? n : 0);
    };
    int rc = reserve_arena(&b.arena, b.arena_bytes, fields);
    if (rc) return rc;
    if (!uv_opt) d_uv = nullptr;
    if (!sxy_opt) d_sxy = nullptr;
    if (!axy_opt) d_axy = nullptr;
    if ((rc = launch_map(src, dst, dst.width, nullptr, d_uv, d_sxy, d_axy, st))) return rc;
    if (uv_opt) LIO_HIP(hipMemcpyAsync(uv_opt, d_uv, n * sizeof(double2), hipMemcpyDeviceToHost, st));
    if (sxy_opt) LIO_HIP(hipMemcpyAsync(sxy_opt, d_sxy, n * sizeof(int2), hipMemcpyDeviceToHost, st));
    if (axy_opt) LIO_HIP(hipMemcpyAsync(axy_opt, d_axy, n * sizeof(uchar2), hipMemcpyDeviceToHost, st));
    LIO_HIP(hipStreamSynchronize(st));
    return kOk;
}

int undistorter_init(UndistortBuf& u) {
    LIO_HIP(u.timer.init());
    return kOk;
}

void undistorter_free(UndistortBuf& u) {
    dev_free(&u.map);
    u.in.free();
    u.out.free();
    u.timer.free();
    u = UndistortBuf{};
}

int undistorter_set_camera(UndistortBuf& u, const CamArg& src, const UdDst& dst, int channels, const uint8_t border[3],
                           hipStream_t st) {
    u.have_camera = false;
    const int map_pitch = (dst.width + 3) & ~3;
    int rc = grow_buf(&u.map, u.map_cap, (int64_t)map_pitch * dst.height);
    if (rc) return rc;
    if ((rc = launch_map(src, dst, map_pitch, u.map, nullptr, nullptr, nullptr, st))) return rc;
    LIO_HIP(hipStreamSynchronize(st));
    u.map_pitch = map_pitch;
    u.sw = src.width, u.sh = src.height, u.dw = dst.width, u.dh = dst.height, u.channels = channels;
    u.border = (uint32_t)border[0] | ((uint32_t)border[1] << 8) | ((uint32_t)border[2] << 16);
    u.have_camera = true;
    return kOk;
}

int undistorter_rectify(UndistortBuf& u, const uint8_t* image, int64_t pitch, hipStream_t st) {
    const int C = u.channels;
    const size_t in_bytes = frame_span(u.sh, pitch, (size_t)u.sw * (size_t)C);
    const int64_t d_pitch = frame_pitch(u.dw, C);
    const int rc = reserve_frames({{&u.in, in_bytes}, {&u.out, (size_t)d_pitch * (size_t)u.dh}});
    if (rc) return rc;
    LIO_HIP(u.timer.mark(kUdUpload, st));
    LIO_HIP(u.in.upload(image, in_bytes, st));
    LIO_HIP(u.timer.mark(kUdKernel, st));
    const dim3 block(64, 4), grid((unsigned)((u.dw + 255) / 256), (unsigned)((u.dh + 3) / 4));
    if (C == 3)
        ud_remap_kernel<3><<<grid, block, 0, st>>>(u.in.dev, pitch, u.sw, u.sh, u.map, u.map_pitch, u.dw, u.dh, u.out.dev,
                                                   d_pitch, u.border);
    else
        ud_remap_kernel<1><<<grid, block, 0, st>>>(u.in.dev, pitch, u.sw, u.sh, u.map, u.map_pitch, u.dw, u.dh, u.out.dev,
                                                   d_pitch, u.border);
    LIO_HIP(hipGetLastError());
    LIO_HIP(u.timer.mark(kUdDownload, st));
    return kOk;
}

int undistorter_run(UndistortBuf& u, const uint8_t* image, int64_t pitch, uint8_t* out, int64_t out_pitch, hipStream_t st) {
    const int rc = undistorter_rectify(u, image, pitch, st);
    if (rc) return rc;
    return download_frame(u.out, u.timer, u.dw, u.dh, u.channels, out, out_pitch, st);
}

}  // namespace lio
