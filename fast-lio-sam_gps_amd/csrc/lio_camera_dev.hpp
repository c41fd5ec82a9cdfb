// lio_camera_dev.hpp — the camera contract on the device (include/lio_gpu.h, lio_project_points), one operation per
// line of it, each stage in its ONLY copy:
//   cam_distort   the lines from r2 = xn xn + yn yn through u = fx xd + cx; v = fy yd + cy: cz_project calls it on a
//                 point's normalised coordinates and ud_map_kernel (lio_undistort.hip) on an output pixel's, so a ray
//                 has the same u, v bits in both
//   cz_project    a point record through the pose, cam_distort and the validity test: the colorizer's kernels
//                 (lio_colorize.hip) and the overlay's stamp (lio_overlay.hip) call it, so a point has the same u, v,
//                 zc and mask in both
// Files that include this are compiled with -ffp-contract=off: no multiply-add is fused.
#pragma once
#include <hip/hip_runtime.h>

#include "lio_camera.hpp"

namespace lio {

struct Distorted {
    double u, v, r2;
};

__device__ __forceinline__ Distorted cam_distort(double xn, double yn, const CamArg& c) {
    const double r2 = xn * xn + yn * yn;
    const double num = 1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2;
    const double den = 1.0 + ((c.k6 * r2 + c.k5) * r2 + c.k4) * r2;
    const double rad = num / den;
    const double a1 = (2.0 * xn) * yn, a2 = r2 + (2.0 * xn) * xn, a3 = r2 + (2.0 * yn) * yn;
    const double xd = xn * rad + (c.p1 * a1 + c.p2 * a2);
    const double yd = yn * rad + (c.p1 * a3 + c.p2 * a1);
    Distorted o;
    o.u = c.fx * xd + c.cx;
    o.v = c.fy * yd + c.cy;
    o.r2 = r2;
    return o;
}

struct Projected {
    double u, v, zc;
    int px, py;  // -1 where invalid
    bool valid;
};

// the contract's projection (include/lio_gpu.h, lio_project_points), one operation per line of it
__device__ __forceinline__ Projected cz_project(const float* __restrict__ p, const CamArg& c) {
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    const double xc = ((c.R[0] * x + c.R[1] * y) + c.R[2] * z) + c.t[0];
    const double yc = ((c.R[3] * x + c.R[4] * y) + c.R[5] * z) + c.t[1];
    const double zc = ((c.R[6] * x + c.R[7] * y) + c.R[8] * z) + c.t[2];
    const double xn = xc / zc, yn = yc / zc;
    const Distorted d = cam_distort(xn, yn, c);  // r2 ... u, v: shared with the undistortion map
    Projected o;
    o.u = d.u;
    o.v = d.v;
    o.zc = zc;
    // every comparison is false on NaN
    o.valid = zc > 0.0 && d.r2 <= c.r2_max && o.u >= 0.0 && o.u < (double)c.width && o.v >= 0.0 && o.v < (double)c.height;
    o.px = o.valid ? (int)o.u : -1;  // truncation only after the test: u = -0.5 is invalid, not pixel 0
    o.py = o.valid ? (int)o.v : -1;
    return o;
}

}  // namespace lio
