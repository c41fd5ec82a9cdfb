// lio_camera_dev.hpp — the distortion stage of the camera contract (include/lio_gpu.h, lio_project_points: the
// lines from r2 = xn xn + yn yn through u = fx xd + cx; v = fy yd + cy), one operation per line of it.  It is
// the ONLY copy: cz_project (lio_colorize.hip) calls it on a point's normalised coordinates and ud_map_kernel
// (lio_undistort.hip) on an output pixel's, so a ray has the same u, v bits in both.  Files that include this
// are compiled with -ffp-contract=off: no multiply-add is fused.
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

}  // namespace lio
