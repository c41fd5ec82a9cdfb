// lio_camera.hpp — what the camera leg's two halves share on the host (lio_colorize.hpp, lio_undistort.hpp): the
// camera a kernel is handed, and the arena of the two one-shot entries on a lio_filter.  The device side of the
// model is lio_camera_dev.hpp, the host path of a frame lio_frame.hpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace lio {

// What a kernel needs of one frame's camera and pose: 16 + 12 doubles and the image size, passed by value.
struct CamArg {
    double fx, fy, cx, cy;
    double k1, k2, p1, p2, k3, k4, k5, k6;
    double r2_max;
    double R[9], t[3];
    int32_t width, height;
};

// scratch of lio_project_points and lio_undistort_map on a lio_filter: one arena for the call's outputs
struct ProjectBuf {
    void* arena = nullptr;
    size_t arena_bytes = 0;
};
void project_free(ProjectBuf& b);

}  // namespace lio
