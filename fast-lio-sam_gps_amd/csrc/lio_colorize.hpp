// lio_colorize.hpp — camera projection and point cloud colorization from images (lio_colorize.hip): the camera
// step of the reference's offline leg — post_process/colorize_pcd.py:31-65, the projection role of
// post_process/lidar_projection/src/lidar_projection.cpp:9-34, and the 8-parameter rational distortion model of
// post_process/undistort_image.py:95-97 — restated in IEEE double operations in a fixed order, with an opt-in
// z-buffer and an accumulation over frames (include/lio_gpu.h: lio_project_points, lio_colorizer_*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lio_camera.hpp"
#include "lio_frame.hpp"

namespace lio {

constexpr int kCzMaxSplat = 8;               // the largest splat radius
constexpr uint32_t kCzInfBits = 0x7f800000u;  // bits of float +inf: an empty depth pixel

// stages of colorizer_add_frame, for ColorizeBuf::timer (event times of the last frame)
enum CzStage { kCzUpload = 0, kCzFill = 1, kCzSplat = 2, kCzResolve = 3, kCzStages = 4 };

// records (device, n x stride) -> uv (n x 2 doubles), zc (n doubles), pix (n x 2 int32, -1 where invalid), valid
// (n uint8), each to the HOST pointer given (uv / zc / pix may be null).  Waits for the stream.
int project_points(ProjectBuf& b, const float* d_pts, int64_t n, int stride, const CamArg& cam, double* uv_opt,
                   double* zc_opt, int32_t* pix_opt, uint8_t* valid, hipStream_t st);

// the state of a lio_colorizer: the cloud and the per-point state stay on the device between frames
struct ColorizeBuf {
    float* pts = nullptr;  // n x stride
    int64_t pts_cap = 0;   // floats
    int64_t n = 0;
    int stride = 0;
    bool have_cloud = false;
    double* best_z = nullptr;  // n
    uint8_t* rgb = nullptr;    // n x 3
    int32_t* frame = nullptr;  // n
    int64_t state_cap = 0;     // points
    FrameStage in;             // the frame's image as uploaded (rows of `pitch` bytes)
    uint32_t* depth = nullptr;  // width x height, a multiple of 4 words
    int64_t depth_cap = 0;
    unsigned long long* count = nullptr;    // the frame's replacements
    unsigned long long* h_count = nullptr;  // pinned: its host copy
    int32_t frames = 0;                     // the running frame number
    StageTimer<kCzStages> timer;
};
int colorizer_init(ColorizeBuf& c);
void colorizer_free(ColorizeBuf& c);
// uploads the cloud and resets the state and the frame number.  Waits for the stream.
int colorizer_set_cloud(ColorizeBuf& c, const float* pts, int64_t n, int stride, hipStream_t st);
int colorizer_reset(ColorizeBuf& c, hipStream_t st);
// one frame: image (host, rows of `pitch` bytes), occlusion as given.  Waits for the stream.
int colorizer_add_frame(ColorizeBuf& c, const CamArg& cam, const uint8_t* image, int64_t pitch, bool bgr, bool occlusion,
                        int splat_radius, float depth_rel, float depth_abs, int64_t* n_updated, hipStream_t st);
// the state to the host pointers given (frame_opt / depth_opt may be null).  Waits for the stream.
int colorizer_get(ColorizeBuf& c, uint8_t* rgb, int32_t* frame_opt, double* depth_opt, hipStream_t st);

}  // namespace lio
