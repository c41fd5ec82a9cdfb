// lio_overlay.hpp — point overlay drawing for the camera leg (lio_overlay.hip): the output of the reference's
// projection tool, the camera image with every projected point drawn as a filled cv::circle, later points over
// earlier ones (post_process/lidar_projection/src/lidar_projection.cpp:113-125), restated as one 64-bit key per pixel
// whose minimum names the pixel's owner (include/lio_gpu.h: lio_overlay_*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lio_camera.hpp"
#include "lio_frame.hpp"
#include "lio_undistort.hpp"

namespace lio {

constexpr int kOvMaxRadius = 15;                     // the largest disc radius
constexpr unsigned long long kOvEmpty = ~0ull;       // the key of a pixel that no point owns
constexpr int64_t kOvMaxPoints = 0xFFFFFFFEll;       // 2^32 - 2: the low word of a key is 0xFFFFFFFF - index
enum OvOrder { kOvDrawOrder = 0, kOvNearest = 1 };  // LIO_OVERLAY_DRAW_ORDER, LIO_OVERLAY_NEAREST

// stages of overlay_draw, for OverlayBuf::timer (event times of the last frame)
enum OvStage { kOvUpload = 0, kOvFill = 1, kOvStamp = 2, kOvCompose = 3, kOvDownload = 4, kOvStages = 5 };

// The disc of radius r as one half-width per |row offset| 0 .. r, from OpenCV's filled midpoint circle.  Built on the
// host and passed to the stamp kernel by value: the kernel holds no circle logic of its own.
struct OvDisc {
    int32_t r;
    uint8_t half[kOvMaxRadius + 1];
};
OvDisc overlay_disc(int radius);

// the state of a lio_overlay: the cloud and its colour sources stay on the device between frames
struct OverlayBuf {
    float* pts = nullptr;  // n x stride
    int64_t pts_cap = 0;   // floats
    int64_t n = 0;
    int stride = 0;
    bool have_cloud = false;
    int32_t* labels = nullptr;  // n, when have_labels
    int64_t labels_cap = 0;
    bool have_labels = false;
    uint8_t* colors = nullptr;  // n x 3, when have_colors
    int64_t colors_cap = 0;     // bytes
    bool have_colors = false;
    uint8_t* palette = nullptr;  // palette_rows x 3
    int64_t palette_cap = 0;     // bytes
    int32_t palette_rows = 0;
    unsigned long long* keys = nullptr;  // height rows of (width rounded up to 4) keys
    int64_t keys_cap = 0;
    int32_t* owner = nullptr;  // height x width, when a draw asks for it
    int64_t owner_cap = 0;
    FrameStage in;                          // the frame as uploaded (rows of the caller's pitch)
    FrameStage out;                         // the drawn frame: rows of frame_pitch(width, 3) bytes
    unsigned long long* count = nullptr;    // the frame's drawn points
    unsigned long long* h_count = nullptr;  // pinned: its host copy
    StageTimer<kOvStages> timer;
};
// the palette starts as the one row 0 255 0 (the tool as shipped draws every point green).  Waits for the stream.
int overlay_init(OverlayBuf& o, hipStream_t st);
void overlay_free(OverlayBuf& o);
// uploads the cloud; the labels and per-point colours of the cloud before it are dropped.  Waits for the stream.
int overlay_set_cloud(OverlayBuf& o, const float* pts, int64_t n, int stride, hipStream_t st);
// n values each, for the cloud that is set; null drops them.  Each waits for the stream.
int overlay_set_labels(OverlayBuf& o, const int32_t* labels, hipStream_t st);
int overlay_set_colors(OverlayBuf& o, const uint8_t* colors, hipStream_t st);
int overlay_set_palette(OverlayBuf& o, const uint8_t* palette, int32_t rows, hipStream_t st);
// one frame: image (host, rows of `pitch` bytes) -> out (host, rows of `out_pitch` bytes, of which 3 * width are
// written), owner_opt (host, height x width) and *n_drawn.  With `u`, `image` is the undistorter's raw frame: it is
// rectified on the device and drawn on there, with one upload and one download.  Waits for the stream.
int overlay_draw(OverlayBuf& o, UndistortBuf* u, const CamArg& cam, const OvDisc& disc, int order, const uint8_t* image,
                 int64_t pitch, uint8_t* out, int64_t out_pitch, int32_t* owner_opt, int64_t* n_drawn, hipStream_t st);

}  // namespace lio
