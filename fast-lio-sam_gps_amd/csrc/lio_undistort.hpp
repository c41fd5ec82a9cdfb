// lio_undistort.hpp — image undistortion (rectification) for the camera leg (lio_undistort.hip): the
// cv2.undistort(img, K, D, None, K) that post_process/undistort_image.py:21-27, decompress_undistort_images.py:28,
// extract_pointcloud_image.py:26-28 and extraction.py:21-22 run on every frame, restated as a fixed-point map
// (1/32 pixel) and an integer bilinear gather (include/lio_gpu.h: lio_undistort_map, lio_undistorter_*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lio_camera.hpp"
#include "lio_frame.hpp"

namespace lio {

constexpr int kUdMaxSize = 32767;  // the largest width or height of either camera: a map record holds int16 taps

// the rectified image's pinhole camera, passed by value with the raw image's CamArg (whose R, t and r2_max are
// not used here)
struct UdDst {
    double fx, fy, cx, cy;
    int32_t width, height;
};

// stages of undistorter_run, for UndistortBuf::timer (event times of the last frame)
enum UdStage { kUdUpload = 0, kUdKernel = 1, kUdDownload = 2, kUdStages = 3 };

// lio_undistort_map on a lio_filter: dst.height x dst.width x 2 values to each HOST pointer given (any may be
// null), through the arena b.  Waits for the stream.
int undistort_map(ProjectBuf& b, const CamArg& src, const UdDst& dst, double* uv_opt, int32_t* sxy_opt, uint8_t* axy_opt,
                  hipStream_t st);

// the state of a lio_undistorter: the packed map of the current camera pair and the staging of one frame
struct UndistortBuf {
    uint2* map = nullptr;  // dst.height rows of map_pitch records (map_pitch: dst.width rounded up to 4)
    int64_t map_cap = 0;   // records
    int map_pitch = 0;
    int sw = 0, sh = 0, dw = 0, dh = 0, channels = 0;
    uint32_t border = 0;  // channel c in bits 8c .. 8c + 7
    bool have_camera = false;
    FrameStage in;   // the frame as uploaded (rows of the caller's pitch)
    FrameStage out;  // the rectified frame: rows of frame_pitch(dw, channels) bytes
    StageTimer<kUdStages> timer;
};
int undistorter_init(UndistortBuf& u);
void undistorter_free(UndistortBuf& u);
// computes and keeps the packed map.  Waits for the stream.
int undistorter_set_camera(UndistortBuf& u, const CamArg& src, const UdDst& dst, int channels, const uint8_t border[3],
                           hipStream_t st);
// one frame: image (host, sh rows of `pitch` bytes) -> out (host, dh rows of `out_pitch` bytes, of which
// channels * dw are written).  Waits for the stream.
int undistorter_run(UndistortBuf& u, const uint8_t* image, int64_t pitch, uint8_t* out, int64_t out_pitch, hipStream_t st);
// the first half of undistorter_run, for a caller that goes on with the frame on the device (lio_exposure.hip):
// upload and gather, enqueued on st and not waited for.  The rectified frame is u.out.dev: dh rows of
// frame_pitch(dw, channels) bytes.
int undistorter_rectify(UndistortBuf& u, const uint8_t* image, int64_t pitch, hipStream_t st);

}  // namespace lio
