// lio_exposure.hpp — exposure adaption for the camera leg (lio_exposure.hip): what the reference runs on every
// rectified frame, post_process/exposure_adaption/CLAHE_region_adjusted.py:6-41 (BGR -> HSV, CLAHE of V, HSV -> BGR)
// and correct_exposure:6-103 (histograms, equalisation or stretch of V, a gamma table), restated as integer and
// float32 operations in a written order (include/lio_gpu.h: lio_exposure_*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lio_undistort.hpp"

namespace lio {

constexpr int kExMaxSize = kUdMaxSize;  // the largest width or height, as for the undistorter
constexpr int kExMaxTiles = 64;         // tiles per direction

// stages of a run, for ExposureBuf::timer (event times of the last run)
enum ExStage { kExUpload = 0, kExHist = 1, kExLut = 2, kExApply = 3, kExDownload = 4, kExStages = 5 };
// stages of a stencil run (lio_overexposure.hpp), for ExposureBuf::stencil_timer
enum OxStage { kOxUpload = 0, kOxKernel = 1, kOxDownload = 2, kOxStages = 3 };

// the tiling of a plane: the extended size, the tile size and the clip value of the contract.  exposure_tiling
// needs no device; kArg with `why` naming the bound.
struct ExTiling {
    int tiles_x = 1, tiles_y = 1;
    int ext_w = 0, ext_h = 0;  // the padded plane
    int tw = 0, th = 0;        // one tile
    int clip = 0;              // 0: no clipping
};
int exposure_tiling(int width, int height, double clip_limit, int tiles_x, int tiles_y, ExTiling* t, const char** why);

// the state of a lio_exposure: the staging of one frame, the histograms and the tables
struct ExposureBuf {
    FrameStage in;   // the frame as uploaded (rows of the caller's pitch)
    FrameStage out;  // the result: rows of frame_pitch(width, channels) bytes
    void* arena = nullptr;  // uint32 hist[tiles][256], then uint8 lut[tiles][256] (remap: lut_v, lut_all)
    size_t arena_bytes = 0;
    uint32_t* h_small = nullptr;  // pinned, 2 x 256 uint32: the histograms down, the two tables up
    size_t h_small_bytes = 0;
    StageTimer<kExStages> timer;
    StageTimer<kOxStages> stencil_timer;  // of the stencil calls (lio_overexposure.hpp), which use in and out alone
};
int exposure_init(ExposureBuf& e);
void exposure_free(ExposureBuf& e);

// image: host, height rows of `pitch` bytes.  hist_v_opt / hist_gray_opt: 256 int64 each.  Waits for the stream.
int exposure_histograms(ExposureBuf& e, const uint8_t* image, int width, int height, int channels, int64_t pitch, int order,
                        int64_t* hist_v_opt, int64_t* hist_gray_opt, hipStream_t st);
// out: host, height rows of `out_pitch` bytes of which channels * width are written.  Waits for the stream.
int exposure_clahe(ExposureBuf& e, const uint8_t* image, int width, int height, int channels, int64_t pitch, int order,
                   const ExTiling& t, uint8_t* out, int64_t out_pitch, hipStream_t st);
int exposure_remap(ExposureBuf& e, const uint8_t* image, int width, int height, int channels, int64_t pitch, int order,
                   const uint8_t* lut_v_opt, const uint8_t* lut_all_opt, uint8_t* out, int64_t out_pitch, hipStream_t st);
// u's configured frame rectified on the device (undistorter_rectify) and adapted there: one upload, one download
int exposure_clahe_undistorted(ExposureBuf& e, UndistortBuf& u, const uint8_t* raw, int64_t pitch, int order, const ExTiling& t,
                               uint8_t* out, int64_t out_pitch, hipStream_t st);

}  // namespace lio
