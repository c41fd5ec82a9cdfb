// lio_overexposure.hpp — the stencil calls of the camera leg (lio_overexposure.hip): the reference's
// post_process/exposure_adaption/solve_overexposure:6-32 (recover_overexposure: BGR -> HSV, a mask V > 200 dilated by
// 5 x 5, cv2.GaussianBlur(v, (15, 15), 0) blended in under the mask, HSV -> BGR) and the 8-bit Gaussian blur on its
// own, restated in integers (include/lio_gpu.h: lio_gaussian_weights, lio_exposure_recover, lio_exposure_gaussian_blur).
// They run on a lio_exposure's frame staging (ExposureBuf in, out) with a stage timer of their own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lio_exposure.hpp"

namespace lio {

constexpr int kOxMaxKsize = 31;   // the Gaussian kernel: odd, 1..31
constexpr int kOxMaxDilate = 15;  // the dilation block: odd, 1..15

// the parameters of a recovery, checked by the caller: threshold 0..255, dilate odd 1..15, w the ksize weights
struct OxRecover {
    int threshold = 200, dilate = 5, ksize = 15;
    uint16_t w[kOxMaxKsize + 1] = {};
};

// the ksize fixed-point weights (8 fractional bits, their sum is 256) of the contract.  Needs no device.  ksize odd
// in 1..31 and sigma finite are the caller's to check.
void gaussian_weights(int ksize, double sigma, uint16_t* w);

// image, out: host, height rows of `pitch` / `out_pitch` bytes of which channels * width are read / written.  Each
// waits for the stream.
int exposure_recover(ExposureBuf& e, const uint8_t* image, int width, int height, int channels, int64_t pitch, int order,
                     const OxRecover& p, uint8_t* out, int64_t out_pitch, hipStream_t st);
int exposure_gaussian_blur(ExposureBuf& e, const uint8_t* image, int width, int height, int channels, int64_t pitch, int ksize,
                           const uint16_t* w, uint8_t* out, int64_t out_pitch, hipStream_t st);
// u's configured frame rectified on the device (undistorter_rectify) and recovered there: one upload, one download
int exposure_recover_undistorted(ExposureBuf& e, UndistortBuf& u, const uint8_t* raw, int64_t pitch, int order, const OxRecover& p,
                                 uint8_t* out, int64_t out_pitch, hipStream_t st);

}  // namespace lio
