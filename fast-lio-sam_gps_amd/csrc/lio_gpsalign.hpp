// lio_gpsalign.hpp — GPS-to-SLAM trajectory alignment and map georeferencing (lio_gpsalign.hip): the offline GPS
// leg of the reference — post_process/align_slam_gps_icp.py:81-156 (icp_alignment), georef_mapmatch.py:115-135
// (align_trajectories_horn) and post_process/georeference_pcd.py:236-244 — restated in IEEE double operations in a
// fixed order (include/lio_gpu.h: lio_gps_align, lio_similarity2d_fit, lio_georeference_xy).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lio {

// Tuning constants of the nearest-neighbour search; NO OUTPUT DEPENDS ON THEM.  Targets go through LDS in tiles of
// kGaTile; the targets are split into chunks of a multiple of kGaTile, at least kGaChunkMin wide, each chunk
// searched by its own workgroups, so that a short trajectory still fills the device (ga_chunk_width).
constexpr int kGaTile = 1024;
constexpr int64_t kGaChunkMin = 2048;
constexpr int64_t kGaMaxChunks = 32;
constexpr int64_t kGaWantGroups = 2048;  // workgroups aimed at: 8 per CU
int64_t ga_chunk_width(int64_t n, int64_t m);

// offsets into the result array of gps_align: the values of LIO_GPSALIGN_* (lio_capi_post.cpp asserts it)
enum GaOut {
    kGaIters = 0, kGaConverged = 1, kGaMeanError = 2, kGaS0 = 3, kGaCA = 4, kGaCB = 6, kGaSc = 8, kGaC = 9, kGaS = 10,
    kGaT = 11, kGaCD = 13, kGaRefScale = 15, kGaRefC = 16, kGaRefS = 17, kGaRefT = 18, kGaTotScale = 20, kGaTotC = 21,
    kGaTotS = 22, kGaTotT = 23, kGaLen = 25
};
// of similarity2d_fit: the values of LIO_SIM2D_*
enum Sim2dOut { kSimScale = 0, kSimC = 1, kSimS = 2, kSimT = 3, kSimLen = 5 };

// status of the two fits beyond lio_scratch.hpp's: the moments admit no similarity (LIO_ERR_STATE)
constexpr int kGaState = -4;

struct GpsAlignBuf {
    void* arena = nullptr;  // one device arena, carved per call (ga_reserve)
    size_t arena_bytes = 0;
    double2 *a_in = nullptr, *b_in = nullptr;  // the uploads; a_in becomes S
    double2 *d = nullptr, *mt = nullptr;       // centred targets (m), matched targets (n)
    double* dist = nullptr;                    // n
    int32_t* nn = nullptr;                     // n
    double* part_d2 = nullptr;                 // chunks x n
    int32_t* part_k = nullptr;                 // chunks x n
    double* part = nullptr;                    // kGaMaxSums x blocks: the block sums of TREE
    double* h_part = nullptr;                  // pinned: their host copy
    size_t h_bytes = 0;
    double* geo_xy = nullptr;                  // lio_georeference_xy's double output
    int64_t geo_cap = 0;
};
void gps_align_free(GpsAlignBuf& g);

// icp_alignment restated (include/lio_gpu.h, lio_gps_align).  gps / slam: host, m x 2 and n x 2 doubles, finite
// (the caller has checked).  aligned (n x 2, host), nn_opt (n, host, may be null), out (kGaLen doubles, host).
// Waits for the stream.  Status: kOk, kArg (a zero-variance point set), kGaState, kHip, kNoMem.
int gps_align(GpsAlignBuf& g, const double* gps, int64_t m, const double* slam, int64_t n, int max_iterations,
              double tolerance, double* aligned, int32_t* nn_opt, double* out, hipStream_t st);

// align_trajectories_horn restated: steps 2-5 of one iteration on n given pairs.  out: kSimLen doubles.
int similarity2d_fit(GpsAlignBuf& g, const double* src, const double* dst, int64_t n, double* out, hipStream_t st);

// records (device, n x stride) -> d_out with x, y georeferenced (other fields copied); xy (device, n x 2 doubles,
// may be null).  p = r00, r01, r10, r11, scale, tx, ty, ox, oy.  Queues on the stream; does not wait.
int georeference_xy(const float* d_in, int64_t n, int stride, const double p[9], float* d_out, double* d_xy,
                    hipStream_t st);

}  // namespace lio
