// lio_capi_util.hpp — what every file of the C-ABI (include/lio_gpu.h) shares: the error reporting and the device
// check (lio_capi_base.hpp), the public code of an internal status, the handle shell, the filter handle and the
// tails its entry points have in common.  Private to lio_capi.cpp (the library level), the online leg's files
// (map, scan context, preprocessing, formats: lio_capi_online.hpp),
// lio_capi_post.cpp (the offline leg on a lio_filter) and lio_capi_camera.cpp (the camera leg); each says
// `using namespace lio::capi`.  The functions are static: each file has its own and the library exports none.
#pragma once
#include "lio_capi_base.hpp"  // fail, HIP_TRY, check_device (shared with the loop-ICP files)

#include <cmath>

#include "lio_camera.hpp"
#include "lio_cluster.hpp"
#include "lio_denoise.hpp"
#include "lio_error.hpp"
#include "lio_kernels.hpp"  // PoseArg, which lio_filter.hpp uses
#include "lio_filter.hpp"
#include "lio_gpsalign.hpp"
#include "lio_kmeans.hpp"
#include "lio_normals.hpp"
#include "lio_plane.hpp"
#include "lio_scratch.hpp"

namespace lio::capi {

static_assert(lio::kOk == LIO_OK && lio::kArg == LIO_ERR_ARG && lio::kHip == LIO_ERR_HIP && lio::kNoMem == LIO_ERR_NOMEM,
              "the internal status codes are the public ones");

// The public code and message of an internal driver's status.  arg_what: the call's wording of kArg.  Every kHip
// has just left the failed HIP call's text in last_error() (LIO_HIP), taken here before fail() replaces it.
static inline int status(int rc, const char* what, const char* arg_what = "bad arguments") {
    if (rc == lio::kOk) return LIO_OK;
    if (rc == lio::kNoMem) return fail(LIO_ERR_NOMEM, std::string(what) + ": out of device memory");
    if (rc == lio::kArg) return fail(LIO_ERR_ARG, std::string(what) + ": " + arg_what);
    const std::string detail = lio::last_error();
    return fail(LIO_ERR_HIP, std::string(what) + " failed (" + detail + ")");
}

template <class T>
static int grow(T** p, int64_t& cap, int64_t need, size_t elems_per = 1) {
    if (lio::grow_buf(p, cap, need, elems_per)) return fail(LIO_ERR_NOMEM, "hipMalloc failed");
    return LIO_OK;
}

static inline bool all_finite(const double* v, int64_t count) {
    for (int64_t i = 0; i < count; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// ---- the handle shell: lio_filter, lio_map, lio_colorizer, lio_undistorter and lio_exposure are a Handle and their buffers ----
struct Handle {
    int dev = 0;
    hipStream_t st = nullptr;
};

// *out = a new H on `device` with a stream of its own.  out_null: the call's wording of a NULL `out`.
template <class H>
static int open_handle(int device, H** out, const char* out_null) {
    if (!out) return fail(LIO_ERR_ARG, out_null);
    *out = nullptr;
    const int rc = check_device(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    H* h = new H();
    h->dev = device;
    if (hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return fail(LIO_ERR_HIP, "hipStreamCreate failed");
    }
    *out = h;
    return LIO_OK;
}

// waits for h's stream, runs free_bufs(*h), ends the stream and deletes h.  A NULL h is nothing to do.
template <class H, class Free>
static int close_handle(H* h, Free&& free_bufs) {
    if (!h) return LIO_OK;
    (void)hipSetDevice(h->dev);
    (void)hipStreamSynchronize(h->st);
    free_bufs(*h);
    (void)hipStreamDestroy(h->st);
    delete h;
    return LIO_OK;
}

// a NULL handle without a device is the missing device (no create can have succeeded), not a bad argument
static inline int null_handle(const void* h, const char* what) {
    if (h) return LIO_OK;
    const int rc = check_device(0);
    if (rc) return rc;
    return fail(LIO_ERR_ARG, std::string(what) + ": handle is NULL");
}

}  // namespace lio::capi

// =============================================================================
// filters
// =============================================================================
struct lio_filter : lio::capi::Handle {
    lio::FilterBuf b;
    float* d_in = nullptr;
    int64_t in_cap = 0;
    float* d_out = nullptr;
    int64_t out_cap = 0;
    int64_t* d_seg = nullptr;
    int64_t seg_cap = 0;
    double* d_T = nullptr;
    int64_t T_cap = 0;
    lio::ImuPose* d_poses = nullptr;
    int64_t poses_cap = 0;
    lio::DenoiseBuf dn;  // lio_sor_filter / lio_radius_first_seed / lio_denoise_slam_map
    lio::ClusterBuf cl;  // lio_euclidean_clusters, lio_dbscan (with dn: the grid, the sorts and the scan)
    lio::PlaneBuf pl;    // lio_segment_plane (with dn: the flags and the scan)
    lio::KMeansBuf km;   // lio_kmeans
    lio::NormalsBuf nm;  // lio_estimate_normals (with dn: the grid)
    lio::GpsAlignBuf ga; // lio_gps_align, lio_similarity2d_fit, lio_georeference_xy
    lio::ProjectBuf pj;  // lio_project_points, lio_undistort_map
};

namespace lio::capi {

// the upload the filter entries open with: `floats` floats at `host` into f->d_in, grown to hold them
static inline int upload_in(lio_filter* f, const float* host, int64_t floats) {
    const int rc = grow(&f->d_in, f->in_cap, floats);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(f->d_in, host, (size_t)floats * sizeof(float), hipMemcpyHostToDevice, f->st));
    return LIO_OK;
}

// the download the filter entries end with: m rows of `stride` floats from f->d_out to `out`, the wait, and
// *n_out = m (n_out may be null)
static inline int download_out(lio_filter* f, int64_t m, int stride, float* out, int64_t* n_out) {
    if (m) HIP_TRY(hipMemcpyAsync(out, f->d_out, (size_t)m * stride * sizeof(float), hipMemcpyDeviceToHost, f->st));
    HIP_TRY(hipStreamSynchronize(f->st));
    if (n_out) *n_out = m;
    return LIO_OK;
}

}  // namespace lio::capi
