// lio_capi_online.hpp — the online leg's two handles (C-ABI lio_map_*, lio_ctx_*, lio_scan_*) and what their files
// share.  Private, like lio_capi_util.hpp, on which it stands.  The files, by concern:
//   lio_capi.cpp          the library level: device count, last error, build info, the ABI's struct sizes
//   lio_capi_map.cpp      lio_map: create / destroy, build, queries, add / delete, the local-map cube
//   lio_capi_scan.cpp     lio_ctx: create / destroy, the scan's buffers, lio_match, the IESKF update, map_incremental,
//                         the readers and the timing
//   lio_capi_prep.cpp     the filter handle's create / destroy, voxel grid, submap voxelize, the sweep preprocessing
//                         on a filter and on a ctx
//   lio_capi_formats.cpp  PointCloud2 decode / encode, PCD write / read, a map from a PCD
// A lio_map owns its stream, the grid, the map-update scratch and the query staging; a lio_ctx borrows the map's
// device and stream and owns one scan: its buffers, the evaluation's result block, the preprocessing scratch.
#pragma once
#include <atomic>
#include <cmath>

#include "lio_capi_util.hpp"
#include "lio_mapupd.hpp"

struct lio_map : lio::capi::Handle {
    uint64_t version = 0;  // bumped by every change of the point set (seeded kNN validity)
    std::atomic<int> n_ctx{0};  // live lio_ctx handles on this map (destroy refuses while > 0)
    lio_map_params p{};
    lio::GridBuf grid;
    lio::MapUpdBuf upd;
    float* d_xyz = nullptr;
    int64_t xyz_cap = 0;
    int64_t n = 0;  // alive points (== grid.n)
    int32_t* d_qidx = nullptr;  // lio_map_nearest_search results
    int64_t qidx_cap = 0;
    float* d_qd2 = nullptr;
    int64_t qd2_cap = 0;
};

namespace lio::capi {
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
};
}  // namespace lio::capi

struct lio_ctx {
    lio_map* map = nullptr;
    double last_launch_ms = 0.0, last_wait_ms = 0.0;  // host side of the last lio_match
    lio_match_params p{};
    int64_t n = 0, cap = 0;
    float* d_body = nullptr;
    const float* body_ext = nullptr;  // lio_scan_bind_device: caller-owned scan (no copy)
    int32_t* d_nn = nullptr;
    float4* d_planes = nullptr;
    uint8_t* d_sel = nullptr;
    double* d_partials = nullptr;
    int64_t part_cap = 0;
    double* d_sums = nullptr;
    double* h_sums = nullptr;    // pinned, host-mapped: [0,32) sums, [32] sequence number, [33] checksum
    double* h_sums_dev = nullptr;  // device view of h_sums
    unsigned long long seq = 0;
    double* d_rows = nullptr;
    int64_t rows_cap = 0;
    int64_t* d_nrows = nullptr;
    lio_pose last_pose{};
    lio_pose knn_pose{};  // pose of the last kNN evaluation (Nearest_Points)
    lio::FarEntry* d_far_q = nullptr;  // far-pass queue (one entry per queued query) and its length
    int64_t far_cap = 0;
    int* d_far_count = nullptr;
    unsigned* d_done = nullptr;  // plane/reuse block counter (last block publishes)
    float* d_d5 = nullptr;  // per point: 5th neighbour d2 of the last kNN
    float* d_dbg = nullptr;  // scratch of the debug readers (lio_get_knn / _planes / _world, lio_ctx_knn_stats)
    int64_t dbg_cap = 0;
    bool have_eval = false;
    bool knn_valid = false;
    uint64_t knn_map_version = 0;  // map version of the last kNN evaluation
    // timing
    bool timing = false;
    lio_kernel_timing tm{};
    lio::capi::EventPair ev_main, ev_fin;
    hipEvent_t ev_marks[8] = {};  // kernel start / stop: near, far, plane, reuse (hipExtLaunchKernel)
    lio::FilterBuf filt;                          // scan preprocessing
    float* d_raw = nullptr;                       // raw records / preprocessed records
    int64_t raw_cap = 0;
    float* d_rec = nullptr;
    int64_t rec_cap = 0;
    lio::ImuPose* d_poses = nullptr;
    int64_t poses_cap = 0;
    float seed_scale = 1.0f;  // lio_ctx_set_seed_scale (test hook: < 1 exercises the seeded pass's guard)
    int64_t undist_n = -1;    // feats_undistort of the last lio_scan_preprocess* (records in filt.c); -1: none
    int undist_stride = 0;
    float* d_kf = nullptr;    // lio_scan_keyframe_cloud output (n x 4)
    int64_t kf_cap = 0;
};

namespace lio::capi {

// Eigen 3.3 quaternionbase_assign_impl<Other,3,3>::run (Geometry/Quaternion.h): rotation matrix ->
// quaternion (w, x, y, z), trace = m00 + (m11 + m22).  Only for callers that hand over matrices
// without the state quaternion (lio_pose.q all zero); the oracle derives it the same way.
static inline void mat_to_quat(const double* m, double* q) {
    auto M = [&](int r, int c) { return m[3 * r + c]; };
    double t = M(0, 0) + (M(1, 1) + M(2, 2));
    double c[4];  // x, y, z, w
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        c[3] = 0.5 * t;
        t = 0.5 / t;
        c[0] = (M(2, 1) - M(1, 2)) * t;
        c[1] = (M(0, 2) - M(2, 0)) * t;
        c[2] = (M(1, 0) - M(0, 1)) * t;
    } else {
        int i = 0;
        if (M(1, 1) > M(0, 0)) i = 1;
        if (M(2, 2) > M(i, i)) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(M(i, i) - M(j, j) - M(k, k) + 1.0);
        c[i] = 0.5 * t;
        t = 0.5 / t;
        c[3] = (M(k, j) - M(j, k)) * t;
        c[j] = (M(j, i) + M(i, j)) * t;
        c[k] = (M(k, i) + M(i, k)) * t;
    }
    q[0] = c[3], q[1] = c[0], q[2] = c[1], q[3] = c[2];
}

static inline bool quat_zero(const double* q) { return q[0] == 0.0 && q[1] == 0.0 && q[2] == 0.0 && q[3] == 0.0; }

// The quaternions take precedence over R / R_LI (include/lio_gpu.h lio_pose): the kernels rotate with
// q / q_LI; a caller that fills only the matrices gets q derived from them.
static inline lio_pose filled(const lio_pose& p) {
    lio_pose o = p;
    if (quat_zero(o.q)) mat_to_quat(o.R, o.q);
    if (quat_zero(o.q_LI)) mat_to_quat(o.R_LI, o.q_LI);
    return o;
}

// Eigen QuaternionBase::toRotationMatrix (q = w, x, y, z; any norm is used as given)
static inline void quat_to_mat(const double* q, double* R) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
    R[3] = txy + twz, R[4] = 1 - (txx + tzz), R[5] = tyz - twx;
    R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1 - (txx + tyy);
}

// geometry slack when an insert leaves the grid: the rebuild reserves room
// around the map (half a local-map cube of travel at the usual 1 m cells)
static inline float map_slack(const lio_map* m) { return 64.f * m->grid.geom.cell; }

static inline const float* body_ptr(const lio_ctx* c) { return c->body_ext ? c->body_ext : c->d_body; }

// ---- lio_capi_scan.cpp
// the scan's buffers hold n points (contents are not kept across a growth); c->n = n, no scan bound, no
// evaluation.  The preprocessing sizes them for its row bound and sets c->n to the count afterwards.
int ctx_reserve(lio_ctx* c, int64_t n);

}  // namespace lio::capi
