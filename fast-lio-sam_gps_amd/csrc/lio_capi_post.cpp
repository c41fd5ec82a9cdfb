// lio_capi_post.cpp — the C-ABI (include/lio_gpu.h) of the offline leg's point cloud steps on a lio_filter:
// statistical outlier removal and the intensity map denoise, Euclidean clusters and DBSCAN, GPS-to-SLAM
// alignment and georeferencing, RANSAC plane segmentation, k-means, surface normals.  The handle's create / destroy are in lio_capi_prep.cpp.
#include <algorithm>

#include "lio_capi_util.hpp"
#include "lio_dbscan.hpp"

using namespace lio::capi;

extern "C" {

// ---- statistical outlier removal, first-seed radius query, intensity map denoise (lio_denoise.hip) ----
int lio_sor_filter(lio_filter* f, const float* pts, int64_t n, int stride, int mean_k, double stddev_mul, int negative,
                   float* out, int64_t* n_out, float* distances_opt, double* stats4_opt) {
    int rc = null_handle(f, "lio_sor_filter");
    if (rc) return rc;
    if (!n_out || n < 0 || (n > 0 && (!pts || !out)) || stride < 3 || stride > lio::kMaxFields || mean_k < 1 ||
        mean_k > 255 || n >= (int64_t)1 << 30)
        return fail(LIO_ERR_ARG, "lio_sor_filter: bad arguments");
    *n_out = 0;
    HIP_TRY(hipSetDevice(f->dev));
    if (n > 0) {
        rc = grow(&f->d_out, f->out_cap, n * stride);
        if (!rc) rc = upload_in(f, pts, n * stride);
        if (rc) return rc;
    }
    int64_t m = 0;
    rc = lio::sor_filter(f->dn, f->d_in, n, stride, mean_k, stddev_mul, negative != 0, f->d_out, &m, distances_opt,
                         stats4_opt, f->st);
    if (rc) return status(rc, "lio_sor_filter");
    return download_out(f, m, stride, out, n_out);
}

int lio_radius_first_seed(lio_filter* f, const float* pts, int64_t n, int stride, const float* seeds_xyz, int64_t ns,
                          float radius, int32_t* seed_out, float* d2_out_opt) {
    int rc = null_handle(f, "lio_radius_first_seed");
    if (rc) return rc;
    if (n < 0 || ns < 0 || (n > 0 && (!pts || !seed_out)) || (ns > 0 && !seeds_xyz) || stride < 3 ||
        stride > lio::kMaxFields || !(radius >= 0.f) || !std::isfinite(radius) || n >= (int64_t)1 << 30 ||
        ns >= (int64_t)1 << 30)
        return fail(LIO_ERR_ARG, "lio_radius_first_seed: bad arguments");
    if (n == 0) return LIO_OK;
    HIP_TRY(hipSetDevice(f->dev));
    rc = lio::denoise_reserve(f->dn, std::max(n, ns));
    if (rc) return status(rc, "lio_radius_first_seed");
    if ((rc = upload_in(f, pts, n * stride))) return rc;
    if (ns) HIP_TRY(hipMemcpyAsync(f->dn.seeds_xyz, seeds_xyz, (size_t)ns * 3 * sizeof(float), hipMemcpyHostToDevice, f->st));
    rc = lio::radius_first_seed(f->dn, f->d_in, n, stride, f->dn.seeds_xyz, ns, radius, f->dn.seed_id, f->dn.seed_d2,
                                f->st);
    if (rc) return status(rc, "lio_radius_first_seed");
    HIP_TRY(hipMemcpyAsync(seed_out, f->dn.seed_id, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, f->st));
    if (d2_out_opt)
        HIP_TRY(hipMemcpyAsync(d2_out_opt, f->dn.seed_d2, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, f->st));
    HIP_TRY(hipStreamSynchronize(f->st));
    return LIO_OK;
}

int lio_denoise_slam_map(lio_filter* f, const float* pts, int64_t n, const lio_denoise_params* p, float* out,
                         int64_t* n_out, int64_t* counts5_opt) {
    int rc = null_handle(f, "lio_denoise_slam_map");
    if (rc) return rc;
    if (!p || !n_out || n < 0 || (n > 0 && (!pts || !out)) || p->mean_k < 1 || p->mean_k > 255 ||
        !(p->cluster_seed_radius >= 0.f) || !(p->denoise_radius >= 0.f) || !std::isfinite(p->cluster_seed_radius) ||
        !std::isfinite(p->denoise_radius) || n >= (int64_t)1 << 29)
        return fail(LIO_ERR_ARG, "lio_denoise_slam_map: bad arguments");
    *n_out = 0;
    if (counts5_opt)
        for (int k = 0; k < 5; ++k) counts5_opt[k] = 0;
    if (n == 0) return LIO_OK;
    HIP_TRY(hipSetDevice(f->dev));
    rc = grow(&f->d_out, f->out_cap, n * 4);
    if (!rc) rc = upload_in(f, pts, n * 4);
    if (rc) return rc;
    const lio::DenoiseParams dp{p->seed_thres,  p->cluster_seed_radius, p->denoise_radius,
                                p->noise_thres, p->mean_k,              p->stddev_mul};
    int64_t m = 0;
    rc = lio::denoise_slam_map(f->dn, f->d_in, n, dp, f->d_out, &m, counts5_opt, f->st);
    if (rc) return status(rc, "lio_denoise_slam_map");
    return download_out(f, m, 4, out, n_out);
}

// ---- Euclidean cluster extraction and DBSCAN, both with per-cluster bounding boxes (lio_cluster.hip, lio_dbscan.hip) ----
// what both entries open with: the argument check (r: tolerance / eps; least: min_size / min_samples), the
// outputs of a call that finds nothing, the device and the upload.  The caller is done when this fails or n == 0.
static int cluster_begin(lio_filter* f, const char* what, const float* pts, int64_t n, int stride, float r, int64_t least,
                         const int32_t* labels_out, int64_t* n_clusters, int64_t cap_clusters, int64_t* offsets_opt,
                         int64_t* stats4_opt) {
    const int rc = null_handle(f, what);
    if (rc) return rc;
    if (!n_clusters || n < 0 || n >= (int64_t)1 << 31 || (n > 0 && (!pts || !labels_out)) || stride < 3 ||
        stride > lio::kMaxFields || !(r > 0.f) || !std::isfinite(r) || least < 1 || cap_clusters < 0)
        return fail(LIO_ERR_ARG, std::string(what) + ": bad arguments");
    *n_clusters = 0;
    if (stats4_opt)
        for (int k = 0; k < 4; ++k) stats4_opt[k] = 0;
    if (offsets_opt) offsets_opt[0] = 0;
    if (n == 0) return LIO_OK;
    HIP_TRY(hipSetDevice(f->dev));
    return upload_in(f, pts, n * stride);
}

// what both entries end with: labels, DBSCAN's core flags, the grouped indices, offsets and boxes of the first
// min(clusters, cap_clusters) clusters, the wait, and the counts (stats[2] = clusters, stats[3] = points in them)
static int cluster_download(lio_filter* f, int64_t n, const int64_t (&stats)[4], int32_t* labels_out, uint8_t* core_opt,
                            int64_t* n_clusters, int64_t cap_clusters, int64_t* offsets_opt, int32_t* indices_opt,
                            float* aabb6_opt, int64_t* stats4_opt) {
    const int64_t m = std::min(stats[2], cap_clusters);
    HIP_TRY(hipMemcpyAsync(labels_out, f->cl.labels, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, f->st));
    if (core_opt) HIP_TRY(hipMemcpyAsync(core_opt, f->cl.rank_of, (size_t)n, hipMemcpyDeviceToHost, f->st));
    if (indices_opt && stats[3])
        HIP_TRY(hipMemcpyAsync(indices_opt, f->cl.indices, (size_t)stats[3] * sizeof(int32_t), hipMemcpyDeviceToHost, f->st));
    if (offsets_opt)
        HIP_TRY(hipMemcpyAsync(offsets_opt, f->cl.offsets, (size_t)(m + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, f->st));
    if (aabb6_opt && m)
        HIP_TRY(hipMemcpyAsync(aabb6_opt, f->cl.aabb, (size_t)m * 6 * sizeof(float), hipMemcpyDeviceToHost, f->st));
    HIP_TRY(hipStreamSynchronize(f->st));
    *n_clusters = stats[2];
    if (stats4_opt)
        for (int k = 0; k < 4; ++k) stats4_opt[k] = stats[k];
    return LIO_OK;
}

int lio_euclidean_clusters(lio_filter* f, const float* pts, int64_t n, int stride, float tolerance, int64_t min_size,
                           int64_t max_size, int32_t* labels_out, int64_t* n_clusters, int64_t cap_clusters,
                           int64_t* offsets_opt, int32_t* indices_opt, float* aabb6_opt, int64_t* stats4_opt) {
    int rc = cluster_begin(f, "lio_euclidean_clusters", pts, n, stride, tolerance, min_size, labels_out, n_clusters,
                           cap_clusters, offsets_opt, stats4_opt);
    if (rc || n == 0) return rc;
    lio::ClusterCounts cc;
    rc = lio::euclidean_clusters(f->dn, f->cl, f->d_in, n, stride, tolerance, min_size, max_size, cap_clusters, &cc, f->st);
    if (rc) return status(rc, "lio_euclidean_clusters");
    return cluster_download(f, n, {cc.finite, cc.components, cc.clusters, cc.clustered_points}, labels_out, nullptr,
                            n_clusters, cap_clusters, offsets_opt, indices_opt, aabb6_opt, stats4_opt);
}

int lio_dbscan(lio_filter* f, const float* pts, int64_t n, int stride, float eps, int64_t min_samples,
               int32_t* labels_out, uint8_t* core_opt, int64_t* n_clusters, int64_t cap_clusters,
               int64_t* offsets_opt, int32_t* indices_opt, float* aabb6_opt, int64_t* stats4_opt) {
    int rc = cluster_begin(f, "lio_dbscan", pts, n, stride, eps, min_samples, labels_out, n_clusters, cap_clusters,
                           offsets_opt, stats4_opt);
    if (rc || n == 0) return rc;
    lio::DbscanCounts dc;
    rc = lio::dbscan(f->dn, f->cl, f->d_in, n, stride, eps, min_samples, cap_clusters, &dc, f->st);
    if (rc) return status(rc, "lio_dbscan");
    return cluster_download(f, n, {dc.finite, dc.core, dc.clusters, dc.clustered_points}, labels_out, core_opt, n_clusters,
                            cap_clusters, offsets_opt, indices_opt, aabb6_opt, stats4_opt);
}

// ---- GPS-to-SLAM trajectory alignment and map georeferencing (lio_gpsalign.hip) ----
static_assert(lio::kGaLen == LIO_GPSALIGN_LEN && lio::kGaIters == LIO_GPSALIGN_ITERATIONS &&
                  lio::kGaConverged == LIO_GPSALIGN_CONVERGED && lio::kGaMeanError == LIO_GPSALIGN_MEAN_ERROR &&
                  lio::kGaS0 == LIO_GPSALIGN_S0 && lio::kGaCA == LIO_GPSALIGN_CA && lio::kGaCB == LIO_GPSALIGN_CB &&
                  lio::kGaSc == LIO_GPSALIGN_SC && lio::kGaC == LIO_GPSALIGN_C && lio::kGaS == LIO_GPSALIGN_S &&
                  lio::kGaT == LIO_GPSALIGN_T && lio::kGaCD == LIO_GPSALIGN_CD && lio::kGaRefScale == LIO_GPSALIGN_REF_SCALE &&
                  lio::kGaRefC == LIO_GPSALIGN_REF_C && lio::kGaRefS == LIO_GPSALIGN_REF_S &&
                  lio::kGaRefT == LIO_GPSALIGN_REF_T && lio::kGaTotScale == LIO_GPSALIGN_TOTAL_SCALE &&
                  lio::kGaTotC == LIO_GPSALIGN_TOTAL_C && lio::kGaTotS == LIO_GPSALIGN_TOTAL_S &&
                  lio::kGaTotT == LIO_GPSALIGN_TOTAL_T && lio::kSimLen == LIO_SIM2D_LEN && lio::kSimScale == LIO_SIM2D_SCALE &&
                  lio::kSimC == LIO_SIM2D_C && lio::kSimS == LIO_SIM2D_S && lio::kSimT == LIO_SIM2D_T &&
                  lio::kGaState == LIO_ERR_STATE,
              "the result offsets of lio_gpsalign.hpp are the public ones");

// the status of the two fits: kGaState carries its own text
static int fit_status(int rc, const char* what, const char* arg_what) {
    if (rc == lio::kGaState) return fail(LIO_ERR_STATE, std::string(what) + ": " + lio::last_error());
    return status(rc, what, arg_what);
}

int lio_gps_align(lio_filter* f, const double* gps_xy, int64_t m, const double* slam_xy, int64_t n, int max_iterations,
                  double tolerance, double* aligned_xy_out, int32_t* nn_out_opt, double* out) {
    const int rc = null_handle(f, "lio_gps_align");
    if (rc) return rc;
    if (!gps_xy || !slam_xy || !aligned_xy_out || !out || n < 1 || m < 1 || n >= (int64_t)1 << 31 ||
        m >= (int64_t)1 << 31 || max_iterations < 1)
        return fail(LIO_ERR_ARG, "lio_gps_align: bad arguments");
    if (!all_finite(gps_xy, 2 * m) || !all_finite(slam_xy, 2 * n))
        return fail(LIO_ERR_ARG, "lio_gps_align: a coordinate is not finite");
    HIP_TRY(hipSetDevice(f->dev));
    return fit_status(lio::gps_align(f->ga, gps_xy, m, slam_xy, n, max_iterations, tolerance, aligned_xy_out, nn_out_opt,
                                     out, f->st),
                      "lio_gps_align", "a point set has zero variance");
}

int lio_similarity2d_fit(lio_filter* f, const double* src_xy, const double* dst_xy, int64_t n, double* out) {
    const int rc = null_handle(f, "lio_similarity2d_fit");
    if (rc) return rc;
    if (!src_xy || !dst_xy || !out || n < 1 || n >= (int64_t)1 << 31)
        return fail(LIO_ERR_ARG, "lio_similarity2d_fit: bad arguments");
    if (!all_finite(src_xy, 2 * n) || !all_finite(dst_xy, 2 * n))
        return fail(LIO_ERR_ARG, "lio_similarity2d_fit: a coordinate is not finite");
    HIP_TRY(hipSetDevice(f->dev));
    return fit_status(lio::similarity2d_fit(f->ga, src_xy, dst_xy, n, out, f->st), "lio_similarity2d_fit", "bad arguments");
}

int lio_georeference_xy(lio_filter* f, const float* pts, int64_t n, int stride, double scale, const double* R4,
                        const double* t2, const double* origin2_opt, float* out, double* xy_out_opt) {
    int rc = null_handle(f, "lio_georeference_xy");
    if (rc) return rc;
    if (!R4 || !t2 || n < 0 || n >= (int64_t)1 << 31 || (n > 0 && (!pts || !out)) || stride < 3 || stride > lio::kMaxFields)
        return fail(LIO_ERR_ARG, "lio_georeference_xy: bad arguments");
    if (n == 0) return LIO_OK;
    HIP_TRY(hipSetDevice(f->dev));
    if ((rc = upload_in(f, pts, n * stride))) return rc;
    if ((rc = grow(&f->d_out, f->out_cap, n * stride))) return rc;
    if (xy_out_opt && (rc = grow(&f->ga.geo_xy, f->ga.geo_cap, n, 2))) return rc;
    const double p[9] = {R4[0], R4[1], R4[2], R4[3], scale, t2[0], t2[1], origin2_opt ? origin2_opt[0] : 0.0,
                         origin2_opt ? origin2_opt[1] : 0.0};
    rc = lio::georeference_xy(f->d_in, n, stride, p, f->d_out, xy_out_opt ? f->ga.geo_xy : nullptr, f->st);
    if (rc) return status(rc, "lio_georeference_xy");
    if (xy_out_opt)
        HIP_TRY(hipMemcpyAsync(xy_out_opt, f->ga.geo_xy, (size_t)n * 2 * sizeof(double), hipMemcpyDeviceToHost, f->st));
    return download_out(f, n, stride, out, nullptr);
}

// ---- RANSAC plane segmentation (lio_plane.hip) ----
int lio_plane_sample_triples(uint64_t seed, int64_t n, int64_t num_iterations, int32_t* out) {
    if (n < 0 || n >= (int64_t)1 << 31 || num_iterations < 0 || num_iterations > (int64_t)1 << 20 ||
        (n >= 3 && num_iterations > 0 && !out))
        return fail(LIO_ERR_ARG, "lio_plane_sample_triples: bad arguments");
    if (n >= 3) lio::plane_sample_triples(seed, n, num_iterations, out);
    return LIO_OK;
}

int lio_segment_plane(lio_filter* f, const float* pts, int64_t n, int stride, float distance_threshold, int ransac_n,
                      int64_t num_iterations, uint64_t seed, const int32_t* triples_opt, float* plane4_out,
                      int64_t* best_iteration, int32_t* inliers_out, int64_t* n_inliers, uint8_t* mask_opt,
                      int64_t* counts_opt, uint64_t* sq_opt, uint8_t* degenerate_opt, double* refit4_opt) {
    int rc = null_handle(f, "lio_segment_plane");
    if (rc) return rc;
    const int64_t K = num_iterations;
    const float thr2 = distance_threshold * distance_threshold;
    if (!plane4_out || !best_iteration || !n_inliers || n < 0 || n >= (int64_t)1 << 31 || (n > 0 && (!pts || !inliers_out)) ||
        stride < 3 || stride > lio::kMaxFields || !(distance_threshold > 0.f) || !std::isfinite(distance_threshold) ||
        !std::isfinite(thr2) || ransac_n != 3 || K < 1 || K > (int64_t)1 << 20)
        return fail(LIO_ERR_ARG, "lio_segment_plane: bad arguments");
    if (triples_opt && !lio::plane_triples_valid(triples_opt, K, n))
        return fail(LIO_ERR_ARG, "lio_segment_plane: a triple holds an index outside [0, n) or a repeated index");
    for (int k = 0; k < 4; ++k) plane4_out[k] = 0.f;
    *best_iteration = -1;
    *n_inliers = 0;
    if (refit4_opt)
        for (int k = 0; k < 4; ++k) refit4_opt[k] = 0.0;
    if (n < 3) {  // no hypothesis at all: every entry counts as skipped
        if (mask_opt && n) std::memset(mask_opt, 0, (size_t)n);
        if (counts_opt) std::memset(counts_opt, 0, (size_t)K * sizeof(int64_t));
        if (sq_opt) std::memset(sq_opt, 0, (size_t)K * sizeof(uint64_t));
        if (degenerate_opt) std::memset(degenerate_opt, 1, (size_t)K);
        return LIO_OK;
    }
    lio::PlaneBuf& pb = f->pl;
    if ((int64_t)pb.h_planes.size() < 4 * K) pb.h_planes.resize((size_t)(4 * K));
    if ((int64_t)pb.h_deg.size() < K) pb.h_deg.resize((size_t)K);
    const int32_t* tri = triples_opt;
    if (!tri) {
        if ((int64_t)pb.h_tri.size() < 3 * K) pb.h_tri.resize((size_t)(3 * K));
        lio::plane_sample_triples(seed, n, K, pb.h_tri.data());
        tri = pb.h_tri.data();
    }
    lio::plane_hypotheses(pts, stride, tri, K, pb.h_planes.data(), pb.h_deg.data());
    HIP_TRY(hipSetDevice(f->dev));
    if ((rc = upload_in(f, pts, n * stride))) return rc;
    lio::PlaneResult pr;
    rc = lio::segment_plane(f->dn, pb, f->d_in, pts, n, stride, distance_threshold, K, refit4_opt != nullptr, &pr, f->st);
    if (rc) return status(rc, "lio_segment_plane");
    if (pr.n_inliers)
        HIP_TRY(hipMemcpyAsync(inliers_out, pb.inliers, (size_t)pr.n_inliers * sizeof(int32_t), hipMemcpyDeviceToHost, f->st));
    if (mask_opt) HIP_TRY(hipMemcpyAsync(mask_opt, pb.mask, (size_t)n, hipMemcpyDeviceToHost, f->st));
    if (counts_opt) HIP_TRY(hipMemcpyAsync(counts_opt, pb.cnt, (size_t)K * sizeof(int64_t), hipMemcpyDeviceToHost, f->st));
    if (sq_opt) HIP_TRY(hipMemcpyAsync(sq_opt, pb.sq, (size_t)K * sizeof(uint64_t), hipMemcpyDeviceToHost, f->st));
    HIP_TRY(hipStreamSynchronize(f->st));
    if (degenerate_opt) std::memcpy(degenerate_opt, pb.h_deg.data(), (size_t)K);
    std::memcpy(plane4_out, pr.plane, sizeof(pr.plane));
    *best_iteration = pr.best;
    *n_inliers = pr.n_inliers;
    if (refit4_opt) std::memcpy(refit4_opt, pr.refit, sizeof(pr.refit));
    return LIO_OK;
}

// ---- k-means with k-means++ seeding and per-cluster boxes (lio_kmeans.hip) ----
// The arguments are judged before the handle, so a bad call is LIO_ERR_ARG with or without a device.
int lio_kmeans(lio_filter* f, const float* pts, int64_t n, int stride, int K, int max_iter, float eps, int attempts,
               uint64_t seed, const float* init_centers_opt, int32_t* labels_out, float* centers_out,
               double* compactness_out, int64_t* counts_opt, float* aabb6_opt, int32_t* seeds_opt,
               uint64_t* attempt_q_opt, int32_t* attempt_iters_opt, int64_t* stats6_opt) {
    if (!centers_out || !compactness_out || n < 0 || n >= (int64_t)1 << 31 || (n > 0 && (!pts || !labels_out)) ||
        stride < 3 || stride > lio::kMaxFields || K < 1 || K > lio::kKmMaxK || attempts < 1 ||
        attempts > lio::kKmMaxAttempts || max_iter < 1 || max_iter > lio::kKmMaxIter || !(eps >= 0.f) || !std::isfinite(eps))
        return fail(LIO_ERR_ARG, "lio_kmeans: bad arguments");
    if (init_centers_opt)
        for (int64_t k = 0; k < (int64_t)attempts * K * 3; ++k)
            if (!std::isfinite(init_centers_opt[k]))
                return fail(LIO_ERR_ARG, "lio_kmeans: an initial centre is not finite");
    if (n < K) return fail(LIO_ERR_ARG, "lio_kmeans: fewer finite points than clusters");
    int rc = null_handle(f, "lio_kmeans");
    if (rc) return rc;
    HIP_TRY(hipSetDevice(f->dev));
    if ((rc = upload_in(f, pts, n * stride))) return rc;
    lio::KMeansArgs ka;
    ka.K = K, ka.max_iter = max_iter, ka.attempts = attempts, ka.eps = eps, ka.seed = seed, ka.init_centers = init_centers_opt;
    lio::KMeansResult kr;
    rc = lio::kmeans(f->km, f->d_in, pts, n, stride, ka, aabb6_opt != nullptr, &kr, f->st);
    if (rc) return status(rc, "lio_kmeans", lio::last_error().c_str());
    HIP_TRY(hipMemcpyAsync(labels_out, kr.labels, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, f->st));
    HIP_TRY(hipStreamSynchronize(f->st));
    std::memcpy(centers_out, kr.centers, (size_t)K * 3 * sizeof(float));
    *compactness_out = std::ldexp((double)kr.attempt_q[kr.best], kr.ed - 31);
    if (counts_opt) std::memcpy(counts_opt, kr.counts, (size_t)K * sizeof(int64_t));
    if (aabb6_opt) std::memcpy(aabb6_opt, kr.aabb, (size_t)K * 6 * sizeof(float));
    if (seeds_opt) std::memcpy(seeds_opt, kr.seeds, (size_t)attempts * K * sizeof(int32_t));
    if (attempt_q_opt) std::memcpy(attempt_q_opt, kr.attempt_q, (size_t)attempts * sizeof(uint64_t));
    if (attempt_iters_opt) std::memcpy(attempt_iters_opt, kr.attempt_iters, (size_t)attempts * sizeof(int32_t));
    if (stats6_opt) {
        const int64_t s6[6] = {kr.nf, kr.best, kr.attempt_iters[kr.best], kr.repairs, kr.ec, kr.ed};
        std::memcpy(stats6_opt, s6, sizeof(s6));
    }
    return LIO_OK;
}

// ---- surface normals and curvature (lio_normals.hip) ----
// The arguments are judged before the handle, so a bad call is LIO_ERR_ARG with or without a device.
int lio_estimate_normals(lio_filter* f, const float* pts, int64_t n, int stride, float radius, int k,
                         const float* viewpoints_opt, int vp_stride, float* normals_out, float* curvature_opt,
                         int32_t* counts_opt, int64_t* stats6_opt) {
    const float r2 = (float)((double)radius * (double)radius);
    if (n < 0 || n >= (int64_t)1 << 31 || (n > 0 && (!pts || !normals_out)) || stride < 3 || stride > lio::kMaxFields ||
        !(radius >= 0.f) || !std::isfinite(radius) || (radius > 0.f && (!(r2 > 0.f) || !std::isfinite(r2))) ||
        (k != 0 && (k < 3 || k > lio::kNmMaxK)) || (k == 0 && !(radius > 0.f)) ||
        (vp_stride != 0 && (vp_stride < 3 || vp_stride > lio::kMaxFields)))
        return fail(LIO_ERR_ARG, "lio_estimate_normals: bad arguments");
    int rc = null_handle(f, "lio_estimate_normals");
    if (rc) return rc;
    if (stats6_opt)
        for (int c = 0; c < 6; ++c) stats6_opt[c] = 0;
    if (n == 0) return LIO_OK;
    HIP_TRY(hipSetDevice(f->dev));
    const int64_t vp_floats = viewpoints_opt ? (vp_stride ? n * vp_stride : 3) : 0;
    if ((rc = upload_in(f, pts, n * stride))) return rc;
    rc = lio::normals_reserve(f->nm, n, vp_floats, k > 0);
    if (rc) return status(rc, "lio_estimate_normals");
    if (vp_floats)
        HIP_TRY(hipMemcpyAsync(f->nm.vp, viewpoints_opt, (size_t)vp_floats * sizeof(float), hipMemcpyHostToDevice, f->st));
    rc = lio::estimate_normals(f->dn, f->nm, f->d_in, n, stride, radius, k, vp_floats ? f->nm.vp : nullptr, vp_stride, f->st);
    if (rc) return status(rc, "lio_estimate_normals");
    HIP_TRY(hipMemcpyAsync(normals_out, f->nm.normals, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, f->st));
    if (curvature_opt)
        HIP_TRY(hipMemcpyAsync(curvature_opt, f->nm.curvature, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, f->st));
    if (counts_opt)
        HIP_TRY(hipMemcpyAsync(counts_opt, f->nm.counts, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, f->st));
    HIP_TRY(hipStreamSynchronize(f->st));
    if (stats6_opt) std::memcpy(stats6_opt, f->nm.h_stats, 6 * sizeof(int64_t));
    return LIO_OK;
}

}  // extern "C"
