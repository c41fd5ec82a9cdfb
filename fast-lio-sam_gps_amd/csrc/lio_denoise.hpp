// lio_denoise.hpp — statistical outlier removal, first-seed radius query and the intensity map denoise
// (lio_denoise.hip): pcl::StatisticalOutlierRemoval [U], KdTreeFLANN::radiusSearch per seed turned round [U],
// FastLioSam::denoise_slam_map (fast_lio_sam.cpp:941-1008).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lio {

// Grid geometry of one search, computed on the device (no host wait during the build).
struct DnGeom {
    float ox, oy, oz;  // AABB minimum of the finite points
    float cell, inv;
    float margin;      // bound on the rounding of a cell face against a point's cell assignment [m]
    int nx, ny, nz;
    uint32_t ncells;
};

// Scratch of the denoise entry points: ONE device arena carved into the buffers below (denoise_reserve lists
// them once, for lio_scratch.hpp's Carver), sized for `cap` points and grown geometrically (counted:
// lio_alloc_count), plus pinned host memory for the SOR distance vector and the small counts.
struct DenoiseBuf {
    void* arena = nullptr;
    size_t arena_bytes = 0;
    int64_t cap = 0;
    // grid build (one search at a time)
    uint32_t *keys = nullptr, *keys_alt = nullptr, *vals = nullptr, *vals_alt = nullptr;
    uint32_t* start = nullptr;  // cap + 66 CSR offsets
    float4* g4 = nullptr;       // points sorted by cell: (x, y, z, input index bits)
    float* part = nullptr;      // AABB partials
    DnGeom* geom = nullptr;
    // results / compaction
    float* dist = nullptr;      // SOR mean distances (-1: not counted)
    uint32_t *flags = nullptr, *pos = nullptr;  // cap + 1 each
    // denoise_slam_map
    float* seeds_xyz = nullptr;  // 3 cap
    int32_t* seed_id = nullptr;
    float* seed_d2 = nullptr;
    uint32_t *idx = nullptr, *idx_alt = nullptr;
    uint64_t *k64 = nullptr, *k64_alt = nullptr;
    float *cloud_a = nullptr, *cloud_b = nullptr;  // 4 cap each
    void* tmp = nullptr;         // hipcub scratch
    size_t tmp_bytes = 0;
    float* h_dist = nullptr;     // pinned, cap floats
    size_t h_dist_bytes = 0;
    uint32_t* h_cnt = nullptr;   // pinned: compaction counts
};

struct DenoiseParams {
    float seed_thres, cluster_seed_radius, denoise_radius, noise_thres;
    int mean_k;
    float stddev_mul;
};

void denoise_free(DenoiseBuf& b);
// every buffer sized for n points (n >= the cloud and the seed count of the calls that follow)
int denoise_reserve(DenoiseBuf& b, int64_t n);

// The building blocks the searches share (lio_cluster.hip uses them too), after denoise_reserve(b, >= n).  Status
// as the entry points' (lio_scratch.hpp): kOk, or kHip with the failed HIP call's text in last_error().
// The grid of the finite points of d_pts in b.g4 (x, y, z, input index; cell order) / b.start (CSR offsets;
// b.start[ncells] = finite points) / b.geom, enqueued (no host wait).  target > 0: cell edge from the density
// (a 3x3x3 block holds about `target` points); target == 0: the edge is fixed_cell.  Either edge grows until
// the grid has at most n + 64 cells.  Uses b.keys / b.vals (and their _alt) and b.part.
int dn_build_grid(DenoiseBuf& b, const float* d_pts, int64_t n, int stride, float target, float fixed_cell,
                  hipStream_t st);
// stable radix sorts over the low `bits` bits, enqueued: (b.keys, b.vals) -> (b.keys_alt, b.vals_alt);
// (b.k64, b.idx) -> (b.k64_alt, b.idx_alt)
int dn_sort32(DenoiseBuf& b, int64_t n, int bits, hipStream_t st);
int dn_sort64(DenoiseBuf& b, int64_t n, int bits, hipStream_t st);
// b.pos = exclusive scan of b.flags[0 .. n]; *count = b.pos[n].  Waits for the stream.
int dn_scan_count(DenoiseBuf& b, int64_t n, int64_t* count, hipStream_t st);
int dn_bit_width(uint32_t v);  // bits needed for v, at least 1

// Kernel A, enqueued: d_dist[i] = mean distance of point i to its mean_k nearest neighbours, -1 for a point that
// is not counted (non-finite, or fewer than mean_k + 1 finite points in the cloud).  A d_dist inside b (b.dist)
// is read after denoise_reserve(b, n): the arena's pointers are set there.
int sor_distances(DenoiseBuf& b, const float* d_pts, int64_t n, int stride, int mean_k, float* d_dist, hipStream_t st);
// pcl::StatisticalOutlierRemoval::applyFilter on device records; d_out capacity n x stride.  Waits for the
// stream (the distance vector crosses to the host for the double sums).  h_dist_out (optional): the n distances
// (0 where not counted); stats4 (optional): mean, stddev, threshold, counted points.
int sor_filter(DenoiseBuf& b, const float* d_pts, int64_t n, int stride, int mean_k, double stddev_mul, bool negative,
               float* d_out, int64_t* n_out, float* h_dist_out, double* stats4, hipStream_t st);
// Kernel B, enqueued: d_seed[i] = lowest seed index with sqdist3(point i, seed) < r2 (strict), or -1;
// d_d2 (optional) that squared distance (0 where none).
int radius_first_seed(DenoiseBuf& b, const float* d_pts, int64_t n, int stride, const float* d_seeds_xyz, int64_t ns,
                      float radius, int32_t* d_seed, float* d_d2, hipStream_t st);
// FastLioSam::denoise_slam_map on PointXYZI records (stride 4); d_out capacity n x 4; counts5 (optional):
// seeds, segmented, after SOR, denoised, remained.
int denoise_slam_map(DenoiseBuf& b, const float* d_pts, int64_t n, const DenoiseParams& p, float* d_out,
                     int64_t* n_out, int64_t* counts5, hipStream_t st);

}  // namespace lio
