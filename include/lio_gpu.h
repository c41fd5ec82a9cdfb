/*
 * lio_gpu.h — C-ABI of the MI355X (gfx950) scan-matching hot path.
 *
 * Drop-in boundary for the reference's hot path:
 *
 *  B-front: FAST-LIO's measurement model `void h_share_model(state_ikfom&,
 *    esekfom::dyn_share_datastruct<double>&)` plus the ikd-Tree it queries
 *    (upstream hku-mars FAST_LIO src/laserMapping.cpp + include/ikd-Tree; the
 *    Kodifly fork is an empty submodule in the reference: .gitmodules:1-3,
 *    launched by fast_lio_sam/launch/run.launch:20-46).  The host IESKF keeps
 *    its 23-dim state; one lio_match() per h-evaluation replaces the per-point
 *    OpenMP loop, and lio_ieskf_update() is the complete
 *    `kf.update_iterated_dyn_share_modified(LASER_POINT_COV, solve_H_time)`.
 *  B-loop: `RegistrationOutput LoopClosure::icpAlignment(src, dst)`
 *    (/root/reference/fast_lio_sam/src/loop_closure.cpp:69-92, declared at
 *    include/loop_closure.h:59-60) — replaced whole by lio_icp_align().
 *
 * Conventions: every call returns int status (LIO_OK = 0, < 0 on error;
 * lio_last_error() gives text).  Host buffers are caller-owned and copied in;
 * handles own device memory; one HIP stream per handle; a handle is not
 * thread-safe, distinct handles may be used concurrently.  No torch types.
 * There is no CPU fallback: without a gfx950 device every compute entry point
 * fails with LIO_ERR_NODEV.
 */
#ifndef LIO_GPU_H
#define LIO_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIO_OK 0
#define LIO_ERR_ARG (-1)
#define LIO_ERR_HIP (-2)
#define LIO_ERR_NODEV (-3)
#define LIO_ERR_STATE (-4)
#define LIO_ERR_NOMEM (-5)

#define LIO_NUM_MATCH_POINTS 5 /* NUM_MATCH_POINTS [U: FAST-LIO common_lib.h] */
#define LIO_STATE_DIM 23       /* state_ikfom DOF [U: FAST-LIO use-ikfom.hpp] */

/* Layout of the per-h-evaluation reduction returned by lio_match() (doubles):
 * H^T H upper triangle of the 6 non-zero columns (extrinsic_est_en = false,
 * kitti.yaml:22) row-major i<=j, H^T h, effct_feat_num, total_residual, h^T h. */
#define LIO_SUMS_HTH 0
#define LIO_SUMS_HTh 21
#define LIO_SUMS_NEFF 27
#define LIO_SUMS_RES 28
#define LIO_SUMS_HH 29
#define LIO_SUMS_LEN 32

/* ------------------------------------------------------------------ device */
int lio_device_count(void);
const char* lio_last_error(void);
const char* lio_build_info(void);
/* Diagnostics (no device needed): device / pinned allocations the library's growth paths (loop ICP, grids,
 * filters, scan buffers, map updates) have made in this process.  A warm loop-closure sequence adds none (bench.py
 * loop_sequence).                                                                                  */
int64_t lio_alloc_count(void);
/* ABI guard (no device needed): sizeof of the public structs, in the order map_params, match_params, pose,
 * state, ieskf_params, ieskf_stats, icp_params, icp_result, localmap, incremental_stats, imu_pose,
 * scan_prep_params, cloud_field, kernel_timing, denoise_params — the first min(n, count) into out; returns the count.
 * A binding built against another header version must refuse the library (an output struct of the wrong
 * size is a buffer overrun: round 4's A/B of a round-2 build segfaulted at exit that way).           */
int lio_abi_struct_sizes(int64_t* out, int n);

/* -------------------------------------------------------------------- map
 * Replaces `KD_TREE<PointType> ikdtree` [U: ikd-Tree ikd_Tree.h]: a dense
 * uniform grid in HBM (points float4 sorted by cell, u32 cell offsets).
 * kNN results are exact; point ids are insertion order (0..size-1).       */
typedef struct lio_map lio_map;

typedef struct lio_map_params {
    float cell_size;        /* grid cell edge [m]; 0 => 1.0                          */
    float downsample_size;  /* filter_size_map (kitti.launch:10) for lio_map_add    */
    int device;             /* HIP device ordinal                                   */
    int reserved;
} lio_map_params;

int lio_map_create(const lio_map_params* p, lio_map** out);
/* Refuses (LIO_ERR_STATE) while lio_ctx handles created on m are alive.    */
int lio_map_destroy(lio_map* m);
/* ikdtree.set_downsample_param(filter_size_map_min) [U: laserMapping.cpp
 * main(), before Build]: changes cell_size / downsample_size in place (a
 * value <= 0 keeps the current one); only while the map holds no points, so
 * every lio_ctx already created on m stays valid.  device must not change. */
int lio_map_set_params(lio_map* m, const lio_map_params* p);
/* ikdtree.Build(points) [U]: replaces the content. xyz: n*3 float, host.
 * A row with a NaN or infinite coordinate keeps its id but is stored as a
 * deleted one: it is no part of the grid and nobody's neighbour.           */
int lio_map_build(lio_map* m, const float* xyz, int64_t n);
/* same, xyz already resident in device memory (e.g. a torch tensor).       */
int lio_map_build_device(lio_map* m, const float* d_xyz, int64_t n);
/* ikdtree.size() [U]: alive points                                        */
int64_t lio_map_size(const lio_map* m);
/* ids ever inserted (alive + deleted); kNN ids index this space            */
int64_t lio_map_num_ids(const lio_map* m);
/* copies the alive map points (id order) to host, lio_map_size()*3 float   */
int lio_map_get_points(lio_map* m, float* xyz_out);
/* every id: xyz (num_ids*3, may be NULL) and alive flags (num_ids, may be NULL) */
int lio_map_get_by_id(lio_map* m, float* xyz_out, uint8_t* alive_out);
/* ikd-Tree Nearest_Search(point, k, Nearest_Points, Point_Distance, max_dist)
 * [U: ikd-Tree ikd_Tree.h; FAST-LIO laserMapping.cpp h_share_model calls it
 * with k = NUM_MATCH_POINTS = 5, max_dist = INFINITY] for a batch of n query
 * points q (n*3 float): the k <= 5 nearest alive map points in ascending
 * (sq-distance, id) order with sq-distance <= max_dist^2 (max_dist <= 0 or
 * INFINITY: unbounded).  idx (n*k, map ids = insertion order, -1 where fewer
 * exist), d2 (n*k, optional, INFINITY where missing).  A query that is not
 * finite has no neighbours.                                                 */
int lio_map_nearest_search(lio_map* m, const float* q, int64_t n, int k, float max_dist, int32_t* idx, float* d2);
/* Coordinates of map ids (Nearest_Points from lio_map_nearest_search /
 * lio_get_knn ids): xyz_out n*3; ids < 0 or unknown give NaN.             */
int lio_map_gather(lio_map* m, const int32_t* ids, int64_t n, float* xyz_out);

/* ---- incremental maintenance ----
 * ikdtree.Add_Points(PointToAdd, downsample_on) [U]: with downsample, per
 * point (in order) the filter_size_map voxel [floor(p/ds)*ds, +ds) keeps only
 * the point nearest its centre (Search_by_range + Delete_by_range +
 * Add_by_point).  n_added (may be NULL): the reference's return value (the
 * number of Add_by_point calls; n for downsample = 0).                      */
int lio_map_add(lio_map* m, const float* xyz, int64_t n, int downsample, int64_t* n_added);
int lio_map_add_device(lio_map* m, const float* d_xyz, int64_t n, int downsample, int64_t* n_added);
/* ikdtree.Delete_Point_Boxes(cub_needrm) [U]: boxes nb x 6 floats
 * (min x y z, max x y z), a point is inside when min <= p < max.           */
int lio_map_delete_boxes(lio_map* m, const float* boxes, int nb, int64_t* n_deleted);

/* lasermap_fov_segment() [U] (FAST-LIO laserMapping.cpp): host helper that
 * keeps the local map cube around the LiDAR and returns the boxes to delete
 * (pass them to lio_map_delete_boxes).  pos_lid = pos + rot * offset_T_L_I.  */
typedef struct lio_localmap {
    float vertex_min[3], vertex_max[3];
    int initialized;
} lio_localmap;
int lio_localmap_update(lio_localmap* lm, const double pos_lid[3], double cube_len, float det_range,
                        float mov_threshold, float boxes_out[18], int* n_boxes);
/* grid geometry: origin[3], cell, dims[3] (as doubles)                     */
int lio_map_get_grid(lio_map* m, double* out7);
/* diagnostics: out8 = [full grid rebuilds so far, slot pool capacity, slots handed out (device bump),
 * alive points, ids, grid cells, flags of the last update (1 outside the grid, 2 pool exhausted,
 * 4 tombstone cell list full: each forces a rebuild), reserved]                                  */
int lio_map_get_stats(lio_map* m, int64_t* out8);
/* Test hook: cap the slot pool at (slots in use after the last rebuild + slot_headroom) and the per-update
 * list of cells holding tombstones at dirty_cells (0: no cap), so that the pool-exhausted (flag 2) and
 * list-full (flag 4) recovery paths run on small maps.                                          */
int lio_map_set_test_limits(lio_map* m, int64_t slot_headroom, int64_t dirty_cells);

/* ------------------------------------------------------------ h-model ctx */
typedef struct lio_ctx lio_ctx;

typedef struct lio_match_params {
    float knn_range_sq; /* 5.0: gate `sqdist[4] > 5` rejects; bounded-search radius^2 */
    float plane_thr;    /* 0.1f: esti_plane(pabcd, points_near, 0.1f)                  */
    double s_coef;      /* 0.9: s = 1 - 0.9*|pd2|/sqrt(|p_body|)                        */
    double s_gate;      /* 0.9: keep if s > 0.9                                         */
} lio_match_params;

/* The parts of state_ikfom the measurement model reads:
 *   p_world = rot * (offset_R_L_I * p_body + t_LI) + t.
 * q / q_LI are state_ikfom's rot / offset_R_L_I (MTK::SO3 = Eigen::Quaternion
 * <double>, stored (w, x, y, z)); the kernels evaluate every `SO3 * v` from
 * them exactly as Eigen's QuaternionBase::_transformVector does.  R / R_LI are
 * the same rotations as row-major matrices.  A caller holding only matrices
 * leaves q (q_LI) all zero: it is then derived from R (R_LI) with Eigen's
 * Matrix3 -> Quaternion conversion.  A non-zero q takes precedence: R / R_LI
 * are then not read by any computation (so a stale R cannot disagree with
 * the kernels' rotation).                                                   */
typedef struct lio_pose {
    double R[9];
    double t[3];
    double R_LI[9];
    double t_LI[3];
    double q[4];
    double q_LI[4];
} lio_pose;

int lio_ctx_create(lio_map* m, const lio_match_params* p, lio_ctx** out);
int lio_ctx_destroy(lio_ctx* c);
/* feats_down_body (n*3 float, LiDAR frame), host / device pointer.         */
int lio_scan_set(lio_ctx* c, const float* body_xyz, int64_t n);
int lio_scan_set_device(lio_ctx* c, const float* d_body_xyz, int64_t n);
/* same without a copy: the ctx reads the caller's device buffer, which must stay valid and
 * unchanged until the next lio_scan_* call on this ctx.                                       */
int lio_scan_bind_device(lio_ctx* c, const float* d_body, int64_t n);
/* One h_share_model evaluation [U]. redo_knn = ekfom_data.converge.
 * sums: LIO_SUMS_LEN doubles (see layout above).                           */
int lio_match(lio_ctx* c, const lio_pose* pose, int redo_knn, double* sums);
/* Debug getters (not on the timed path):
 *   Nearest_Points ids + sq-distances (n*5, -1 / +inf where fewer than 5),
 *   normvec (a,b,c,pd2 for selected points) + point_selected_surf,
 *   feats_down_world for the pose of the last lio_match.                    */
int lio_get_knn(lio_ctx* c, int32_t* idx, float* d2);
int lio_get_planes(lio_ctx* c, float* abcd_pd2, uint8_t* sel);
int lio_get_world(lio_ctx* c, float* world);
/* ekfom_data.h_x rows (6 non-zero columns) + h of the selected points, in
 * point order, for the dof < 23 branch of the IESKF: rows = 7 doubles each. */
int lio_get_h_rows(lio_ctx* c, double* rows, int64_t max_rows, int64_t* n_rows);
/* Diagnostics: one kNN evaluation (same results as lio_match(redo_knn=1))
 * that also reports, per point, {cells scanned, map points scanned, last
 * shell visited} (stats3: n*3 int32).                                     */
int lio_ctx_knn_stats(lio_ctx* c, const lio_pose* pose, double* sums, int32_t* stats3);

/* ------------------------------------------------------------------ IESKF */
typedef struct lio_state { /* state_ikfom [U], quaternions are (w, x, y, z) */
    double pos[3];
    double rot[4];
    double offset_R_L_I[4];
    double offset_T_L_I[3];
    double vel[3];
    double bg[3];
    double ba[3];
    double grav[3];
} lio_state;

typedef struct lio_ieskf_params {
    double laser_point_cov; /* LASER_POINT_COV = 0.001 [U]                  */
    int max_iteration;      /* NUM_MAX_ITERATIONS = max_iteration = 3 (kitti.launch:8) */
    double epsi;            /* convergence limit per state dim = 0.001 [U]  */
} lio_ieskf_params;

typedef struct lio_ieskf_stats {
    int h_evals;    /* h_share_model calls                               */
    int knn_calls;  /* of which redid the kNN (ekfom_data.converge)      */
    int converged;  /* exited through t > 1 (1) or the iteration cap (0) */
    int n_eff;      /* effct_feat_num of the last evaluation             */
    double res_mean;/* res_mean_last                                     */
    double solve_ms;/* host time in the 23-dim algebra                   */
    double wall_ms; /* host wall time of the whole call                  */
    double launch_ms;/* host time enqueueing the evaluations' kernels     */
    double wait_ms; /* host time waiting for the evaluations' results    */
} lio_ieskf_stats;

/* esekf::update_iterated_dyn_share_modified(R, solve_time) [U IKFoM];
 * x and P (23x23 row-major) are updated in place.  Default: the host loop
 * (one h-evaluation launch + one zero-copy result per iteration, 23-dim
 * algebra on the host).                                                     */
int lio_ieskf_update(lio_ctx* c, lio_state* x, double* P, const lio_ieskf_params* p, lio_ieskf_stats* st);
/* Test hook: the seeded kNN pass's bound (later kNN evaluations of a scan) is
 * multiplied by scale in (0, 1]; < 1 shrinks it below the true 5th distance so
 * the not-full guard (whole-box far search) is exercised.  Default 1.        */
int lio_ctx_set_seed_scale(lio_ctx* c, float scale);

/* ---------------------------------------------------------------- loop ICP */
typedef struct lio_icp lio_icp;

typedef struct lio_icp_params {
    double max_corr_dist;   /* icp_max_corr_dist_ = 1.5 * loop_detection_radius (fast_lio_sam.cpp:73) */
    double trans_eps;       /* setTransformationEpsilon(0.01)   loop_closure.cpp:8  */
    double fitness_eps;     /* setEuclideanFitnessEpsilon(0.01) loop_closure.cpp:9  */
    int max_iter;           /* setMaximumIterations(50)         loop_closure.cpp:10 */
    double rot_eps;         /* 0 => PCL default 1 - trans_eps                        */
    double score_threshold; /* icp_score_threshold (config.yaml:16)                   */
    float cell_size;        /* target grid cell [m]; 0 => 1.0                        */
    int device;
    /* How TransformationEstimationSVD's Umeyama step is evaluated (LIO_ICP_UMEYAMA_*).
     * 0 (LIO_ICP_UMEYAMA_DEFAULT, a zero-initialised struct) = 2: the reference's arithmetic.
     * 1..3: PCL float modes — TransformationEstimationSVD<PointXYZI, PointXYZI, float>'s pcl::umeyama
     *    (loop_closure.h:42, aligned at loop_closure.cpp:81) restated in float with the float summation
     *    order of a given PCL/Eigen build (parity with a real PCL build unpinned: no PCL here):
     *    1 sequential-order restatement: means and sigma's depth as single sequential chains;
     *    2 Eigen 3.3 model (32 KiB L1): sequential means, sigma by Eigen's GEMM — depth blocked by
     *      kc = 680, res += alpha * block sum — THE DEFAULT;
     *    3 as 2 with a 48 KiB L1 (kc = 1016).
     *    The sequential float chains are evaluated in parallel and verified bit-exact on the GPU
     *    (lio_seqsum: predicted binades, event replay, full verification; serial kernel fallback);
     *    float JacobiSVD on the host.  Sharded (world > 1): every rank's accepted correspondence ids
     *    ride the records' all-gather and every rank evaluates the float chains over the whole
     *    source, so the transform is the one-rank transform bit for bit.
     * -1 (LIO_ICP_UMEYAMA_DOUBLE, opt-in): the statistics in double about a fixed centre — faster, but
     *    1.2-1.9e-4 from PCL's float arithmetic at C4 (outside the 1e-5 parity bar).      */
    int umeyama_float;
} lio_icp_params;
#define LIO_ICP_UMEYAMA_DEFAULT 0
#define LIO_ICP_UMEYAMA_PCL_SEQ 1
#define LIO_ICP_UMEYAMA_PCL_GEMM32 2
#define LIO_ICP_UMEYAMA_PCL_GEMM48 3
#define LIO_ICP_UMEYAMA_DOUBLE (-1)

typedef struct lio_icp_result {  /* RegistrationOutput (loop_closure.h:21-27) + diagnostics */
    int is_valid;
    int is_converged;
    double score;          /* getFitnessScore()                         */
    float T[16];           /* getFinalTransformation(), row-major        */
    int iterations;
    int state;             /* convergence state: 0 none, 1 iter, 2 transform, 3 abs mse, 4 rel mse, 5 no corr */
    double last_mse;
    int64_t last_corr;
} lio_icp_result;

/* Exchange hook for sharded ICP (one process per GPU): all-gather `n` doubles
 * from every rank into recv (world*n, rank order).  NULL => single rank.   */
typedef int (*lio_allgather_fn)(const double* send, int64_t n, double* recv, void* user);

int lio_icp_create(const lio_icp_params* p, lio_icp** out);
int lio_icp_destroy(lio_icp* h);
int lio_icp_set_target(lio_icp* h, const float* xyz, int64_t n);         /* setInputTarget */
int lio_icp_set_source(lio_icp* h, const float* xyz, int64_t n);         /* setInputSource */
/* Shard the source's fixed 4096-point blocks over `world` ranks.          */
int lio_icp_set_shard(lio_icp* h, int rank, int world, lio_allgather_fn fn, void* user);
/* Host-only helpers of the sharded path (no device needed): the contiguous
 * source range a rank owns (whole 4096-point records), and the rank-order
 * combination of all-gathered records into the 17 Umeyama statistics
 * [n, sum p(3), sum q(3), sum q p^T(9), sum d2].  recv = world slots of
 * ceil(records/world)*20 doubles, as lio_allgather_fn delivers them.       */
int lio_icp_shard_range(int64_t n_source, int rank, int world, int64_t* begin, int64_t* count);
int lio_icp_combine(const double* recv, int64_t n_source, int world, double* out17);
/* Host mirrors of the sharded float chains' exchange (no device; the kernels run the same code):
 * lio_seq_shard_offsets — every rank's block-sum message (rank r at recv + r * stride: [0] the window's
 * element count, then per chain c at 8 + 2 c nb_slot its 1024-element blocks' (double sum, sum |x|)) -> rank
 * `rank`'s starting prefix, drift variance and the common floor of chains 0 .. nch-1, its first global index
 * and the total (gbase_nglobal[2]); lio_seq_shard_merge — every rank's event message (header: [0] n, [1] overflow bits,
 * [2 + c] increment total, [11 + c] event count, [20 + c] first element; at 32 + 2 slot c the events:
 * increment prefix bits, then position | value bits << 32) -> chain `chain`'s global lists (pos, P, x) and
 * nev_ptot_bad = {events, longest list, problems (1 own overflow, 2 over the slot, 4 over evs)}.          */
int lio_seq_shard_offsets(const double* recv, int64_t stride, int64_t nb_slot, int rank, int world, int nch,
                          double* off0, double* var0, int32_t* floor_e, int64_t* gbase_nglobal);
int lio_seq_shard_merge(const double* recv, int64_t stride, int world, int slot, int chain, int64_t evs,
                        int32_t* pos, uint64_t* P, float* x, int32_t* nev_ptot_bad, uint64_t* ptot, float* x0);
/* Host half of the float fidelity modes (no device needed): sums16 = the float sums the GPU
 * returns per pass [sum src xyz(3), sum tgt xyz(3), count (uint32 bits), sigma accumulator (9,
 * row-major target x source): unscaled for order 1] -> the incremental transform (row-major 4x4
 * float) through the float JacobiSVD (pcl::umeyama(src, dst, false) [U], Eigen 3.3 Umeyama.h).  */
int lio_icp_umeyama_pcl_float(const float* sums16, float* T16);
/* As above for summation order `order` (lio_icp_params.umeyama_float 1..3: orders 2 / 3 return sigma
 * already scaled by 1/n, as Eigen's GEMM leaves it).                                            */
int lio_icp_umeyama_pcl_float_order(const float* sums16, int order, float* T16);
/* Diagnostics of the float fidelity modes: out4 = [verification re-passes, serial fallbacks, events of
 * the last pass (max over chains), passes run] since the handle was created.  Test hook: flags bit 0
 * makes the first seqsum pass skip its grid-coarsening event rule (verification then fails and the
 * re-pass path runs); flags & 4 reports a compaction look-back time-out on every pass (the pass then
 * re-compacts on the serial kernels and clears the flag); evcap > 0 caps the events per chain
 * (overflow -> the serial fallback).                                                              */
int lio_icp_get_fidelity_stats(lio_icp* h, int64_t* out4);
/* Test hook: the 16 floats of the last alignment's last correspondence pass (not the getFitnessScore pass),
 * exactly as handed to the host Umeyama — the sums16 of lio_icp_umeyama_pcl_float_order; also valid when
 * that pass ended with fewer than 3 pairs (state 5).  Sharded, every rank reports its own copy.
 * LIO_ERR_STATE with the double statistics or before any pass has run.                            */
int lio_icp_get_umeyama_stats(lio_icp* h, float* out16);
int lio_icp_set_fidelity_debug(lio_icp* h, int flags, int64_t evcap);
/* Test hook: sequential float sums of 6 interleaved chains (x: n x 6 host floats) on `device` through
 * the seqsum path — sums6[c] = fl(...fl(x[0][c] + x[1][c]) ... + x[n-1][c]); passes_out = passes used
 * (-1: the serial kernel was needed).                                                             */
int lio_seqsum6(int device, const float* x, int64_t n, int flags, float* sums6, int* passes_out);
/* Device-side exchange (the form to use with RCCL): per pass the statistics kernel writes this rank's
 * records into a DEVICE send buffer, `fn` enqueues the all-gather of n doubles per rank into the
 * device recv buffer (world * n, rank order) ordered on `stream` (RCCL in-stream, or a collective on
 * torch.cuda.ExternalStream(stream)), the handle enqueues the record-order sum behind it and reads 17
 * doubles back: one host wait per pass, no host copies of the records.  Buffers: the handle's own,
 * or the caller's (lio_icp_set_exchange_buffers, e.g. tensors a collective library registered);
 * capacity lio_icp_exchange_len(n_source, world) doubles per rank.  The n of a call may be less than
 * the capacity and differs between the calls of a pass, the same on every rank: the records (double
 * statistics, fitness passes); in the PCL float modes (the default) three all-gathers per pass — the
 * records followed by the window's chain totals, the window's float-chain event lists (and its first
 * pairs), the window's GEMM depth blocks (lio_icp_stats.cpp, lio_seqsum.hpp); recv holds rank r at r * n. */
typedef int (*lio_allgather_dev_fn)(const double* d_send, int64_t n, double* d_recv, void* stream, void* user);
int lio_icp_set_shard_device(lio_icp* h, int rank, int world, lio_allgather_dev_fn fn, void* user);
int lio_icp_exchange_len(int64_t n_source, int world, int64_t* n_per_rank);
int lio_icp_set_exchange_buffers(lio_icp* h, double* d_send, double* d_recv, int64_t n_per_rank);
/* Multi-process exchanges in C++ (no callback into the caller per pass; lio_icp_mp.cpp):
 *  RCCL: rank 0 calls lio_rccl_unique_id, the caller broadcasts the 128 bytes to every rank ONCE (e.g. over
 *  torch.distributed), then every rank calls lio_icp_set_shard_rccl (collective: ncclCommInitRank on the
 *  handle's device); per pass ncclAllGather is enqueued on the handle's stream and the records are summed in
 *  record order behind it.  The communicator is owned by the handle.                                       */
int lio_rccl_unique_id(uint8_t* id128);
int lio_icp_set_shard_rccl(lio_icp* h, int rank, int world, const uint8_t* id128);
/*  Shared memory (ranks on one node without RCCL, e.g. several ranks on one GPU): `name` = a POSIX shm name
 *  ("/..."), rank 0 opens first (the caller orders it, e.g. a barrier), max_source_points sizes the segment.
 *  The bare primitive (host only, no device): lio_shm_exchange_* — n doubles from every rank, rank order.  */
int lio_icp_set_shard_shm(lio_icp* h, int rank, int world, const char* name, int64_t max_source_points);
int lio_shm_exchange_open(const char* name, int rank, int world, int64_t n_per_rank, void** out);
int lio_shm_exchange_allgather(void* ex, const double* send, int64_t n, double* recv);
int lio_shm_exchange_close(void* ex);
/* barrier timeout of an exchange (default 60 s; tests shorten it).  A timed-out barrier POISONS the
 * segment: every later all-gather on it, on every rank, fails (the arrival count is no longer exact).   */
int lio_shm_exchange_set_timeout(void* ex, double seconds);
/* align(guess) + getFitnessScore() + is_valid decision (loop_closure.cpp:81-90).
 * aligned_opt (n*3, this rank's shard only when sharded) may be NULL.      */
int lio_icp_align(lio_icp* h, const float* guess16, lio_icp_result* out, float* aligned_opt);
/* Diagnostics: the 1-NN of the last pass (after lio_icp_align: the
 * getFitnessScore pass) per source point of this rank's shard: target index
 * (input order of lio_icp_set_target) and float squared distance.          */
int lio_icp_get_correspondences(lio_icp* h, int32_t* ids, float* d2);
/* Single-process multi-GPU loop ICP for a C++ host: one
 * lio_icp per device (devices NULL => 0 .. n_gpus-1), the source sharded in
 * 4096-point records, the target replicated; per iteration the ranks' records
 * are all-gathered over RCCL (ncclCommInitAll + ncclAllGather; librccl is
 * opened at creation) and summed in record order, so the transform is
 * bit-identical to one GPU.  LIO_ICP_EXCHANGE=host (or the same device listed
 * twice) swaps the records through host memory instead.  A failed rank aborts
 * the group (recreate it).  Replaces LoopClosure's ICP instance
 * (loop_closure.cpp:3-14) when several GPUs serve the loop-closure thread.  */
typedef struct lio_icp_group lio_icp_group;
int lio_icp_group_create(const lio_icp_params* p, int n_gpus, const int* devices, lio_icp_group** out);
int lio_icp_group_destroy(lio_icp_group* g);
int lio_icp_group_size(const lio_icp_group* g);
int lio_icp_group_uses_rccl(const lio_icp_group* g);
int lio_icp_group_set_target(lio_icp_group* g, const float* xyz, int64_t n);
int lio_icp_group_set_source(lio_icp_group* g, const float* xyz, int64_t n);
/* as lio_icp_align; aligned_opt is the whole n*3 cloud (each rank fills its shard) */
int lio_icp_group_align(lio_icp_group* g, const float* guess16, lio_icp_result* out, float* aligned_opt);
/* One-shot form (SURVEY §8(b) signature): n_gpus <= 1 runs on p->device, n_gpus > 1 on devices
 * p->device .. p->device + n_gpus - 1 through lio_icp_group.                                     */
int icp_align(const float* src_xyz, int64_t ns, const float* dst_xyz, int64_t nd, const lio_icp_params* p,
              int n_gpus, float* T_out, double* fitness, int* converged, int* iters, float* aligned_xyz_opt);

/* FAST-LIO map_incremental() [U] for the ctx's current scan: world points
 * with the final pose, Nearest_Points from the ctx's last kNN evaluation
 * (lio_match / lio_ieskf_update with redo), PointToAdd / PointNoNeedDownsample
 * classification on filter_size_map (double, as laserMapping), then
 * Add_Points(PointToAdd, true) and Add_Points(PointNoNeedDownsample, false)
 * on the ctx's map.  Invalidates the ctx's kNN lists.                      */
typedef struct lio_incremental_stats {
    int64_t n_to_add;           /* PointToAdd.size()                          */
    int64_t n_no_downsample;    /* PointNoNeedDownsample.size()               */
    int64_t n_skipped;          /* points not added                           */
    int64_t n_added_downsample; /* Add_Points(PointToAdd, true) return value  */
} lio_incremental_stats;
int lio_map_incremental(lio_ctx* c, const lio_pose* pose, double filter_size_map, lio_incremental_stats* st);
/* pose of the ctx's last kNN evaluation (the pose Nearest_Points belong to) */
int lio_ctx_get_knn_pose(lio_ctx* c, lio_pose* out);

/* ------------------------------------------ filters */
typedef struct lio_filter lio_filter;
int lio_filter_create(int device, lio_filter** out);
int lio_filter_destroy(lio_filter* f);

/* pcl::VoxelGrid<PointT>::filter, PCL 1.10 applyFilter [U] (FAST-LIO downSizeFilterSurf,
 * voxelizePcd utilities.hpp:161-183): pts is n x stride floats (x, y, z first; stride 3..8);
 * every field is averaged per voxel (downsample_all_data_ = true), summed in input order inside
 * a voxel (PCL's std::sort order there is unspecified); output in voxel-index order (out capacity
 * n x stride); non-finite points are dropped; index overflow returns the input unchanged (as PCL). */
int lio_voxel_grid(lio_filter* f, const float* pts, int64_t n, int stride, const float leaf[3], float* out,
                   int64_t* n_out);

/* One side of LoopClosure::setSrcAndDstCloud (loop_closure.cpp:42-67): the nk keyframe clouds
 * (segments [seg_off[k], seg_off[k+1]) of pts) each through transformPcd(cloud, pose_k)
 * (utilities.hpp:132-143: pcl::transformPointCloud with a double 4x4, row-major poses16[16k..]),
 * concatenated in order, then voxelizePcd(voxel_res). */
int lio_submap_voxelize(lio_filter* f, const float* pts, const int64_t* seg_off, int nk, int stride,
                        const double* poses16, float voxel_res, float* out, int64_t* n_out);

/* FAST-LIO front-end preprocessing of one raw scan [U]: Preprocess selection (every
 * point_filter_num-th point with |p| > blind), ImuProcess::UndistortPcl (sort by the per-point
 * time offset in ms, field time_field; backward propagation through the IMU poses of the scan
 * to the scan-end state `end`), then downSizeFilterSurf (VoxelGrid, filter_size_surf; 0 = off). */
typedef struct lio_imu_pose {  /* set_pose6d: offset from scan start [s], acc, gyr, vel, pos, rot */
    double offset_time;
    double acc[3], gyr[3], vel[3], pos[3];
    double rot[9];
} lio_imu_pose;
typedef struct lio_scan_prep_params {
    int point_filter_num;   /* kitti.launch:6 = 4 */
    float blind;            /* kitti.yaml:13 = 2 */
    float filter_size_surf; /* kitti.launch:9 = 0.5 */
    int time_field;         /* index of the time offset [ms] in a record (FAST-LIO's curvature) */
} lio_scan_prep_params;
/* to host memory: out capacity n x stride, *n_out records (x, y, z, ... averaged)            */
int lio_preprocess(lio_filter* f, const float* raw, int64_t n, int stride, const lio_scan_prep_params* p,
                   const lio_imu_pose* poses, int n_poses, const lio_pose* end, float* out, int64_t* n_out);
/* straight into the ctx's scan (feats_down_body) without a host round trip; *n_down points */
int lio_scan_preprocess(lio_ctx* c, const float* raw, int64_t n, int stride, const lio_scan_prep_params* p,
                        const lio_imu_pose* poses, int n_poses, const lio_pose* end, int64_t* n_down);

/* feats_undistort of the ctx's last lio_scan_preprocess*: the undistorted, time-sorted records
 * before downSizeFilterSurf — what FAST-LIO publishes on /cloud_registered with dense_publish_en
 * (kitti.yaml:31), transformed to the world frame, and what fast_lio_sam keeps per keyframe
 * (pose_pcd.hpp:37-39).  *n_points (and *stride) always set; out (cap_points records) optional.    */
int lio_scan_get_undistorted(lio_ctx* c, float* out, int64_t cap_points, int64_t* n_points, int* stride);
/* The keyframe cloud fast_lio_sam builds from FAST-LIO's /cloud_registered, on the device: out (n x 4:
 * x, y, z, intensity) = T16 * pointBodyToWorld(pose, feats_undistort), T16 row-major double — pass
 * pose_eig_.inverse() for PosePcd::pcd_ (pose_pcd.hpp:22-42; utilities.hpp:132-143 transformPcd order).
 * out = NULL: count only.                                                                          */
int lio_scan_keyframe_cloud(lio_ctx* c, const lio_pose* pose, const double* T16, float* out, int64_t cap_points,
                            int64_t* n_points);

/* ---------------------------------- outlier removal and the intensity map denoise
 * The back end's denoise (fast_lio_sam.cpp:262-365, 575-680, 941-1008; config.yaml:32-42) and its parts.
 * Squared distances are float ((dx*dx + dy*dy) + dz*dz) everywhere; non-finite points are nobody's neighbour. */

/* pcl::StatisticalOutlierRemoval<PointT>::applyFilter, PCL 1.10 [U]: pts is n x stride floats (x, y, z first;
 * stride 3..8), mean_k 1..255.  Per finite point the mean distance to its mean_k nearest neighbours (the
 * mean_k + 1 smallest squared distances, itself included, the first dropped; double square roots added in
 * ascending order); non-finite points, and every point when fewer than mean_k + 1 finite points exist, get
 * distance 0 and are not counted.  mean / stddev over the counted points in PCL's double loop, threshold =
 * mean + stddev_mul * stddev; a point is removed when its distance is > threshold (negative: when <=), so a
 * NaN threshold (no counted point) keeps every point.  out: the kept records in input order (capacity
 * n x stride).  distances_opt (n, may be NULL); stats4_opt (may be NULL) = mean, stddev, threshold, counted. */
int lio_sor_filter(lio_filter* f, const float* pts, int64_t n, int stride, int mean_k, double stddev_mul, int negative,
                   float* out, int64_t* n_out, float* distances_opt, double* stats4_opt);

/* KdTreeFLANN::radiusSearch per seed [U], turned round: per cloud point (n x stride records) the lowest index s
 * of the ns seeds (ns x 3 floats) with squared distance < r2, r2 = (float)((double)radius * radius), strict
 * (-1: none), and that squared distance (d2_out_opt, may be NULL; 0 where none).  Non-finite points and
 * seeds never match.                                                                                       */
int lio_radius_first_seed(lio_filter* f, const float* pts, int64_t n, int stride, const float* seeds_xyz, int64_t ns,
                          float radius, int32_t* seed_out, float* d2_out_opt);

typedef struct lio_denoise_params { /* /denoise/... (fast_lio_sam.cpp:89-96, config.yaml:32-42) */
    float seed_thres;          /* 2800 */
    float cluster_seed_radius; /* 0.1 (config.yaml), 1.0 (source default) */
    float denoise_radius;      /* 0.5 */
    float noise_thres;         /* 2700 */
    int mean_k;                /* sor/MeanK: 200 (config.yaml), 50 (source default) */
    float stddev_mul;          /* sor/StddevMulThresh: 0.2 (config.yaml), 1.0 (source default) */
} lio_denoise_params;

/* FastLioSam::denoise_slam_map (fast_lio_sam.cpp:941-1008 with denoise_map :575-646 and
 * clustering_and_denoise :332-365) on PointXYZI records (n x 4: x, y, z, intensity):
 *   seeds     = points with intensity > seed_thres, in input order;
 *   segmented = points with intensity != 0 that have a seed within cluster_seed_radius, ordered by the
 *               claiming (lowest) seed index, then ascending squared distance to that seed, THEN POINT INDEX
 *               (the reference leaves equal distances to FLANN's order; the index tie-break is this
 *               library's contract);
 *   remained  = points with intensity != 0 that are not segmented, in input order (points whose input
 *               intensity is exactly 0 disappear, as in the reference);
 *   denoised  = SOR(mean_k, stddev_mul) of segmented, order kept, then without every point of intensity
 *               < noise_thres that has a seed within denoise_radius;
 *   out       = denoised followed by remained (capacity n x 4).
 * counts5_opt (may be NULL) = seeds, segmented, after SOR, denoised, remained.                             */
int lio_denoise_slam_map(lio_filter* f, const float* pts, int64_t n, const lio_denoise_params* p, float* out,
                         int64_t* n_out, int64_t* counts5_opt);

/* pcl::EuclideanClusterExtraction<PointT>::extract, PCL 1.10 [U] (clustering_and_denoise,
 * fast_lio_sam.cpp:343-363: tolerance 0.5, min 10, max 25000), with the axis-aligned bounding box per cluster
 * of the offline pipeline (post_process/clustering.py:39-75), restated as sets.  pts is n x stride floats
 * (x, y, z first; stride 3..8), n < 2^31.
 *   edge      two finite points i != j are joined when float ((dx*dx + dy*dy) + dz*dz) < r2,
 *             r2 = (float)((double)tolerance * tolerance), strict (lio_radius_first_seed's rule);
 *   cluster   a connected component of that graph (PCL's seed loop in index order with `processed` flags
 *             reaches the whole component of every unprocessed seed; the points of a size-rejected
 *             component stay processed, and max_size does not stop the growth, it only rejects);
 *   accepted  min_size <= size <= max_size (min_size > max_size is legal: no cluster);
 *   order     point indices ascend inside a cluster; clusters by size descending, THEN LOWEST MEMBER INDEX
 *             ASCENDING (PCL's final sort leaves equal sizes unspecified; the index tie-break is this
 *             library's contract);
 *   non-finite points are in no cluster and nobody's neighbour.
 * labels_out (n): the rank of the point's cluster in that order, -1 for non-finite points and for points of
 * rejected components.  *n_clusters: accepted clusters.  indices_opt (n, may be NULL): all accepted points in
 * cluster order.  offsets_opt (cap_clusters + 1, may be NULL) and aabb6_opt (6 x cap_clusters, may be NULL:
 * float min x, y, z, max x, y, z over the members) are filled for the first min(*n_clusters, cap_clusters)
 * clusters (offsets: one entry more, the end of the last of them); cap_clusters = 0 with NULLs is the
 * "count only" call.  stats4_opt (may be NULL) = finite points, components, accepted clusters, points in them.
 * LIO_ERR_ARG before any device work: tolerance non-finite or <= 0, min_size < 1, stride outside 3..8, n < 0
 * or n >= 2^31, cap_clusters < 0, NULL n_clusters, NULL pts or labels_out with n > 0.                          */
int lio_euclidean_clusters(lio_filter* f, const float* pts, int64_t n, int stride, float tolerance, int64_t min_size,
                           int64_t max_size, int32_t* labels_out, int64_t* n_clusters, int64_t cap_clusters,
                           int64_t* offsets_opt, int32_t* indices_opt, float* aabb6_opt, int64_t* stats4_opt);

/* DBSCAN with one core flag per point and one axis-aligned bounding box per cluster: the second clustering
 * method of the offline pipeline (post_process/clustering.py:30-36, cluster_with_dbscan: eps 0.5, min_samples
 * 10), scikit-learn's DBSCAN [U] restated as sets.  pts is n x stride floats (x, y, z first; stride 3..8),
 * 0 <= n < 2^31; eps finite and > 0; min_samples >= 1.  No float contraction, as everywhere in the library.
 *   neighbour finite points i and j (j = i included) are neighbours when float ((dx*dx + dy*dy) + dz*dz) <= e2,
 *             e2 = (float)((double)eps * eps).  THE TEST IS INCLUSIVE: a pair at exactly eps is a pair of
 *             neighbours (DBSCAN's definition and scikit-learn's radius_neighbors), unlike the strict < of
 *             lio_euclidean_clusters and lio_radius_first_seed, which follow PCL;
 *   core      a finite point is core when it has >= min_samples neighbours, itself counted;
 *   cluster   a connected component of the neighbour graph restricted to core points.  CLUSTERS ARE NUMBERED BY
 *             THEIR LOWEST CORE INDEX, ASCENDING (scikit-learn opens clusters in index order at unlabelled core
 *             points and expands each fully; stated here as this library's contract);
 *   border    a finite non-core point with at least one core neighbour takes THE LOWEST-NUMBERED CLUSTER AMONG
 *             ITS CORE NEIGHBOURS' CLUSTERS (the cluster that reaches it first; this library's contract) and
 *             spreads the cluster no further;
 *   noise     every other finite point and every non-finite point: label -1.  A non-finite point is nobody's
 *             neighbour.  There is no size filter.
 * labels_out (n): the number of the point's cluster, -1 for noise.  core_opt (n, may be NULL): 1 for a core
 * point, else 0.  *n_clusters: the clusters.  indices_opt (n, may be NULL): all clustered points in cluster
 * order, indices ascending inside a cluster.  offsets_opt (cap_clusters + 1, may be NULL) and aabb6_opt
 * (6 x cap_clusters, may be NULL: float min x, y, z, max x, y, z over all members, border points included) are
 * filled for the first min(*n_clusters, cap_clusters) clusters (offsets: one entry more, the end of the last of
 * them); cap_clusters = 0 with NULLs is the "count only" call.  stats4_opt (may be NULL) = finite points, core
 * points, clusters, clustered points; the noise among the finite points is [0] - [3].
 * LIO_ERR_ARG before any device work: eps non-finite or <= 0, min_samples < 1, stride outside 3..8, n < 0 or
 * n >= 2^31, cap_clusters < 0, NULL n_clusters, NULL pts or labels_out with n > 0.  Repeated calls and any
 * scheduling of the device give identical results.                                                          */
int lio_dbscan(lio_filter* f, const float* pts, int64_t n, int stride, float eps, int64_t min_samples,
               int32_t* labels_out, uint8_t* core_opt, int64_t* n_clusters, int64_t cap_clusters,
               int64_t* offsets_opt, int32_t* indices_opt, float* aabb6_opt, int64_t* stats4_opt);

/* RANSAC plane segmentation: Open3D's PointCloud::SegmentPlane [U] as the offline pipeline calls it for ground
 * removal (post_process/clustering.py:21-28: distance_threshold 0.2, ransac_n 3, num_iterations 1000), restated
 * as a contract of this library (Open3D's std::mt19937 sampling and the float sum behind its RMSE tie-break
 * cannot be reproduced bit for bit).  pts is n x stride floats (x, y, z first; stride 3..8), 0 <= n < 2^31.
 * All hypothesis arithmetic is float32 in the written order without contraction, division and square root
 * correctly rounded.
 *   hypotheses  K = num_iterations of them, 1 <= K <= 2^20; ransac_n must be 3.  The triple of hypothesis t is
 *               triples_opt[3 t ..] (K x 3) when given, else the built-in counter-based sampler's
 *               (lio_plane_sample_triples with `seed`).  n < 3 gives no hypothesis at all: "no plane".
 *   plane       of (p0, p1, p2): e1 = p1 - p0, e2 = p2 - p0; (nx, ny, nz) = (e1y e2z - e1z e2y,
 *               e1z e2x - e1x e2z, e1x e2y - e1y e2x); len = sqrtf((nx nx + ny ny) + nz nz);
 *               (a, b, c) = (nx, ny, nz) / len; d = -((a p0x + b p0y) + c p0z).  The hypothesis is DEGENERATE,
 *               and skipped, unless len is finite and > 0 and d is finite (collinear points, duplicates,
 *               non-finite members).  The sign of the normal is left as computed.
 *   score       dist_i = fabsf(((a x + b y) + c z) + d); point i is an inlier iff dist_i < distance_threshold
 *               (strict, float: a non-finite point is never one); count = the inliers; the error is a
 *               fixed-point sum, independent of the order of summation: thr2 = thr * thr (float, must be
 *               finite), (m, e) = frexp(thr2), q_i = (uint64) floor((double)(float)(dist_i * dist_i) * 2^(32 - e))
 *               (< 2^32), sq = the sum of q_i over the inliers.
 *   winner      the non-degenerate hypothesis that minimises (-count, sq, t): Open3D ranks by fitness, then by
 *               RMSE (for equal counts the smaller squared sum); THE LOWEST HYPOTHESIS INDEX t among equals is
 *               this library's tie-break.  Every hypothesis degenerate, or n < 3: "no plane" — status 0,
 *               *best_iteration = -1, no inliers, plane (0, 0, 0, 0).
 *   departures  from Open3D: all K hypotheses are always evaluated (its `probability` early exit only drops
 *               later hypotheses; a parallel evaluation has no use for it), and the returned inliers are
 *               those of the winning hypothesis plane (as Open3D >= 0.13 [U]), not of the refit.
 * plane4_out: (a, b, c, d) of the winner; *best_iteration: its t.  inliers_out (capacity n): the inliers'
 * indices ascending, *n_inliers of them.  mask_opt (n, may be NULL): 1 for an inlier.  counts_opt (K int64) and
 * sq_opt (K uint64), may be NULL: every hypothesis's score, 0 for a degenerate one; degenerate_opt (K, may be
 * NULL): 1 for a degenerate one (all 1 when n < 3).  refit4_opt (4 doubles, may be NULL): the least-squares
 * plane through the inliers (Open3D's GetPlaneFromPoints [U]) — second moments in double about the
 * lowest-index inlier, reduced on the device in a fixed order, the eigenvector of the smallest eigenvalue of
 * the covariance as the normal, signed so that its dot product with the winner's (a, b, c) is >= 0,
 * d = -n . centroid; with fewer than 3 inliers the winner plane widened to double.
 * LIO_ERR_ARG before any device work: distance_threshold <= 0, NaN or infinite (or its float square infinite),
 * stride outside 3..8, n < 0 or n >= 2^31, num_iterations outside 1..2^20, ransac_n != 3, a triple with an
 * index outside [0, n) or a repeated index, NULL plane4_out / best_iteration / n_inliers, NULL pts or
 * inliers_out with n > 0.  Repeated calls give bit-identical results.                                        */
int lio_segment_plane(lio_filter* f, const float* pts, int64_t n, int stride, float distance_threshold, int ransac_n,
                      int64_t num_iterations, uint64_t seed, const int32_t* triples_opt, float* plane4_out,
                      int64_t* best_iteration, int32_t* inliers_out, int64_t* n_inliers, uint8_t* mask_opt,
                      int64_t* counts_opt, uint64_t* sq_opt, uint8_t* degenerate_opt, double* refit4_opt);
/* The built-in sampler of lio_segment_plane, host only (no device needed): out (num_iterations x 3) = the
 * triples of distinct indices in [0, n).  All arithmetic mod 2^64: r(c) = mix(seed + (c + 1) * 0x9E3779B97F4A7C15),
 * mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31)
 * (splitmix64).  i0 = r(3t) % n; i1 = r(3t + 1) % (n - 1), + 1 if >= i0; i2 = r(3t + 2) % (n - 2), + 1 if
 * >= min(i0, i1), then + 1 if >= max(i0, i1).  n < 3 writes nothing (status 0).  LIO_ERR_ARG: n < 0 or
 * n >= 2^31, num_iterations < 0 or > 2^20, NULL out with something to write.                                   */
int lio_plane_sample_triples(uint64_t seed, int64_t n, int64_t num_iterations, int32_t* out);

/* k-means with k-means++ seeding and one bounding box per cluster: the cv::kmeans call of the reference's
 * projection tool (post_process/lidar_projection/src/lidar_projection.cpp:82-92: K 5, TermCriteria(EPS +
 * MAX_ITER, 100, 0.1), 3 attempts, KMEANS_PP_CENTERS), OpenCV's procedure [U] followed step by step and restated
 * as a contract of this library; it is not bit parity with cv::kmeans or cv::RNG.  pts is n x stride floats (x,
 * y, z first; stride 3..8), 0 <= n < 2^31; 1 <= K <= 64, 1 <= attempts <= 16, 1 <= max_iter <= 1000, eps finite
 * and >= 0.  All float arithmetic is in the written order without contraction, as everywhere in the library.
 *   points    a point with a non-finite x, y or z takes no part: label -1, in no sum.  nf = the finite points.
 *             nf < K is LIO_ERR_ARG (OpenCV asserts N >= K [U]): before any device work when n < K (n = 0 included:
 *             K >= 1 > nf), else after the counting pass; nothing is written.
 *   scales    from the finite points' box (lo, hi per axis).  Coordinates: A = the largest of |lo|, |hi| over the
 *             axes, (m, ec) = frexp(A) (ec = 0 when A = 0), qx_i = (int64) rint((double) x_i 2^(31 - ec)): exact in
 *             double, |qx_i| <= 2^31.  Distances: ex = hi_x - lo_x (float; ey, ez alike), D2 = (ex ex + ey ey) +
 *             ez ez (float; must be finite, else LIO_ERR_ARG), (m, ed) = frexp(D2) (ed = 0 when D2 = 0),
 *             q(d) = (uint64) floor((double) d 2^(31 - ed)) < 2^32 for every squared distance d inside the box.
 *             d2(p, c) = (dx dx + dy dy) + dz dz in float with dx = p_x - c_x.  Every sum below is an integer sum.
 *   draws     mod 2^64: r(c) = mix(seed + (c + 1) 0x9E3779B97F4A7C15), mix as in lio_plane_sample_triples;
 *             attempt a, centre k, trial j uses c = (a K + k) 3 + j (centre 0: j = 0).
 *   seeding   per attempt, unless init_centers_opt (attempts x K x 3 finite floats) replaces it: OpenCV's
 *             generateCentersPP with 3 trials [U].  Centre 0 is the (r(c) mod nf)-th finite point in index
 *             order; w_i = q(d2(p_i, centre 0)), 0 for a non-finite point.  For k = 1 .. K - 1: sum0 = sum w_i;
 *             trial j: u = r(c) >> 11, t = (u sum0) >> 53 (128-bit product), the candidate ci is the lowest
 *             index whose inclusive prefix sum of w exceeds t (the lowest finite index when sum0 = 0),
 *             w'_i = min(q(d2(p_i, p_ci)), w_i), s = sum w'_i; the trial with the smallest s wins, THE LOWEST j
 *             AMONG EQUALS; its ci is centre k and w becomes its w'.
 *   Lloyd     [U] assign every finite point to the centre with the smallest d2 (strict < over ascending k: THE
 *             LOWEST k WINS A TIE), it = 1.  Then repeat: per cluster cnt_k and S_k = sum (qx, qy, qz); for k
 *             ascending with cnt_k = 0 the repair: mk = the cluster with the largest count (lowest index among
 *             equals), its member with the largest float d2 to mk's current mean (THE LOWEST INDEX AMONG EQUALS:
 *             this library's tie-break) moves to k (label, both counts, both sums); c_k = (float)(((double) S_k
 *             / (double) cnt_k) 2^(ec - 31)) per axis; shift = max over k of (tx tx + ty ty) + tz tz in double,
 *             tx = the float c_new,x - c_old,x widened; it += 1; stop when it == max(max_iter, 2) or
 *             shift <= (double) eps * eps, else assign again.  AT THE STOP THE LABELS ARE NOT REASSIGNED: every
 *             centre is exactly the mean of its members.  cq = sum q(d2(p_i, c_label_i)) over the finite points.
 *   result    the attempt with the smallest cq, the lowest attempt among equals.
 * labels_out (n); centers_out (K x 3); *compactness_out = (double) cq 2^(ed - 31).  May be NULL, each of them:
 * counts_opt (K); aabb6_opt (K x 6: float min x, y, z, max x, y, z over each cluster's members); seeds_opt
 * (attempts x K: the chosen point indices, -1 everywhere with init_centers_opt); attempt_q_opt / attempt_iters_opt
 * (per attempt cq and it); stats6_opt = nf, best attempt, its it, repairs over all attempts, ec, ed.
 * Centres are float32, as OpenCV's: at map coordinates of 8e5 m a float ulp is 6 cm, so subtract an origin
 * first (lio_georeference_xy offers one).
 * LIO_ERR_ARG before any device work, with or without a device: every range above, a non-finite
 * init_centers_opt entry, NULL pts / labels_out with n > 0, NULL centers_out / compactness_out, n < K.
 * Repeated calls and any scheduling of the device give identical bits; a repeated call of one size allocates
 * nothing (lio_alloc_count).                                                                                    */
int lio_kmeans(lio_filter* f, const float* pts, int64_t n, int stride, int K, int max_iter, float eps,
               int attempts, uint64_t seed, const float* init_centers_opt,
               int32_t* labels_out, float* centers_out, double* compactness_out,
               int64_t* counts_opt, float* aabb6_opt, int32_t* seeds_opt,
               uint64_t* attempt_q_opt, int32_t* attempt_iters_opt, int64_t* stats6_opt);

/* Surface normals and curvature per point: pcl::NormalEstimation (setKSearch / setRadiusSearch) [U] and Open3D's
 * estimate_normals with its hybrid search [U], PCL's procedure followed step by step and restated as a contract
 * of this library, checked exactly against a numpy restatement; it is not bit parity with PCL, whose float
 * covariance and eigen33 are not pinned here.  pts is n x stride floats (x, y, z first; stride 3..8),
 * 0 <= n < 2^31; radius 0 or finite and > 0; k 0 or 3..255; not both 0.  No float contraction anywhere.
 *   neighbours  d2(i, j) = float ((dx*dx + dy*dy) + dz*dz).  For a finite point i the candidates are the finite
 *               points j, j = i included; with radius > 0 those with d2 < r2, r2 = (float)((double)radius *
 *               radius): THE TEST IS STRICT (PCL's rule).  With k > 0 and more than k candidates N_i is the k
 *               smallest under (d2, THEN INDEX j).  k alone is setKSearch, radius alone setRadiusSearch, both
 *               Open3D's hybrid.  m_i = |N_i|.  A non-finite point is nobody's neighbour: NaN outputs, count 0.
 *               m_i < 3: NaN outputs, the count still reported.
 *   moments     integer sums, independent of the order.  B_i = r2 when radius > 0, else the largest d2 in N_i;
 *               (mant, e) = frexp((double)B_i), h = ceil(e / 2), s = 2^(15 - h); per neighbour o = p_j - p_i in
 *               float, q_a = (int64) rint((double)o_a s) (|q_a| <= 2^15); S_a = sum q_a, S_ab = sum q_a q_b in
 *               int64; M_ab = (double)S_ab - ((double)S_a (double)S_b) / (double)m; T = (M_00 + M_11) + M_22.
 *               B_i = 0, or T > 0 false: the point is DEGENERATE, NaN outputs.
 *   eigenvector IEEE double, + - * / sqrt only: cyclic Jacobi.  A = M, V = I, at most 10 sweeps; before each
 *               sweep stop when A_01, A_02 and A_12 are all exactly 0.  A sweep visits (p, q) = (0, 1), (0, 2),
 *               (1, 2), r the third index, a pair with A_pq = 0 skipped: theta = (A_qq - A_pp) / (2 A_pq);
 *               t = 1 / (|theta| + sqrt(theta theta + 1)), negated when theta < 0; c = 1 / sqrt(t t + 1);
 *               s = t c; A_pp -= t A_pq; A_qq += t A_pq; A_pq = 0; (A_rp, A_rq) <- (c A_rp - s A_rq,
 *               s A_rp + c A_rq); every row of V likewise.  lambda = the diagonal; the column of V of the
 *               smallest lambda, THE LOWEST INDEX AMONG EQUALS, is the normal; curvature = |lambda| / T.
 *   orientation with a viewpoint v: s = ((v_x - x) n_x + (v_y - y) n_y) + (v_z - z) n_z in double, the normal
 *               flipped when s < 0 (a NaN s flips nothing).  viewpoints_opt: vp_stride 0 = one viewpoint of 3
 *               floats for the whole cloud, vp_stride 3..8 = one row per point (a SLAM map needs the pose that
 *               saw each point).  NULL: flipped when n_z < 0, or n_z = 0 and n_y < 0, or n_z = n_y = 0 and
 *               n_x < 0.
 * normals_out (n x 3 floats, rounded from double); may be NULL, each of them: curvature_opt (n floats), counts_opt
 * (n: m_i), stats6_opt = finite points, points with a normal, finite points with m < 3, degenerate points, the
 * largest m, the sum of m.
 * LIO_ERR_ARG before any device work, with or without a device: every range above, a radius > 0 whose r2 is 0
 * or infinite, vp_stride not 0 or 3..8, NULL pts / normals_out with n > 0; nothing is written.  Repeated calls and any scheduling of the device give
 * identical bits; a repeated call of one size allocates nothing (lio_alloc_count).                             */
int lio_estimate_normals(lio_filter* f, const float* pts, int64_t n, int stride, float radius, int k,
                         const float* viewpoints_opt, int vp_stride,
                         float* normals_out, float* curvature_opt, int32_t* counts_opt, int64_t* stats6_opt);

/* ------------------------------- GPS-to-SLAM trajectory alignment and map georeferencing (offline GPS leg) */
/* Layout of lio_gps_align's result (doubles).  Pairs are (x, y); a rotation is (c, s) for [[c, -s], [s, c]]. */
#define LIO_GPSALIGN_ITERATIONS 0  /* iterations run                                                          */
#define LIO_GPSALIGN_CONVERGED 1   /* 1 when |prev - mean_error| < tolerance stopped the loop                 */
#define LIO_GPSALIGN_MEAN_ERROR 2  /* the last mean_error                                                     */
#define LIO_GPSALIGN_S0 3          /* the initial scale                                                       */
#define LIO_GPSALIGN_CA 4          /* centroid of slam_xy (2)                                                 */
#define LIO_GPSALIGN_CB 6          /* centroid of gps_xy (2)                                                  */
#define LIO_GPSALIGN_SC 8          /* the last iteration's increment: scale,                                  */
#define LIO_GPSALIGN_C 9           /*   rotation c,                                                           */
#define LIO_GPSALIGN_S 10          /*   rotation s,                                                           */
#define LIO_GPSALIGN_T 11          /*   translation (2),                                                      */
#define LIO_GPSALIGN_CD 13         /*   centroid of the matched targets (2)                                   */
#define LIO_GPSALIGN_REF_SCALE 15  /* THE REFERENCE'S RETURN TRIPLE: scale,                                   */
#define LIO_GPSALIGN_REF_C 16      /*   rotation c,                                                           */
#define LIO_GPSALIGN_REF_S 17      /*   rotation s,                                                           */
#define LIO_GPSALIGN_REF_T 18      /*   translation (2)                                                       */
#define LIO_GPSALIGN_TOTAL_SCALE 20 /* the TOTAL similarity slam_xy -> GPS frame: scale,                      */
#define LIO_GPSALIGN_TOTAL_C 21    /*   rotation c,                                                           */
#define LIO_GPSALIGN_TOTAL_S 22    /*   rotation s,                                                           */
#define LIO_GPSALIGN_TOTAL_T 23    /*   translation (2)                                                       */
#define LIO_GPSALIGN_LEN 25
/* Layout of lio_similarity2d_fit's result (doubles): scale, rotation c, s, translation (2). */
#define LIO_SIM2D_SCALE 0
#define LIO_SIM2D_C 1
#define LIO_SIM2D_S 2
#define LIO_SIM2D_T 3
#define LIO_SIM2D_LEN 5

/* icp_alignment of the reference's offline GPS leg (post_process/align_slam_gps_icp.py:81-156): a 2-D similarity,
 * with scale, between the SLAM trajectory (the source, slam_xy: n x 2 doubles) and the projected GPS track (the
 * target, gps_xy: m x 2 doubles; the projection from WGS84 is the caller's) by point-to-point ICP.  This is the
 * library's own restatement, exact to the bit: every operation is an IEEE double + - x / sqrt in the written
 * order, no multiply-add is fused on host or device, and every sum is TREE.
 *   TREE(v)   the only summation: v in blocks of 256 consecutive elements, the last padded with +0.0; inside a
 *             block a[i] = a[i] + a[i + w] for i < w, for w = 128, 64, ..., 1; THE BLOCK SUMS ARE ADDED IN
 *             ASCENDING BLOCK ORDER into a scalar that starts at 0.0 (the TREE order: this library's contract).
 *   start     cA = (TREE(Ax) / n, TREE(Ay) / n) over the source A, cB likewise over the target B (/ m);
 *             Ac = A - cA, Bc = B - cB; sA = sqrt(TREE(Acx Acx + Acy Acy)), sB likewise; s0 = sB / sA if
 *             sA > 1e-8, else 1; S = s0 Ac, D = Bc.
 *   iteration i = 0 .. max_iterations - 1:
 *     1 nearest neighbour: source j takes the target k with the smallest d2 = (dx dx) + (dy dy), dx = Sx[j] -
 *       Dx[k], dy = Sy[j] - Dy[k]; AN EQUAL d2 GOES TO THE LOWEST INDEX k; dist[j] = sqrt(d2).  The comparison is
 *       on d2, not on the rooted distance as in numpy: the two differ only where two distinct d2 round to one
 *       square root (this library's contract).
 *     2 cs = (TREE(Sx) / n, TREE(Sy) / n); cd = (TREE(Mx) / n, TREE(My) / n) over the matched targets M[j] = D[k_j].
 *     3 with a = S - cs, b = M - cd: h00 = TREE(ax bx), h01 = TREE(ax by), h10 = TREE(ay bx), h11 = TREE(ay by),
 *       saa = TREE(ax ax + ay ay), sbb = TREE(bx bx + by by).
 *     4 p = h00 + h11, q = h01 - h10, r = sqrt(p p + q q); (c, s) = (p / r, q / r), or (1, 0) when r == 0: the
 *       proper rotation that maximises tr(R H), which in 2-D is the reference's SVD with its determinant fix.
 *     5 sc = sqrt(sbb) / sqrt(saa) (the reference's norm ratio, not the least-squares scale);
 *       t = cd - sc (R cs) with R v = (c vx - s vy, s vx + c vy).
 *     6 S <- (sc (c Sx - s Sy) + tx, sc (s Sx + c Sy) + ty).
 *     7 mean_error = TREE(dist) / n (the distances from before step 6, as in the reference); stop with converged = 1
 *       if |prev - mean_error| < tolerance, else prev = mean_error; prev starts at +inf.
 * aligned_xy_out (n x 2): the final S, in the centred frame — add cB for the GPS frame.  nn_out_opt (n, may be
 * NULL): the last iteration's indices k_j.  out: LIO_GPSALIGN_LEN doubles, offsets above.
 *   reference return  THE REFERENCE'S RETURN TRIPLE, by its own closing formula (align_slam_gps_icp.py:152-154):
 *             scale = s0 sc, R = (c, s), T = cB + sc (R v), v = cd - s0 (R^T u), u = cB - t, R^T u = (c ux + s uy,
 *             c uy - s ux) — of the LAST iteration only.  It chains the last increment with the initial scale, not
 *             the accumulated transform: a quirk of the reference, reproduced under that name (the reference-return
 *             quirk) for callers that compare with the script.
 *   total     the similarity that maps slam_xy to the aligned points in the GPS frame, composed on the host: start
 *             (S, C, Sn) = (s0, 1, 0), T = -(s0 cA); per iteration S <- sc S, (C, Sn) <- (c C - s Sn, s C + c Sn),
 *             T <- sc (R T) + t; at the end T <- T + cB.  This is what georeferencing wants.
 * LIO_ERR_ARG before any device work: a NULL pointer (nn_out_opt excepted), n < 1, m < 1, n or m >= 2^31,
 * max_iterations < 1, a non-finite coordinate (a host scan); after the start: sA or sB is 0 (the reference raises on
 * "zero variance").  LIO_ERR_STATE: saa == 0 or sc not finite in an iteration.  Repeated calls give identical bits. */
int lio_gps_align(lio_filter* f, const double* gps_xy, int64_t m, const double* slam_xy, int64_t n, int max_iterations,
                  double tolerance, double* aligned_xy_out, int32_t* nn_out_opt, double* out);
/* align_trajectories_horn (georef_mapmatch.py:115-135; the timestamp-matched scripts): steps 2-5 of one iteration
 * of lio_gps_align on the n given pairs, M = dst_xy paired one to one with S = src_xy, in the same TREE order.
 * out: LIO_SIM2D_LEN doubles: dst ~ scale R src + t.  LIO_ERR_ARG: a NULL pointer, n < 1 or >= 2^31, a non-finite
 * coordinate.  LIO_ERR_STATE: saa == 0 (one pair, or all sources equal) or a scale that is not finite.           */
int lio_similarity2d_fit(lio_filter* f, const double* src_xy, const double* dst_xy, int64_t n, double* out);
/* The map transform of post_process/georeference_pcd.py:236-244 on point records (n x stride floats, x, y, z
 * first; stride 3..8; 0 <= n < 2^31).  Per point, in double from the float32 x, y, in this order:
 *   gx = ((x r00) + (y r01)) scale + tx - ox,  gy = ((x r10) + (y r11)) scale + ty - oy
 * with R4 = r00, r01, r10, r11, t2 = tx, ty and origin2_opt = ox, oy (NULL: 0, 0, the reference's behaviour).
 * out (n x stride): the records with x, y replaced by (float)gx, (float)gy, every other field bit-copied.
 * xy_out_opt (n x 2 doubles, may be NULL): gx, gy at full precision.  At national-grid magnitudes (HK1980:
 * about 8e5 m) a float32 x, y quantises to 6 cm; a non-zero origin near the map keeps the float32 records
 * fine-grained, and is the reason the parameter exists.  LIO_ERR_ARG: NULL R4 / t2, NULL pts or out with n > 0,
 * stride outside 3..8, n < 0 or >= 2^31.                                                                        */
int lio_georeference_xy(lio_filter* f, const float* pts, int64_t n, int stride, double scale, const double* R4,
                        const double* t2, const double* origin2_opt, float* out, double* xy_out_opt);

/* ------------------------------- camera projection and point cloud colorization from images (offline camera leg) */
/* A camera: pinhole intrinsics, the 8-parameter rational distortion model of OpenCV (post_process/
 * undistort_image.py:95-97) and the image size.  dist = k1 k2 p1 p2 k3 k4 k5 k6; all zero is a pinhole.  r2_max
 * bounds the squared normalised radius (+inf: no limit): a rational model is only meaningful inside the field it
 * was calibrated on, and a far-off-axis point can fold back into the image beyond it.                            */
typedef struct lio_camera {
    double fx, fy, cx, cy;
    double dist[8];
    double r2_max;
    int32_t width, height;
} lio_camera;
/* occlusion: 0 (the reference: none) or 1 (the z-buffer below); splat_radius 0..8; depth_rel, depth_abs >= 0:
 * the visibility tolerance; bgr: 1 when the image's channel order is B G R (OpenCV's, as in the script), 0 for
 * R G B.  NULL where a function takes these means {0, 0, 0, 0, 1}.                                               */
typedef struct lio_colorize_params {
    int32_t occlusion;
    int32_t splat_radius;
    float depth_rel;
    float depth_abs;
    int32_t bgr;
} lio_colorize_params;
/* sizeof of the two structs above, in that order, as lio_abi_struct_sizes does for the earlier ones (whose list
 * is closed: callers compare its length); returns their number.                                                  */
int lio_abi_camera_struct_sizes(int64_t* out, int n);

/* The projection of post_process/colorize_pcd.py:31-47 (projectPointsToImagePlane's role in post_process/
 * lidar_projection/src/lidar_projection.cpp:9-34) on point records (n x stride floats, x, y, z first; stride
 * 3..8; 0 <= n < 2^31).  Rt: 12 doubles, row-major 3 x 3 R, then t; it maps points to the camera frame.  This is
 * the library's own restatement, exact to the bit: per point, in IEEE double, nothing fused, in this order:
 *   x, y, z widened to double;
 *   c_k = ((R[k][0] x + R[k][1] y) + R[k][2] z) + t[k] for the rows k of R: xc, yc, zc;
 *   xn = xc / zc; yn = yc / zc; r2 = xn xn + yn yn;
 *   num = 1 + ((k3 r2 + k2) r2 + k1) r2; den = 1 + ((k6 r2 + k5) r2 + k4) r2; rad = num / den;
 *   a1 = 2 xn yn; a2 = r2 + 2 xn xn; a3 = r2 + 2 yn yn;
 *   xd = xn rad + (p1 a1 + p2 a2); yd = yn rad + (p1 a3 + p2 a1);
 *   u = fx xd + cx; v = fy yd + cy;
 *   valid = zc > 0 && r2 <= r2_max && u >= 0 && u < width && v >= 0 && v < height (EVERY COMPARISON IS FALSE ON
 *   NaN: the script's test, colorize_pcd.py:47, with r2_max added);
 *   px = (int)u; py = (int)v: TRUNCATION ONLY AFTER THE TEST (u = -0.5 is invalid, it is not pixel 0).
 * With an all-zero dist, rad == 1 and the tangential term is +0, so u is bit for bit the script's fx * (x / z) +
 * cx.  The script's R @ P.T + t goes through BLAS and differs from this fixed order in the last bits of some
 * coordinates; the C++ tool's float formulation (K p) / p_z is another rounding and is NOT reproduced.
 * uv_opt (n x 2 doubles: u, v), zc_opt (n doubles), pix_opt (n x 2 int32: px, py, -1 -1 where invalid) may be
 * NULL; valid: n uint8.  LIO_ERR_ARG before any device work, with a message that names the bound: a NULL cam, Rt
 * or valid, NULL pts with n > 0, n < 0 or >= 2^31, stride outside 3..8, width or height below 1, width x height >=
 * 2^31, a non-finite intrinsic, distortion or pose entry, r2_max NaN or negative.                                */
int lio_project_points(lio_filter* f, const float* pts, int64_t n, int stride, const lio_camera* cam, const double* Rt,
                       double* uv_opt, double* zc_opt, int32_t* pix_opt, uint8_t* valid);

/* Colours of a point cloud from any number of camera frames.  The cloud and the per-point state stay on the
 * device between frames; a frame uploads its image and 12 + 16 doubles.  Per-point state: best_z (double, starts
 * at +inf), rgb (3 x uint8, starts at 0), frame (int32, starts at -1).
 *   frame     a frame's CANDIDATES are its valid points (lio_project_points); with occlusion, the visible ones.
 *             A candidate replaces the state iff zc < best_z — STRICT, SO ON A TIE THE EARLIER FRAME STAYS — and
 *             the state takes zc, the colour of pixel (px, py) IN R G B ORDER whatever the image's order, and the
 *             running frame number (0 for the first frame after set_cloud or reset).
 *   occlusion (opt-in; the reference has none: points behind a wall take the wall's colour) a depth image D of
 *             width x height uint32 starts at the bits of float +inf; every valid point has zf = (float)zc, rounded
 *             to nearest, and writes D[q] = min(D[q], bits(zf)) for every pixel q = (px + dx, py + dy) with |dx|,
 *             |dy| <= splat_radius inside the image.  zf >= 0, so unsigned order on the bits is float order and the
 *             minimum does not depend on the order of arrival.  A valid point is VISIBLE iff
 *             zf <= (D[py][px] * (1.0f + depth_rel)) + depth_abs, in float, nothing fused.  A point always sees its
 *             own splat; it is hidden only by something in front of it by more than the tolerance.
 * With one frame and no occlusion this is colorize_pcd.py: frame >= 0 is its mask, rgb / 255.0 (0.5 where frame <
 * 0) its double colours bit for bit.  Blending of several frames is out of scope: the nearest view wins.
 * image: height rows of `pitch` bytes, 3 bytes per pixel; only 3 x width bytes of the last row are read.
 * LIO_ERR_ARG before any device work, with a message that names the bound: a NULL pointer (frame_opt and depth_opt
 * excepted; pts may be NULL when n == 0), n < 0 or >= 2^31, stride outside 3..8, the camera and pose conditions of
 * lio_project_points, pitch < 3 x width, splat_radius outside 0..8, a negative or non-finite tolerance.
 * LIO_ERR_STATE: add_frame or get before set_cloud.  Repeated sequences give identical bits; from the second frame
 * of one size on nothing is allocated (lio_alloc_count).                                                          */
typedef struct lio_colorizer lio_colorizer;
int lio_colorizer_create(int device, const lio_colorize_params* params, lio_colorizer** out);
int lio_colorizer_destroy(lio_colorizer* h);
int lio_colorizer_set_params(lio_colorizer* h, const lio_colorize_params* params);
/* uploads the cloud, resets the state and the frame number */
int lio_colorizer_set_cloud(lio_colorizer* h, const float* pts, int64_t n, int stride);
/* n_updated: the number of points whose state this frame replaced */
int lio_colorizer_add_frame(lio_colorizer* h, const lio_camera* cam, const double* Rt, const uint8_t* image, int64_t pitch,
                            int64_t* n_updated);
/* rgb: n x 3 uint8; frame_opt: n int32 (-1: never coloured); depth_opt: n doubles (best_z, +inf likewise) */
int lio_colorizer_get(lio_colorizer* h, uint8_t* rgb, int32_t* frame_opt, double* depth_opt);
/* the state back to its start; the cloud stays */
int lio_colorizer_reset(lio_colorizer* h);
/* device time of the last add_frame in ms (stream events): upload (staging copy included), depth fill, splat,
 * resolve (without occlusion: 0, 0 and the fused kernel)                                                          */
int lio_colorizer_get_timing(lio_colorizer* h, double* ms4);

/* ------------------------------------------------------------- image undistortion (rectification; camera leg) */
/* The image operation the reference's camera scripts run on every frame before anything reads it:
 * cv2.undistort(img, K, D, None, K) (post_process/undistort_image.py:21-27, decompress_undistort_images.py:28,
 * extract_pointcloud_image.py:26-28, extraction.py:21-22).  The contract is the library's own, exact to the bit.
 *   cameras   src: the raw image's lio_camera (intrinsics, dist, width, height).  dst_opt: the rectified image's
 *             fx fy cx cy width height; NULL means src's values, which is the scripts' call; its dist must be all
 *             zero.  r2_max of both is ignored (OpenCV has no such bound here).  Widths and heights of both are in
 *             1..32767 (OpenCV's short map range; a map record packs into 8 bytes).
 *   map       for the output pixel in column j and row i, in IEEE double, nothing fused, in this order:
 *               xn = ((double)j - dst.cx) / dst.fx;  yn = ((double)i - dst.cy) / dst.fy;
 *             then exactly the lines of lio_project_points from r2 = xn xn + yn yn through u = fx xd + cx;
 *             v = fy yd + cy with src's coefficients (one device function serves both entries).
 *   quantise  OpenCV's CV_16SC2 fixed-point map with INTER_BITS = 5: qu = rint(u * 32.0), qv = rint(v * 32.0), TIES
 *             TO EVEN.  If !(fabs(qu) < 2^30 && fabs(qv) < 2^30) (THE TEST IS FALSE ON NaN) the pixel is FAR: sx = sy
 *             = INT32_MIN, ax = ay = 0.  Otherwise, with qu and qv taken as int: sx = qu >> 5 (arithmetic shift:
 *             floor), ax = qu & 31; sy, ay likewise.
 *   sample    INTER_LINEAR with BORDER_CONSTANT per tap: the taps (sx, sy) (sx + 1, sy) (sx, sy + 1) (sx + 1, sy + 1)
 *             have the integer weights (32 - ax)(32 - ay), ax (32 - ay), (32 - ax) ay, ax ay.  A tap outside 0 <= x
 *             < src.width, 0 <= y < src.height contributes the border value of its channel and is NEVER LOADED, even
 *             when its weight is 0 (the last column of an identity map has sx + 1 == width).  Per channel
 *             out = (sum w p + 512) >> 10.  A FAR pixel is the border value.
 * As far as we read OpenCV's source this is its remap: the 32 x 32 bilinear table entries (32 - a)(32 - b) / 1024
 * are exact in float, scaled by 2^15 they are integers that sum to 32768 (its sum correction never fires), and
 * (sum 32 w p + 2^14) >> 15 equals the line above.  AGREEMENT WITH cv2.undistort IS THIS READING OF ITS SOURCE AND IS
 * UNVERIFIED: OpenCV was not available where this was written, and its own map arithmetic before the 1/32-pixel
 * rounding (SIMD, incremental row terms) depends on its version and is not reproduced.
 * images: uint8, channels 1 or 3, the channel order is irrelevant.  Input: src.height rows of `pitch` bytes;
 * output: dst.height rows of `out_pitch` bytes.  Only channels x width bytes of a row are read or written: the
 * output's padding bytes are left untouched.  border_opt: 3 uint8 (one per channel); NULL means 0 0 0, the scripts'
 * default.
 *
 * lio_undistort_map: the map alone, dst.height x dst.width x 2 values each, row-major (any may be NULL): uv, the
 * unquantised u, v; sxy: sx, sy; axy: ax, ay.
 * lio_undistorter: set_camera computes the packed map and keeps it on the device; run uploads a frame, gathers
 * and downloads through staging that is reused across frames.  get_timing: device ms of the last run from stream
 * events: upload (its staging copy included), kernel, download (the device-to-host copy; the rows then go to
 * `out` on the host).
 * LIO_ERR_ARG before any device work, with a message that names the bound: a NULL src, image, out or ms3, a width
 * or height outside 1..32767, a non-finite intrinsic or coefficient, dst fx or fy equal to 0, a non-zero dst dist,
 * channels not 1 or 3, pitch < channels x src.width, out_pitch < channels x dst.width.  The checks that need no
 * handle are made before the handle is looked at.  LIO_ERR_STATE: run before set_camera.  From the second run of
 * one size on nothing is allocated (lio_alloc_count); repeated runs give identical bits.                        */
int lio_undistort_map(lio_filter* f, const lio_camera* src, const lio_camera* dst_opt, double* uv_opt, int32_t* sxy_opt,
                      uint8_t* axy_opt);
typedef struct lio_undistorter lio_undistorter;
int lio_undistorter_create(int device, lio_undistorter** out);
int lio_undistorter_destroy(lio_undistorter* h);
int lio_undistorter_set_camera(lio_undistorter* h, const lio_camera* src, const lio_camera* dst_opt, int channels,
                               const uint8_t* border_opt);
int lio_undistorter_run(lio_undistorter* h, const uint8_t* image, int64_t pitch, uint8_t* out, int64_t out_pitch);
int lio_undistorter_get_timing(lio_undistorter* h, double* ms3);

/* ------------------------------------------- wire / disk formats (§8(f) row 4) */
/* One output column of a packed point record: byte offset, sensor_msgs/PointField datatype
 * (INT8 1, UINT8 2, INT16 3, UINT16 4, INT32 5, UINT32 6, FLOAT32 7, FLOAT64 8; 0 = absent -> 0)
 * and a scale (1 = exact; e.g. a time unit -> ms as FAST-LIO's time_unit_scale).                 */
typedef struct lio_cloud_field {
    int32_t offset;
    int32_t datatype;
    float scale;
} lio_cloud_field;
/* sensor_msgs/PointCloud2 data (n_points records of point_step bytes) -> float records with one
 * column per field (pcl::fromROSMsg's field copy; other datatypes are converted to float).     */
int lio_cloud2_decode(lio_filter* f, const uint8_t* data, int64_t n_points, int32_t point_step, int is_bigendian,
                      const lio_cloud_field* fields, int n_fields, float* out);
/* float records -> little-endian FLOAT32 fields at the given offsets, other bytes zero
 * (pcl::toROSMsg of PointXYZI: x 0, y 4, z 8, intensity 16, point_step 32).                   */
int lio_cloud2_encode(lio_filter* f, const float* rec, int64_t n, int stride, const lio_cloud_field* fields,
                      int n_fields, int32_t point_step, uint8_t* data);
/* lio_scan_preprocess straight from the PointCloud2 bytes of a raw scan; fields[5] = x, y, z,
 * intensity, time (scaled to ms): one upload, decode + preprocessing on the device.            */
int lio_scan_preprocess_cloud2(lio_ctx* c, const uint8_t* data, int64_t n_points, int32_t point_step,
                               int is_bigendian, const lio_cloud_field fields[5], const lio_scan_prep_params* p,
                               const lio_imu_pose* poses, int n_poses, const lio_pose* end, int64_t* n_down);
/* pcl::io::savePCDFileBinary (fast_lio_sam.cpp:925-932): header + packed float32 fields.       */
int lio_pcd_write_binary(const char* path, const float* rec, int64_t n, int stride, const char* const* names);
/* PCD v0.7 reader (DATA ascii | binary): POINTS and the float columns named in `want`
 * (absent fields read 0).  out == NULL returns the point count only.                           */
int lio_pcd_read(lio_filter* f, const char* path, const char* const* want, int n_want, float* out, int64_t cap,
                 int64_t* n_points);
/* a saved map (x y z of a PCD file) straight into the GPU grid (ikdtree.Build)                   */
int lio_map_build_pcd(lio_map* m, const char* path);

/* ----------------------------------------------------------------- timing */
typedef struct lio_kernel_timing {
    int64_t knn_launches;   double knn_ms;     /* kNN h-evaluation: near + far + plane kernels  */
    int64_t reuse_launches; double reuse_ms;   /* converge=false re-evaluation kernel         */
    int64_t icp_launches;   double icp_ms;     /* ICP correspondence + statistics kernels     */
    int64_t near_launches;  double near_ms;    /* kNN near pass (inside knn_ms)                */
    int64_t far_launches;   double far_ms;     /* kNN far pass (inside knn_ms)                 */
    int64_t plane_launches; double plane_ms;   /* plane / H / reduction pass (inside knn_ms)   */
    int64_t icp_nn_launches; double icp_nn_ms; /* ICP correspondence kernel alone (inside icp_ms) */
} lio_kernel_timing;

/* When enabled, every front-end kernel is launched with hipExtLaunchKernel's
 * start / stop events — the kernel's own execution span, as rocprofv3 reports
 * it (no launch gaps) — and the spans accumulate here (knn_ms = near + far +
 * plane).  The ICP handle brackets its pass (both kernels) with events, and its
 * correspondence kernel alone (icp_nn_ms).                                    */
int lio_ctx_set_timing(lio_ctx* c, int enable);
int lio_ctx_get_timing(lio_ctx* c, lio_kernel_timing* out);
int lio_ctx_reset_timing(lio_ctx* c);
int lio_icp_set_timing(lio_icp* h, int enable);
int lio_icp_get_timing(lio_icp* h, lio_kernel_timing* out);

/* ------------------------------------------------------ point overlay drawing (filled discs; offline camera leg) */
/* The output of the reference's projection tool (post_process/lidar_projection/src/lidar_projection.cpp:113-125): the
 * camera image with every projected point drawn as a filled cv::circle of 3 pixels, later points over earlier ones.
 * The contract is the library's own, exact to the bit.
 *   inputs   the colorizer's point records (n x stride float32, stride 3..8, x y z first; 0 <= n <= 2^32 - 2), a
 *            lio_camera and a pose Rt of 12 doubles, an image of height x width x 3 uint8 with a row pitch, a radius
 *            r in 0..15, an order mode, one colour source.
 *   project  lio_project_points above, with distortion and r2_max: u, v, zc and valid are its bits (one device
 *            function serves both).  The tool's float (K p) / p_z is another rounding and is NOT reproduced.
 *   centre   cxi = (int)rint(u), cyi = (int)rint(v) in double, TIES TO EVEN, which is what cv::circle does to a
 *            Point2f.  THE CENTRE IS ROUNDED ONLY AFTER THE VALIDITY TEST on the unrounded u, v: a valid point may get
 *            a centre at x == width or y == height.  THE DISC IS CLIPPED TO THE IMAGE, NEVER WRAPPED.
 *   disc     the pixel set of OpenCV's filled midpoint circle: dx = r, dy = 0, err = 0, plus = 1, minus = 2 r - 1;
 *            while dx >= dy: the rows cy +- dy take the columns cx - dx .. cx + dx and the rows cy +- dx the columns
 *            cx - dy .. cx + dy; then dy += 1; err += plus; plus += 2; if err > 0: err -= minus; dx -= 1; minus -= 2.
 *            Equivalently ONE HALF-WIDTH PER |ROW OFFSET|: r = 0: {0} (1 pixel); 1: {1, 0} (5); 2: {2, 1, 0} (13);
 *            3: {3, 2, 2, 0} (29); 4: {4, 3, 3, 2, 0} (49).  The table of the call's r is built on the host; the
 *            kernel holds no circle logic.  AGREEMENT WITH cv2.circle IS OUR READING OF ITS SOURCE AND IS UNVERIFIED:
 *            OpenCV was not available where this was written.
 *   owner    each pixel has one 64-bit key, all ones where empty.  Each drawn point i puts
 *            key_i = (hi << 32) | (0xFFFFFFFF - i) on every pixel of its clipped disc and THE MINIMUM STAYS.
 *            LIO_OVERLAY_DRAW_ORDER: hi = 0, so the highest index wins: exactly the tool's sequential loop, where
 *            later circles overwrite earlier ones.  LIO_OVERLAY_NEAREST: hi = the bits of (float)zc, rounded to
 *            nearest; zc > 0, so unsigned order is float order: the nearest point wins, and ON EQUAL FLOAT DEPTH THE
 *            HIGHER INDEX WINS.  One code path; the result does not depend on the device's schedule.
 *   colour   three bytes in the image's own channel order, NO SWIZZLE.  Exactly one source applies: per-point colours
 *            (n x 3 uint8) if set; otherwise labels (n int32) with the palette of P >= 1 rows: A POINT WITH label < 0
 *            IS NOT DRAWN AT ALL AND OWNS NOTHING, any other takes palette[label % P]; otherwise the palette's row 0
 *            for every point.  The palette starts as the one row 0 255 0: the tool as shipped draws every point green.
 *   outputs  out: each owned pixel is its owner's colour, EVERY OTHER PIXEL BYTE FOR BYTE THE INPUT'S; only 3 x width
 *            bytes of a row are read or written: the padding of the caller's rows is left untouched (out may be
 *            image).  owner_opt (may be NULL): height x width int32, the owning point's index or -1; it needs
 *            n < 2^31.  n_drawn: the number of points that were valid and not skipped by their label.
 * lio_overlay: the cloud, labels, per-point colours and palette stay on the device between frames.  set_cloud drops
 *   the labels and per-point colours of the cloud before it.  set_labels / set_colors: n is the cloud's; NULL drops
 *   the source; setting one while the other is set is LIO_ERR_ARG.  params NULL means {3, LIO_OVERLAY_DRAW_ORDER}.
 * lio_overlay_draw_undistorted: the undistorter's configured 3-channel frame is rectified and drawn on with ONE UPLOAD
 *   AND ONE DOWNLOAD; the result equals lio_undistorter_run followed by lio_overlay_draw bit for bit (the tool reads
 *   rectified images: this is its real path).  cam: the rectified image's camera, of the undistorter's output size;
 *   pitch: the raw image's.  Both handles must be on one device.
 * lio_overlay_get_timing: device ms of the last draw from stream events: upload (its staging copy included; in the
 *   chained call the undistorter's upload and gather), fill, stamp, compose, download.
 * The handle is looked at first: every entry is LIO_ERR_NODEV without a device (there is no CPU path).  LIO_ERR_ARG
 * before any device work, with a message that names the bound: a NULL out, cam, Rt, image, n_drawn, palette or ms5
 * (pts may be NULL when n == 0), a radius outside 0..15, an order that is neither mode, n < 0 or > 2^32 - 2, stride
 * outside 3..8, an n of labels or colours that is not the cloud's, rows < 1, the camera and pose conditions of
 * lio_project_points, pitch or out_pitch < 3 x width, owner_opt with n >= 2^31.  LIO_ERR_STATE: labels, colours or a
 * draw before set_cloud.  From the second frame of one size on nothing is allocated (lio_alloc_count); repeated draws
 * give identical bits.                                                                                              */
#define LIO_OVERLAY_DRAW_ORDER 0
#define LIO_OVERLAY_NEAREST 1
typedef struct lio_overlay_params {
    int32_t radius; /* 0..15; the tool: 3 */
    int32_t order;  /* LIO_OVERLAY_DRAW_ORDER (the tool) or LIO_OVERLAY_NEAREST */
} lio_overlay_params;
/* sizeof of the struct above, a third list as lio_abi_camera_struct_sizes is the second (both earlier lists are
 * closed: callers compare their lengths); returns the number of its entries.                                     */
int lio_abi_overlay_struct_sizes(int64_t* out, int n);
typedef struct lio_overlay lio_overlay;
int lio_overlay_create(int device, const lio_overlay_params* params, lio_overlay** out);
int lio_overlay_destroy(lio_overlay* h);
int lio_overlay_set_cloud(lio_overlay* h, const float* pts, int64_t n, int stride);
int lio_overlay_set_labels(lio_overlay* h, const int32_t* labels, int64_t n);
int lio_overlay_set_colors(lio_overlay* h, const uint8_t* colors, int64_t n);
int lio_overlay_set_palette(lio_overlay* h, const uint8_t* palette, int32_t rows);
int lio_overlay_draw(lio_overlay* h, const lio_camera* cam, const double* Rt, const uint8_t* image, int64_t pitch, uint8_t* out,
                     int64_t out_pitch, int32_t* owner_opt, int64_t* n_drawn);
int lio_overlay_draw_undistorted(lio_overlay* h, lio_undistorter* undistorter, const lio_camera* cam, const double* Rt,
                                 const uint8_t* raw_image, int64_t pitch, uint8_t* out, int64_t out_pitch, int32_t* owner_opt,
                                 int64_t* n_drawn);
int lio_overlay_get_timing(lio_overlay* h, double* ms5);

/* -------------------------------------------------------- exposure adaption (CLAHE on V, table remaps; camera leg) */
/* What the reference runs on every rectified frame: post_process/exposure_adaption/CLAHE_region_adjusted.py:6-41
 * (adapt_exposure: BGR -> HSV, CLAHE of V with clip 2.0 and 8 x 8 tiles, HSV -> BGR) and correct_exposure:6-103
 * (detect_exposure on the gray histogram, then equalizeHist or a 5..95 percentile stretch of V and a gamma table).
 * The contract is the library's own, exact to the bit.  All float operations are IEEE float32, rounded one at a
 * time, in the order written, nothing fused; rint is TIES TO EVEN; sat clamps to 0..255.  AGREEMENT WITH cv2 IS OUR
 * READING OF ITS SOURCE AND IS UNVERIFIED: OpenCV was not available where this was written.
 *   images   uint8, channels 1 or 3, width and height in 1..32767, rows of `pitch` bytes.  Only channels x width
 *            bytes of a row are read or written: the output's padding bytes are left untouched.
 *   order    0 = B G R (what cv2.imread gives), 1 = R G B.  It only says which byte is r and which is b below; the
 *            output has the input's order.
 *   BGR -> HSV  (our reading of OpenCV's 8-bit path, hsv_shift = 12, H range 180, all integer)
 *            sdiv[i] = rint((255 << 12) / i), hdiv[i] = rint((180 << 12) / (6 i)) for i = 1..255, computed in double;
 *            sdiv[0] = hdiv[0] = 0.  v = max(b, g, r); vmin = min(b, g, r); d = v - vmin;
 *            s = (d sdiv[v] + 2048) >> 12;
 *            h0 = g - b if v == r, else b - r + 2 d if v == g, else r - g + 4 d;
 *            h = (h0 hdiv[d] + 2048) >> 12 (arithmetic shift); if h < 0, h += 180.  h is in 0..179.
 *            With 1 channel V is the pixel itself and no conversion is made.
 *   HSV -> BGR  (our reading of OpenCV's float path behind the 8-bit entry)
 *            hs = 0x1.111112p-5f (the float nearest 1/30), k = 0x1.010102p-8f (the float nearest 1/255);
 *            hf = (float)h hs; sf = (float)s k; vf = (float)v k.  If s == 0: b = g = r = vf.  Otherwise
 *            sec = floor(hf); f = hf - (float)sec; if sec >= 6: sec = 0, f = 0;
 *            t0 = vf; t1 = vf (1 - sf); t2 = vf (1 - sf f); t3 = vf (1 - sf (1 - f));
 *            (b, g, r) = t[...] by sector: {1,3,0} {1,0,2} {3,0,1} {0,2,1} {0,1,3} {2,1,0}.
 *            Each output channel is sat(rint(x 255.0f)).
 *   CLAHE of a plane  (our reading of OpenCV's clahe.cpp; clip_limit double, tiles_x and tiles_y in 1..64)
 *     padding  if W % tiles_x == 0 and H % tiles_y == 0 the extended plane is the plane.  Otherwise it is padded on
 *              the right by tiles_x - W % tiles_x columns and at the bottom by tiles_y - H % tiles_y rows: A DIMENSION
 *              THAT DIVIDES EVENLY IS THEN PADDED BY A WHOLE tiles_x OR tiles_y (OpenCV's quirk, kept).  The border is
 *              REFLECT_101: x >= W reads 2 (W - 1) - x.  A pad larger than the dimension - 1 is LIO_ERR_ARG.
 *     tiles    tw = extW / tiles_x; th = extH / tiles_y; area = tw th.
 *     clip     clip = 0 if clip_limit <= 0; otherwise clip = max((int)(clip_limit area / 256), 1), computed in double;
 *              NaN, or a value >= 2^31, is LIO_ERR_ARG.
 *     per tile a 256-bin histogram of the tile of the extended plane (reflected pixels count).  If clip > 0:
 *              excess = sum max(hist - clip, 0); hist = min(hist, clip); batch = excess / 256; res = excess - 256
 *              batch; every bin gains batch; if res > 0: step = max(256 / res, 1) and bin k gets one more iff k % step
 *              == 0 and k / step < res (the closed form of OpenCV's loop).  lut[i] = sat(rint((float)cum[i] scale)),
 *              cum the inclusive prefix sum, scale = 255.0f / (float)area.
 *     apply    per pixel (x, y) of the unpadded plane, p = plane[y][x]:
 *              txf = (float)x (1.0f / (float)tw) - 0.5f; tx1 = floor(txf); xa = txf - (float)tx1; xa1 = 1 - xa; then
 *              tx2 = min(tx1 + 1, tiles_x - 1) and tx1 = max(tx1, 0); rows likewise with th;
 *              res = (L[ty1][tx1][p] xa1 + L[ty1][tx2][p] xa) ya1 + (L[ty2][tx1][p] xa1 + L[ty2][tx2][p] xa) ya;
 *              out = sat(rint(res)).
 *   gray     (detect_exposure only; our reading of OpenCV 4's 15-bit path)
 *            gray = (3735 b + 19235 g + 9798 r + 16384) >> 15.
 * The script's v / 255 -> clip -> * 255 -> uint8 step in float32 is the identity on 0..255 and is not performed.
 *
 * lio_exposure_histograms: 256 int64 each (either may be NULL): hist_v of V (the channel maximum; with 1 channel the
 *   plane), hist_gray of gray (with 1 channel the plane).
 * lio_exposure_clahe: 1 channel: CLAHE of the plane.  3 channels: adapt_exposure: BGR -> HSV, CLAHE of V, H and S
 *   unchanged, HSV -> BGR.
 * lio_exposure_remap: 3 channels with lut_v: the HSV round trip with V = lut_v[V]; then, if lut_all is given, every
 *   channel goes through it (the gamma step).  lut_v NULL: no round trip, a plain cv2.LUT.  1 channel: lut_v, then
 *   lut_all, on the plane.  Each table is 256 uint8.  Both NULL is LIO_ERR_ARG.
 * lio_exposure_clahe_undistorted: the undistorter's configured frame is rectified and adapted with ONE UPLOAD AND ONE
 *   DOWNLOAD; the result equals lio_undistorter_run followed by lio_exposure_clahe bit for bit.  Both handles must
 *   be on one device (LIO_ERR_ARG); LIO_ERR_STATE before lio_undistorter_set_camera.  The undistorter must not be in
 *   use by another thread meanwhile.
 * lio_exposure_get_timing: device ms of the last run from stream events: upload (its staging copy included; in the
 *   chained call the undistorter's upload and gather), histogram, LUT, apply, download.
 * LIO_ERR_ARG before any device work, with a message that names the bound: a NULL image, out, raw_image or ms5, a
 * width or height outside 1..32767, channels not 1 or 3, order not 0 or 1, tiles_x or tiles_y outside 1..64, pitch or
 * out_pitch < channels x width, the padding bound and the clip bounds above, both tables NULL.  The checks that need
 * no handle are made before the handle is looked at.  There is no CPU path: LIO_ERR_NODEV without a device.  From the
 * second frame of one size on nothing is allocated (lio_alloc_count); repeated runs give identical bits.          */
typedef struct lio_exposure lio_exposure;
int lio_exposure_create(int device, lio_exposure** out);
int lio_exposure_destroy(lio_exposure* h);
int lio_exposure_histograms(lio_exposure* h, const uint8_t* image, int width, int height, int channels, int64_t pitch,
                            int order, int64_t* hist_v_opt, int64_t* hist_gray_opt);
int lio_exposure_clahe(lio_exposure* h, const uint8_t* image, int width, int height, int channels, int64_t pitch, int order,
                       double clip_limit, int tiles_x, int tiles_y, uint8_t* out, int64_t out_pitch);
int lio_exposure_remap(lio_exposure* h, const uint8_t* image, int width, int height, int channels, int64_t pitch, int order,
                       const uint8_t* lut_v_opt, const uint8_t* lut_all_opt, uint8_t* out, int64_t out_pitch);
int lio_exposure_clahe_undistorted(lio_exposure* h, lio_undistorter* undistorter, const uint8_t* raw_image, int64_t pitch,
                                   int order, double clip_limit, int tiles_x, int tiles_y, uint8_t* out, int64_t out_pitch);
int lio_exposure_get_timing(lio_exposure* h, double* ms5);

/* ------------------------------ overexposure recovery and the 8-bit Gaussian blur (stencils on a lio_exposure) */
/* The third script of post_process/exposure_adaption: solve_overexposure:6-32 (recover_overexposure: BGR -> HSV, a
 * mask V > 200, cv2.dilate of it with a 5 x 5 block of ones, cv2.GaussianBlur(v, (15, 15), 0), np.where(mask > 0,
 * blurred_v, v), the new V merged with the old H and S, HSV -> BGR), and cv2.GaussianBlur of an 8-bit image as a call
 * of its own.  The contract is the library's own, integer-only on the device and exact to the bit; it is our reading
 * of OpenCV 4's 8-bit paths (ufixedpoint16 rows, ufixedpoint32 columns).  AGREEMENT WITH cv2 IS OUR READING OF ITS
 * SOURCE AND IS UNVERIFIED: OpenCV was not available where this was written.
 *   images, order, pitches   exactly those of lio_exposure_* above: uint8, channels 1 or 3, width and height in
 *            1..32767, only channels x width bytes of a row read or written.
 *   V        max(b, g, r); with 1 channel the pixel itself.
 *   mask     m0(x, y) = V(x, y) > threshold, STRICT, threshold in 0..255 (script: 200).  rd = (dilate - 1) / 2, dilate
 *            ODD in 1..15 (script: 5).  M(x, y) = OR of m0 over |dx| <= rd, |dy| <= rd, taken ONLY OVER POSITIONS
 *            INSIDE THE IMAGE (cv2.dilate's default constant border, which never wins a maximum).
 *   weights  lio_gaussian_weights: k = ksize uint16 values with 8 fractional bits that SUM TO 256, computed on the host;
 *            ksize ODD in 1..31 (script: 15), sigma a double (script: 0), NaN or +-inf is LIO_ERR_ARG.
 *            If sigma <= 0 and k <= 7, g is OpenCV's fixed table: {1}, {.25, .5, .25}, {.0625, .25, .375, .25, .0625},
 *            {.03125, .109375, .21875, .28125, .21875, .109375, .03125}.  Otherwise, all in double:
 *            s = sigma > 0 ? sigma : ((k - 1) 0.5 - 1) 0.3 + 0.8; x = i - (k - 1) 0.5;
 *            t[i] = exp(((-0.5 / (s s)) x) x); g[i] = t[i] (1 / sum t), the sum taken from i = 0 up.
 *            Fixed point with error diffusion over the left half, err = 0 at the start; for i = 0 .. k / 2 - 1:
 *            a = g[i] 256 + err; w[i] = w[k - 1 - i] = rint(a), TIES TO EVEN; err = a - w[i].
 *            Then w[k / 2] = 256 - 2 sum w[i].  k = 15, sigma = 0 gives 1 3 6 12 20 30 36 40 36 30 20 12 6 3 1.
 *            The device only ever sees these integers.
 *   blur     r = k / 2.  Hrow(x, y) = sum_j w[j] V(refl(x + j - r, W), y), at most 65 280: it fits 16 bits.
 *            B(x, y) = (sum_j w[j] Hrow(x, refl(y + j - r, H)) + 32768) >> 16.
 *            refl is REFLECT_101 APPLIED UNTIL THE INDEX IS IN RANGE: n == 1: 0; otherwise q = p mod 2 (n - 1)
 *            (non-negative) and refl = q < n ? q : 2 (n - 1) - q.  An image narrower than the radius is legal.
 *   blend    V' = M ? B : V.
 *   output   3 channels: (h, s) from the BGR -> HSV above of the pixel, then the HSV -> BGR above of (h, s, V') ON
 *            EVERY PIXEL, MASKED OR NOT (the script round-trips the whole frame, and the round trip is lossy).
 *            1 channel: V'.
 *
 * lio_gaussian_weights: ksize values to w.  Host only: it needs no device and no handle.
 * lio_exposure_gaussian_blur: the blur above on each channel of a 1- or 3-channel image, as cv2.GaussianBlur(img,
 *   (k, k), sigma): a square kernel, one sigma for both axes.  ksize 1 is the identity.
 * lio_exposure_recover: the recovery.  p_opt NULL means the script's {200, 5, 15, 0}.
 * lio_exposure_recover_undistorted: the undistorter's configured frame is rectified and recovered with ONE UPLOAD AND
 *   ONE DOWNLOAD; the result equals lio_undistorter_run followed by lio_exposure_recover bit for bit.  The device and
 *   state rules are those of lio_exposure_clahe_undistorted.
 * lio_exposure_get_stencil_timing: device ms of the last of the three calls above from stream events: upload (its
 *   staging copy included; in the chained call the undistorter's upload and gather), the kernel, download.
 *   lio_exposure_get_timing and its five stages are those of the earlier calls alone.
 * LIO_ERR_ARG before any device work, with a message that names the bound: the image bounds of lio_exposure_*, a NULL
 * image, out, raw_image, w or ms3, a threshold outside 0..255, a dilate even or outside 1..15, a ksize even or outside
 * 1..31, a sigma that is not finite, pitch or out_pitch < channels x width.  The checks that need no handle are made
 * before the handle is looked at.  There is no CPU path: LIO_ERR_NODEV without a device.  From the second frame of
 * one size on nothing is allocated (lio_alloc_count); repeated runs give identical bits.                          */
struct lio_recover_params {
    int threshold; /* 0..255; the script: 200 */
    int dilate;    /* odd, 1..15; the script: 5 */
    int ksize;     /* odd, 1..31; the script: 15 */
    double sigma;  /* <= 0: from ksize; the script: 0 */
};
typedef struct lio_recover_params lio_recover_params;
int lio_gaussian_weights(int ksize, double sigma, uint16_t* w);
int lio_exposure_gaussian_blur(lio_exposure* h, const uint8_t* image, int width, int height, int channels, int64_t pitch,
                               int ksize, double sigma, uint8_t* out, int64_t out_pitch);
int lio_exposure_recover(lio_exposure* h, const uint8_t* image, int width, int height, int channels, int64_t pitch, int order,
                         const lio_recover_params* p_opt, uint8_t* out, int64_t out_pitch);
int lio_exposure_recover_undistorted(lio_exposure* h, lio_undistorter* undistorter, const uint8_t* raw_image, int64_t pitch,
                                     int order, const lio_recover_params* p_opt, uint8_t* out, int64_t out_pitch);
int lio_exposure_get_stencil_timing(lio_exposure* h, double* ms3);

#ifdef __cplusplus
}
#endif
#endif /* LIO_GPU_H */
