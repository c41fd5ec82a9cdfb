// lio_capi_scan.cpp — the C-ABI (include/lio_gpu.h) of the h_share_model context: create / destroy, the scan's
// buffers (lio_scan_set*, lio_scan_bind_device), lio_match and the IESKF update that iterates it, lio_map_incremental
// on the scan's kNN lists, the readers (lio_get_*) and the kernel timing.  make_args, read_result, wait_result and
// match_impl are one translation unit with lio_match and lio_ieskf_update: the per-evaluation path inlines them.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>

#include "ieskf.hpp"
#include "lio_capi_online.hpp"

using namespace lio::capi;

// everything a context owns (a context that lio_ctx_create could only half build included)
static void ctx_free(lio_ctx& c) {
    lio::dev_free(&c.d_body, &c.d_nn, &c.d_planes, &c.d_sel, &c.d_partials, &c.d_sums, &c.d_rows, &c.d_nrows,
                  &c.d_far_q, &c.d_far_count, &c.d_done, &c.d_d5, &c.d_dbg, &c.d_raw,
                  &c.d_rec, &c.d_poses, &c.d_kf);
    lio::host_free(&c.h_sums);
    for (hipEvent_t* e : {&c.ev_main.a, &c.ev_main.b, &c.ev_fin.a, &c.ev_fin.b})
        if (*e) (void)hipEventDestroy(*e);
    for (hipEvent_t e : c.ev_marks)
        if (e) (void)hipEventDestroy(e);
    lio::filter_free(c.filt);
}

int lio::capi::ctx_reserve(lio_ctx* c, int64_t n) {
    // the five are allocated all or nothing, so d_body stands for all of them (a capacity of 0 leaves it null too)
    if (n > c->cap || !c->d_body) {
        const int64_t cap = std::max<int64_t>(n, c->cap + c->cap / 2);
        c->cap = 0;  // a failed reallocation below leaves no buffer that looks usable
        if (lio::dev_alloc_all({lio::dev_req(c->d_body, cap * 3), lio::dev_req(c->d_nn, cap * 5),
                                lio::dev_req(c->d_planes, cap), lio::dev_req(c->d_sel, cap + 64),
                                lio::dev_req(c->d_d5, cap)}))
            return fail(LIO_ERR_NOMEM, "scan buffers: hipMalloc failed");
        c->cap = cap;
    }
    int rc = grow(&c->d_partials, c->part_cap, (int64_t)lio::match_blocks((int)n) * 32 + 32);
    if (rc) return rc;
    rc = grow(&c->d_far_q, c->far_cap, lio::far_entries(n));  // every query may be queued
    if (rc) return rc;
    c->n = n;
    c->body_ext = nullptr;
    c->have_eval = false;
    c->knn_valid = false;
    return LIO_OK;
}

extern "C" {

int lio_ctx_create(lio_map* m, const lio_match_params* p, lio_ctx** out) {
    if (!m || !out) return fail(LIO_ERR_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(m->dev));
    auto* c = new lio_ctx();
    c->map = m;
    ++m->n_ctx;
    if (p)
        c->p = *p;
    else
        c->p = lio_match_params{5.0f, 0.1f, 0.9, 0.9};
    if (hipMalloc(&c->d_sums, 32 * sizeof(double)) != hipSuccess ||
        hipHostMalloc(&c->h_sums, 40 * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&c->h_sums_dev), c->h_sums, 0) != hipSuccess ||
        hipMalloc(&c->d_nrows, sizeof(int64_t)) != hipSuccess ||
        hipMalloc(&c->d_far_count, sizeof(int)) != hipSuccess ||
        hipMemsetAsync(c->d_far_count, 0, sizeof(int), m->st) != hipSuccess || hipMalloc(&c->d_done, 64) != hipSuccess ||
        hipMemsetAsync(c->d_done, 0, 64, m->st) != hipSuccess) {  // on the map's stream: it does not wait for the null stream
        --m->n_ctx;
        ctx_free(*c);
        delete c;
        return fail(LIO_ERR_NOMEM, "context allocation failed");
    }
    for (EventPair* e : {&c->ev_main, &c->ev_fin}) {
        (void)hipEventCreate(&e->a);
        (void)hipEventCreate(&e->b);
    }
    for (hipEvent_t& e : c->ev_marks) (void)hipEventCreate(&e);
    *out = c;
    return LIO_OK;
}

int lio_ctx_destroy(lio_ctx* c) {
    if (!c) return LIO_OK;
    (void)hipSetDevice(c->map->dev);
    (void)hipStreamSynchronize(c->map->st);
    ctx_free(*c);
    --c->map->n_ctx;
    delete c;
    return LIO_OK;
}

int lio_scan_set(lio_ctx* c, const float* body, int64_t n) {
    if (!c || n < 0 || (n > 0 && !body) || n >= (int64_t)1 << 30) return fail(LIO_ERR_ARG, "lio_scan_set: bad arguments");
    HIP_TRY(hipSetDevice(c->map->dev));
    int rc = ctx_reserve(c, n);
    if (rc) return rc;
    if (n) HIP_TRY(hipMemcpyAsync(c->d_body, body, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, c->map->st));
    return LIO_OK;
}

int lio_scan_set_device(lio_ctx* c, const float* d_body, int64_t n) {
    if (!c || n < 0 || (n > 0 && !d_body) || n >= (int64_t)1 << 30) return fail(LIO_ERR_ARG, "lio_scan_set_device: bad arguments");
    HIP_TRY(hipSetDevice(c->map->dev));
    int rc = ctx_reserve(c, n);
    if (rc) return rc;
    if (n)
        HIP_TRY(hipMemcpyAsync(c->d_body, d_body, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToDevice, c->map->st));
    return LIO_OK;
}

int lio_scan_bind_device(lio_ctx* c, const float* d_body, int64_t n) {
    if (!c || n < 0 || (n > 0 && !d_body) || n >= (int64_t)1 << 30) return fail(LIO_ERR_ARG, "lio_scan_bind_device: bad arguments");
    HIP_TRY(hipSetDevice(c->map->dev));
    int rc = ctx_reserve(c, n);
    if (rc) return rc;
    c->body_ext = n ? d_body : nullptr;
    return LIO_OK;
}

static_assert(sizeof(lio_pose) == sizeof(lio::PoseArg), "lio_pose / PoseArg layout");

static lio::MatchArgs make_args(lio_ctx* c, const lio_pose& pose_in) {
    lio::MatchArgs a{};
    const lio_pose pose = filled(pose_in);
    std::memcpy(&a.pose, &pose, sizeof(lio::PoseArg));
    a.grid = lio::grid_view(c->map->grid);
    a.body = body_ptr(c);
    a.map_by_id = c->map->grid.by_id;
    a.nn_idx = c->d_nn;
    a.nn_d5 = c->d_d5;
    a.seed_scale = c->seed_scale;
    a.planes = c->d_planes;
    a.sel = c->d_sel;
    a.partials = c->d_partials;
    a.n = (int)c->n;
    // every point with d2 <= range lies within ceil(sqrt(range)/cell)+1 shells
    a.max_shell = (int)std::ceil(std::sqrt((double)c->p.knn_range_sq) / a.grid.cell) + 1;
    a.dbg = nullptr;
    a.sums_out = c->h_sums_dev;
    a.seq_out = reinterpret_cast<unsigned long long*>(c->h_sums_dev + 32);
    a.seq = 0;
    a.far_q = c->d_far_q;
    a.far_count = c->d_far_count;
    a.done_count = c->d_done;
    a.range_sq = c->p.knn_range_sq;
    a.plane_thr = c->p.plane_thr;
    a.s_coef = c->p.s_coef;
    a.s_gate = c->p.s_gate;
    return a;
}

static void accum_event(EventPair& e, int64_t& launches, double& ms) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, e.a, e.b) == hipSuccess) {
        ms += t;
        ++launches;
    }
}

// Wait until the evaluation's last block has published sequence number `seq`
// (zero-copy result, no copy / stream-sync round trip).  The GPU stores the
// sums, the number and a checksum of both unordered (lio_match.hip
// publish_host), so a result counts only when the number matches AND the
// sums read after it hash to the checksum; once the stream is idle every word
// has landed, so a stream error, or an idle stream whose words still do not
// match, ends the wait with an error.
static uint64_t mix64(uint64_t z) {  // splitmix64 finaliser, as publish_host
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static bool read_result(const lio_ctx* c, unsigned long long seq, double* sums) {
    const volatile uint64_t* w = reinterpret_cast<const volatile uint64_t*>(c->h_sums);
    if (w[32] != seq) return false;
    uint64_t h = 0, bits[LIO_SUMS_LEN];
    for (int l = 0; l < LIO_SUMS_LEN; ++l) {
        bits[l] = w[l];
        h ^= mix64(bits[l] ^ ((uint64_t)l * 0x9e3779b97f4a7c15ull));
    }
    if ((h ^ mix64(seq)) != w[33]) return false;
    std::memcpy(sums, bits, sizeof(bits));
    return true;
}

// The fast path is one cached load per spin.  The stream is queried by elapsed time, not by spin count: first
// kFirstQuery after the launch (longer than a healthy evaluation at the usual scan sizes, so a result that is
// about to land never waits behind a runtime call), then every kQueryPeriod.
static int wait_result(lio_ctx* c, unsigned long long seq, double* sums, std::chrono::steady_clock::time_point launched) {
    constexpr std::chrono::microseconds kFirstQuery{80}, kQueryPeriod{50};
    auto next = launched + kFirstQuery;
    for (uint64_t it = 0;; ++it) {
        if (read_result(c, seq, sums)) return LIO_OK;
        if ((it & 63) != 63) continue;  // the clock itself every 64 spins
        const auto now = std::chrono::steady_clock::now();
        if (now < next) continue;
        next = now + kQueryPeriod;
        const hipError_t e = hipStreamQuery(c->map->st);
        if (e != hipSuccess && e != hipErrorNotReady)
            return fail(LIO_ERR_HIP, std::string("lio_match: ") + hipGetErrorString(e));
        if (e == hipSuccess && !read_result(c, seq, sums))
            return fail(LIO_ERR_HIP, "lio_match: evaluation produced no result");
    }
}

static int match_impl(lio_ctx* c, const lio_pose* pose_in, int redo_knn, double* sums);

int lio_match(lio_ctx* c, const lio_pose* pose_in, int redo_knn, double* sums) {
    if (!c || !pose_in || !sums) return fail(LIO_ERR_ARG, "lio_match: bad arguments");
    return match_impl(c, pose_in, redo_knn, sums);
}

static int match_impl(lio_ctx* c, const lio_pose* pose_in, int redo_knn, double* sums) {
    const lio_pose pose_f = filled(*pose_in);
    const lio_pose* pose = &pose_f;
    if (c->map->grid.n_ids == 0) return fail(LIO_ERR_STATE, "lio_match: map is empty (call lio_map_build)");
    if (!redo_knn && !c->knn_valid) return fail(LIO_ERR_STATE, "lio_match: redo_knn=0 before any kNN evaluation");
    if (!redo_knn && c->knn_map_version != c->map->version)
        return fail(LIO_ERR_STATE, "lio_match: redo_knn=0 but the map changed since this scan's kNN evaluation");
    HIP_TRY(hipSetDevice(c->map->dev));
    hipStream_t st = c->map->st;
    lio::MatchArgs a = make_args(c, *pose);
    if (c->map->n == 0 && c->n > 0) {
        // every map point deleted (Delete_Point_Boxes): Nearest_Search finds
        // nothing, no point is effective ("No Effective Points!")
        HIP_TRY(hipMemsetAsync(c->d_nn, 0xff, c->n * 5 * sizeof(int32_t), st));
        HIP_TRY(hipMemsetAsync(c->d_sel, 0, c->n, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (c->n == 0 || c->map->n == 0) {
        std::memset(sums, 0, LIO_SUMS_LEN * sizeof(double));
        c->last_pose = *pose;
        c->have_eval = true;
        c->knn_valid = true;
        c->knn_map_version = c->map->version;
        c->knn_pose = *pose;
        return LIO_OK;
    }
    a.seq = ++c->seq;
    // later kNN evaluations of the same scan against the same map start from the previous lists
    a.prior = (redo_knn && c->knn_valid && c->knn_map_version == c->map->version) ? 1 : 0;
    const auto t0 = std::chrono::steady_clock::now();
    if (c->timing) HIP_TRY(hipEventRecord(c->ev_main.a, st));
    lio::launch_h_model(a, redo_knn != 0, st, c->timing ? c->ev_marks : nullptr);
    if (c->timing) HIP_TRY(hipEventRecord(c->ev_main.b, st));
    HIP_TRY(hipGetLastError());
    const auto t1 = std::chrono::steady_clock::now();
    int rc = wait_result(c, a.seq, sums, t1);
    if (rc) return rc;
    const auto t2 = std::chrono::steady_clock::now();
    c->last_launch_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    c->last_wait_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
    if (c->timing) {
        HIP_TRY(hipEventSynchronize(c->ev_main.b));
        if (redo_knn) {  // kernel spans (hipExtLaunchKernel events): no launch gaps, as rocprofv3 reports
            const double before = c->tm.near_ms + c->tm.far_ms + c->tm.plane_ms;
            EventPair n{c->ev_marks[0], c->ev_marks[1]}, f{c->ev_marks[2], c->ev_marks[3]},
                p{c->ev_marks[4], c->ev_marks[5]};
            accum_event(n, c->tm.near_launches, c->tm.near_ms);
            if (a.max_shell > 1) accum_event(f, c->tm.far_launches, c->tm.far_ms);
            accum_event(p, c->tm.plane_launches, c->tm.plane_ms);
            c->tm.knn_ms += (c->tm.near_ms + c->tm.far_ms + c->tm.plane_ms) - before;
            ++c->tm.knn_launches;
        } else {
            EventPair r{c->ev_marks[6], c->ev_marks[7]};
            accum_event(r, c->tm.reuse_launches, c->tm.reuse_ms);
        }
    }
    c->last_pose = *pose;
    c->have_eval = true;
    if (redo_knn) {
        c->knn_valid = true;
        c->knn_map_version = c->map->version;
        c->knn_pose = *pose;
    }
    return LIO_OK;
}

int lio_ctx_knn_stats(lio_ctx* c, const lio_pose* pose, double* sums, int32_t* stats3) {
    if (!c || !pose || !sums || !stats3) return fail(LIO_ERR_ARG, "lio_ctx_knn_stats: bad arguments");
    if (c->map->n == 0) return fail(LIO_ERR_STATE, "lio_ctx_knn_stats: map is empty");
    HIP_TRY(hipSetDevice(c->map->dev));
    hipStream_t st = c->map->st;
    if (c->n == 0) return LIO_OK;
    static_assert(sizeof(int) == sizeof(float), "the debug scratch holds either");
    int rc = grow(&c->d_dbg, c->dbg_cap, c->n * 3);
    if (rc) return rc;
    lio::MatchArgs a = make_args(c, *pose);
    a.dbg = reinterpret_cast<int*>(c->d_dbg);
    a.seq = ++c->seq;
    lio::launch_h_model(a, true, st);
    hipError_t e2 = hipMemcpyAsync(stats3, c->d_dbg, c->n * 3 * sizeof(int), hipMemcpyDeviceToHost, st);
    hipError_t e3 = hipStreamSynchronize(st);
    if (e2 != hipSuccess || e3 != hipSuccess) return fail(LIO_ERR_HIP, "lio_ctx_knn_stats failed");
    rc = wait_result(c, a.seq, sums, std::chrono::steady_clock::now());
    if (rc) return rc;
    c->last_pose = *pose;
    c->knn_pose = *pose;
    c->have_eval = true;
    c->knn_valid = true;
    c->knn_map_version = c->map->version;
    return LIO_OK;
}

int lio_ctx_get_knn_pose(lio_ctx* c, lio_pose* out) {
    if (!c || !out) return fail(LIO_ERR_ARG, "bad arguments");
    if (!c->knn_valid) return fail(LIO_ERR_STATE, "lio_ctx_get_knn_pose: no kNN evaluation");
    *out = c->knn_pose;
    return LIO_OK;
}

int lio_map_incremental(lio_ctx* c, const lio_pose* pose, double filter_size_map, lio_incremental_stats* st) {
    if (!c || !pose || !(filter_size_map > 0.0)) return fail(LIO_ERR_ARG, "lio_map_incremental: bad arguments");
    if (c->n > 0 && !c->knn_valid && c->map->n > 0)
        return fail(LIO_ERR_STATE, "lio_map_incremental: no kNN evaluation for this scan (Nearest_Points)");
    if (c->n > 0 && c->map->n > 0 && c->knn_map_version != c->map->version)
        return fail(LIO_ERR_STATE, "lio_map_incremental: the map changed since this scan's kNN evaluation");
    lio_map* m = c->map;
    HIP_TRY(hipSetDevice(m->dev));
    lio::IncrArgs a{};
    const lio_pose pf = filled(*pose);
    std::memcpy(&a.pose, &pf, sizeof(lio::PoseArg));
    const lio_pose pk = filled(c->knn_pose);
    std::memcpy(&a.pose_knn, &pk, sizeof(lio::PoseArg));
    a.body = body_ptr(c);
    a.nn_idx = c->d_nn;
    a.n = (int)c->n;
    a.fs = filter_size_map;
    a.range_sq = c->p.knn_range_sq;
    int64_t out[4] = {0, 0, 0, 0};
    int rc = 0;
    if (m->grid.n_ids == 0) {  // ikdtree.Build on the first scan is the caller's job (lio_map_build)
        return fail(LIO_ERR_STATE, "lio_map_incremental: map is empty (build it from the first scan)");
    }
    rc = lio::map_incremental(m->grid, m->upd, a, m->p.downsample_size, map_slack(m), out, m->st);
    HIP_TRY(hipStreamSynchronize(m->st));
    m->n = m->grid.n;
    ++m->version;
    c->knn_valid = false;  // ids/grid changed
    if (st) {
        st->n_to_add = out[0];
        st->n_no_downsample = out[1];
        st->n_skipped = out[2];
        st->n_added_downsample = out[3];
    }
    return status(rc, "lio_map_incremental", "invalid points");
}

// One of launch_debug's three outputs at the last evaluation's pose, through the context's debug scratch, on the
// host when it returns: per point 3 floats of the world position, the 5 neighbour d2 or the plane's 4.
enum DebugOut { kDbgWorld = 3, kDbgD2 = 5, kDbgPlanes = 4 };
static int read_debug(lio_ctx* c, DebugOut which, float* out, const char* what) {
    const int64_t count = c->n * (int)which;
    int rc = grow(&c->d_dbg, c->dbg_cap, count);
    if (rc) return rc;
    float* d = c->d_dbg;
    hipStream_t st = c->map->st;
    lio::launch_debug(make_args(c, c->last_pose), which == kDbgWorld ? d : nullptr, which == kDbgD2 ? d : nullptr,
                      which == kDbgPlanes ? d : nullptr, st);
    hipError_t e = hipMemcpyAsync(out, d, count * sizeof(float), hipMemcpyDeviceToHost, st);
    (void)hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(LIO_ERR_HIP, std::string(what) + " copy failed");
    return LIO_OK;
}

int lio_get_knn(lio_ctx* c, int32_t* idx, float* d2) {
    if (!c || !c->have_eval) return fail(LIO_ERR_STATE, "lio_get_knn: no evaluation yet");
    HIP_TRY(hipSetDevice(c->map->dev));
    hipStream_t st = c->map->st;
    if (c->n == 0) return LIO_OK;
    if (idx) HIP_TRY(hipMemcpyAsync(idx, c->d_nn, c->n * 5 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (d2)
        if (int rc = read_debug(c, kDbgD2, d2, "lio_get_knn")) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return LIO_OK;
}

int lio_get_planes(lio_ctx* c, float* abcd_pd2, uint8_t* sel) {
    if (!c || !c->have_eval) return fail(LIO_ERR_STATE, "lio_get_planes: no evaluation yet");
    HIP_TRY(hipSetDevice(c->map->dev));
    hipStream_t st = c->map->st;
    if (c->n == 0) return LIO_OK;
    if (sel) HIP_TRY(hipMemcpyAsync(sel, c->d_sel, c->n, hipMemcpyDeviceToHost, st));
    if (abcd_pd2)
        if (int rc = read_debug(c, kDbgPlanes, abcd_pd2, "lio_get_planes")) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return LIO_OK;
}

int lio_get_world(lio_ctx* c, float* world) {
    if (!c || !world || !c->have_eval) return fail(LIO_ERR_STATE, "lio_get_world: no evaluation yet");
    HIP_TRY(hipSetDevice(c->map->dev));
    if (c->n == 0) return LIO_OK;
    return read_debug(c, kDbgWorld, world, "lio_get_world");
}

int lio_get_h_rows(lio_ctx* c, double* rows, int64_t max_rows, int64_t* n_rows) {
    if (!c || !n_rows || (max_rows > 0 && !rows)) return fail(LIO_ERR_ARG, "lio_get_h_rows: bad arguments");
    if (!c->have_eval) return fail(LIO_ERR_STATE, "lio_get_h_rows: no evaluation yet");
    HIP_TRY(hipSetDevice(c->map->dev));
    hipStream_t st = c->map->st;
    int rc = grow(&c->d_rows, c->rows_cap, std::max<int64_t>(max_rows, 1) * 7);
    if (rc) return rc;
    lio::launch_h_rows(make_args(c, c->last_pose), c->d_rows, max_rows, c->d_nrows, st);
    int64_t nr = 0;
    HIP_TRY(hipMemcpyAsync(&nr, c->d_nrows, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t ncopy = std::min(nr, max_rows);
    if (ncopy > 0) {
        HIP_TRY(hipMemcpyAsync(rows, c->d_rows, ncopy * 7 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    *n_rows = nr;
    return LIO_OK;
}

// =============================================================================
// IESKF
// =============================================================================
static lio::host::State to_host(const lio_state& s) {
    lio::host::State x;
    std::memcpy(x.pos, s.pos, sizeof(x.pos));
    x.rot = {s.rot[0], s.rot[1], s.rot[2], s.rot[3]};
    x.offR = {s.offset_R_L_I[0], s.offset_R_L_I[1], s.offset_R_L_I[2], s.offset_R_L_I[3]};
    std::memcpy(x.offT, s.offset_T_L_I, sizeof(x.offT));
    std::memcpy(x.vel, s.vel, sizeof(x.vel));
    std::memcpy(x.bg, s.bg, sizeof(x.bg));
    std::memcpy(x.ba, s.ba, sizeof(x.ba));
    std::memcpy(x.grav, s.grav, sizeof(x.grav));
    return x;
}
static void from_host(const lio::host::State& x, lio_state& s) {
    std::memcpy(s.pos, x.pos, sizeof(x.pos));
    s.rot[0] = x.rot.w; s.rot[1] = x.rot.x; s.rot[2] = x.rot.y; s.rot[3] = x.rot.z;
    s.offset_R_L_I[0] = x.offR.w; s.offset_R_L_I[1] = x.offR.x; s.offset_R_L_I[2] = x.offR.y; s.offset_R_L_I[3] = x.offR.z;
    std::memcpy(s.offset_T_L_I, x.offT, sizeof(x.offT));
    std::memcpy(s.vel, x.vel, sizeof(x.vel));
    std::memcpy(s.bg, x.bg, sizeof(x.bg));
    std::memcpy(s.ba, x.ba, sizeof(x.ba));
    std::memcpy(s.grav, x.grav, sizeof(x.grav));
}

static lio_pose state_pose(const lio::host::State& s) {  // the pose an evaluation at state s uses
    lio_pose pose;
    lio::host::quat_to_mat(s.rot, pose.R);
    lio::host::quat_to_mat(s.offR, pose.R_LI);
    pose.q[0] = s.rot.w, pose.q[1] = s.rot.x, pose.q[2] = s.rot.y, pose.q[3] = s.rot.z;
    pose.q_LI[0] = s.offR.w, pose.q_LI[1] = s.offR.x, pose.q_LI[2] = s.offR.y, pose.q_LI[3] = s.offR.z;
    std::memcpy(pose.t, s.pos, sizeof(pose.t));
    std::memcpy(pose.t_LI, s.offT, sizeof(pose.t_LI));
    return pose;
}

int lio_ctx_set_seed_scale(lio_ctx* c, float scale) {
    if (!c || !(scale > 0.f && scale <= 1.f)) return fail(LIO_ERR_ARG, "lio_ctx_set_seed_scale: scale in (0, 1]");
    c->seed_scale = scale;
    return LIO_OK;
}

int lio_ieskf_update(lio_ctx* c, lio_state* xs, double* P, const lio_ieskf_params* p, lio_ieskf_stats* st) {
    if (!c || !xs || !P) return fail(LIO_ERR_ARG, "lio_ieskf_update: bad arguments");
    const auto t_call = std::chrono::steady_clock::now();
    lio_ieskf_params pp = p ? *p : lio_ieskf_params{0.001, 3, 0.001};
    lio::host::State x = to_host(*xs);
    lio::host::Mat Pm(P, P + LIO_STATE_DIM * LIO_STATE_DIM);
    int err = LIO_OK;
    double launch_ms = 0.0, wait_ms = 0.0;
    auto hfn = [&](const lio::host::State& s, bool redo, bool want_rows, lio::host::HModel& hm) -> int {
        if (want_rows) {
            const int64_t want = (int64_t)hm.sums[LIO_SUMS_NEFF];
            hm.rows.assign((size_t)std::max<int64_t>(want, 1) * 7, 0.0);
            int64_t nr = 0;
            int rc = lio_get_h_rows(c, hm.rows.data(), want, &nr);
            if (rc) return err = rc;
            hm.rows.resize((size_t)std::min(nr, want) * 7);
            return 0;
        }
        const lio_pose pose = state_pose(s);
        hm.rows.clear();
        c->last_launch_ms = c->last_wait_ms = 0.0;
        int rc = match_impl(c, &pose, redo ? 1 : 0, hm.sums);
        if (rc) return err = rc;
        launch_ms += c->last_launch_ms;
        wait_ms += c->last_wait_ms;
        return 0;
    };
    lio::host::IeskfResult r;
    int rc = lio::host::update_iterated(x, Pm, pp.laser_point_cov, pp.max_iteration, pp.epsi, hfn, r);
    if (rc) return err ? err : fail(LIO_ERR_STATE, "IESKF: singular matrix");
    from_host(x, *xs);
    std::memcpy(P, Pm.data(), sizeof(double) * LIO_STATE_DIM * LIO_STATE_DIM);
    if (st) {
        st->h_evals = r.h_evals;
        st->knn_calls = r.knn_calls;
        st->converged = r.converged;
        st->n_eff = r.n_eff;
        st->res_mean = r.res_mean;
        st->solve_ms = r.solve_ms;
        st->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
        st->launch_ms = launch_ms;
        st->wait_ms = wait_ms;
    }
    return LIO_OK;
}

// =============================================================================
// timing
// =============================================================================
int lio_ctx_set_timing(lio_ctx* c, int enable) {
    if (!c) return fail(LIO_ERR_ARG, "NULL ctx");
    c->timing = enable != 0;
    return LIO_OK;
}
int lio_ctx_get_timing(lio_ctx* c, lio_kernel_timing* out) {
    if (!c || !out) return fail(LIO_ERR_ARG, "bad arguments");
    *out = c->tm;
    return LIO_OK;
}
int lio_ctx_reset_timing(lio_ctx* c) {
    if (!c) return fail(LIO_ERR_ARG, "NULL ctx");
    c->tm = lio_kernel_timing{};
    return LIO_OK;
}

}  // extern "C"
