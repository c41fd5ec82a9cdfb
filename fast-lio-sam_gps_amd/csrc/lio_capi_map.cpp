// lio_capi_map.cpp — the C-ABI (include/lio_gpu.h) of the map handle: create / destroy, build, the point and kNN
// queries, add / delete (ikd-Tree's Add_Points, Delete_Point_Boxes) and the local-map cube (lasermap_fov_segment).
// lio_map_incremental works on a scan's kNN lists and is in lio_capi_scan.cpp; lio_map_build_pcd in lio_capi_formats.cpp.
#include <algorithm>
#include <cmath>
#include <vector>

#include "lio_capi_online.hpp"

using namespace lio::capi;

extern "C" {

int lio_map_create(const lio_map_params* p, lio_map** out) {
    lio_map_params pp{};
    if (p) pp = *p;
    if (!(pp.cell_size > 0.f)) pp.cell_size = 1.0f;
    if (!(pp.downsample_size > 0.f)) pp.downsample_size = 0.5f;
    const int rc = open_handle(pp.device, out, "out is NULL");
    if (rc) return rc;
    (*out)->p = pp;
    (*out)->grid.gapped = true;  // per-cell blocks: map_incremental updates in O(points changed)
    return LIO_OK;
}

int lio_map_destroy(lio_map* m) {
    if (m && m->n_ctx.load() > 0)
        return fail(LIO_ERR_STATE, "lio_map_destroy: h_share_model contexts still use this map (lio_ctx_destroy them first)");
    return close_handle(m, [](lio_map& h) {
        lio::grid_free(h.grid);
        lio::mapupd_free(h.upd);
        lio::dev_free(&h.d_xyz, &h.d_qidx, &h.d_qd2);
    });
}

int lio_map_set_params(lio_map* m, const lio_map_params* p) {
    if (!m || !p) return fail(LIO_ERR_ARG, "lio_map_set_params: bad arguments");
    if (m->grid.n_ids > 0) return fail(LIO_ERR_STATE, "lio_map_set_params: map already holds points (call before Build)");
    if (p->device != m->dev) return fail(LIO_ERR_ARG, "lio_map_set_params: device cannot change");
    if (p->cell_size > 0.f) m->p.cell_size = p->cell_size;
    if (p->downsample_size > 0.f) m->p.downsample_size = p->downsample_size;
    return LIO_OK;
}

static int map_build_impl(lio_map* m, const float* d_xyz, int64_t n) {
    int rc = lio::grid_build(m->grid, d_xyz, n, m->p.cell_size, m->st);
    if (rc) return status(rc, "grid build", "invalid points (empty, too many, or non-finite)");
    // the map_incremental scratch for a scan of up to 256 k points (C3 131 k, C5 ~30 k undistorted), so the
    // stream's first update allocates nothing; larger scans grow it then
    rc = lio::mapupd_presize(m->upd, (int64_t)1 << 18, m->st);
    if (rc) return status(rc, "map update scratch");
    HIP_TRY(hipStreamSynchronize(m->st));
    m->n = m->grid.n;
    ++m->version;
    return LIO_OK;
}

int lio_map_build(lio_map* m, const float* xyz, int64_t n) {
    if (!m || (!xyz && n > 0) || n <= 0) return fail(LIO_ERR_ARG, "lio_map_build: bad arguments");
    HIP_TRY(hipSetDevice(m->dev));
    int rc = grow(&m->d_xyz, m->xyz_cap, n, 3);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(m->d_xyz, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, m->st));
    return map_build_impl(m, m->d_xyz, n);
}

int lio_map_build_device(lio_map* m, const float* d_xyz, int64_t n) {
    if (!m || !d_xyz || n <= 0) return fail(LIO_ERR_ARG, "lio_map_build_device: bad arguments");
    HIP_TRY(hipSetDevice(m->dev));
    return map_build_impl(m, d_xyz, n);
}

int64_t lio_map_size(const lio_map* m) { return m ? m->n : 0; }
int64_t lio_map_num_ids(const lio_map* m) { return m ? m->grid.n_ids : 0; }

static int map_by_id_host(lio_map* m, std::vector<float4>& tmp) {
    tmp.resize(m->grid.n_ids);
    if (m->grid.n_ids == 0) return LIO_OK;
    HIP_TRY(hipSetDevice(m->dev));
    HIP_TRY(hipMemcpyAsync(tmp.data(), m->grid.by_id, m->grid.n_ids * sizeof(float4), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));
    return LIO_OK;
}

int lio_map_get_points(lio_map* m, float* xyz_out) {
    if (!m || !xyz_out) return fail(LIO_ERR_ARG, "bad arguments");
    std::vector<float4> tmp;
    int rc = map_by_id_host(m, tmp);
    if (rc) return rc;
    int64_t k = 0;
    for (const float4& p : tmp) {
        if (p.w == 0.f) continue;
        xyz_out[3 * k] = p.x;
        xyz_out[3 * k + 1] = p.y;
        xyz_out[3 * k + 2] = p.z;
        ++k;
    }
    return LIO_OK;
}

int lio_map_get_by_id(lio_map* m, float* xyz_out, uint8_t* alive_out) {
    if (!m) return fail(LIO_ERR_ARG, "bad arguments");
    std::vector<float4> tmp;
    int rc = map_by_id_host(m, tmp);
    if (rc) return rc;
    for (size_t i = 0; i < tmp.size(); ++i) {
        if (xyz_out) {
            xyz_out[3 * i] = tmp[i].x;
            xyz_out[3 * i + 1] = tmp[i].y;
            xyz_out[3 * i + 2] = tmp[i].z;
        }
        if (alive_out) alive_out[i] = tmp[i].w != 0.f;
    }
    return LIO_OK;
}

int lio_map_nearest_search(lio_map* m, const float* q, int64_t n, int k, float max_dist, int32_t* idx, float* d2) {
    if (!m || n < 0 || k < 1 || k > 5 || (n > 0 && (!q || !idx)) || n >= (int64_t)1 << 30 || std::isnan(max_dist))
        return fail(LIO_ERR_ARG, "lio_map_nearest_search: bad arguments (k must be 1..5)");
    if (m->grid.n_ids == 0) return fail(LIO_ERR_STATE, "lio_map_nearest_search: map is empty (call lio_map_build)");
    if (n == 0) return LIO_OK;
    HIP_TRY(hipSetDevice(m->dev));
    int rc = grow(&m->d_xyz, m->xyz_cap, n, 3);
    if (!rc) rc = grow(&m->d_qidx, m->qidx_cap, n * k);
    if (!rc && d2) rc = grow(&m->d_qd2, m->qd2_cap, n * k);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(m->d_xyz, q, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, m->st));
    const lio::GridDev g = lio::grid_view(m->grid);
    const bool unbounded = !(max_dist > 0.f) || std::isinf(max_dist);
    const float bound = unbounded ? INFINITY : max_dist * max_dist;
    const int max_shell = unbounded ? 0x3fffffff : (int)std::ceil(max_dist / g.cell) + 1;
    lio::launch_map_knn(g, m->d_xyz, (int)n, bound, max_shell, k, m->d_qidx, d2 ? m->d_qd2 : nullptr, m->st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(idx, m->d_qidx, (size_t)n * k * sizeof(int32_t), hipMemcpyDeviceToHost, m->st));
    if (d2) HIP_TRY(hipMemcpyAsync(d2, m->d_qd2, (size_t)n * k * sizeof(float), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));
    return LIO_OK;
}

int lio_map_gather(lio_map* m, const int32_t* ids, int64_t n, float* xyz_out) {
    if (!m || n < 0 || (n > 0 && (!ids || !xyz_out))) return fail(LIO_ERR_ARG, "lio_map_gather: bad arguments");
    if (n == 0) return LIO_OK;
    HIP_TRY(hipSetDevice(m->dev));
    int rc = grow(&m->d_qidx, m->qidx_cap, n);
    if (!rc) rc = grow(&m->d_xyz, m->xyz_cap, n, 3);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(m->d_qidx, ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, m->st));
    lio::map_gather_ids(m->grid, m->d_qidx, n, m->d_xyz, m->st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(xyz_out, m->d_xyz, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, m->st));
    HIP_TRY(hipStreamSynchronize(m->st));
    return LIO_OK;
}

int lio_map_add_device(lio_map* m, const float* d_xyz, int64_t n, int downsample, int64_t* n_added) {
    if (!m || n < 0 || (n > 0 && !d_xyz)) return fail(LIO_ERR_ARG, "lio_map_add: bad arguments");
    HIP_TRY(hipSetDevice(m->dev));
    int64_t out[2] = {0, 0};
    if (m->grid.n_ids == 0 && !downsample && n > 0) {  // empty map: a plain add is a build
        int rc = lio_map_build_device(m, d_xyz, n);
        if (n_added) *n_added = n;
        return rc;
    }
    int rc = lio::map_add_device(m->grid, m->upd, d_xyz, n, downsample != 0, m->p.downsample_size, map_slack(m), out,
                                 m->st);
    HIP_TRY(hipStreamSynchronize(m->st));
    m->n = m->grid.n;
    ++m->version;
    if (n_added) *n_added = out[0];
    return status(rc, "lio_map_add", "invalid points");
}

int lio_map_add(lio_map* m, const float* xyz, int64_t n, int downsample, int64_t* n_added) {
    if (!m || n < 0 || (n > 0 && !xyz)) return fail(LIO_ERR_ARG, "lio_map_add: bad arguments");
    if (n == 0) {
        if (n_added) *n_added = 0;
        return LIO_OK;
    }
    HIP_TRY(hipSetDevice(m->dev));
    int rc = grow(&m->d_xyz, m->xyz_cap, n, 3);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(m->d_xyz, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, m->st));
    return lio_map_add_device(m, m->d_xyz, n, downsample, n_added);
}

int lio_map_delete_boxes(lio_map* m, const float* boxes, int nb, int64_t* n_deleted) {
    if (!m || nb < 0 || (nb > 0 && !boxes)) return fail(LIO_ERR_ARG, "lio_map_delete_boxes: bad arguments");
    HIP_TRY(hipSetDevice(m->dev));
    int64_t nd = 0;
    int rc = lio::map_delete_boxes(m->grid, m->upd, boxes, nb, map_slack(m), &nd, m->st);
    HIP_TRY(hipStreamSynchronize(m->st));
    m->n = m->grid.n;
    ++m->version;
    if (n_deleted) *n_deleted = nd;
    return status(rc, "lio_map_delete_boxes", "invalid points");
}

// lasermap_fov_segment() [U]: float box vertices, MOV_THRESHOLD * DET_RANGE
// trigger distance, mov_dist = max((cube_len - 2*MOV_THRESHOLD*DET_RANGE)*0.5*0.9,
// DET_RANGE*(MOV_THRESHOLD-1)) (double, stored float).
int lio_localmap_update(lio_localmap* lm, const double pos_lid[3], double cube_len, float det_range,
                        float mov_threshold, float boxes_out[18], int* n_boxes) {
    if (!lm || !pos_lid || !boxes_out || !n_boxes) return fail(LIO_ERR_ARG, "lio_localmap_update: bad arguments");
    *n_boxes = 0;
    if (!lm->initialized) {
        for (int i = 0; i < 3; ++i) {
            lm->vertex_min[i] = (float)(pos_lid[i] - cube_len / 2.0);
            lm->vertex_max[i] = (float)(pos_lid[i] + cube_len / 2.0);
        }
        lm->initialized = 1;
        return LIO_OK;
    }
    float dist_to_edge[3][2];
    bool need_move = false;
    for (int i = 0; i < 3; ++i) {
        dist_to_edge[i][0] = (float)std::fabs(pos_lid[i] - lm->vertex_min[i]);
        dist_to_edge[i][1] = (float)std::fabs(pos_lid[i] - lm->vertex_max[i]);
        if (dist_to_edge[i][0] <= mov_threshold * det_range || dist_to_edge[i][1] <= mov_threshold * det_range)
            need_move = true;
    }
    if (!need_move) return LIO_OK;
    lio_localmap nw = *lm;
    const float mov_dist = (float)std::max((cube_len - 2.0 * mov_threshold * det_range) * 0.5 * 0.9,
                                           (double)(det_range * (mov_threshold - 1)));
    for (int i = 0; i < 3; ++i) {
        float bmin[3], bmax[3];
        for (int d = 0; d < 3; ++d) {
            bmin[d] = lm->vertex_min[d];
            bmax[d] = lm->vertex_max[d];
        }
        bool add = false;
        if (dist_to_edge[i][0] <= mov_threshold * det_range) {
            nw.vertex_max[i] -= mov_dist;
            nw.vertex_min[i] -= mov_dist;
            bmin[i] = lm->vertex_max[i] - mov_dist;
            add = true;
        } else if (dist_to_edge[i][1] <= mov_threshold * det_range) {
            nw.vertex_max[i] += mov_dist;
            nw.vertex_min[i] += mov_dist;
            bmax[i] = lm->vertex_min[i] + mov_dist;
            add = true;
        }
        if (add) {
            float* b = boxes_out + 6 * (*n_boxes);
            for (int d = 0; d < 3; ++d) {
                b[d] = bmin[d];
                b[3 + d] = bmax[d];
            }
            ++*n_boxes;
        }
    }
    *lm = nw;
    return LIO_OK;
}

int lio_map_get_grid(lio_map* m, double* out7) {
    if (!m || !out7) return fail(LIO_ERR_ARG, "bad arguments");
    const lio::GridGeom& g = m->grid.geom;
    out7[0] = g.ox;
    out7[1] = g.oy;
    out7[2] = g.oz;
    out7[3] = g.cell;
    out7[4] = g.nx;
    out7[5] = g.ny;
    out7[6] = g.nz;
    return LIO_OK;
}

int lio_map_set_test_limits(lio_map* m, int64_t slot_headroom, int64_t dirty_cells) {
    if (!m || slot_headroom < 0 || dirty_cells < 0) return fail(LIO_ERR_ARG, "lio_map_set_test_limits: bad arguments");
    m->grid.slots_extra = slot_headroom;
    m->upd.dcap_limit = dirty_cells;
    return LIO_OK;
}

int lio_map_get_stats(lio_map* m, int64_t* out8) {
    if (!m || !out8) return fail(LIO_ERR_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(m->dev));
    uint32_t bump = 0;
    if (m->grid.bump) {
        HIP_TRY(hipMemcpyAsync(&bump, m->grid.bump, sizeof(bump), hipMemcpyDeviceToHost, m->st));
        HIP_TRY(hipStreamSynchronize(m->st));
    }
    out8[0] = m->grid.rebuilds;
    out8[1] = m->grid.slots_cap;
    out8[2] = bump;
    out8[3] = m->grid.n;
    out8[4] = m->grid.n_ids;
    out8[5] = m->grid.geom.ncells;
    out8[6] = m->upd.h_cnt ? (int64_t)m->upd.h_cnt[9] : 0;  // lio_mapupd.hip kCFlags
    out8[7] = 0;
    return LIO_OK;
}

}  // extern "C"
