// lio_capi_camera.cpp — the C-ABI (include/lio_gpu.h) of the camera leg: lio_project_points and
// lio_undistort_map on a lio_filter, the lio_colorizer, the lio_undistorter, the lio_exposure and the lio_overlay.
#include <limits>

#include "lio_capi_util.hpp"
#include "lio_colorize.hpp"
#include "lio_exposure.hpp"
#include "lio_overexposure.hpp"
#include "lio_overlay.hpp"
#include "lio_undistort.hpp"

using namespace lio::capi;

// ---- what the four frame handles share ----
// The tail of a create: the buffers' init, and a handle whose init fails is closed again: *out stays NULL.
template <class H, class Init>
static int init_handle(H** out, const char* what, Init&& init, int (*destroy)(H*)) {
    const int rc = status(init(**out), what);
    if (rc) {
        destroy(*out);
        *out = nullptr;
    }
    return rc;
}

// the body of a get_timing, after its NULL checks
template <int N>
static int stage_times(const lio::StageTimer<N>& t, double* ms) {
    for (int k = 0; k < N; ++k) ms[k] = t.ms[k];
    return LIO_OK;
}

// `name` (pitch or out_pitch) holds a row of the image; `of`: which image, where the call has two
static int pitch_arg(const std::string& what, const char* name, int64_t pitch, int channels, int width, const char* of = "") {
    if (pitch >= (int64_t)channels * width) return LIO_OK;
    return fail(LIO_ERR_ARG, what + ": " + name + " must be at least channels x width bytes" + of);
}

extern "C" {

// ---- the camera of both halves ----
// the finite checks: the intrinsics of cam and of the second camera (cam again where there is one), then cam's
// coefficients
static int camera_finite(const std::string& what, const lio_camera* cam, const lio_camera* second) {
    const double k[8] = {cam->fx, cam->fy, cam->cx, cam->cy, second->fx, second->fy, second->cx, second->cy};
    if (!all_finite(k, 8)) return fail(LIO_ERR_ARG, what + ": an intrinsic (fx, fy, cx, cy) is not finite");
    if (!all_finite(cam->dist, 8)) return fail(LIO_ERR_ARG, what + ": a distortion coefficient is not finite");
    return LIO_OK;
}

// cam's intrinsics, coefficients and size; R and t stay zero and r2_max has no limit
static lio::CamArg cam_arg(const lio_camera* cam) {
    lio::CamArg a{};
    a.fx = cam->fx, a.fy = cam->fy, a.cx = cam->cx, a.cy = cam->cy;
    a.k1 = cam->dist[0], a.k2 = cam->dist[1], a.p1 = cam->dist[2], a.p2 = cam->dist[3];
    a.k3 = cam->dist[4], a.k4 = cam->dist[5], a.k5 = cam->dist[6], a.k6 = cam->dist[7];
    a.r2_max = std::numeric_limits<double>::infinity();
    a.width = cam->width, a.height = cam->height;
    return a;
}

// ---- camera projection and point cloud colorization (lio_colorize.hip) ----
// The camera and pose checks shared by lio_project_points and lio_colorizer_add_frame: every failure names its bound.
static int camera_arg(const std::string& what, const lio_camera* cam, const double* Rt, lio::CamArg* a) {
    if (!cam) return fail(LIO_ERR_ARG, what + ": cam is NULL");
    if (!Rt) return fail(LIO_ERR_ARG, what + ": Rt is NULL");
    if (cam->width < 1 || cam->height < 1) return fail(LIO_ERR_ARG, what + ": width and height must be at least 1");
    if ((int64_t)cam->width * (int64_t)cam->height >= (int64_t)1 << 31)
        return fail(LIO_ERR_ARG, what + ": width x height must be below 2^31");
    if (const int rc = camera_finite(what, cam, cam)) return rc;
    if (!all_finite(Rt, 12)) return fail(LIO_ERR_ARG, what + ": a pose entry of Rt is not finite");
    if (!(cam->r2_max >= 0.0)) return fail(LIO_ERR_ARG, what + ": r2_max must be >= 0 (+inf: no limit) and not NaN");
    *a = cam_arg(cam);
    a->r2_max = cam->r2_max;
    for (int i = 0; i < 9; ++i) a->R[i] = Rt[i];
    for (int i = 0; i < 3; ++i) a->t[i] = Rt[9 + i];
    return LIO_OK;
}

static int cloud_arg(const std::string& what, const float* pts, int64_t n, int stride) {
    if (n < 0 || n >= (int64_t)1 << 31) return fail(LIO_ERR_ARG, what + ": n must be in 0 .. 2^31 - 1");
    if (stride < 3 || stride > lio::kMaxFields) return fail(LIO_ERR_ARG, what + ": stride must be in 3..8");
    if (!pts && n > 0) return fail(LIO_ERR_ARG, what + ": pts is NULL");
    return LIO_OK;
}

int lio_project_points(lio_filter* f, const float* pts, int64_t n, int stride, const lio_camera* cam, const double* Rt,
                       double* uv_opt, double* zc_opt, int32_t* pix_opt, uint8_t* valid) {
    const char* what = "lio_project_points";
    int rc = null_handle(f, what);
    if (rc) return rc;
    if ((rc = cloud_arg(what, pts, n, stride))) return rc;
    lio::CamArg a{};
    if ((rc = camera_arg(what, cam, Rt, &a))) return rc;
    if (!valid) return fail(LIO_ERR_ARG, std::string(what) + ": valid is NULL");
    if (n == 0) return LIO_OK;
    HIP_TRY(hipSetDevice(f->dev));
    if ((rc = upload_in(f, pts, n * stride))) return rc;
    return status(lio::project_points(f->pj, f->d_in, n, stride, a, uv_opt, zc_opt, pix_opt, valid, f->st), what);
}

static const lio_colorize_params kColorizeDefaults = {0, 0, 0.f, 0.f, 1};

static int colorize_params_arg(const char* what, const lio_colorize_params* p) {
    if (p->splat_radius < 0 || p->splat_radius > lio::kCzMaxSplat)
        return fail(LIO_ERR_ARG, std::string(what) + ": splat_radius must be in 0..8");
    if (!(p->depth_rel >= 0.f) || !std::isfinite(p->depth_rel) || !(p->depth_abs >= 0.f) || !std::isfinite(p->depth_abs))
        return fail(LIO_ERR_ARG, std::string(what) + ": depth_rel and depth_abs must be finite and >= 0");
    return LIO_OK;
}

struct lio_colorizer : Handle {
    lio_colorize_params p = kColorizeDefaults;
    lio::ColorizeBuf c;
};

int lio_colorizer_destroy(lio_colorizer* h) {
    return close_handle(h, [](lio_colorizer& z) { lio::colorizer_free(z.c); });
}

// a handle whose params or init fail is closed again: *out stays NULL.  Written out: the params come before the
// init, and *out is NULL before the handle is closed.
int lio_colorizer_create(int device, const lio_colorize_params* params, lio_colorizer** out) {
    int rc = open_handle(device, out, "lio_colorizer_create: out is NULL");
    if (rc) return rc;
    lio_colorizer* h = *out;
    if (params && !(rc = colorize_params_arg("lio_colorizer_create", params))) h->p = *params;
    if (!rc) rc = status(lio::colorizer_init(h->c), "lio_colorizer_create");
    if (rc) {
        *out = nullptr;
        lio_colorizer_destroy(h);
    }
    return rc;
}

int lio_colorizer_set_params(lio_colorizer* h, const lio_colorize_params* params) {
    int rc = null_handle(h, "lio_colorizer_set_params");
    if (rc) return rc;
    if (!params) return fail(LIO_ERR_ARG, "lio_colorizer_set_params: params is NULL");
    if ((rc = colorize_params_arg("lio_colorizer_set_params", params))) return rc;
    h->p = *params;
    return LIO_OK;
}

int lio_colorizer_set_cloud(lio_colorizer* h, const float* pts, int64_t n, int stride) {
    const char* what = "lio_colorizer_set_cloud";
    int rc = null_handle(h, what);
    if (rc) return rc;
    if ((rc = cloud_arg(what, pts, n, stride))) return rc;
    HIP_TRY(hipSetDevice(h->dev));
    return status(lio::colorizer_set_cloud(h->c, pts, n, stride, h->st), what);
}

int lio_colorizer_add_frame(lio_colorizer* h, const lio_camera* cam, const double* Rt, const uint8_t* image, int64_t pitch,
                            int64_t* n_updated) {
    const std::string what = "lio_colorizer_add_frame";
    int rc = null_handle(h, what.c_str());
    if (rc) return rc;
    lio::CamArg a{};
    if ((rc = camera_arg(what, cam, Rt, &a))) return rc;
    if (!image) return fail(LIO_ERR_ARG, what + ": image is NULL");
    if (!n_updated) return fail(LIO_ERR_ARG, what + ": n_updated is NULL");
    if (pitch < 3 * (int64_t)cam->width) return fail(LIO_ERR_ARG, what + ": pitch must be at least 3 x width bytes");
    if (!h->c.have_cloud) return fail(LIO_ERR_STATE, what + ": no cloud (call lio_colorizer_set_cloud first)");
    *n_updated = 0;
    HIP_TRY(hipSetDevice(h->dev));
    return status(lio::colorizer_add_frame(h->c, a, image, pitch, h->p.bgr != 0, h->p.occlusion != 0, h->p.splat_radius,
                                           h->p.depth_rel, h->p.depth_abs, n_updated, h->st),
                  what.c_str());
}

int lio_colorizer_get(lio_colorizer* h, uint8_t* rgb, int32_t* frame_opt, double* depth_opt) {
    int rc = null_handle(h, "lio_colorizer_get");
    if (rc) return rc;
    if (!rgb) return fail(LIO_ERR_ARG, "lio_colorizer_get: rgb is NULL");
    if (!h->c.have_cloud) return fail(LIO_ERR_STATE, "lio_colorizer_get: no cloud (call lio_colorizer_set_cloud first)");
    HIP_TRY(hipSetDevice(h->dev));
    return status(lio::colorizer_get(h->c, rgb, frame_opt, depth_opt, h->st), "lio_colorizer_get");
}

int lio_colorizer_reset(lio_colorizer* h) {
    int rc = null_handle(h, "lio_colorizer_reset");
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->dev));
    return status(lio::colorizer_reset(h->c, h->st), "lio_colorizer_reset");
}

int lio_colorizer_get_timing(lio_colorizer* h, double* ms4) {
    int rc = null_handle(h, "lio_colorizer_get_timing");
    if (rc) return rc;
    if (!ms4) return fail(LIO_ERR_ARG, "lio_colorizer_get_timing: ms4 is NULL");
    return stage_times(h->c.timer, ms4);
}

// ---- image undistortion (lio_undistort.hip) ----
// The camera checks shared by lio_undistort_map and lio_undistorter_set_camera; they need no device and come before
// the handle is looked at.  dst_opt NULL: src's intrinsics and size.
static int undistort_cams_arg(const std::string& what, const lio_camera* src, const lio_camera* dst_opt, lio::CamArg* a,
                              lio::UdDst* d) {
    if (!src) return fail(LIO_ERR_ARG, what + ": src is NULL");
    const lio_camera* dst = dst_opt ? dst_opt : src;
    for (const lio_camera* c : {src, dst})
        if (c->width < 1 || c->width > lio::kUdMaxSize || c->height < 1 || c->height > lio::kUdMaxSize)
            return fail(LIO_ERR_ARG, what + ": width and height must be in 1..32767");
    if (const int rc = camera_finite(what, src, dst)) return rc;
    if (dst->fx == 0.0 || dst->fy == 0.0) return fail(LIO_ERR_ARG, what + ": dst fx and fy must not be 0");
    if (dst_opt)
        for (double v : dst_opt->dist)
            if (!(v == 0.0)) return fail(LIO_ERR_ARG, what + ": dst dist must be all zero (the rectified image is a pinhole)");
    *a = cam_arg(src);
    *d = lio::UdDst{dst->fx, dst->fy, dst->cx, dst->cy, dst->width, dst->height};
    return LIO_OK;
}

int lio_undistort_map(lio_filter* f, const lio_camera* src, const lio_camera* dst_opt, double* uv_opt, int32_t* sxy_opt,
                      uint8_t* axy_opt) {
    const char* what = "lio_undistort_map";
    lio::CamArg a{};
    lio::UdDst d{};
    int rc = undistort_cams_arg(what, src, dst_opt, &a, &d);
    if (rc) return rc;
    if ((rc = null_handle(f, what))) return rc;
    HIP_TRY(hipSetDevice(f->dev));
    return status(lio::undistort_map(f->pj, a, d, uv_opt, sxy_opt, axy_opt, f->st), what);
}

struct lio_undistorter : Handle {
    lio::UndistortBuf u;
};

int lio_undistorter_destroy(lio_undistorter* h) {
    return close_handle(h, [](lio_undistorter& z) { lio::undistorter_free(z.u); });
}

int lio_undistorter_create(int device, lio_undistorter** out) {
    const int rc = open_handle(device, out, "lio_undistorter_create: out is NULL");
    if (rc) return rc;
    return init_handle(out, "lio_undistorter_create", [](lio_undistorter& z) { return lio::undistorter_init(z.u); },
                       lio_undistorter_destroy);
}

int lio_undistorter_set_camera(lio_undistorter* h, const lio_camera* src, const lio_camera* dst_opt, int channels,
                               const uint8_t* border_opt) {
    const char* what = "lio_undistorter_set_camera";
    lio::CamArg a{};
    lio::UdDst d{};
    int rc = undistort_cams_arg(what, src, dst_opt, &a, &d);
    if (rc) return rc;
    if (channels != 1 && channels != 3) return fail(LIO_ERR_ARG, std::string(what) + ": channels must be 1 or 3");
    if ((rc = null_handle(h, what))) return rc;
    const uint8_t black[3] = {0, 0, 0};
    HIP_TRY(hipSetDevice(h->dev));
    return status(lio::undistorter_set_camera(h->u, a, d, channels, border_opt ? border_opt : black, h->st), what);
}

// a frame through a configured undistorter: the checks lio_undistorter_run and lio_exposure_clahe_undistorted share
static int undistorter_frame_arg(const std::string& what, const lio::UndistortBuf& u, int64_t pitch, int64_t out_pitch) {
    if (!u.have_camera) return fail(LIO_ERR_STATE, what + ": no camera (call lio_undistorter_set_camera first)");
    if (const int rc = pitch_arg(what, "pitch", pitch, u.channels, u.sw, " of the raw image")) return rc;
    return pitch_arg(what, "out_pitch", out_pitch, u.channels, u.dw, " of the rectified image");
}

int lio_undistorter_run(lio_undistorter* h, const uint8_t* image, int64_t pitch, uint8_t* out, int64_t out_pitch) {
    const std::string what = "lio_undistorter_run";
    if (!image) return fail(LIO_ERR_ARG, what + ": image is NULL");
    if (!out) return fail(LIO_ERR_ARG, what + ": out is NULL");
    int rc = null_handle(h, what.c_str());
    if (rc) return rc;
    if ((rc = undistorter_frame_arg(what, h->u, pitch, out_pitch))) return rc;
    HIP_TRY(hipSetDevice(h->dev));
    return status(lio::undistorter_run(h->u, image, pitch, out, out_pitch, h->st), what.c_str());
}

int lio_undistorter_get_timing(lio_undistorter* h, double* ms3) {
    const int rc = null_handle(h, "lio_undistorter_get_timing");
    if (rc) return rc;
    if (!ms3) return fail(LIO_ERR_ARG, "lio_undistorter_get_timing: ms3 is NULL");
    return stage_times(h->u.timer, ms3);
}

// ---- exposure adaption (lio_exposure.hip) ----
// The checks of an image and its result that need no device; they come before the handle is looked at.  out may
// be absent (lio_exposure_histograms).
static int exposure_image_arg(const std::string& what, const void* image, int width, int height, int channels, int64_t pitch,
                              int order, const void* out, bool has_out, int64_t out_pitch) {
    if (!image) return fail(LIO_ERR_ARG, what + ": image is NULL");
    if (has_out && !out) return fail(LIO_ERR_ARG, what + ": out is NULL");
    if (width < 1 || width > lio::kExMaxSize || height < 1 || height > lio::kExMaxSize)
        return fail(LIO_ERR_ARG, what + ": width and height must be in 1..32767");
    if (channels != 1 && channels != 3) return fail(LIO_ERR_ARG, what + ": channels must be 1 or 3");
    if (order != 0 && order != 1) return fail(LIO_ERR_ARG, what + ": order must be 0 (B G R) or 1 (R G B)");
    if (const int rc = pitch_arg(what, "pitch", pitch, channels, width)) return rc;
    return has_out ? pitch_arg(what, "out_pitch", out_pitch, channels, width) : LIO_OK;
}

static int exposure_tiles_arg(const std::string& what, int tiles_x, int tiles_y) {
    if (tiles_x < 1 || tiles_x > lio::kExMaxTiles || tiles_y < 1 || tiles_y > lio::kExMaxTiles)
        return fail(LIO_ERR_ARG, what + ": tiles_x and tiles_y must be in 1..64");
    return LIO_OK;
}

static int exposure_tiling_arg(const std::string& what, int width, int height, double clip_limit, int tiles_x, int tiles_y,
                               lio::ExTiling* t) {
    const char* why = "";
    if (lio::exposure_tiling(width, height, clip_limit, tiles_x, tiles_y, t, &why)) return fail(LIO_ERR_ARG, what + ": " + why);
    return LIO_OK;
}

struct lio_exposure : Handle {
    lio::ExposureBuf e;
};

int lio_exposure_destroy(lio_exposure* h) {
    return close_handle(h, [](lio_exposure& z) { lio::exposure_free(z.e); });
}

int lio_exposure_create(int device, lio_exposure** out) {
    const int rc = open_handle(device, out, "lio_exposure_create: out is NULL");
    if (rc) return rc;
    return init_handle(out, "lio_exposure_create", [](lio_exposure& z) { return lio::exposure_init(z.e); }, lio_exposure_destroy);
}

int lio_exposure_histograms(lio_exposure* h, const uint8_t* image, int width, int height, int channels, int64_t pitch,
                            int order, int64_t* hist_v_opt, int64_t* hist_gray_opt) {
    const char* what = "lio_exposure_histograms";
    int rc = exposure_image_arg(what, image, width, height, channels, pitch, order, nullptr, false, 0);
    if (rc) return rc;
    if ((rc = null_handle(h, what))) return rc;
    HIP_TRY(hipSetDevice(h->dev));
    return status(lio::exposure_histograms(h->e, image, width, height, channels, pitch, order, hist_v_opt, hist_gray_opt, h->st),
                  what);
}

int lio_exposure_clahe(lio_exposure* h, const uint8_t* image, int width, int height, int channels, int64_t pitch, int order,
                       double clip_limit, int tiles_x, int tiles_y, uint8_t* out, int64_t out_pitch) {
    const char* what = "lio_exposure_clahe";
    int rc = exposure_image_arg(what, image, width, height, channels, pitch, order, out, true, out_pitch);
    if (rc) return rc;
    if ((rc = exposure_tiles_arg(what, tiles_x, tiles_y))) return rc;
    lio::ExTiling t{};
    if ((rc = exposure_tiling_arg(what, width, height, clip_limit, tiles_x, tiles_y, &t))) return rc;
    if ((rc = null_handle(h, what))) return rc;
    HIP_TRY(hipSetDevice(h->dev));
    return status(lio::exposure_clahe(h->e, image, width, height, channels, pitch, order, t, out, out_pitch, h->st), what);
}

int lio_exposure_remap(lio_exposure* h, const uint8_t* image, int width, int height, int channels, int64_t pitch, int order,
                       const uint8_t* lut_v_opt, const uint8_t* lut_all_opt, uint8_t* out, int64_t out_pitch) {
    const char* what = "lio_exposure_remap";
    int rc = exposure_image_arg(what, image, width, height, channels, pitch, order, out, true, out_pitch);
    if (rc) return rc;
    if (!lut_v_opt && !lut_all_opt) return fail(LIO_ERR_ARG, std::string(what) + ": lut_v_opt and lut_all_opt are both NULL");
    if ((rc = null_handle(h, what))) return rc;
    HIP_TRY(hipSetDevice(h->dev));
    return status(lio::exposure_remap(h->e, image, width, height, channels, pitch, order, lut_v_opt, lut_all_opt, out, out_pitch,
                                      h->st),
                  what);
}

int lio_exposure_clahe_undistorted(lio_exposure* h, lio_undistorter* undistorter, const uint8_t* raw_image, int64_t pitch,
                                   int order, double clip_limit, int tiles_x, int tiles_y, uint8_t* out, int64_t out_pitch) {
    const std::string what = "lio_exposure_clahe_undistorted";
    if (!raw_image) return fail(LIO_ERR_ARG, what + ": raw_image is NULL");
    if (!out) return fail(LIO_ERR_ARG, what + ": out is NULL");
    if (order != 0 && order != 1) return fail(LIO_ERR_ARG, what + ": order must be 0 (B G R) or 1 (R G B)");
    int rc = exposure_tiles_arg(what, tiles_x, tiles_y);
    if (rc) return rc;
    if (!(clip_limit == clip_limit)) return fail(LIO_ERR_ARG, what + ": clip_limit x tile area / 256 must be below 2^31 and not NaN");
    if ((rc = null_handle(h, what.c_str()))) return rc;
    if (!undistorter) return fail(LIO_ERR_ARG, what + ": undistorter is NULL");
    if (undistorter->dev != h->dev) return fail(LIO_ERR_ARG, what + ": both handles must be on one device");
    const lio::UndistortBuf& u = undistorter->u;
    if ((rc = undistorter_frame_arg(what, u, pitch, out_pitch))) return rc;
    lio::ExTiling t{};
    if ((rc = exposure_tiling_arg(what, u.dw, u.dh, clip_limit, tiles_x, tiles_y, &t))) return rc;
    HIP_TRY(hipSetDevice(h->dev));
    // the undistorter's own stream is idle between its calls (each waits for it): its buffers are used on h's stream
    return status(lio::exposure_clahe_undistorted(h->e, undistorter->u, raw_image, pitch, order, t, out, out_pitch, h->st),
                  what.c_str());
}

int lio_exposure_get_timing(lio_exposure* h, double* ms5) {
    if (!ms5) return fail(LIO_ERR_ARG, "lio_exposure_get_timing: ms5 is NULL");
    const int rc = null_handle(h, "lio_exposure_get_timing");
    if (rc) return rc;
    return stage_times(h->e.timer, ms5);
}

// ---- overexposure recovery and the 8-bit Gaussian blur (lio_overexposure.hip) ----
// The kernel's size and sigma; they need no device.
static int gaussian_arg(const std::string& what, int ksize, double sigma) {
    if (ksize < 1 || ksize > lio::kOxMaxKsize || ksize % 2 == 0) return fail(LIO_ERR_ARG, what + ": ksize must be odd and in 1..31");
    if (!all_finite(&sigma, 1)) return fail(LIO_ERR_ARG, what + ": sigma must be finite");
    return LIO_OK;
}

// p_opt NULL: the script's 200 / 5 / 15 / 0.  Fills the weights.
static int recover_arg(const std::string& what, const lio_recover_params* p_opt, lio::OxRecover* p) {
    double sigma = 0.0;
    if (p_opt) {
        p->threshold = p_opt->threshold, p->dilate = p_opt->dilate, p->ksize = p_opt->ksize;
        sigma = p_opt->sigma;
    }
    if (p->threshold < 0 || p->threshold > 255) return fail(LIO_ERR_ARG, what + ": threshold must be in 0..255");
    if (p->dilate < 1 || p->dilate > lio::kOxMaxDilate || p->dilate % 2 == 0)
        return fail(LIO_ERR_ARG, what + ": dilate must be odd and in 1..15");
    if (const int rc = gaussian_arg(what, p->ksize, sigma)) return rc;
    lio::gaussian_weights(p->ksize, sigma, p->w);
    return LIO_OK;
}

int lio_gaussian_weights(int ksize, double sigma, uint16_t* w) {
    const char* what = "lio_gaussian_weights";
    if (!w) return fail(LIO_ERR_ARG, std::string(what) + ": w is NULL");
    if (const int rc = gaussian_arg(what, ksize, sigma)) return rc;
    lio::gaussian_weights(ksize, sigma, w);
    return LIO_OK;
}

int lio_exposure_gaussian_blur(lio_exposure* h, const uint8_t* image, int width, int height, int channels, int64_t pitch,
                               int ksize, double sigma, uint8_t* out, int64_t out_pitch) {
    const char* what = "lio_exposure_gaussian_blur";
    int rc = exposure_image_arg(what, image, width, height, channels, pitch, 0, out, true, out_pitch);
    if (rc) return rc;
    if ((rc = gaussian_arg(what, ksize, sigma))) return rc;
    uint16_t w[lio::kOxMaxKsize + 1] = {};
    lio::gaussian_weights(ksize, sigma, w);
    if ((rc = null_handle(h, what))) return rc;
    HIP_TRY(hipSetDevice(h->dev));
    return status(lio::exposure_gaussian_blur(h->e, image, width, height, channels, pitch, ksize, w, out, out_pitch, h->st), what);
}

int lio_exposure_recover(lio_exposure* h, const uint8_t* image, int width, int height, int channels, int64_t pitch, int order,
                         const lio_recover_params* p_opt, uint8_t* out, int64_t out_pitch) {
    const char* what = "lio_exposure_recover";
    int rc = exposure_image_arg(what, image, width, height, channels, pitch, order, out, true, out_pitch);
    if (rc) return rc;
    lio::OxRecover p{};
    if ((rc = recover_arg(what, p_opt, &p))) return rc;
    if ((rc = null_handle(h, what))) return rc;
    HIP_TRY(hipSetDevice(h->dev));
    return status(lio::exposure_recover(h->e, image, width, height, channels, pitch, order, p, out, out_pitch, h->st), what);
}

int lio_exposure_recover_undistorted(lio_exposure* h, lio_undistorter* undistorter, const uint8_t* raw_image, int64_t pitch,
                                     int order, const lio_recover_params* p_opt, uint8_t* out, int64_t out_pitch) {
    const std::string what = "lio_exposure_recover_undistorted";
    if (!raw_image) return fail(LIO_ERR_ARG, what + ": raw_image is NULL");
    if (!out) return fail(LIO_ERR_ARG, what + ": out is NULL");
    if (order != 0 && order != 1) return fail(LIO_ERR_ARG, what + ": order must be 0 (B G R) or 1 (R G B)");
    lio::OxRecover p{};
    int rc = recover_arg(what, p_opt, &p);
    if (rc) return rc;
    if ((rc = null_handle(h, what.c_str()))) return rc;
    if (!undistorter) return fail(LIO_ERR_ARG, what + ": undistorter is NULL");
    if (undistorter->dev != h->dev) return fail(LIO_ERR_ARG, what + ": both handles must be on one device");
    if ((rc = undistorter_frame_arg(what, undistorter->u, pitch, out_pitch))) return rc;
    HIP_TRY(hipSetDevice(h->dev));
    // as in lio_exposure_clahe_undistorted: the undistorter's buffers are used on h's stream
    return status(lio::exposure_recover_undistorted(h->e, undistorter->u, raw_image, pitch, order, p, out, out_pitch, h->st),
                  what.c_str());
}

int lio_exposure_get_stencil_timing(lio_exposure* h, double* ms3) {
    if (!ms3) return fail(LIO_ERR_ARG, "lio_exposure_get_stencil_timing: ms3 is NULL");
    const int rc = null_handle(h, "lio_exposure_get_stencil_timing");
    if (rc) return rc;
    return stage_times(h->e.stencil_timer, ms3);
}

// ---- point overlay drawing (lio_overlay.hip) ----
static const lio_overlay_params kOverlayDefaults = {3, LIO_OVERLAY_DRAW_ORDER};
static_assert(LIO_OVERLAY_DRAW_ORDER == lio::kOvDrawOrder && LIO_OVERLAY_NEAREST == lio::kOvNearest, "the order modes are the public ones");

struct lio_overlay : Handle {
    lio_overlay_params p = kOverlayDefaults;
    lio::OvDisc disc = lio::overlay_disc(kOverlayDefaults.radius);
    lio::OverlayBuf o;
};

int lio_overlay_destroy(lio_overlay* h) {
    return close_handle(h, [](lio_overlay& z) { lio::overlay_free(z.o); });
}

// the device first (LIO_ERR_NODEV without one, whatever the params), then the params, then the handle
int lio_overlay_create(int device, const lio_overlay_params* params, lio_overlay** out) {
    const std::string what = "lio_overlay_create";
    if (!out) return fail(LIO_ERR_ARG, what + ": out is NULL");
    *out = nullptr;
    int rc = check_device(device);
    if (rc) return rc;
    if (params && (params->radius < 0 || params->radius > lio::kOvMaxRadius)) return fail(LIO_ERR_ARG, what + ": radius must be in 0..15");
    if (params && params->order != LIO_OVERLAY_DRAW_ORDER && params->order != LIO_OVERLAY_NEAREST)
        return fail(LIO_ERR_ARG, what + ": order must be 0 (LIO_OVERLAY_DRAW_ORDER) or 1 (LIO_OVERLAY_NEAREST)");
    if ((rc = open_handle(device, out, "lio_overlay_create: out is NULL"))) return rc;
    if (params) (*out)->p = *params, (*out)->disc = lio::overlay_disc(params->radius);
    return init_handle(out, what.c_str(), [](lio_overlay& z) { return lio::overlay_init(z.o, z.st); }, lio_overlay_destroy);
}

int lio_overlay_set_cloud(lio_overlay* h, const float* pts, int64_t n, int stride) {
    const std::string what = "lio_overlay_set_cloud";
    const int rc = null_handle(h, what.c_str());
    if (rc) return rc;
    if (n < 0 || n > lio::kOvMaxPoints) return fail(LIO_ERR_ARG, what + ": n must be in 0 .. 2^32 - 2");
    if (stride < 3 || stride > lio::kMaxFields) return fail(LIO_ERR_ARG, what + ": stride must be in 3..8");
    if (!pts && n > 0) return fail(LIO_ERR_ARG, what + ": pts is NULL");
    HIP_TRY(hipSetDevice(h->dev));
    return status(lio::overlay_set_cloud(h->o, pts, n, stride, h->st), what.c_str());
}

// what set_labels and set_colors share: the cloud is set, the values are as many as its points, and the other
// per-point source is not set (exactly one colour source applies)
static int overlay_source_arg(const std::string& what, const lio_overlay* h, const void* values, int64_t n, bool other,
                              const char* other_name) {
    if (!values) return LIO_OK;  // drops the source
    if (!h->o.have_cloud) return fail(LIO_ERR_STATE, what + ": no cloud (call lio_overlay_set_cloud first)");
    if (n != h->o.n) return fail(LIO_ERR_ARG, what + ": n must be the number of points of the cloud");
    if (other) return fail(LIO_ERR_ARG, what + ": " + other_name + " are set: one colour source at a time (drop them with NULL first)");
    return LIO_OK;
}

int lio_overlay_set_labels(lio_overlay* h, const int32_t* labels, int64_t n) {
    const std::string what = "lio_overlay_set_labels";
    int rc = null_handle(h, what.c_str());
    if (rc) return rc;
    if ((rc = overlay_source_arg(what, h, labels, n, h->o.have_colors, "per-point colours"))) return rc;
    HIP_TRY(hipSetDevice(h->dev));
    return status(lio::overlay_set_labels(h->o, labels, h->st), what.c_str());
}

int lio_overlay_set_colors(lio_overlay* h, const uint8_t* colors, int64_t n) {
    const std::string what = "lio_overlay_set_colors";
    int rc = null_handle(h, what.c_str());
    if (rc) return rc;
    if ((rc = overlay_source_arg(what, h, colors, n, h->o.have_labels, "labels"))) return rc;
    HIP_TRY(hipSetDevice(h->dev));
    return status(lio::overlay_set_colors(h->o, colors, h->st), what.c_str());
}

int lio_overlay_set_palette(lio_overlay* h, const uint8_t* palette, int32_t rows) {
    const std::string what = "lio_overlay_set_palette";
    const int rc = null_handle(h, what.c_str());
    if (rc) return rc;
    if (!palette) return fail(LIO_ERR_ARG, what + ": palette is NULL");
    if (rows < 1) return fail(LIO_ERR_ARG, what + ": rows must be at least 1");
    HIP_TRY(hipSetDevice(h->dev));
    return status(lio::overlay_set_palette(h->o, palette, rows, h->st), what.c_str());
}

// the checks lio_overlay_draw and lio_overlay_draw_undistorted share, the handle's first; `image`: the call's name of it
static int overlay_frame_arg(const std::string& what, const lio_overlay* h, const lio_camera* cam, const double* Rt,
                             const uint8_t* image, const char* image_name, const uint8_t* out, const int64_t* n_drawn,
                             lio::CamArg* a) {
    int rc = null_handle(h, what.c_str());
    if (rc) return rc;
    if ((rc = camera_arg(what, cam, Rt, a))) return rc;
    if (!image) return fail(LIO_ERR_ARG, what + ": " + image_name + " is NULL");
    if (!out) return fail(LIO_ERR_ARG, what + ": out is NULL");
    if (!n_drawn) return fail(LIO_ERR_ARG, what + ": n_drawn is NULL");
    return LIO_OK;
}

// after the handle: the cloud is set, and the owner image's int32 holds every index of it
static int overlay_state_arg(const std::string& what, const lio_overlay* h, const int32_t* owner_opt) {
    if (!h->o.have_cloud) return fail(LIO_ERR_STATE, what + ": no cloud (call lio_overlay_set_cloud first)");
    if (owner_opt && h->o.n > (int64_t)std::numeric_limits<int32_t>::max())
        return fail(LIO_ERR_ARG, what + ": owner_opt holds int32 indices: the cloud must have fewer than 2^31 points");
    return LIO_OK;
}

int lio_overlay_draw(lio_overlay* h, const lio_camera* cam, const double* Rt, const uint8_t* image, int64_t pitch, uint8_t* out,
                     int64_t out_pitch, int32_t* owner_opt, int64_t* n_drawn) {
    const std::string what = "lio_overlay_draw";
    lio::CamArg a{};
    int rc = overlay_frame_arg(what, h, cam, Rt, image, "image", out, n_drawn, &a);
    if (rc) return rc;
    if ((rc = pitch_arg(what, "pitch", pitch, 3, cam->width))) return rc;
    if ((rc = pitch_arg(what, "out_pitch", out_pitch, 3, cam->width))) return rc;
    if ((rc = overlay_state_arg(what, h, owner_opt))) return rc;
    *n_drawn = 0;
    HIP_TRY(hipSetDevice(h->dev));
    return status(lio::overlay_draw(h->o, nullptr, a, h->disc, h->p.order, image, pitch, out, out_pitch, owner_opt, n_drawn, h->st),
                  what.c_str());
}

int lio_overlay_draw_undistorted(lio_overlay* h, lio_undistorter* undistorter, const lio_camera* cam, const double* Rt,
                                 const uint8_t* raw_image, int64_t pitch, uint8_t* out, int64_t out_pitch, int32_t* owner_opt,
                                 int64_t* n_drawn) {
    const std::string what = "lio_overlay_draw_undistorted";
    lio::CamArg a{};
    int rc = overlay_frame_arg(what, h, cam, Rt, raw_image, "raw_image", out, n_drawn, &a);
    if (rc) return rc;
    if (!undistorter) return fail(LIO_ERR_ARG, what + ": undistorter is NULL");
    if (undistorter->dev != h->dev) return fail(LIO_ERR_ARG, what + ": both handles must be on one device");
    lio::UndistortBuf& u = undistorter->u;
    if ((rc = undistorter_frame_arg(what, u, pitch, out_pitch))) return rc;
    if (u.channels != 3) return fail(LIO_ERR_ARG, what + ": the undistorter must be set up for 3 channels");
    if (cam->width != u.dw || cam->height != u.dh)
        return fail(LIO_ERR_ARG, what + ": cam's width and height must be those of the undistorter's rectified image");
    if ((rc = overlay_state_arg(what, h, owner_opt))) return rc;
    *n_drawn = 0;
    HIP_TRY(hipSetDevice(h->dev));
    // as in lio_exposure_clahe_undistorted: the undistorter's buffers are used on h's stream
    return status(lio::overlay_draw(h->o, &u, a, h->disc, h->p.order, raw_image, pitch, out, out_pitch, owner_opt, n_drawn, h->st),
                  what.c_str());
}

int lio_overlay_get_timing(lio_overlay* h, double* ms5) {
    const int rc = null_handle(h, "lio_overlay_get_timing");
    if (rc) return rc;
    if (!ms5) return fail(LIO_ERR_ARG, "lio_overlay_get_timing: ms5 is NULL");
    return stage_times(h->o.timer, ms5);
}

}  // extern "C"
