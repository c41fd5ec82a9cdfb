// The camera mirrors of include/lio_gpu.hpp as a C++ maintainer uses them: CameraModel, project_points and
// Colorizer — the calls of post_process/colorize_pcd.py:31-65 and of projectPointsToImagePlane
// (post_process/lidar_projection/src/lidar_projection.cpp:9-34).  On the GPU every output is checked bit for bit
// against the contract written out here in plain C++ (this file is built with -ffp-contract=off): the projection
// in its written order, a sequential z-buffer, the strict-less accumulation.  Exit 77: no device.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "lio_gpu.hpp"

using lio_gpu::PointXYZI;

static uint32_t g_state = 13579u;
static double frand() {  // [0, 1)
    g_state = g_state * 1664525u + 1013904223u;
    return (double)(g_state >> 8) * (1.0 / 16777216.0);
}

struct P {
    double u, v, zc;
    int px, py;
    bool valid;
};

// the contract's projection (lio_gpu.h, lio_project_points)
static P project(const PointXYZI& q, const lio_gpu::CameraModel& c, const std::array<double, 12>& Rt) {
    const double x = q.x, y = q.y, z = q.z;
    const double xc = ((Rt[0] * x + Rt[1] * y) + Rt[2] * z) + Rt[9];
    const double yc = ((Rt[3] * x + Rt[4] * y) + Rt[5] * z) + Rt[10];
    const double zc = ((Rt[6] * x + Rt[7] * y) + Rt[8] * z) + Rt[11];
    const double xn = xc / zc, yn = yc / zc;
    const double r2 = xn * xn + yn * yn;
    const double k1 = c.dist[0], k2 = c.dist[1], p1 = c.dist[2], p2 = c.dist[3], k3 = c.dist[4], k4 = c.dist[5], k5 = c.dist[6],
                 k6 = c.dist[7];
    const double num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
    const double den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2;
    const double rad = num / den;
    const double a1 = (2.0 * xn) * yn, a2 = r2 + (2.0 * xn) * xn, a3 = r2 + (2.0 * yn) * yn;
    const double xd = xn * rad + (p1 * a1 + p2 * a2);
    const double yd = yn * rad + (p1 * a3 + p2 * a1);
    P o;
    o.u = c.fx * xd + c.cx;
    o.v = c.fy * yd + c.cy;
    o.zc = zc;
    o.valid = zc > 0.0 && r2 <= c.r2_max && o.u >= 0.0 && o.u < (double)c.width && o.v >= 0.0 && o.v < (double)c.height;
    o.px = o.valid ? (int)o.u : -1;
    o.py = o.valid ? (int)o.v : -1;
    return o;
}

static uint32_t float_bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, sizeof b);
    return b;
}

struct State {
    std::vector<double> best_z;
    std::vector<uint8_t> rgb;
    std::vector<int32_t> frame;
    int32_t frames = 0;
    explicit State(size_t n) : best_z(n, std::numeric_limits<double>::infinity()), rgb(3 * n, 0), frame(n, -1) {}
};

// one frame of the accumulation; the image is B G R, rows of `pitch` bytes
static int64_t add_frame(State& s, const std::vector<PointXYZI>& cloud, const lio_gpu::CameraModel& c,
                         const std::array<double, 12>& Rt, const std::vector<uint8_t>& img, int64_t pitch, bool occlusion,
                         int radius, float rel, float abs_) {
    std::vector<P> pr(cloud.size());
    for (size_t i = 0; i < cloud.size(); ++i) pr[i] = project(cloud[i], c, Rt);
    std::vector<uint32_t> D((size_t)c.width * (size_t)c.height, 0x7f800000u);
    if (occlusion)
        for (const P& p : pr) {
            if (!p.valid) continue;
            const uint32_t zb = float_bits((float)p.zc);
            for (int qy = std::max(p.py - radius, 0); qy <= std::min(p.py + radius, c.height - 1); ++qy)
                for (int qx = std::max(p.px - radius, 0); qx <= std::min(p.px + radius, c.width - 1); ++qx) {
                    uint32_t& d = D[(size_t)qy * (size_t)c.width + (size_t)qx];
                    d = std::min(d, zb);
                }
        }
    int64_t updated = 0;
    for (size_t i = 0; i < cloud.size(); ++i) {
        const P& p = pr[i];
        if (!p.valid) continue;
        if (occlusion) {
            float d;
            std::memcpy(&d, &D[(size_t)p.py * (size_t)c.width + (size_t)p.px], sizeof d);
            const float bound = (d * (1.0f + rel)) + abs_;
            if (!((float)p.zc <= bound)) continue;
        }
        if (!(p.zc < s.best_z[i])) continue;
        const uint8_t* q = &img[(size_t)p.py * (size_t)pitch + (size_t)p.px * 3];
        s.best_z[i] = p.zc;
        s.rgb[3 * i] = q[2], s.rgb[3 * i + 1] = q[1], s.rgb[3 * i + 2] = q[0];
        s.frame[i] = s.frames;
        ++updated;
    }
    ++s.frames;
    return updated;
}

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}

int main() {
    try {
        lio_gpu::FilterGPU f;
        // a 96 x 64 camera with the rig's 5-parameter distortion scaled to it, rows padded to 300 bytes
        lio_gpu::CameraModel cam;
        cam.fx = 70.0, cam.fy = 71.0, cam.cx = 47.3, cam.cy = 32.6;
        cam.dist = {-0.2972345646, 0.08469466538, -0.0004248149362, -0.000175399726, 0.0, 0.0, 0.0, 0.0};
        cam.r2_max = 1.5;
        cam.width = 96, cam.height = 64;
        const int64_t pitch = 300;
        std::vector<std::vector<uint8_t>> imgs(3, std::vector<uint8_t>((size_t)(cam.height * pitch)));
        for (auto& im : imgs)
            for (uint8_t& b : im) b = (uint8_t)(256.0 * frand());
        // three poses: small rotations about y and x, the camera moved along its axis
        std::vector<std::array<double, 12>> poses;
        for (double a : {0.0, 0.25, -0.2}) {
            const double c = std::cos(a), s = std::sin(a);
            poses.push_back({c, 0.0, s, 0.0, 1.0, 0.0, -s, 0.0, c, 0.1 * a, -0.05, 1.0 + a});
        }
        // a wall of 3000 points at z ~ 4 and 1500 nearer points in front of a part of it; some behind the camera
        std::vector<PointXYZI> cloud(4500);
        for (size_t i = 0; i < cloud.size(); ++i) {
            const bool nearer = i >= 3000;
            const double z = nearer ? 1.5 + 0.5 * frand() : (i % 50 == 0 ? -3.0 : 4.0 + 0.01 * frand());
            cloud[i] = {(float)((nearer ? 1.2 : 8.0) * (frand() - 0.5)), (float)((nearer ? 1.0 : 6.0) * (frand() - 0.5)), (float)z,
                        (float)(255.0 * frand())};
        }

        lio_gpu::Projection pr;
        lio_gpu::project_points(f, cloud, cam, poses[1], pr);
        size_t n_valid = 0;
        for (size_t i = 0; i < cloud.size(); ++i) {
            const P e = project(cloud[i], cam, poses[1]);
            const bool ok = std::memcmp(&pr.uv[2 * i], &e.u, 8) == 0 && std::memcmp(&pr.uv[2 * i + 1], &e.v, 8) == 0 &&
                            std::memcmp(&pr.zc[i], &e.zc, 8) == 0 && pr.pix[2 * i] == e.px && pr.pix[2 * i + 1] == e.py &&
                            (pr.valid[i] != 0) == e.valid;
            if (!ok) {
                std::printf("FAIL: project_points differs from the contract written out in C++ at point %zu\n", i);
                return 1;
            }
            n_valid += e.valid;
        }
        if (n_valid < 500 || n_valid > 4000) {
            std::printf("FAIL: the scene does not exercise the mask (%zu valid)\n", n_valid);
            return 1;
        }
        std::printf("project_points: %zu of %zu points valid\n", n_valid, cloud.size());

        lio_gpu::Colorizer<PointXYZI> cz;
        std::vector<uint8_t> rgb;
        std::vector<int32_t> frame;
        std::vector<double> depth;
        try {  // no cloud yet: the library's state error
            cz.colors(rgb, frame);
            std::printf("FAIL: colors() before setInputCloud was accepted\n");
            return 1;
        } catch (const lio_gpu::Error& e) {
            if (e.code != LIO_ERR_STATE) throw;
        }
        cz.setInputCloud(&cloud);
        for (int occlusion = 0; occlusion < 2; ++occlusion) {
            const int radius = occlusion ? 2 : 0;
            const float rel = occlusion ? 0.05f : 0.f, abs_ = occlusion ? 0.02f : 0.f;
            cz.setOcclusion(occlusion != 0, radius, rel, abs_);
            cz.reset();
            State st(cloud.size());
            // the three poses, then the first again with another image: every depth ties, the first frame stays
            const int order[4] = {0, 1, 2, 0};
            for (int k = 0; k < 4; ++k) {
                const std::vector<uint8_t>& im = imgs[(size_t)(k == 3 ? 1 : order[k])];
                const int64_t got = cz.addFrame(cam, poses[(size_t)order[k]], im.data(), pitch);
                const int64_t want = add_frame(st, cloud, cam, poses[(size_t)order[k]], im, pitch, occlusion != 0, radius, rel, abs_);
                if (got != want || (k == 3 && got != 0)) {
                    std::printf("FAIL: frame %d (occlusion %d) replaced %lld points, the contract says %lld\n", k, occlusion,
                                (long long)got, (long long)want);
                    return 1;
                }
            }
            cz.colors(rgb, frame, &depth);
            if (rgb != st.rgb || frame != st.frame || !same_bits(depth, st.best_z)) {
                std::printf("FAIL: the state differs from the contract written out in C++ (occlusion %d)\n", occlusion);
                return 1;
            }
            const size_t coloured = (size_t)std::count_if(frame.begin(), frame.end(), [](int32_t v) { return v >= 0; });
            std::printf("occlusion %d: %zu of %zu points coloured over 4 frames\n", occlusion, coloured, cloud.size());
        }
        std::printf("ALL OK\n");
        return 0;
    } catch (const lio_gpu::Error& e) {
        std::printf("%s\n", e.what());
        return e.code == LIO_ERR_NODEV ? 77 : 1;
    }
}
