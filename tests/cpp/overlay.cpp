// The overlay mirror of include/lio_gpu.hpp as a C++ maintainer uses it: PointOverlay draws one seeded frame the way
// post_process/lidar_projection/src/lidar_projection.cpp:113-125 does (a filled disc per projected point) and prints
// digests of the owner image, the drawn image with its row padding, and the number of points drawn.
// tests/test_cpp_overlay.py builds the same scene with the same generator (tests/overlay_ref.py: cpp_scene) and
// compares the digests with the contract restated in numpy.  Exit 77: no device.
#include <array>
#include <cstdio>
#include <vector>

#include "lio_gpu.hpp"

using lio_gpu::PointXYZI;

static uint32_t g_state = 24680u;
static double frand() {  // [0, 1)
    g_state = g_state * 1664525u + 1013904223u;
    return (double)(g_state >> 8) * (1.0 / 16777216.0);
}

static unsigned long long fnv1a(const void* data, size_t bytes) {
    unsigned long long h = 0xCBF29CE484222325ull;
    const uint8_t* p = static_cast<const uint8_t*>(data);
    for (size_t i = 0; i < bytes; ++i) h = (h ^ p[i]) * 0x100000001B3ull;
    return h;
}

int main() {
    try {
        // a 96 x 64 camera with the rig's 5-parameter distortion scaled to it, rows padded to 300 bytes
        lio_gpu::CameraModel cam;
        cam.fx = 70.0, cam.fy = 71.0, cam.cx = 47.3, cam.cy = 32.6;
        cam.dist = {-0.2972345646, 0.08469466538, -0.0004248149362, -0.000175399726, 0.0, 0.0, 0.0, 0.0};
        cam.r2_max = 1.5;
        cam.width = 96, cam.height = 64;
        const int64_t pitch = 300;
        const std::array<double, 12> Rt = {0.96875, 0.0, 0.25, 0.0, 1.0, 0.0, -0.25, 0.0, 0.96875, 0.05, -0.05, 1.25};
        std::vector<uint8_t> image((size_t)(cam.height * pitch));
        for (uint8_t& b : image) b = (uint8_t)(256.0 * frand());
        // 1500 points in front of the camera, every 50th behind it; labels -1 .. 5 against a palette of 3 rows
        std::vector<PointXYZI> cloud(1500);
        std::vector<int32_t> labels(cloud.size());
        for (size_t i = 0; i < cloud.size(); ++i) {
            const double z = i % 50 == 0 ? -3.0 : 1.5 + 4.0 * frand();
            const double x = 6.0 * (frand() - 0.5);
            const double y = 4.0 * (frand() - 0.5);
            const double intensity = 255.0 * frand();
            cloud[i] = {(float)x, (float)y, (float)z, (float)intensity};
            labels[i] = (int32_t)(7.0 * frand()) - 1;
        }
        const std::vector<std::array<uint8_t, 3>> palette = {{255, 0, 0}, {0, 0, 255}, {255, 255, 0}};

        // the nearest point wins, in its cluster's colour; the result goes to a copy's rows
        lio_gpu::PointOverlay<PointXYZI> nearest(3, true);
        std::vector<int32_t> owner;
        try {  // no cloud yet: the library's state error
            std::vector<uint8_t> out(image);
            nearest.draw(cam, Rt, image.data(), out.data(), pitch, pitch);
            std::printf("FAIL: draw() before setInputCloud was accepted\n");
            return 1;
        } catch (const lio_gpu::Error& e) {
            if (e.code != LIO_ERR_STATE) throw;
        }
        nearest.setInputCloud(&cloud);
        nearest.setPalette(palette);
        nearest.setLabels(&labels);
        std::vector<uint8_t> out(image);
        long long drawn = (long long)nearest.draw(cam, Rt, image.data(), out.data(), pitch, pitch, &owner);
        std::printf("nearest: owner=%016llx image=%016llx n_drawn=%lld\n", fnv1a(owner.data(), owner.size() * sizeof(int32_t)),
                    fnv1a(out.data(), out.size()), drawn);

        // the tool as shipped: draw order, every point green, drawn in place
        lio_gpu::PointOverlay<PointXYZI> tool;
        tool.setInputCloud(&cloud);
        out = image;
        drawn = (long long)tool.draw(cam, Rt, out.data(), out.data(), pitch, pitch, &owner);
        std::printf("tool: owner=%016llx image=%016llx n_drawn=%lld\n", fnv1a(owner.data(), owner.size() * sizeof(int32_t)),
                    fnv1a(out.data(), out.size()), drawn);
        const std::array<double, 5> ms = tool.timing();
        if (!(ms[2] > 0.0) || !(ms[3] > 0.0)) {
            std::printf("FAIL: the stamp and compose stages report no time\n");
            return 1;
        }
        std::printf("ALL OK\n");
        return 0;
    } catch (const lio_gpu::Error& e) {
        std::printf("%s\n", e.what());
        return e.code == LIO_ERR_NODEV ? 77 : 1;
    }
}
