// The undistortion mirrors of include/lio_gpu.hpp as a C++ maintainer uses them: Undistorter and undistort_map —
// the cv2.undistort(img, K, D, None, K) of post_process/undistort_image.py:21-27 on one frame.
//
//     undistort_api <scene.bin> <result.bin>
//
// scene.bin: 32 doubles, then the raw image (height rows of `pitch` bytes).  The doubles: src fx fy cx cy [0..3],
// dist [4..11], width height [12, 13]; has_dst [14], dst fx fy cx cy [15..18], width height [19, 20]; channels [21];
// border [22..24]; pitch [25]; out_pitch [26]; the byte the output buffer is filled with beforehand [27].
// result.bin: the output buffer (dst height rows of out_pitch bytes, padding included), then the map's sxy (int32)
// and axy (uint8).  tests/test_cpp_undistort.py writes the scenes and compares the bytes with Python's.
// Exit 77: no device.
#include <array>
#include <cstdio>
#include <vector>

#include "lio_gpu.hpp"

static bool read_all(const char* path, std::vector<uint8_t>& data) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    data.resize(n > 0 ? (size_t)n : 0);
    const bool ok = data.empty() || std::fread(data.data(), 1, data.size(), f) == data.size();
    std::fclose(f);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::printf("usage: undistort_api <scene.bin> <result.bin>\n");
        return 2;
    }
    std::vector<uint8_t> scene;
    if (!read_all(argv[1], scene) || scene.size() < 32 * sizeof(double)) {
        std::printf("FAIL: cannot read the scene %s\n", argv[1]);
        return 1;
    }
    const double* d = reinterpret_cast<const double*>(scene.data());
    lio_gpu::CameraModel src, dst;
    src.fx = d[0], src.fy = d[1], src.cx = d[2], src.cy = d[3];
    for (size_t k = 0; k < 8; ++k) src.dist[k] = d[4 + k];
    src.width = (int)d[12], src.height = (int)d[13];
    const bool has_dst = d[14] != 0.0;
    dst.fx = d[15], dst.fy = d[16], dst.cx = d[17], dst.cy = d[18];
    dst.width = (int)d[19], dst.height = (int)d[20];
    const int channels = (int)d[21];
    const std::array<uint8_t, 3> border = {(uint8_t)d[22], (uint8_t)d[23], (uint8_t)d[24]};
    const int64_t pitch = (int64_t)d[25], out_pitch = (int64_t)d[26];
    const uint8_t fill = (uint8_t)d[27];
    const uint8_t* image = scene.data() + 32 * sizeof(double);
    const int ow = has_dst ? dst.width : src.width, oh = has_dst ? dst.height : src.height;
    if (pitch < 1 || out_pitch < 1 || ow < 1 || oh < 1 || src.height < 1 ||
        scene.size() < 32 * sizeof(double) + (size_t)src.height * (size_t)pitch) {
        std::printf("FAIL: the scene is shorter than its header says\n");
        return 1;
    }
    try {
        lio_gpu::Undistorter ud;
        std::vector<uint8_t> out((size_t)oh * (size_t)out_pitch, fill), again;
        try {  // no camera yet: the library's state error
            ud.undistort(image, out.data(), pitch, out_pitch);
            std::printf("FAIL: undistort() before setCamera was accepted\n");
            return 1;
        } catch (const lio_gpu::Error& e) {
            if (e.code != LIO_ERR_STATE) throw;
        }
        ud.setCamera(src, has_dst ? &dst : nullptr, channels, border);
        ud.undistort(image, out.data(), pitch, out_pitch);
        again.assign(out.size(), fill);
        ud.undistort(image, again.data(), pitch, out_pitch);
        if (again != out) {
            std::printf("FAIL: a repeated frame gave other bytes\n");
            return 1;
        }
        const std::array<double, 3> ms = ud.timing();
        for (double v : ms)
            if (!(v >= 0.0)) {
                std::printf("FAIL: timing() returned %g\n", v);
                return 1;
            }
        lio_gpu::FilterGPU f;
        lio_gpu::UndistortMap map;
        lio_gpu::undistort_map(f, src, has_dst ? &dst : nullptr, map);
        FILE* o = std::fopen(argv[2], "wb");
        if (!o || std::fwrite(out.data(), 1, out.size(), o) != out.size() ||
            std::fwrite(map.sxy.data(), sizeof(int32_t), map.sxy.size(), o) != map.sxy.size() ||
            std::fwrite(map.axy.data(), 1, map.axy.size(), o) != map.axy.size()) {
            std::printf("FAIL: cannot write %s\n", argv[2]);
            return 1;
        }
        std::fclose(o);
        std::printf("%d x %d x %d -> %d x %d: upload %.3f ms, kernel %.3f ms, download %.3f ms\n", src.width, src.height,
                    channels, ow, oh, ms[0], ms[1], ms[2]);
        std::printf("ALL OK\n");
        return 0;
    } catch (const lio_gpu::Error& e) {
        std::printf("%s\n", e.what());
        return e.code == LIO_ERR_NODEV ? 77 : 1;
    }
}
