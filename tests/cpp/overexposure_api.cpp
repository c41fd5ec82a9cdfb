// The stencil mirrors of include/lio_gpu.hpp as a C++ maintainer uses them: Exposure::recover (the
// recover_overexposure of post_process/exposure_adaption/solve_overexposure:6-32), Exposure::gaussian_blur and
// lio_gpu::gaussian_weights.
//
//     overexposure_api --weights <ksize> <sigma>     the weights, one line of numbers (no device)
//     overexposure_api <scene.bin> <result.bin>
//
// scene.bin: 16 doubles, then the image (height rows of `pitch` bytes).  The doubles: width height channels order
// [0..3], pitch out_pitch [4, 5], the byte the output buffers are filled with beforehand [6], threshold dilate ksize
// sigma [7..10].
// result.bin: the recover output buffer (height rows of out_pitch bytes, padding included), then the gaussian_blur
// output buffer likewise.  The FNV-1a 64 hash of each is printed ("recover <hex>", "gaussian_blur <hex>");
// tests/test_cpp_overexposure.py writes the scene and compares the hashes with the numpy restatement's.
// Exit 77: no device.
#include <array>
#include <cstdio>
#include <cstdlib>
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

static uint64_t fnv1a(const std::vector<uint8_t>& data) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint8_t b : data) h = (h ^ b) * 0x100000001b3ull;
    return h;
}

int main(int argc, char** argv) {
    try {
        if (argc == 4 && std::string(argv[1]) == "--weights") {
            const std::vector<uint16_t> w = lio_gpu::gaussian_weights(std::atoi(argv[2]), std::atof(argv[3]));
            for (size_t i = 0; i < w.size(); ++i) std::printf("%d%c", (int)w[i], i + 1 < w.size() ? ' ' : '\n');
            return 0;
        }
        if (argc != 3) {
            std::printf("usage: overexposure_api --weights <ksize> <sigma> | <scene.bin> <result.bin>\n");
            return 2;
        }
        std::vector<uint8_t> scene;
        constexpr size_t kHead = 16 * sizeof(double);
        if (!read_all(argv[1], scene) || scene.size() < kHead) {
            std::printf("FAIL: cannot read the scene %s\n", argv[1]);
            return 1;
        }
        const double* d = reinterpret_cast<const double*>(scene.data());
        const int width = (int)d[0], height = (int)d[1], channels = (int)d[2], order = (int)d[3];
        const int64_t pitch = (int64_t)d[4], out_pitch = (int64_t)d[5];
        const uint8_t fill = (uint8_t)d[6];
        lio_gpu::RecoverParams p;
        p.threshold = (int)d[7], p.dilate = (int)d[8], p.ksize = (int)d[9], p.sigma = d[10];
        if (width < 1 || height < 1 || pitch < 1 || out_pitch < 1 || scene.size() < kHead + (size_t)height * (size_t)pitch) {
            std::printf("FAIL: the scene is shorter than its header says\n");
            return 1;
        }
        const uint8_t* image = scene.data() + kHead;
        lio_gpu::Exposure ex;
        std::vector<uint8_t> out((size_t)height * (size_t)out_pitch, fill), again(out.size(), fill), blurred(out.size(), fill);
        ex.recover(image, width, height, channels, out.data(), p, order, pitch, out_pitch);
        const std::array<double, 3> ms = ex.stencil_timing();
        ex.recover(image, width, height, channels, again.data(), p, order, pitch, out_pitch);
        if (again != out) {
            std::printf("FAIL: a repeated frame gave other bytes\n");
            return 1;
        }
        for (double v : ms)
            if (!(v >= 0.0)) {
                std::printf("FAIL: stencil_timing() returned %g\n", v);
                return 1;
            }
        ex.gaussian_blur(image, width, height, channels, blurred.data(), p.ksize, p.sigma, pitch, out_pitch);
        try {  // an even kernel: the library's argument error
            ex.gaussian_blur(image, width, height, channels, again.data(), 4, 0.0, pitch, out_pitch);
            std::printf("FAIL: gaussian_blur() with an even ksize was accepted\n");
            return 1;
        } catch (const lio_gpu::Error& e) {
            if (e.code != LIO_ERR_ARG) throw;
        }
        FILE* o = std::fopen(argv[2], "wb");
        bool ok = o != nullptr;
        ok = ok && std::fwrite(out.data(), 1, out.size(), o) == out.size();
        ok = ok && std::fwrite(blurred.data(), 1, blurred.size(), o) == blurred.size();
        if (o) std::fclose(o);
        if (!ok) {
            std::printf("FAIL: cannot write %s\n", argv[2]);
            return 1;
        }
        std::printf("%d x %d x %d: upload %.3f ms, kernel %.3f ms, download %.3f ms\n", width, height, channels, ms[0], ms[1], ms[2]);
        std::printf("recover %016llx\ngaussian_blur %016llx\n", (unsigned long long)fnv1a(out), (unsigned long long)fnv1a(blurred));
        std::printf("ALL OK\n");
        return 0;
    } catch (const lio_gpu::Error& e) {
        std::printf("%s\n", e.what());
        return e.code == LIO_ERR_NODEV ? 77 : 1;
    }
}
