// The exposure mirrors of include/lio_gpu.hpp as a C++ maintainer uses them: Exposure and the table helpers — the
// adapt_exposure of post_process/exposure_adaption/CLAHE_region_adjusted.py:6-41 and the tables of correct_exposure.
//
//     exposure_api --luts                      gamma_lut(0.8) and gamma_lut(1.2), 256 numbers per line (no device)
//     exposure_api <scene.bin> <result.bin>
//
// scene.bin: 16 doubles, the image (height rows of `pitch` bytes), lut_v (256 bytes), lut_all (256 bytes).  The
// doubles: width height channels order [0..3], pitch out_pitch [4, 5], the byte the output buffers are filled with
// beforehand [6], clip_limit tiles_x tiles_y [7..9].
// result.bin: the CLAHE output buffer (height rows of out_pitch bytes, padding included), the remap output buffer
// (lut_v and lut_all) likewise, hist_v and hist_gray (256 int64 each), then 256 bytes each of gamma_lut(0.8),
// gamma_lut(1.2), equalize_lut(hist_v) and stretch_lut(hist_v) (zeros where its percentiles are equal).
// tests/test_cpp_exposure.py writes the scenes and compares the bytes with the numpy restatement.  Exit 77: no device.
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

static void print_lut(const lio_gpu::ExposureLut& lut) {
    for (size_t i = 0; i < lut.size(); ++i) std::printf("%d%c", (int)lut[i], i + 1 < lut.size() ? ' ' : '\n');
}

int main(int argc, char** argv) {
    if (argc == 2 && std::string(argv[1]) == "--luts") {
        print_lut(lio_gpu::gamma_lut(0.8));
        print_lut(lio_gpu::gamma_lut(1.2));
        return 0;
    }
    if (argc != 3) {
        std::printf("usage: exposure_api --luts | <scene.bin> <result.bin>\n");
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
    const double clip_limit = d[7];
    const int tiles_x = (int)d[8], tiles_y = (int)d[9];
    if (width < 1 || height < 1 || pitch < 1 || out_pitch < 1 || scene.size() < kHead + (size_t)height * (size_t)pitch + 512) {
        std::printf("FAIL: the scene is shorter than its header says\n");
        return 1;
    }
    const uint8_t* image = scene.data() + kHead;
    lio_gpu::ExposureLut lut_v{}, lut_all{};
    std::memcpy(lut_v.data(), image + (size_t)height * (size_t)pitch, 256);
    std::memcpy(lut_all.data(), image + (size_t)height * (size_t)pitch + 256, 256);
    try {
        lio_gpu::Exposure ex;
        std::vector<uint8_t> out((size_t)height * (size_t)out_pitch, fill), again, mapped(out.size(), fill);
        ex.clahe(image, width, height, channels, out.data(), clip_limit, tiles_x, tiles_y, order, pitch, out_pitch);
        const std::array<double, 5> ms = ex.timing();
        again.assign(out.size(), fill);
        ex.clahe(image, width, height, channels, again.data(), clip_limit, tiles_x, tiles_y, order, pitch, out_pitch);
        if (again != out) {
            std::printf("FAIL: a repeated frame gave other bytes\n");
            return 1;
        }
        for (double v : ms)
            if (!(v >= 0.0)) {
                std::printf("FAIL: timing() returned %g\n", v);
                return 1;
            }
        ex.remap(image, width, height, channels, &lut_v, &lut_all, mapped.data(), order, pitch, out_pitch);
        try {  // no table at all: the library's argument error
            ex.remap(image, width, height, channels, nullptr, nullptr, again.data(), order, pitch, out_pitch);
            std::printf("FAIL: remap() without a table was accepted\n");
            return 1;
        } catch (const lio_gpu::Error& e) {
            if (e.code != LIO_ERR_ARG) throw;
        }
        lio_gpu::ExposureHist hist_v{}, hist_gray{};
        ex.histograms(image, width, height, channels, &hist_v, &hist_gray, order, pitch);
        const lio_gpu::ExposureLut g08 = lio_gpu::gamma_lut(0.8), g12 = lio_gpu::gamma_lut(1.2), eq = lio_gpu::equalize_lut(hist_v);
        lio_gpu::ExposureLut st{};
        if (lio_gpu::hist_percentile(hist_v, 5.0) != lio_gpu::hist_percentile(hist_v, 95.0)) st = lio_gpu::stretch_lut(hist_v);
        FILE* o = std::fopen(argv[2], "wb");
        bool ok = o != nullptr;
        ok = ok && std::fwrite(out.data(), 1, out.size(), o) == out.size();
        ok = ok && std::fwrite(mapped.data(), 1, mapped.size(), o) == mapped.size();
        ok = ok && std::fwrite(hist_v.data(), sizeof(int64_t), 256, o) == 256;
        ok = ok && std::fwrite(hist_gray.data(), sizeof(int64_t), 256, o) == 256;
        for (const lio_gpu::ExposureLut& t : {g08, g12, eq, st}) ok = ok && std::fwrite(t.data(), 1, 256, o) == 256;
        if (o) std::fclose(o);
        if (!ok) {
            std::printf("FAIL: cannot write %s\n", argv[2]);
            return 1;
        }
        std::printf("%d x %d x %d, %d x %d tiles: upload %.3f ms, histogram %.3f ms, LUT %.3f ms, apply %.3f ms, download %.3f ms"
                    " (%s)\n",
                    width, height, channels, tiles_x, tiles_y, ms[0], ms[1], ms[2], ms[3], ms[4],
                    lio_gpu::detect_exposure(hist_gray) > 0 ? "overexposed" : (lio_gpu::detect_exposure(hist_gray) < 0 ? "underexposed" : "well-exposed"));
        std::printf("ALL OK\n");
        return 0;
    } catch (const lio_gpu::Error& e) {
        std::printf("%s\n", e.what());
        return e.code == LIO_ERR_NODEV ? 77 : 1;
    }
}
