// frame_rows.cpp — the byte arithmetic of csrc/lio_frame.hpp on the host alone (no HIP, no GPU): the span and the
// device pitch of a pitched image, and copy_rows, the copy of a result to the caller's rows.
// Built with -fsanitize=address,undefined by tests/test_frame_rows.py: the source and the destination are heap
// blocks of exactly their span, so a read or a write one byte past the last row's pixels is a sanitizer report.
#define LIO_FRAME_NO_HIP
#include "../../fast-lio-sam_gps_amd/csrc/lio_frame.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {

int failures = 0;
#define CHECK(cond)                                                 \
    do {                                                            \
        if (!(cond)) {                                              \
            std::printf("FAIL line %d: %s\n", __LINE__, #cond);     \
            ++failures;                                             \
        }                                                           \
    } while (0)

constexpr uint8_t kSentinel = 0xee, kSrcPad = 0xcc;  // pixel values stay below 200

uint8_t pixel(int row, size_t byte) { return (uint8_t)((row * 131 + byte * 7 + 1) % 200); }

void run(int width, int channels, int rows, int64_t dst_pitch, int64_t src_pitch) {
    const size_t row_bytes = (size_t)width * (size_t)channels;
    const size_t src_span = lio::frame_span(rows, src_pitch, row_bytes);
    const size_t dst_span = lio::frame_span(rows, dst_pitch, row_bytes);
    auto* src = static_cast<uint8_t*>(std::malloc(src_span));
    auto* dst = static_cast<uint8_t*>(std::malloc(dst_span));
    CHECK(src && dst);
    if (!src || !dst) return;
    std::memset(src, kSrcPad, src_span);
    std::memset(dst, kSentinel, dst_span);
    for (int i = 0; i < rows; ++i)
        for (size_t b = 0; b < row_bytes; ++b) src[(size_t)i * (size_t)src_pitch + b] = pixel(i, b);

    lio::copy_rows(dst, dst_pitch, src, src_pitch, row_bytes, rows);

    size_t bad_pixels = 0, bad_padding = 0;
    for (size_t at = 0; at < dst_span; ++at) {
        const int i = (int)(at / (size_t)dst_pitch);
        const size_t b = at % (size_t)dst_pitch;
        if (b < row_bytes)
            bad_pixels += dst[at] != pixel(i, b);
        else
            bad_padding += dst[at] != kSentinel;
    }
    if (bad_pixels || bad_padding)
        std::printf("width %d channels %d rows %d dst_pitch %lld src_pitch %lld: %zu pixel bytes differ, %zu padding bytes "
                    "written\n",
                    width, channels, rows, (long long)dst_pitch, (long long)src_pitch, bad_pixels, bad_padding);
    CHECK(bad_pixels == 0);
    CHECK(bad_padding == 0);
    std::free(src);
    std::free(dst);
}

}  // namespace

int main() {
    // the span: the last row ends after its pixels; one row is its pixels whatever the pitch
    CHECK(lio::frame_span(1, 4096, 15) == 15);
    CHECK(lio::frame_span(1, 15, 15) == 15);
    CHECK(lio::frame_span(5, 16, 15) == 4 * 16 + 15);
    // the largest image of the camera leg with a padded pitch: past 2^31, exact as a size_t
    const int64_t big_pitch = 3 * 32767 + 7;
    CHECK(lio::frame_span(32767, big_pitch, 3 * 32767) == (size_t)32766 * (size_t)98308 + (size_t)98301);
    CHECK(lio::frame_span(32767, big_pitch, 3 * 32767) == (size_t)3221258229ull);
    CHECK(lio::frame_span(32767, big_pitch, 3 * 32767) > ((size_t)1 << 31));

    // the device pitch: channels * width rounded up to 4
    CHECK(lio::frame_pitch(1, 1) == 4);
    CHECK(lio::frame_pitch(4, 1) == 4);
    CHECK(lio::frame_pitch(5, 3) == 16);
    CHECK(lio::frame_pitch(32767, 3) == 98304);

    const int widths[] = {1, 3, 4, 5, 67}, chans[] = {1, 3}, heights[] = {1, 2, 5};
    int cases = 0;
    for (int w : widths)
        for (int c : chans)
            for (int h : heights) {
                const int64_t row_bytes = (int64_t)w * c;
                const int64_t pitches[] = {row_bytes, lio::frame_pitch(w, c), row_bytes + 7};
                for (int64_t dp : pitches)
                    for (int64_t sp : pitches) run(w, c, h, dp, sp), ++cases;
            }
    CHECK(cases == 5 * 2 * 3 * 9);
    if (failures) return 1;
    std::printf("ALL OK\n");
    return 0;
}
