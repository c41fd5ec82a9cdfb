// lio_frame.hpp — the host path of one camera frame, shared by the camera leg's four handles (ColorizeBuf,
// UndistortBuf, ExposureBuf, OverlayBuf).  Host only, header only.
//   frame_span, frame_pitch, copy_rows              the byte arithmetic of a pitched image and the copy to a caller's rows
//   FrameStage, reserve_frames                      a device buffer and its pinned twin: reserve, upload, download, free
//   StageTimer<N>                                   the events of N stages and their times in ms
//   download_frame                                  the tail of a call that returns an image
//
// The first section needs no HIP header: define LIO_FRAME_NO_HIP before the include to get it alone
// (tests/cpp/frame_rows.cpp does).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace lio {

// the bytes from the first pixel to the last: the last row ends after its row_bytes, so nothing past it is read
// from (or written to) a caller's buffer
inline size_t frame_span(int rows, int64_t pitch, size_t row_bytes) { return (size_t)(rows - 1) * (size_t)pitch + row_bytes; }

// the device row pitch of a result: channels * width rounded up to 4 bytes (the kernels store full groups of 4
// pixels as dwords)
inline int64_t frame_pitch(int width, int channels) { return (int64_t)(((size_t)width * (size_t)channels + 3) & ~(size_t)3); }

// `rows` rows of row_bytes each; the padding of dst is not touched, that of src not read
inline void copy_rows(uint8_t* dst, int64_t dst_pitch, const uint8_t* src, int64_t src_pitch, size_t row_bytes, int rows) {
    if (dst_pitch == src_pitch && row_bytes == (size_t)src_pitch)
        std::memcpy(dst, src, row_bytes * (size_t)rows);
    else
        for (int i = 0; i < rows; ++i)
            std::memcpy(dst + (size_t)i * (size_t)dst_pitch, src + (size_t)i * (size_t)src_pitch, row_bytes);
}

}  // namespace lio

#ifndef LIO_FRAME_NO_HIP
#include <initializer_list>

#include "lio_scratch.hpp"

namespace lio {

// floor of the pinned image staging (grow_pinned)
constexpr size_t kImageStageFloor = (size_t)1 << 20;

// One image on the device and its pinned twin on the host.  The transfers return the HIP status: LIO_HIP(s.upload(..)).
struct FrameStage {
    uint8_t* dev = nullptr;
    size_t dev_bytes = 0;
    uint8_t* host = nullptr;
    size_t host_bytes = 0;

    // the staging copy, then the copy up: both belong to the stage whose events surround the call
    hipError_t upload(const uint8_t* image, size_t bytes, hipStream_t st) {
        std::memcpy(host, image, bytes);
        return hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, st);
    }
    hipError_t download(size_t bytes, hipStream_t st) { return hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st); }
    void free() {
        dev_free(&dev);
        host_free(&host);
        dev_bytes = host_bytes = 0;
    }
};

// Every stage of the list holds its bytes (0: that stage is left alone): the pinned halves first, then the device
// halves, each in the order of the list.  A call reserves before it enqueues anything: hipFree synchronises the device.
struct FrameNeed {
    FrameStage* s;
    size_t bytes;
};
inline int reserve_frames(std::initializer_list<FrameNeed> needs) {
    int rc = kOk;
    for (const FrameNeed& n : needs)
        if (!rc && n.bytes) rc = grow_pinned(&n.s->host, n.s->host_bytes, n.bytes, kImageStageFloor);
    for (const FrameNeed& n : needs)
        if (!rc && n.bytes) rc = grow_scratch(reinterpret_cast<void**>(&n.s->dev), n.s->dev_bytes, n.bytes);
    return rc;
}

// Stage k of a call runs from ev[k] to ev[k + 1]; ms holds the times of the last call that finished.
template <int N>
struct StageTimer {
    hipEvent_t ev[N + 1] = {};
    float ms[N] = {};

    hipError_t init() {
        for (hipEvent_t& e : ev)
            if (const hipError_t rc = hipEventCreate(&e)) return rc;
        return hipSuccess;
    }
    void free() {
        for (hipEvent_t& e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
    }
    // the boundaries first .. last, back to back: stages first .. last - 1 are skipped and take no time
    hipError_t mark(int first, int last, hipStream_t st) {
        for (int k = first; k <= last; ++k)
            if (const hipError_t rc = hipEventRecord(ev[k], st)) return rc;
        return hipSuccess;
    }
    hipError_t mark(int k, hipStream_t st) { return mark(k, k, st); }
    // the wait for the stream, then the stage times
    hipError_t finish(hipStream_t st) {
        if (const hipError_t rc = hipStreamSynchronize(st)) return rc;
        for (int k = 0; k < N; ++k)
            if (const hipError_t rc = hipEventElapsedTime(&ms[k], ev[k], ev[k + 1])) return rc;
        return hipSuccess;
    }
};

// The tail of a call whose result is s.dev, `rows` rows of frame_pitch(width, channels) bytes: the copy down as the
// last stage, the wait and the stage times, then the caller's rows: channels * width bytes each, its padding is
// not touched.
template <int N>
int download_frame(FrameStage& s, StageTimer<N>& t, int width, int rows, int channels, uint8_t* out, int64_t out_pitch,
                   hipStream_t st) {
    const int64_t d_pitch = frame_pitch(width, channels);
    LIO_HIP(s.download((size_t)d_pitch * (size_t)rows, st));
    LIO_HIP(t.mark(N, st));
    LIO_HIP(t.finish(st));
    copy_rows(out, out_pitch, s.host, d_pitch, (size_t)width * (size_t)channels, rows);
    return kOk;
}

}  // namespace lio
#endif  // LIO_FRAME_NO_HIP
