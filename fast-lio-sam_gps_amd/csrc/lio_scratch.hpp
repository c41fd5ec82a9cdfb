// lio_scratch.hpp — the host-side plumbing every scratch struct shares.  Host only, header only.
//   status codes, LIO_HIP, nblk(), grown()          every driver
//   Carver, carve_arena, reserve_arena              the one-arena reserves: DenoiseBuf, ClusterBuf, PlaneBuf (sized by a
//                                                   capacity the caller keeps), GpsAlignBuf, ProjectBuf, ExposureBuf (sized
//                                                   per call)
//   dev_free, dev_alloc_all, grow_buf, grow_scratch device buffers: FilterBuf, GridBuf, MapUpdBuf, ColorizeBuf,
//                                                   UndistortBuf, ExposureBuf, FrameStage and the C-ABI's handles
//   host_free, grow_pinned                          pinned host buffers: the sweep staging (FilterBuf), the image staging
//                                                   (FrameStage in lio_frame.hpp, which ColorizeBuf, UndistortBuf and
//                                                   ExposureBuf hold), GpsAlignBuf::h_part, DenoiseBuf::h_dist,
//                                                   ExposureBuf::h_small
// The hipcub sort / scan pair is in lio_scratch_cub.hpp.
//
// The first section needs no HIP header: define LIO_SCRATCH_NO_HIP before the include to get it alone
// (tests/cpp/scratch_layout.cpp does).
#pragma once
#include <cstddef>
#include <cstdint>

namespace lio {

// status of the internal drivers; the values of LIO_OK, LIO_ERR_ARG, LIO_ERR_HIP and LIO_ERR_NOMEM
// (lio_capi_util.hpp asserts it and turns them into the public code and message)
constexpr int kOk = 0, kArg = -1, kHip = -2, kNoMem = -5;

// Carves one arena into 256-byte-aligned slots.  A reserve lists its fields ONCE, in a function of a Carver&,
// and carve_arena runs that function twice: over Carver{} to measure (every field is set to null, bytes() is
// the arena size), then over Carver{arena} to assign.  A zero-count field takes no space.
class Carver {
public:
    explicit Carver(void* base = nullptr) : base_(static_cast<uint8_t*>(base)) {}
    template <class T>
    void operator()(T*& p, size_t count) {
        p = reinterpret_cast<T*>(take(count * sizeof(T)));
    }
    void operator()(void*& p, size_t bytes) { p = take(bytes); }
    size_t bytes() const { return off_; }

private:
    uint8_t* take(size_t bytes) {
        uint8_t* at = base_ ? base_ + off_ : nullptr;
        off_ += (bytes + 255) & ~(size_t)255;
        return at;
    }
    uint8_t* base_;
    size_t off_ = 0;
};

// The two passes of a reserve.  fields(Carver&) lists every field once; alloc(bytes) returns a block of at least
// the measured size, or null when it cannot: the fields then stay null.  Returns where the assign pass ends,
// which is the measured size.
template <class Fields, class Alloc>
size_t carve_arena(Fields&& fields, Alloc&& alloc) {
    Carver measure;
    fields(measure);
    void* block = alloc(measure.bytes());
    if (!block) return measure.bytes();
    Carver assign(block);
    fields(assign);
    return assign.bytes();
}

}  // namespace lio

#ifndef LIO_SCRATCH_NO_HIP
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <string>

#include "lio_error.hpp"

// A failed HIP call leaves "<call>: <hipGetErrorString>" in last_error() and returns kHip; the C-ABI's status
// message appends that text (lio_capi_util.hpp status()).
#define LIO_HIP(x)                                                                      \
    do {                                                                                \
        const hipError_t e_ = (x);                                                      \
        if (e_ != hipSuccess) {                                                         \
            ::lio::last_error() = std::string(#x) + ": " + hipGetErrorString(e_);       \
            return ::lio::kHip;                                                         \
        }                                                                               \
    } while (0)

namespace lio {

inline int nblk(int64_t n) { return (int)std::max<int64_t>(1, (n + 255) / 256); }

// the capacity that holds `need` after `cap`: geometric (1.5x), at least `floor`
template <class N>
N grown(N need, N cap, N floor = 0) {
    return std::max(std::max(need, cap + cap / 2), floor);
}

// hipFree and null every pointer given (null ones are skipped)
template <class... T>
void dev_free(T**... p) {
    ((*p ? (void)hipFree(*p) : (void)0, *p = nullptr), ...);
}

// hipHostFree and null every pointer given (null ones are skipped)
template <class... T>
void host_free(T**... p) {
    ((*p ? (void)hipHostFree(*p) : (void)0, *p = nullptr), ...);
}

// One device buffer of a multi-buffer reserve: dev_alloc_all({dev_req(b.keys, c), dev_req(b.head, c + 1), ...})
struct DevReq {
    void** p;
    size_t bytes;
};
template <class T>
DevReq dev_req(T*& p, size_t count) {
    return {reinterpret_cast<void**>(&p), count * sizeof(T)};
}

// Frees every buffer of the list, then allocates them in order (each counted: lio_alloc_count).  All or
// nothing: on a failure every buffer of the list is null again and the status is kNoMem, so the caller's
// capacity (set to 0 before the call, to the new value after a kOk) never describes freed memory.
inline int dev_alloc_all(std::initializer_list<DevReq> reqs) {
    for (const DevReq& r : reqs) dev_free(r.p);
    for (const DevReq& r : reqs) {
        count_alloc();
        if (hipMalloc(r.p, r.bytes) != hipSuccess) {
            *r.p = nullptr;
            for (const DevReq& q : reqs) dev_free(q.p);
            return kNoMem;
        }
    }
    return kOk;
}

// *p holds at least `need` elements of elems_per T each (contents are not kept across a growth); cap in
// elements.  kNoMem leaves *p null and cap 0.
template <class T>
int grow_buf(T** p, int64_t& cap, int64_t need, size_t elems_per = 1, int64_t floor = 0) {
    if (need <= cap && *p) return kOk;
    const int64_t c = grown(need, cap, floor);
    cap = 0;
    const int rc = dev_alloc_all({dev_req(*p, (size_t)c * elems_per)});
    if (rc == kOk) cap = c;
    return rc;
}

// the byte scratch of the sorts and scans: as grow_buf, with a 1 MiB floor, so calls of slightly varying size
// do not re-allocate (hipFree synchronises the device)
inline int grow_scratch(void** p, size_t& bytes, size_t need, size_t floor = (size_t)1 << 20) {
    if (need <= bytes && *p) return kOk;
    const size_t c = grown(need, bytes, floor);
    bytes = 0;
    const int rc = dev_alloc_all({{p, c}});
    if (rc == kOk) bytes = c;
    return rc;
}

// carve_arena over *arena, which grow_scratch keeps at least as large as the fields measure (`bytes` is its size).
// A reserve with a capacity policy of its own measures its capacity, not the call: it frees *arena and zeroes
// `bytes` first and passes floor 0, and the arena is then exactly the measured size.
template <class Fields>
int reserve_arena(void** arena, size_t& bytes, Fields&& fields, size_t floor = (size_t)1 << 20) {
    int rc = kOk;
    carve_arena(fields, [&](size_t need) -> void* {
        rc = grow_scratch(arena, bytes, need, floor);
        return rc ? nullptr : *arena;
    });
    return rc;
}

// pinned host memory: *p holds at least `need` bytes (contents are not kept across a growth), grown as grow_buf
// grows and counted (lio_alloc_count).  kNoMem leaves *p null and bytes 0.
template <class T>
int grow_pinned(T** p, size_t& bytes, size_t need, size_t floor) {
    if (need <= bytes && *p) return kOk;
    const size_t c = grown(need, bytes, floor);
    host_free(p);
    bytes = 0;
    count_alloc();
    if (hipHostMalloc(reinterpret_cast<void**>(p), c, hipHostMallocDefault) != hipSuccess) {
        *p = nullptr;
        return kNoMem;
    }
    bytes = c;
    return kOk;
}

}  // namespace lio
#endif  // LIO_SCRATCH_NO_HIP
