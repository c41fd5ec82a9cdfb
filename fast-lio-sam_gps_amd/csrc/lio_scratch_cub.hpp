// lio_scratch_cub.hpp — the hipcub "query bytes, check or grow, run" pair, once: a stable radix sort of
// (key, value) pairs and an exclusive sum, both enqueued on a stream.  Two scratch policies:
//   kFixedScratch  the scratch was sized at reserve time for the whole capacity (DenoiseBuf): too small is an
//                  error, no call allocates
//   kGrowScratch   the scratch grows on demand (FilterBuf, MapUpdBuf; GridBuf, which sizes it once per
//                  rebuild for the largest of its sort and scans): grow_scratch, counted
#pragma once
#include <hipcub/hipcub.hpp>

#include "lio_scratch.hpp"

namespace lio {

enum ScratchPolicy { kFixedScratch, kGrowScratch };

// tmp holds `need` bytes, by the policy
inline int cub_scratch(void*& tmp, size_t& tmp_bytes, size_t need, ScratchPolicy policy) {
    if (need <= tmp_bytes && tmp) return kOk;
    if (policy == kGrowScratch) return grow_scratch(&tmp, tmp_bytes, need);
    last_error() = "denoise scratch smaller than the sort / scan needs";
    return kHip;
}

// stable sort of (kin, vin)[0 .. n) on key bits [0, bits) into (kout, vout)
template <class K, class V>
int cub_sort_pairs(void*& tmp, size_t& tmp_bytes, ScratchPolicy policy, const K* kin, K* kout, const V* vin, V* vout,
                   int64_t n, int bits, hipStream_t st) {
    size_t bytes = 0;
    LIO_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, kin, kout, vin, vout, (int)n, 0, bits, st));
    const int rc = cub_scratch(tmp, tmp_bytes, bytes, policy);
    if (rc) return rc;
    bytes = tmp_bytes;
    LIO_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, kin, kout, vin, vout, (int)n, 0, bits, st));
    return kOk;
}

// out[0 .. n) = exclusive sum of in[0 .. n).  In / Out are hipcub's iterator types as the caller passes them
// (a const input pointer selects another instantiation of hipcub's kernels than a mutable one).
template <class In, class Out>
int cub_exclusive_sum(void*& tmp, size_t& tmp_bytes, ScratchPolicy policy, In in, Out out, int64_t n, hipStream_t st) {
    size_t bytes = 0;
    LIO_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, (int)n, st));
    const int rc = cub_scratch(tmp, tmp_bytes, bytes, policy);
    if (rc) return rc;
    bytes = tmp_bytes;
    LIO_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, bytes, in, out, (int)n, st));
    return kOk;
}

}  // namespace lio
