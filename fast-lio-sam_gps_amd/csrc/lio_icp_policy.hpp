// lio_icp_policy.hpp — the decisions of the loop ICP's float statistics that need no device: what follows a
// pass whose chains failed their verification or outgrew their lists (next_step), the per-rank event slot of the
// next exchange (next_slot), and the pinned word the host polls for a pass's statistics (Mailbox).  No HIP
// include: tests/cpp/icp_policy.cpp builds this header alone.  Used by lio_icp_stats.cpp.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>

namespace lio::icp {

constexpr int kMaxPasses = 4;  // per chain set (means, sigma); the verification makes any pass count safe

// what the statistics' finish loop does next
enum class Step { Done, RepassMeans, RepassSigma, ReexchangeMeans, ReexchangeSigma, Serial };

// the status words of a pass (pcl_pack's out[16], [17]; sharded: [20] .. [22], every rank's combined)
struct PassStatus {
    uint32_t bad = 0;   // chains that failed their verification (means bits 0-5, sigma 8-16)
    uint32_t over = 0;  // chains whose event list overflowed (same bits)
    uint32_t xf = 0;    // exchange flags, means | sigma << 8: 1 a list longer than its slot, 2 / 4 hard failures
    int mm = 0, ms = 0; // the longest per-rank event list of the means / sigma chains
};

struct PassCounters {
    int mpass = 1, spass = 1;  // passes the means / sigma chains have had
    int reexchanges = 0;
};

// One decision of the finish loop, the counters advanced for the step returned.  One rank passes xf = 0 and
// never gets a re-exchange.  `cap` is the largest event slot the exchange buffers hold (ev_slot_cap).
//   look-back time-out                                   Serial: the pairs themselves cannot be trusted
//   nothing bad, nothing over                            Done
//   only a list longer than its slot (no hard flag, both lists within cap, fewer than 2 re-exchanges so far)
//                                                        the same lists again with the slot they need: the means'
//                                                        (sigma restarts from pass 1) iff xf & 1, else sigma's
//   an overflow                                          Serial: more passes only add events
//   a means chain bad                                    RepassMeans (sigma restarts from pass 1) while mpass < 4
//   a sigma chain bad                                    RepassSigma while spass < 4
//   otherwise                                            Serial
inline Step next_step(const PassStatus& s, int64_t cap, bool lb_timeout, PassCounters& c) {
    if (lb_timeout) return Step::Serial;
    if ((s.bad | s.over) == 0) return Step::Done;
    const bool hard = (s.xf & (2u | 4u | 0x200u)) != 0;
    if (!hard && (s.xf & (1u | 0x100u)) && s.mm <= cap && s.ms <= cap && c.reexchanges < 2) {
        ++c.reexchanges;
        if (!(s.xf & 1u)) return Step::ReexchangeSigma;
        c.spass = 1;
        return Step::ReexchangeMeans;
    }
    if (s.over) return Step::Serial;
    if (s.bad & 0x3fu) {
        if (c.mpass >= kMaxPasses) return Step::Serial;
        ++c.mpass;
        c.spass = 1;
        return Step::RepassMeans;
    }
    if (c.spass >= kMaxPasses) return Step::Serial;
    ++c.spass;
    return Step::RepassSigma;
}

// the per-rank event slot for the next exchange: 1.5 x the longest list of this one (every rank saw the same
// lists, so every rank picks the same slot), in steps of 256, at least 1024, at most `cap`, and never below the
// current slot (a pass-1 list is longer than a later pass's: a slot that shrank in between would make every
// alignment's first pass re-exchange)
inline int next_slot(int longest, int cur, int64_t cap) {
    const int64_t want = ((int64_t)longest * 3 / 2 + 256 + 255) / 256 * 256;
    return (int)std::min<int64_t>(std::max<int64_t>(std::max<int64_t>(want, 1024), cur), cap);
}

// The pinned, host-mapped word a one-rank pass's pack stores its sequence number into, last, and the host polls.
// post() hands out the next number and zeroes the word first; 0 is never a number.  So whatever the word held
// (a copy of a device buffer's never-written word, an earlier pack's number), arrived() is false until the
// pack that was given the number has stored it.  Every number a pack gets comes from post().
class Mailbox {
public:
    explicit Mailbox(void* word = nullptr, uint32_t last = 0) : w_(static_cast<volatile uint32_t*>(word)), seq_(last) {}
    uint32_t post() {
        *w_ = 0;
        std::atomic_thread_fence(std::memory_order_release);  // the zero is in place before the launch is
        if (++seq_ == 0) seq_ = 1;
        return seq_;
    }
    bool arrived(uint32_t seq) const { return *w_ == seq; }

private:
    volatile uint32_t* w_;
    uint32_t seq_;
};

}  // namespace lio::icp
