// sweep_select.cpp — the row selection of a sweep upload (csrc/lio_sweep_select.hpp) on the host alone (no HIP, no
// GPU): the plan's pieces, concatenated, the row count and the sorted flag against a sequential restatement, over
// every record width, both ends of the time field's range, point_filter_num 1 / 3 / 4, tiny and odd row counts and
// 1 / 2 / 8 pieces (more pieces than candidate rows included).  Source and destination are malloc'ed at exactly
// their sizes and the program is built with -fsanitize=address,undefined by tests/test_sweep_select.py: a read past
// the sweep or a write past a piece's share of the destination is a sanitizer report.
#include "../../fast-lio-sam_gps_amd/csrc/lio_sweep_select.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

namespace {

constexpr float kBlind = 2.0f;

enum Pattern { kRising, kRandom, kBoundaryStep, kNan, kBlindEdge, kFirstHalfDropped, kPatterns };

uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

// row i of the pattern: coordinates outside the blind radius unless the pattern drops the row, the time at field
// tf, the row index in every other field
void fill(Pattern pat, float* raw, int64_t n, int stride, int tf, int every, int pieces) {
    const int64_t ub = lio::sweep_candidates(n, every);
    const int64_t per = (ub + pieces - 1) / pieces;  // the first piece boundary, in candidate rows
    uint32_t seed = 12345u + (uint32_t)(n * 31 + stride * 7 + tf);
    for (int64_t i = 0; i < n; ++i) {
        float* q = raw + i * stride;
        for (int f = 0; f < stride; ++f) q[f] = (float)(i * 8 + f);
        q[0] = 3.0f + (float)(i % 5), q[1] = -1.0f, q[2] = 0.5f;
        float t = (float)i - 3.0f;                    // rising, from negative times
        if (i == 3) t = -0.0f;                        // -0.0f sorts before +0.0f, which it is not equal to as a key
        switch (pat) {
            case kRising: break;
            case kRandom: t = (float)(int32_t)(lcg(seed) >> 8) * 1e-3f - 8000.f; break;
            case kBoundaryStep:  // rising inside every piece, one step down where the second piece begins
                if (pieces > 1 && i / every >= per) t -= (float)n + 8.0f;
                break;
            case kNan:
                if (i % 3 == 1) q[i % 2] = std::numeric_limits<float>::quiet_NaN();
                break;
            case kBlindEdge:  // |p| == blind exactly is dropped (the test is strict), the next float is kept
                q[1] = q[2] = 0.0f;
                q[0] = (i % 2) ? kBlind : std::nextafter(kBlind, 4.0f);
                if (i % 7 == 6) q[0] = -kBlind;
                break;
            case kFirstHalfDropped:
                if (i < n / 2) q[0] = 0.25f, q[1] = 0.0f, q[2] = -0.25f;
                break;
            default: break;
        }
        q[tf] = t;
    }
}

// the selection, sequentially: rows i % every == 0 outside the blind radius, in input order; sorted: their time
// keys (sign-flipped bit patterns, as the device sorts them) never decrease
bool restate(const float* raw, int64_t n, int stride, int every, float blind, int tf, std::vector<float>& rows) {
    bool sorted = true;
    uint32_t prev = 0;
    for (int64_t i = 0; i < n; i += every) {
        const float* q = raw + i * stride;
        if (!(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] > blind * blind)) continue;
        uint32_t tb;
        std::memcpy(&tb, &q[tf], 4);
        const uint32_t key = (tb & 0x80000000u) ? ~tb : (tb | 0x80000000u);
        if (!rows.empty() && key < prev) sorted = false;
        prev = key;
        rows.insert(rows.end(), q, q + stride);
    }
    return sorted;
}

int failures = 0, cases = 0;

void run(Pattern pat, int stride, int tf, int every, int64_t n, int pieces) {
    ++cases;
    auto* raw = static_cast<float*>(std::malloc((size_t)n * stride * sizeof(float)));
    const int64_t ub = lio::sweep_candidates(n, every);
    auto* dst = static_cast<float*>(std::malloc((size_t)ub * stride * sizeof(float)));
    fill(pat, raw, n, stride, tf, every, pieces);
    std::vector<float> want;
    const bool want_sorted = restate(raw, n, stride, every, kBlind, tf, want);
    const lio::SweepSelection s = lio::select_sweep(raw, n, stride, every, kBlind, tf, dst, pieces);
    std::vector<float> got;
    bool plan_ok = s.plan.pieces == pieces;
    int64_t total = 0;
    for (int t = 0; t < s.plan.pieces && plan_ok; ++t) {
        const int64_t at = s.plan.src_row[t], k = s.plan.rows[t];
        plan_ok = at >= 0 && k >= 0 && at + k <= ub && (t == 0 || at >= s.plan.src_row[t - 1] + s.plan.rows[t - 1]);
        if (!plan_ok) break;
        got.insert(got.end(), dst + at * stride, dst + (at + k) * stride);
        total += k;
    }
    const bool same = plan_ok && total == s.rows && got.size() == want.size() &&
                      (want.empty() || std::memcmp(got.data(), want.data(), want.size() * sizeof(float)) == 0);
    if (!same || s.sorted != want_sorted) {
        std::printf("FAIL pattern %d stride %d tf %d every %d n %lld pieces %d: plan_ok %d rows %lld (want %zu) sorted %d (want %d)\n",
                    (int)pat, stride, tf, every, (long long)n, pieces, (int)plan_ok, (long long)s.rows,
                    want.size() / stride, (int)s.sorted, (int)want_sorted);
        ++failures;
    }
    std::free(dst);
    std::free(raw);
}

}  // namespace

int main() {
    const int64_t counts[] = {0, 1, 2, 3, 4, 5, 37, 64, 1000};
    for (int pat = 0; pat < kPatterns; ++pat)
        for (int stride = 4; stride <= 8; ++stride)
            for (int tf : {3, stride - 1})
                for (int every : {1, 3, 4})
                    for (int64_t n : counts)
                        for (int pieces : {1, 2, 8}) run((Pattern)pat, stride, tf, every, n, pieces);
    if (failures) return 1;
    std::printf("ALL OK (%d cases)\n", cases);
    return 0;
}
