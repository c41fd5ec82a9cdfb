// lio_sweep_select.hpp — the row selection of a sweep upload, host arithmetic alone (no HIP; tests/cpp/sweep_select.cpp
// builds it by itself under the sanitizers).  Preprocess's whole selection is made while packing, since the host
// reads every row then anyway: i % point_filter_num == 0 and x*x + y*y + z*z > blind^2, in float and in that
// order as the device's scan_key_kernel, so the device gets exactly the selected rows, in input order.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "lio_pieces.hpp"

namespace lio {

// rows i % every == 0 with x*x + y*y + z*z > blind2 (float, left to right: scan_key_kernel's order) copied to
// d in input order; every row is written at the cursor and the cursor advances by the keep flag (no branch
// on the data); sorted: the kept rows' time keys (scan_key_kernel's) never decrease
template <int S>
int64_t select_rows(const float* __restrict__ raw, int64_t n, int every, float blind2, int tf, float* __restrict__ d,
                    bool& sorted, uint32_t& first_key, uint32_t& last_key) {
    int64_t k = 0;
    uint32_t prev = 0, unsorted = 0, first = 0xffffffffu;
    for (int64_t i = 0; i < n; i += every) {
        const float* q = raw + i * S;
        float r[S];
        for (int f = 0; f < S; ++f) r[f] = q[f];
        const uint32_t keep = (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) > blind2 ? 1u : 0u;
        uint32_t tb;
        std::memcpy(&tb, &r[tf], 4);
        const uint32_t key = (tb & 0x80000000u) ? ~tb : (tb | 0x80000000u);  // scan_key_kernel's time key
        unsorted |= keep & (key < prev ? 1u : 0u);
        first = (keep && k == 0) ? key : first;
        prev = keep ? key : prev;
        for (int f = 0; f < S; ++f) d[k * S + f] = r[f];
        k += keep;
    }
    sorted = unsorted == 0;
    first_key = first;
    last_key = prev;
    return k;
}

// Large sweeps are packed in up to kMaxPieces contiguous pieces, each at its own offset of the destination (the
// upper bound of its rows): the plan lists them, and the device reads the concatenation through the piece table.
struct StagePlan {
    int pieces = 0;
    int64_t src_row[kMaxPieces] = {};  // first destination row of the piece
    int64_t rows[kMaxPieces] = {};     // its selected rows
};

struct SweepSelection {
    StagePlan plan;
    int64_t rows = 0;    // selected rows of all pieces
    bool sorted = true;  // their times are non-decreasing: the stable time sort is the identity, the device skips it
};

inline int64_t sweep_candidates(int64_t n, int every) { return (n + every - 1) / every; }  // rows i % every == 0

// The n raw rows of `stride` (4..8) floats selected into dst, which holds sweep_candidates(n, every) * stride
// floats; every >= 1, 1 <= pieces <= kMaxPieces.  Piece t packs its share of the candidate rows at that share's
// own offset of dst; run(pieces, fn) calls fn(t) for every t in [0, pieces), in any order and on any threads.
template <class Run>
SweepSelection select_sweep(const float* raw, int64_t n, int stride, int every, float blind, int time_field, float* dst,
                            int pieces, Run&& run) {
    const int64_t ub = sweep_candidates(n, every);
    const float blind2 = blind * blind;
    const int64_t per = (ub + pieces - 1) / pieces;  // candidate rows per piece
    int64_t k[kMaxPieces] = {};
    bool srt[kMaxPieces] = {};
    uint32_t first[kMaxPieces] = {}, last[kMaxPieces] = {};
    auto piece = [&](int t) {
        const int64_t c0 = std::min(ub, t * per), c1 = std::min(ub, c0 + per);
        const float* src = raw + c0 * every * stride;
        const int64_t nn = std::min(n - c0 * every, (c1 - c0) * every);  // raw rows of the piece
        float* d = dst + c0 * stride;
        bool s = true;
        switch (stride) {  // the record width as a constant: the row copy unrolls, the loop stays branch-free
            case 4: k[t] = select_rows<4>(src, nn, every, blind2, time_field, d, s, first[t], last[t]); break;
            case 5: k[t] = select_rows<5>(src, nn, every, blind2, time_field, d, s, first[t], last[t]); break;
            case 6: k[t] = select_rows<6>(src, nn, every, blind2, time_field, d, s, first[t], last[t]); break;
            case 7: k[t] = select_rows<7>(src, nn, every, blind2, time_field, d, s, first[t], last[t]); break;
            default: k[t] = select_rows<8>(src, nn, every, blind2, time_field, d, s, first[t], last[t]); break;
        }
        srt[t] = s;
    };
    run(pieces, piece);
    SweepSelection out;
    uint32_t prev = 0;
    bool any = false;
    out.plan.pieces = pieces;
    for (int t = 0; t < pieces; ++t) {
        out.plan.src_row[t] = std::min(ub, t * per);
        out.plan.rows[t] = k[t];
        out.rows += k[t];
        if (!k[t]) continue;
        out.sorted = out.sorted && srt[t] && (!any || prev <= first[t]);  // and across the piece boundary
        prev = last[t];
        any = true;
    }
    return out;
}

// the pieces one after the other on the calling thread
inline SweepSelection select_sweep(const float* raw, int64_t n, int stride, int every, float blind, int time_field,
                                   float* dst, int pieces) {
    return select_sweep(raw, n, stride, every, blind, time_field, dst, pieces, [](int np, auto& fn) {
        for (int t = 0; t < np; ++t) fn(t);
    });
}

}  // namespace lio
