// lio_pieces.hpp — the most pieces a sweep is packed in: the host's packing plan (lio_sweep_select.hpp) and the
// device's piece table (RowPieces in lio_filter.hpp) share it.  No HIP.
#pragma once

namespace lio {
constexpr int kMaxPieces = 8;
}
