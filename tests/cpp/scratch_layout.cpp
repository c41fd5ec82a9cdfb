// scratch_layout.cpp — the arena carver of csrc/lio_scratch.hpp on the host alone (no HIP, no GPU): one field
// list run twice, over Carver{} to measure and over Carver{block} to assign, first by hand and then through
// carve_arena, the helper every reserve runs (with aligned_alloc where the reserves grow a device arena).
// Built with -fsanitize=address,undefined by tests/test_scratch_layout.py: a slot that overlaps its neighbour
// or leaves the block is a failed check here and a sanitizer report on the writes.
#define LIO_SCRATCH_NO_HIP
#include "../../fast-lio-sam_gps_amd/csrc/lio_scratch.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {

struct alignas(16) Vec16 {
    float v[4];
};

struct Mixed {  // element sizes 1, 4, 8, 16 and a byte block, as the DenoiseBuf / ClusterBuf / PlaneBuf mix them
    uint8_t* mask = nullptr;
    uint32_t* keys = nullptr;
    uint32_t* none = nullptr;  // always zero elements
    double* mom = nullptr;
    Vec16* pts = nullptr;
    uint32_t* head = nullptr;  // n + 1
    void* tmp = nullptr;       // 3 n + 7 bytes
};

void fields(Mixed& m, size_t n, lio::Carver& at) {
    at(m.mask, n), at(m.keys, n), at(m.none, 0), at(m.mom, n), at(m.pts, n), at(m.head, n + 1), at(m.tmp, 3 * n + 7);
}

size_t carve(Mixed& m, size_t n, lio::Carver at) {
    fields(m, n, at);
    return at.bytes();
}

int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAIL line %d (n = %zu): %s\n", __LINE__, n, #cond); \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

template <class T>
void touch(T* p, size_t count) {  // the first and the last element can be written
    if (!count) return;
    std::memset(p, 0xa5, sizeof(T));
    std::memset(p + (count - 1), 0x5a, sizeof(T));
}

void run(size_t n) {
    Mixed m;
    const size_t total = carve(m, n, lio::Carver{});
    CHECK(!m.mask && !m.keys && !m.none && !m.mom && !m.pts && !m.head && !m.tmp);  // measuring assigns nothing
    CHECK(total % 256 == 0 && total > 0);
    auto* block = static_cast<uint8_t*>(std::aligned_alloc(256, total));
    CHECK(block != nullptr);
    if (!block) return;
    CHECK(carve(m, n, lio::Carver{block}) == total);  // the measured size is the end of the assign pass

    const struct {
        const void* p;
        size_t bytes;
    } slot[] = {{m.mask, n},      {m.keys, 4 * n},       {m.none, 0},         {m.mom, 8 * n},
                {m.pts, 16 * n},  {m.head, 4 * (n + 1)}, {m.tmp, 3 * n + 7}};
    size_t expect = 0;  // slots follow each other in list order, each rounded up to 256 bytes
    for (const auto& s : slot) {
        const size_t off = (size_t)(static_cast<const uint8_t*>(s.p) - block);
        CHECK(off % 256 == 0);
        CHECK(off == expect);               // no overlap, no gap beyond the rounding
        CHECK(off + s.bytes <= total);
        expect = off + ((s.bytes + 255) / 256) * 256;
    }
    CHECK(expect == total);
    CHECK((const void*)m.none == (const void*)m.mom);  // a zero-count field takes no space: it aliases the next
    if (n == 0) CHECK((const void*)m.mask == (const void*)m.keys && (const void*)m.mom == (const void*)m.pts);

    touch(m.mask, n), touch(m.keys, n), touch(m.mom, n), touch(m.pts, n), touch(m.head, n + 1);
    touch(static_cast<uint8_t*>(m.tmp), 3 * n + 7);
    if (n) {  // the writes stayed in their own slots
        CHECK(m.mask[0] == 0xa5 || n == 1);
        CHECK(m.mask[n - 1] == 0x5a && m.keys[n - 1] == 0x5a5a5a5au && m.head[n] == 0x5a5a5a5au);
    }

    // the same list through carve_arena: it asks for the measured size once, ends where the hand-run assign pass
    // ends, and puts every field where the hand-run two passes put it
    Mixed h;
    size_t asked = 0, calls = 0;
    uint8_t* hblock = nullptr;
    const size_t end = lio::carve_arena([&](lio::Carver& at) { fields(h, n, at); },
                                        [&](size_t bytes) -> void* {
                                            asked = bytes, ++calls;
                                            return hblock = static_cast<uint8_t*>(std::aligned_alloc(256, bytes));
                                        });
    CHECK(calls == 1 && asked == total && end == total);
    CHECK(hblock != nullptr);
    if (hblock) {
        auto same = [&](const void* a, const void* b) {
            return static_cast<const uint8_t*>(a) - hblock == static_cast<const uint8_t*>(b) - block;
        };
        CHECK(same(h.mask, m.mask) && same(h.keys, m.keys) && same(h.none, m.none) && same(h.mom, m.mom));
        CHECK(same(h.pts, m.pts) && same(h.head, m.head) && same(h.tmp, m.tmp));
        touch(h.mask, n), touch(h.keys, n), touch(h.mom, n), touch(h.pts, n), touch(h.head, n + 1);
        touch(static_cast<uint8_t*>(h.tmp), 3 * n + 7);
        std::free(hblock);
    }
    // an allocation that fails leaves every field null and still reports the measured size
    Mixed z;
    CHECK(lio::carve_arena([&](lio::Carver& at) { fields(z, n, at); }, [](size_t) -> void* { return nullptr; }) == total);
    CHECK(!z.mask && !z.keys && !z.none && !z.mom && !z.pts && !z.head && !z.tmp);
    std::free(block);
}

}  // namespace

int main() {
    const size_t counts[] = {0, 1, 255, 257, 4097};
    for (size_t n : counts) run(n);
    if (failures) return 1;
    std::printf("ALL OK\n");
    return 0;
}
