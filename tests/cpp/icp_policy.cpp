// The loop ICP's HIP-free decisions (csrc/lio_icp_policy.hpp): the re-pass policy over its status words, the event
// slot, the polled mailbox.  Every expected value is written out from the rules, none computed by the code under
// test.  tests/test_icp_policy.py builds this with the address and undefined-behaviour sanitizers and runs it.
#include "../../fast-lio-sam_gps_amd/csrc/lio_icp_policy.hpp"

#include <cstdint>
#include <cstdio>

using namespace lio::icp;

static int failures = 0;

static const char* name(Step s) {
    switch (s) {
        case Step::Done: return "Done";
        case Step::RepassMeans: return "RepassMeans";
        case Step::RepassSigma: return "RepassSigma";
        case Step::ReexchangeMeans: return "ReexchangeMeans";
        case Step::ReexchangeSigma: return "ReexchangeSigma";
        case Step::Serial: return "Serial";
    }
    return "?";
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

struct In {
    uint32_t bad, over, xf;
    int mm, ms;
    bool lb;
    int mpass, spass, reex;
};
struct Out {
    Step step;
    int mpass, spass, reex;
};

constexpr int64_t kCap = 4096;

static void expect(int line, const In& in, const Out& want) {
    PassStatus s;
    s.bad = in.bad;
    s.over = in.over;
    s.xf = in.xf;
    s.mm = in.mm;
    s.ms = in.ms;
    PassCounters c;
    c.mpass = in.mpass;
    c.spass = in.spass;
    c.reexchanges = in.reex;
    const Step got = next_step(s, kCap, in.lb, c);
    if (got != want.step || c.mpass != want.mpass || c.spass != want.spass || c.reexchanges != want.reex) {
        std::printf("FAIL line %d: got %s (mpass %d spass %d reexchanges %d), want %s (%d %d %d)\n", line, name(got), c.mpass,
                    c.spass, c.reexchanges, name(want.step), want.mpass, want.spass, want.reex);
        ++failures;
    }
}
#define EXPECT(...) expect(__LINE__, __VA_ARGS__)

static void test_policy() {
    constexpr uint32_t M = 0x01, S = 0x100;  // a bad / overflowed means chain, sigma chain
    //      bad over xf     mm   ms   lb     mpass spass reex        step                   mpass spass reex
    // a look-back time-out: Serial at once, whatever the words say, the counters untouched
    EXPECT({0, 0, 0, 0, 0, true, 1, 1, 0}, {Step::Serial, 1, 1, 0});
    EXPECT({M, 0, 1, 10, 10, true, 2, 3, 1}, {Step::Serial, 2, 3, 1});
    // nothing bad, nothing over: Done (exchange flags alone start nothing)
    EXPECT({0, 0, 0, 0, 0, false, 1, 1, 0}, {Step::Done, 1, 1, 0});
    EXPECT({0, 0, 1 | 0x100, 10, 10, false, 1, 1, 0}, {Step::Done, 1, 1, 0});
    EXPECT({0, 0, 2, 10, 10, false, 3, 2, 1}, {Step::Done, 3, 2, 1});

    // one rank (xf = 0): never a re-exchange
    EXPECT({M, 0, 0, 0, 0, false, 1, 1, 0}, {Step::RepassMeans, 2, 1, 0});
    EXPECT({M, 0, 0, 0, 0, false, 1, 3, 0}, {Step::RepassMeans, 2, 1, 0});  // sigma restarts from pass 1
    EXPECT({M, 0, 0, 0, 0, false, 3, 2, 0}, {Step::RepassMeans, 4, 1, 0});  // mpass 3: one more
    EXPECT({M, 0, 0, 0, 0, false, 4, 2, 0}, {Step::Serial, 4, 2, 0});       // mpass 4: no more
    EXPECT({0x20, 0, 0, 0, 0, false, 1, 1, 0}, {Step::RepassMeans, 2, 1, 0});  // the last means bit
    EXPECT({0x40, 0, 0, 0, 0, false, 1, 1, 0}, {Step::RepassSigma, 1, 2, 0});  // bit 6 is no means chain
    EXPECT({M | S, 0, 0, 0, 0, false, 2, 2, 0}, {Step::RepassMeans, 3, 1, 0});  // the means go first
    EXPECT({S, 0, 0, 0, 0, false, 1, 1, 0}, {Step::RepassSigma, 1, 2, 0});
    EXPECT({S, 0, 0, 0, 0, false, 4, 3, 0}, {Step::RepassSigma, 4, 4, 0});  // spass 3: one more (mpass does not matter)
    EXPECT({S, 0, 0, 0, 0, false, 1, 4, 0}, {Step::Serial, 1, 4, 0});       // spass 4: no more
    EXPECT({0, M, 0, 0, 0, false, 1, 1, 0}, {Step::Serial, 1, 1, 0});       // an overflow: more passes only add events
    EXPECT({0, S, 0, 0, 0, false, 1, 1, 0}, {Step::Serial, 1, 1, 0});
    EXPECT({M, M, 0, 0, 0, false, 1, 1, 0}, {Step::Serial, 1, 1, 0});
    EXPECT({S, M, 0, 0, 0, false, 1, 1, 0}, {Step::Serial, 1, 1, 0});

    // sharded: a list longer than its slot and nothing else -> the same lists again
    EXPECT({0, M, 1, 3000, 0, false, 1, 1, 0}, {Step::ReexchangeMeans, 1, 1, 1});
    EXPECT({0, M, 1, 3000, 0, false, 2, 3, 0}, {Step::ReexchangeMeans, 2, 1, 1});  // spass back to 1, mpass kept
    EXPECT({0, S, 0x100, 0, 3000, false, 2, 3, 0}, {Step::ReexchangeSigma, 2, 3, 1});  // both kept
    EXPECT({0, M | S, 1 | 0x100, 3000, 3000, false, 1, 2, 0}, {Step::ReexchangeMeans, 1, 1, 1});  // both: the means' form
    EXPECT({M, 0, 1, 3000, 0, false, 1, 1, 0}, {Step::ReexchangeMeans, 1, 1, 1});  // a bad chain beside it: still first
    // reexchanges 1: one more; 2: none, and the words decide as on one rank
    EXPECT({0, M, 1, 3000, 0, false, 1, 1, 1}, {Step::ReexchangeMeans, 1, 1, 2});
    EXPECT({0, M, 1, 3000, 0, false, 1, 1, 2}, {Step::Serial, 1, 1, 2});
    EXPECT({M, 0, 1, 3000, 0, false, 1, 1, 2}, {Step::RepassMeans, 2, 1, 2});
    EXPECT({S, 0, 0x100, 0, 3000, false, 1, 1, 1}, {Step::ReexchangeSigma, 1, 1, 2});
    EXPECT({S, 0, 0x100, 0, 3000, false, 1, 1, 2}, {Step::RepassSigma, 1, 2, 2});
    // the longest lists: equal to the cap still fits, one above does not
    EXPECT({0, M, 1, 4096, 0, false, 1, 1, 0}, {Step::ReexchangeMeans, 1, 1, 1});
    EXPECT({0, M, 1, 4097, 0, false, 1, 1, 0}, {Step::Serial, 1, 1, 0});
    EXPECT({0, S, 0x100, 0, 4096, false, 1, 1, 0}, {Step::ReexchangeSigma, 1, 1, 1});
    EXPECT({0, S, 0x100, 0, 4097, false, 1, 1, 0}, {Step::Serial, 1, 1, 0});
    EXPECT({0, M, 1, 4096, 4097, false, 1, 1, 0}, {Step::Serial, 1, 1, 0});  // either list
    EXPECT({M, 0, 1, 4097, 0, false, 1, 1, 0}, {Step::RepassMeans, 2, 1, 0});  // no overflow: the re-pass rules
    // each hard flag alone forbids the re-exchange
    EXPECT({0, M, 1 | 2, 3000, 0, false, 1, 1, 0}, {Step::Serial, 1, 1, 0});
    EXPECT({0, M, 1 | 4, 3000, 0, false, 1, 1, 0}, {Step::Serial, 1, 1, 0});
    EXPECT({0, M, 1 | 0x200, 3000, 0, false, 1, 1, 0}, {Step::Serial, 1, 1, 0});
    EXPECT({M, 0, 1 | 2, 3000, 0, false, 1, 1, 0}, {Step::RepassMeans, 2, 1, 0});
    EXPECT({S, 0, 0x100 | 0x200, 0, 3000, false, 1, 1, 0}, {Step::RepassSigma, 1, 2, 0});
    EXPECT({S, 0, 0x100 | 4, 0, 3000, false, 1, 4, 0}, {Step::Serial, 1, 4, 0});
    // a hard flag without a slot flag, and no flag at all with bad words: the one-rank rules
    EXPECT({M, 0, 2, 0, 0, false, 1, 1, 0}, {Step::RepassMeans, 2, 1, 0});
    EXPECT({S, 0, 0, 100, 100, false, 1, 1, 0}, {Step::RepassSigma, 1, 2, 0});
    // a flag bit no rule names changes nothing
    EXPECT({0, M, 1 | 0x400, 3000, 0, false, 1, 1, 0}, {Step::ReexchangeMeans, 1, 1, 1});
    CHECK(kMaxPasses == 4);
}

static void test_next_slot() {
    // want = 1.5 x the longest list + 256, rounded up to 256; at least 1024, never below cur, at most cap
    CHECK(next_slot(0, 0, 4096) == 1024);       // the floor
    CHECK(next_slot(100, 512, 4096) == 1024);   // want 406 -> 512, cur 512: the floor
    CHECK(next_slot(512, 1024, 4096) == 1024);  // want 768 + 256 = 1024 exactly
    CHECK(next_slot(513, 1024, 4096) == 1280);  // want 769 + 256 = 1025 -> 1280
    CHECK(next_slot(1000, 1024, 4096) == 1792); // want 1500 + 256 = 1756 -> 1792
    CHECK(next_slot(1001, 1024, 4096) == 1792); // 1501 (integer 3 / 2) + 256 = 1757 -> 1792
    CHECK(next_slot(1024, 1024, 4096) == 1792); // 1536 + 256 = 1792 exactly
    CHECK(next_slot(1025, 1024, 4096) == 2048); // 1537 + 256 = 1793 -> 2048
    CHECK(next_slot(10, 2048, 4096) == 2048);   // never shrinks
    CHECK(next_slot(1000, 2048, 4096) == 2048);
    CHECK(next_slot(2300, 2048, 4096) == 3840); // 3450 + 256 = 3706 -> 3840
    CHECK(next_slot(2400, 2048, 4096) == 4096); // 3600 + 256 = 3856 -> 4096, the cap itself
    CHECK(next_slot(4000, 2048, 4096) == 4096); // clamped to the cap
    CHECK(next_slot(4000, 2048, 8192) == 6400); // 6000 + 256 = 6256 -> 6400
    CHECK(next_slot(0, 8192, 4096) == 4096);    // the cap wins over the current slot
}

static void test_mailbox() {
    uint32_t word = 0xdeadbeefu;
    Mailbox a(&word);
    CHECK(a.post() == 1 && word == 0);
    CHECK(!a.arrived(1));
    word = 1;
    CHECK(a.arrived(1) && !a.arrived(2));
    CHECK(a.post() == 2 && word == 0);
    // wrap-around: 0 is skipped
    Mailbox b(&word, 0xFFFFFFFEu);
    CHECK(b.post() == 0xFFFFFFFFu);
    word = 0xFFFFFFFFu;
    CHECK(b.arrived(0xFFFFFFFFu));
    CHECK(b.post() == 1 && word == 0);
    CHECK(!b.arrived(1) && !b.arrived(0xFFFFFFFFu));
    Mailbox w(&word, 0xFFFFFFFFu);
    CHECK(w.post() == 1);
    CHECK(w.post() == 2);
    // the fallback-copy case: the word holds, stale, exactly the number the next post() hands out
    Mailbox m(&word, 6);
    word = 7;
    const uint32_t seq = m.post();
    CHECK(seq == 7);
    CHECK(word == 0);
    CHECK(!m.arrived(seq));  // not fooled: the pack has not run
    word = 6;                // an older pack's number
    CHECK(!m.arrived(seq));
    word = 7;                // the pack's store
    CHECK(m.arrived(seq));
    // a stale value at the wrap
    Mailbox z(&word, 0xFFFFFFFFu);
    word = 1;
    CHECK(z.post() == 1 && !z.arrived(1));
    word = 1;
    CHECK(z.arrived(1));
}

int main() {
    test_policy();
    test_next_slot();
    test_mailbox();
    if (failures) {
        std::printf("%d FAILED\n", failures);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
