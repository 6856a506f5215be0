// The host's wait for k_step's report (wepp_amd/csrc/info_wait.hpp) driven by fake callables: a word that the "device"
// writes at a time of the fake clock, a stream that completes or fails at another.  A program of its own, built plain
// and under AddressSanitizer + UBSan by tests/test_info_wait.py.  Prints "ok" when every case holds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../wepp_amd/csrc/info_wait.hpp"

using namespace wepp;

namespace {

constexpr int STREAM_BUSY = -1, STREAM_DONE = 0, STREAM_FAULT = 719;   // (a positive code: returned as it is)
constexpr uint64_t NEVER = ~0ull;

// the world of one wait: the clock advances a microsecond per look at it; the word holds `before` until `word_at` and
// `after` from then on; the stream is busy until `stream_at` and answers `stream_then` from then on
struct World {
    uint64_t t = 0;
    uint32_t before = 0, after = 0;
    uint64_t word_at = NEVER, stream_at = NEVER;
    int stream_then = STREAM_DONE;
    uint64_t first_query = NEVER, last_look = 0;
    InfoWaitResult wait(uint32_t want) {
        return wait_info_word(
            want, [&]() { last_look = t; return t >= word_at ? after : before; },
            [&]() { if (first_query == NEVER) first_query = t; return t >= stream_at ? stream_then : STREAM_BUSY; },
            [&]() { return t++; });
    }
};

int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); failures++; } \
    } while (0)

}  // namespace

int main() {
    static_assert(info_seq_word(437) == 448 && info_block_words(437) == 464 && info_seq_word(448) == 448, "the sequence word has a line of its own");
    static_assert(info_next_seq(0) == 1 && info_next_seq(41) == 42 && info_next_seq(0xFFFFFFFFu) == 1, "sequence numbers skip zero");
    {   // the word is there at the first look: no query, no second look
        World w; w.before = 7; w.after = 7; w.word_at = 0;
        const InfoWaitResult r = w.wait(7);
        CHECK(r.what == InfoWait::arrived && r.looks == 1 && r.queries == 0 && r.error == 0);
    }
    {   // the word arrives while the wait spins
        World w; w.before = 6; w.after = 7; w.word_at = 50;
        const InfoWaitResult r = w.wait(7);
        CHECK(r.what == InfoWait::arrived && r.queries == 0 && w.last_look >= 50 && w.last_look < 60);
    }
    {   // ... behind the yield threshold, in front of the first query
        World w; w.before = 6; w.after = 7; w.word_at = INFO_WAIT_SPIN_US + 300;
        const InfoWaitResult r = w.wait(7);
        CHECK(r.what == InfoWait::arrived && r.queries == 0 && w.last_look >= INFO_WAIT_SPIN_US + 300);
    }
    {   // ... behind the first queries of a stream that is still busy
        World w; w.before = 6; w.after = 7; w.word_at = INFO_WAIT_QUERY_US + 3 * INFO_WAIT_QUERY_EVERY_US + 10;
        const InfoWaitResult r = w.wait(7);
        CHECK(r.what == InfoWait::arrived && r.queries >= 3 && r.queries <= 5);
        CHECK(w.first_query >= INFO_WAIT_QUERY_US && w.first_query < INFO_WAIT_QUERY_US + 8);
    }
    {   // the word never arrives and the stream runs dry: lost, and the loop returns
        World w; w.before = 6; w.after = 7; w.stream_at = INFO_WAIT_QUERY_US + 1000;
        const InfoWaitResult r = w.wait(7);
        CHECK(r.what == InfoWait::lost && r.queries >= 4 && w.t < INFO_WAIT_QUERY_US + 1000 + 2 * INFO_WAIT_QUERY_EVERY_US);
    }
    {   // the stream is complete at the first query and the word came in with it: the last look takes it
        World w; w.before = 6; w.after = 7; w.stream_at = 0; w.word_at = INFO_WAIT_QUERY_US + 1;
        const InfoWaitResult r = w.wait(7);
        CHECK(r.what == InfoWait::arrived || r.what == InfoWait::lost);      // (by a microsecond of the fake clock; either ends the wait)
        CHECK(r.queries == 1);
    }
    {   // the stream reports an error: that error
        World w; w.before = 6; w.after = 7; w.stream_at = 100; w.stream_then = STREAM_FAULT;
        const InfoWaitResult r = w.wait(7);
        CHECK(r.what == InfoWait::stream_error && r.error == STREAM_FAULT && r.queries == 1);
    }
    {   // the word of the PREVIOUS call is not this call's: the wait goes on until this call's arrives
        World w; w.before = 6; w.after = 7; w.word_at = 900;
        const InfoWaitResult r = w.wait(7);
        CHECK(r.what == InfoWait::arrived && r.looks > 100 && w.last_look >= 900);
    }
    {   // ... and when it never does, the previous word is not taken at the end either
        World w; w.before = 6; w.after = 6; w.stream_at = 0;
        const InfoWaitResult r = w.wait(7);
        CHECK(r.what == InfoWait::lost);
    }
    {   // ... nor a word from the future (a block another call wrote)
        World w; w.before = 8; w.after = 8; w.stream_at = 0;
        const InfoWaitResult r = w.wait(7);
        CHECK(r.what == InfoWait::lost);
    }
    if (failures) return 1;
    puts("ok");
    return 0;
}
