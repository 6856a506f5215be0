// info_wait.hpp -- the host's wait for the routing counters k_step reports (walk_kernels.hip: the report; capi.cpp:
// place_device).  The first wave of k_step copies the counters k_route left on the device into the lane's report
// block in host memory and then stores the call's sequence number behind them; the host polls that word.  The wait is a
// function of three callables -- read the word, query the caller's stream, the clock -- so that it runs without a
// GPU (tests/cxx/info_wait_main.cpp).  It spins first, then yields the core between looks, and from INFO_WAIT_QUERY_US
// on it also asks the stream at intervals: a stream in error ends the wait with that error, a stream that has run dry
// without the word having arrived ends it as lost.  It never waits without bound for a word nothing will write.
#pragma once
#include <cstdint>
#include <thread>

namespace wepp {

constexpr uint64_t INFO_WAIT_SPIN_US = 200;       // spinning (the routing kernel of a million reads takes ~40 us)
constexpr uint64_t INFO_WAIT_QUERY_US = 2000;     // first query of the stream (a long queue in front of this call)
constexpr uint64_t INFO_WAIT_QUERY_EVERY_US = 250;

// the report block: the counters, then -- on a cache line of its own -- the sequence word
constexpr uint32_t info_seq_word(uint32_t counter_words) { return (counter_words + 15u) / 16u * 16u; }
constexpr uint32_t info_block_words(uint32_t counter_words) { return info_seq_word(counter_words) + 16u; }

// sequence numbers of a lane: 1, 2, ... and never 0, the value of a block nothing has reported into
constexpr uint32_t info_next_seq(uint32_t seq) { return seq + 1u ? seq + 1u : 1u; }

enum class InfoWait : int { arrived = 0, stream_error = 1, lost = 2 };
struct InfoWaitResult {
    InfoWait what;
    int error;          // stream_error: what query_stream returned
    uint32_t looks;     // reads of the word
    uint32_t queries;   // queries of the stream
};

// read_word() -> uint32_t: an acquire load of the sequence word.
// query_stream() -> int: 0 = everything queued so far has completed, < 0 = not yet, > 0 = an error (returned as it is).
// now_us() -> uint64_t: a monotonic clock in microseconds.
template <typename ReadWord, typename QueryStream, typename NowUs>
inline InfoWaitResult wait_info_word(uint32_t want, ReadWord&& read_word, QueryStream&& query_stream, NowUs&& now_us) {
    InfoWaitResult r{InfoWait::arrived, 0, 0, 0};
    const uint64_t t0 = now_us();
    uint64_t next_query = t0 + INFO_WAIT_QUERY_US;
    for (;;) {
        r.looks++;
        if (read_word() == want) return r;
        const uint64_t t = now_us();
        if (t >= next_query) {
            r.queries++;
            const int q = query_stream();
            if (q > 0) { r.what = InfoWait::stream_error; r.error = q; return r; }
            if (q == 0) {
                // the kernel that reports has ended: its store is out, or it never made one
                r.looks++;
                if (read_word() != want) r.what = InfoWait::lost;
                return r;
            }
            next_query = t + INFO_WAIT_QUERY_EVERY_US;
        }
        if (t - t0 > INFO_WAIT_SPIN_US) std::this_thread::yield();
    }
}

}  // namespace wepp
