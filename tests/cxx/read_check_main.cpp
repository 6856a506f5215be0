// read_check_main.cpp -- wepp_amd/csrc/read_check.hpp on the CPU, under the sanitizers (tests/test_read_check.py):
// the range check of a host batch against a naive one, who stages and who sends which offset of a pipelined batch,
// and the cut of a batch into sub-batches and chunks.  Prints "ok ..." and returns 0, or says what differs and returns 1.
//
// Arrays the functions under test index are heap arrays of exactly the size they may touch: one word too far is the
// sanitizer's finding.
//   read_check_main         the suite's run
//   read_check_main full    check 1 over all twelve words per slot (3 positions x ref {0,1} x mut {0,1}): 6.7e9 batches,
//                           hours -- the suite's run enumerates six word classes, see range_check_exhaustive()
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "../../wepp_amd/csrc/read_check.hpp"

using namespace wepp;

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu, SENTINEL = 0xDEADBEEFu;
std::atomic<int> g_failures{0};
std::atomic<unsigned long long> g_cases{0};

#define FAIL(...) do { if (g_failures++ < 20) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } while (0)

uint32_t word_of(uint32_t pos, uint32_t ref, uint32_t mut) { return pos | (ref << 20) | (mut << 24); }
uint32_t pos_of(uint32_t w) { return w & 0xFFFFFu; }
bool zero_mask(uint32_t w) { return ((w >> 20) & 15u) == 0 || ((w >> 24) & 15u) == 0; }

struct Verdict { uint32_t bad = NONE; int what = 0; };

// the naive check: read by read -- its offsets, then the order of its positions, then its masks.  It looks at a word
// only once the read's offsets have been found inside [0, nw].
Verdict naive(const uint32_t* off, const uint32_t* word, uint64_t nw, uint32_t lo, uint32_t hi) {
    for (uint32_t r = lo; r < hi; r++) {
        const uint64_t b = off[r], e = off[r + 1];
        if (b > nw || e > nw || e < b) return Verdict{r, 0};
        for (uint64_t k = b; k + 1 < e; k++)
            if (pos_of(word[k + 1]) <= pos_of(word[k])) return Verdict{r, 1};
        for (uint64_t k = b; k < e; k++)
            if (zero_mask(word[k])) return Verdict{r, 2};
    }
    return Verdict{};
}

bool offsets_valid(const uint32_t* off, uint64_t nw, uint32_t lo, uint32_t hi) {
    if (off[lo] > nw) return false;
    for (uint32_t r = lo; r < hi; r++)
        if (off[r + 1] < off[r] || off[r + 1] > nw) return false;
    return true;
}

// every [lo, hi) of a batch of `n_reads` reads, without and with a staging buffer, against the naive check; with
// staging, the words of the range have arrived when its offsets are valid and every other word of the buffer is as it was
unsigned compare_ranges(const uint32_t* off, uint32_t n_reads, const uint32_t* word, uint32_t n_words, uint64_t nw, uint32_t* stage) {
    unsigned cases = 0;
    for (uint32_t lo = 0; lo <= n_reads; lo++)
        for (uint32_t hi = lo; hi <= n_reads; hi++) {
            const Verdict want = naive(off, word, nw, lo, hi);
            const bool valid = offsets_valid(off, nw, lo, hi);
            for (int staged = 0; staged < 2; staged++) {
                if (staged) for (uint32_t k = 0; k < n_words; k++) stage[k] = SENTINEL;
                Verdict got;
                check_reads(off, word, nw, lo, hi, staged ? stage : nullptr, got.bad, got.what);
                cases++;
                if (got.bad != want.bad || (want.bad != NONE && got.what != want.what))
                    FAIL("range check: offsets %u %u %u %u, nw %llu, range [%u, %u), staging %d: read %u kind %d, naive says read %u kind %d",
                         off[0], off[1], off[2], off[3], (unsigned long long)nw, lo, hi, staged, got.bad, got.what, want.bad, want.what);
                for (uint32_t k = 0; k < n_words && staged; k++) {
                    const bool moved = valid && k >= off[lo] && k < off[hi];
                    if (stage[k] != (moved ? word[k] : SENTINEL))
                        FAIL("staging: offsets %u %u %u %u, range [%u, %u), staging %d: word %u is %08x", off[0], off[1], off[2], off[3], lo, hi, staged, k, stage[k]);
                }
            }
        }
    return cases;
}

// Check 1, first enumeration: all batches of 3 reads of 0 - 3 words each, valid offsets.
// The whole alphabet is 12 words per slot (position 1 - 3, ref mask 0 / 1, mut mask 0 / 1): (1 + 12 + 144 + 1728)^3 =
// 6.7e9 batches, hours under the sanitizers (`full`).  The suite's run enumerates the six classes (position, some mask is
// zero) -- (1 + 6 + 36 + 216)^3 = 17.4 M batches -- and makes every zero-masked word one of ref = 0, mut = 0, both = 0 in
// turn, the turn moving with the slot and the batch: every order of positions, every placement of empty reads and of
// zero-masked words among them is there, each of the three kinds of zero mask in every slot; what is left to `full` are
// the mixtures of kinds within one batch.  Thread t of T takes the batches whose code is t modulo T.
void range_check_exhaustive(bool full, uint32_t t, uint32_t T) {
    const uint32_t A = full ? 12 : 6;
    unsigned long long cases = 0;
    for (uint32_t l0 = 0; l0 <= 3; l0++)
        for (uint32_t l1 = 0; l1 <= 3; l1++)
            for (uint32_t l2 = 0; l2 <= 3; l2++) {
                const uint32_t n = l0 + l1 + l2;
                const uint32_t off[4] = {0, l0, l0 + l1, n};
                std::unique_ptr<uint32_t[]> word(new uint32_t[n]), stage(new uint32_t[n]);
                uint64_t codes = 1;
                for (uint32_t i = 0; i < n; i++) codes *= A;
                for (uint64_t code = t; code < codes; code += T) {
                    uint64_t c = code;
                    for (uint32_t i = 0; i < n; i++, c /= A) {
                        const uint32_t cls = (uint32_t)(c % A), pos = 1 + cls % 3;
                        if (full) word[i] = word_of(pos, (cls / 3) & 1u, cls / 6);
                        else if (cls < 3) word[i] = word_of(pos, 1, 1);
                        else {
                            const uint32_t kind = (uint32_t)((i + code) % 3);
                            word[i] = word_of(pos, kind == 1 ? 1 : 0, kind == 0 ? 1 : 0);   // ref = 0, mut = 0, both = 0
                        }
                    }
                    cases += compare_ranges(off, 3, word.get(), n, n, stage.get());
                }
            }
    g_cases += cases;
}

// Check 1, second enumeration: offsets that descend or leave the word array.  Every offset from 0 - 3 against a word
// array of 2 (the naive check stops at a read's offsets before it looks at its words), the two words over the six classes.
void range_check_bad_offsets() {
    const uint32_t nw = 2;
    std::unique_ptr<uint32_t[]> word(new uint32_t[nw]), stage(new uint32_t[nw]);
    for (uint32_t o = 0; o < 256; o++) {
        const uint32_t off[4] = {o & 3u, (o >> 2) & 3u, (o >> 4) & 3u, (o >> 6) & 3u};
        for (uint32_t c = 0; c < 36; c++) {
            word[0] = word_of(1 + c % 3, (c % 6) < 3 ? 1 : 0, 1);
            word[1] = word_of(1 + (c / 6) % 3, 1, (c / 6) < 3 ? 1 : 0);
            g_cases += compare_ranges(off, 3, word.get(), nw, nw, stage.get());
        }
    }
}

BatchGeometry geometry_of(uint32_t n_reads, uint32_t S, uint32_t C, uint32_t PS) {
    BatchGeometry g;
    g.n_reads = n_reads; g.S = S; g.C = C; g.CPS = C / S; g.PS = PS;
    return g;
}

// Checks 2 and 3: every offset index of [0, n_reads] is copied by exactly one staging task, every read checked by exactly
// one; what the upload of a chunk sends has been staged by a chunk it waits for (round 3's fault: the end offset of a
// chunk staged by the next one), and every offset goes up, twice at most where a sub-batch starts.
//
// EXPECTED DIFFERENCE, recorded and not fixed here: the rules name a chunk's first and last PART, and hold as long as
// every part holds a read.  Where a part is empty (fewer reads than C x PS) an offset may be staged by two tasks -- the
// same four bytes from the same place -- or by a chunk its upload does not wait for.  wepp_place_batch never gets
// there: it cuts a batch into several chunks from 65 536 reads on, into 71 chunks of 64 parts at the very most.  Such
// geometries are counted (KNOWN_EMPTY_PART_DIFFERENCES of the enumeration below); every read is checked by exactly one
// task in them too.
constexpr unsigned KNOWN_EMPTY_PART_DIFFERENCES = 115;

void ownership_and_upload() {
    const uint32_t reads[] = {1, 2, 3, 5, 64, 65, 1000}, chunks[] = {1, 2, 4, 8}, parts[] = {1, 2, 3, 5};
    unsigned known = 0;
    for (uint32_t n : reads)
        for (uint32_t C : chunks)
            for (uint32_t S = 1; S <= C; S++)
                for (uint32_t PS : parts) {
                    if (C % S) continue;
                    const BatchGeometry g = geometry_of(n, S, C, PS);
                    std::vector<uint32_t> off_tasks(n + 1, 0), off_chunks(n + 1, 0), read_tasks(n, 0), sent(n + 1, 0);   // (off_chunks: a bit per chunk that stages the offset)
                    bool empty_part = false;
                    unsigned differs = 0;
                    for (uint32_t ck = 0; ck < C; ck++)
                        for (uint32_t part = 0; part < PS; part++) {
                            const StageRange r = stage_range(g, ck, part);
                            g_cases++;
                            if (r.read_lo > r.read_hi || r.read_hi > n || r.off_hi > n + 1) { FAIL("stage_range(%u reads, C %u, PS %u; %u, %u) leaves the batch", n, C, PS, ck, part); continue; }
                            empty_part = empty_part || r.read_lo == r.read_hi;
                            for (uint32_t o = r.off_lo; o < r.off_hi; o++) { off_tasks[o]++; off_chunks[o] |= 1u << ck; }
                            for (uint32_t q = r.read_lo; q < r.read_hi; q++) read_tasks[q]++;
                        }
                    for (uint32_t q = 0; q < n; q++)
                        if (read_tasks[q] != 1) FAIL("%u reads, S %u, C %u, PS %u: read %u is checked by %u tasks", n, S, C, PS, q, read_tasks[q]);
                    for (uint32_t o = 0; o <= n; o++)
                        if (off_tasks[o] != 1) {
                            differs++;
                            if (!empty_part) FAIL("%u reads, S %u, C %u, PS %u: offset %u is staged by %u tasks", n, S, C, PS, o, off_tasks[o]);
                        }
                    for (uint32_t k = 0; k < S; k++)
                        for (uint32_t ck = k * g.CPS; ck < (k + 1) * g.CPS; ck++) {
                            const UploadRange u = upload_range(g, k, ck);
                            g_cases++;
                            if (u.off_hi > n + 1 || u.wait_lo > ck) { FAIL("upload_range(%u reads, S %u, C %u; %u, %u) leaves the batch", n, S, C, k, ck); continue; }
                            const uint32_t waited = (2u << ck) - (1u << u.wait_lo);      // chunks wait_lo .. ck
                            for (uint32_t o = u.off_lo; o < u.off_hi; o++) {
                                sent[o]++;
                                if (!(off_chunks[o] & waited)) {
                                    differs++;
                                    if (!empty_part) FAIL("%u reads, S %u, C %u, PS %u: chunk %u sends offset %u and waits for chunks %u .. %u, none of which stages it", n, S, C, PS, ck, o, u.wait_lo, ck);
                                }
                            }
                        }
                    std::vector<uint32_t> may_twice(n + 1, 0);
                    for (uint32_t k = 1; k < S; k++) may_twice[g.sub_lo(k)] = 1;
                    for (uint32_t o = 0; o <= n; o++)
                        if (sent[o] < 1 || sent[o] > 1 + may_twice[o]) {
                            differs++;
                            if (!empty_part) FAIL("%u reads, S %u, C %u, PS %u: offset %u goes up %u times", n, S, C, PS, o, sent[o]);
                        }
                    if (differs) known++;
                }
    if (known != KNOWN_EMPTY_PART_DIFFERENCES) FAIL("%u geometries with an empty staging part differ from the ownership rules, %u are recorded", known, KNOWN_EMPTY_PART_DIFFERENCES);
}

// Check 4: the cut of a batch.  The rule for S is the one of wepp_place_batch before the cut became a function: one
// device call below 2^16 reads and with per_node_scores; else the knob (the handle's before the environment's), else 2
// from 2^19 reads when the pool has two workers, n_reads >> 21 beyond; 8 at most.
void geometry() {
    const uint32_t around[] = {1u << 16, 1u << 19, 1u << 21}, workers_of[] = {0, 1, 2, 15}, min_chunks_of[] = {1, 3, 4, 64};
    for (uint32_t centre : around)
        for (uint32_t n = centre - 1; n <= centre + 1; n++)
            for (uint32_t knob = 0; knob <= 9; knob++)
                for (uint32_t env = 0; env <= 9; env++)
                    for (uint32_t workers : workers_of)
                        for (int pns = 0; pns < 2; pns++)
                            for (uint32_t min_chunks : min_chunks_of) {
                                const BatchGeometry g = batch_geometry(n, knob, env, workers, pns != 0, min_chunks);
                                g_cases++;
                                const bool big = n >= (1u << 16);
                                const uint32_t k = knob ? knob : env;
                                uint32_t S = 1;
                                if (big && !pns) {
                                    S = k ? k : (workers >= 2 && n >= (1u << 19)) ? 2u : 1u;
                                    if (!k && (n >> 21) > S) S = n >> 21;
                                    if (S > 8) S = 8;
                                }
                                bool ok = g.n_reads == n && g.big == big && g.S == S && g.S >= 1 && g.S <= 8 && g.C >= 1 && g.C % g.S == 0 &&
                                          g.CPS * g.S == g.C && g.PS >= 1 && g.PO >= 1 && g.two_launchers == (big && S > 1 && workers >= 2);
                                if (big) ok = ok && g.C >= min_chunks && g.C < min_chunks + g.S && g.PO == 4 && (uint64_t)g.C * g.PS >= 4 * (workers + 1);
                                else ok = ok && g.C == 1 && g.PS == 1 && g.PO == 1;
                                ok = ok && g.sub_lo(0) == 0 && g.sub_lo(g.S) == n && g.chunk_lo(0) == 0 && g.chunk_lo(g.C) == n;
                                for (uint32_t s = 0; s < g.S && ok; s++) ok = g.sub_lo(s) <= g.sub_lo(s + 1);
                                for (uint32_t c = 0; c < g.C && ok; c++) ok = g.chunk_lo(c) <= g.chunk_lo(c + 1);
                                if (!ok) FAIL("batch_geometry(%u reads, knob %u, env %u, %u workers, per_node_scores %d, min_chunks %u): S %u (want %u) C %u CPS %u PS %u PO %u",
                                              n, knob, env, workers, pns, min_chunks, g.S, S, g.C, g.CPS, g.PS, g.PO);
                            }
}

void read_csr() {
    const uint32_t ok_off[3] = {0, 1, 1}, late[3] = {1, 1, 2}, down[3] = {0, 2, 1}, word[2] = {word_of(1, 1, 1), word_of(2, 1, 1)};
    g_cases += 5;
    if (check_read_csr(ok_off, word, 2) != WEPP_OK) FAIL("check_read_csr rejects a valid CSR");
    if (check_read_csr(nullptr, word, 2) != WEPP_EINVAL) FAIL("check_read_csr takes a null read_off");
    if (check_read_csr(late, word, 2) != WEPP_EINVAL) FAIL("check_read_csr takes read_off[0] = 1");
    if (check_read_csr(down, word, 2) != WEPP_EINVAL || std::strcmp(wepp_last_error(), "read_off not monotone")) FAIL("check_read_csr takes descending offsets");
    if (check_read_csr(ok_off, nullptr, 2) != WEPP_EINVAL) FAIL("check_read_csr takes a null read_word with words to read");
}

}  // namespace

int main(int argc, char** argv) {
    const bool full = argc > 1 && !std::strcmp(argv[1], "full");
    {
        const uint32_t T = 4;
        std::vector<std::thread> threads;
        for (uint32_t t = 0; t < T; t++) threads.emplace_back(range_check_exhaustive, full, t, T);
        for (std::thread& th : threads) th.join();
    }
    range_check_bad_offsets();
    ownership_and_upload();
    geometry();
    read_csr();
    if (g_failures) {
        std::fprintf(stderr, "%d differences in %llu cases\n", g_failures.load(), g_cases.load());
        return 1;
    }
    std::printf("ok %llu cases; %u geometries with an empty staging part differ as recorded\n", g_cases.load(), KNOWN_EMPTY_PART_DIFFERENCES);
    return 0;
}
