// resolve_host_sanitized.cpp -- the host-only code of wepp_epp_resolve under AddressSanitizer + UBSan on the CPU
// (tests/test_resolve_host_sanitized.py): the reader of residual_mutations.txt (wepp_amd/host/residual_file.hpp), the
// checks on the residual list and its stable order by position (wepp_amd/csrc/resolve_host.hpp).
#include <cstdio>
#include <random>
#include <sstream>

#include "../../wepp_amd/csrc/resolve_host.hpp"
#include "../../wepp_amd/host/residual_file.hpp"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static bool refused(const std::string& text, const std::string& reference, const char* what) {
    std::istringstream in(text);
    try {
        parse_residual_mutations(in, "r.txt", reference);
    } catch (const MAT::mat_error& e) {
        return std::string(e.what()).find(what) != std::string::npos;
    }
    return false;
}

int main() {
    const std::string reference = "ACGTACGTNRAC";      // 12 bases; N at 9, R at 10
    {
        std::istringstream in("3T,0.25\r\n\n1A,0.5,7,x\n12Y,\n3T,0.26\n2C,1,\n");
        auto r = parse_residual_mutations(in, "r.txt", reference);
        CHECK(r.size() == 5);
        CHECK(r[0].position == 3 && r[0].nuc == 'T' && r[0].mut_nuc == 8 && r[0].ref_nuc == 4 && r[0].key == "3T:0.25");
        CHECK(r[1].position == 1 && r[1].mut_nuc == 1 && r[1].ref_nuc == 1 && r[1].key == "1A:0.5:7:x");
        CHECK(r[2].position == 12 && r[2].mut_nuc == 10 && r[2].ref_nuc == 2 && r[2].key == "12Y:");
        CHECK(r[3].key == "3T:0.26");                   // the same mutation under other values is another key
        CHECK(r[4].key == "2C:1:");
    }
    CHECK(refused("3T,1\n3T,1\n", reference, "more than once"));
    CHECK(refused("3T\n", reference, "no comma"));
    CHECK(refused("13A,1\n", reference, "outside the reference"));
    CHECK(refused("0A,1\n", reference, "outside the reference"));
    CHECK(refused("99999999999A,1\n", reference, "<position><letter>"));
    CHECK(refused("3N,1\n", reference, "codec"));
    CHECK(refused("3V,1\n", reference, "codec"));       // get_nuc_id has no 'V'
    CHECK(refused("3t,1\n", reference, "codec"));
    CHECK(refused("3,1\n", reference, "<position><letter>"));
    CHECK(refused("T,1\n", reference, "<position><letter>"));
    CHECK(refused("T3,1\n", reference, "<position><letter>"));
    CHECK(refused("-3T,1\n", reference, "<position><letter>"));
    CHECK(refused(",1\n", reference, "<position><letter>"));
    CHECK(refused("9A,1\n", reference, "not one of A, C, G, T"));
    CHECK(refused("10A,1\n", reference, "not one of A, C, G, T"));

    {
        const uint32_t ok[] = {wepp_pack_read_word(1, 1, 2, 0), wepp_pack_read_word(60, 8, 8, 0), wepp_pack_read_word(7, 4, 14, 0)};
        CHECK(wepp::resolve_check_residual(3, ok, 60) == WEPP_OK);
        CHECK(wepp::resolve_check_residual(0, nullptr, 60) == WEPP_OK);
        CHECK(wepp::resolve_check_residual(3, ok, 59) == WEPP_EINVAL);
        const uint32_t bad[] = {wepp_pack_read_word(0, 1, 2, 0), wepp_pack_read_word(5, 1, 0, 0), wepp_pack_read_word(5, 1, 15, 0),
                                wepp_pack_read_word(5, 3, 2, 0), wepp_pack_read_word(5, 0, 2, 0), wepp_pack_read_word(0xFFFFF, 1, 2, 0)};
        for (uint32_t w : bad) CHECK(wepp::resolve_check_residual(1, &w, 0xFFFFFu - 1) == WEPP_EINVAL);
        CHECK(std::string(wepp_last_error()).find("residual mutation 0") != std::string::npos);
    }
    {
        std::mt19937 rng(7);
        std::vector<uint32_t> pos, word, idx;
        wepp::resolve_sort_residual(0, nullptr, pos, word, idx);
        CHECK(pos.empty() && word.empty() && idx.empty());
        for (int round = 0; round < 50; round++) {
            const uint32_t n = 1 + rng() % 200;
            std::vector<uint32_t> res(n);
            for (auto& w : res) w = wepp_pack_read_word(1 + rng() % 20, 1u << (rng() % 4), 1 + rng() % 14, 0);
            wepp::resolve_sort_residual(n, res.data(), pos, word, idx);
            CHECK(pos.size() == n && word.size() == n && idx.size() == n);
            for (uint32_t i = 0; i < n; i++) {
                CHECK(word[i] == res[idx[i]] && pos[i] == (word[i] & 0xFFFFFu));
                if (i) CHECK(pos[i - 1] < pos[i] || (pos[i - 1] == pos[i] && idx[i - 1] < idx[i]));   // stable
            }
        }
    }
    printf("ok\n");
    return 0;
}
