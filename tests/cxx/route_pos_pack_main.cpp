// The word k_route classifies a (read, position) by (wepp_amd/csrc/route_pos.hpp), on the host: round trip, saturation
// of the length field and its recognition, for the width the build gives (-DWEPP_RT_LEN_BITS=n; 24 by default).
// Built and run by tests/test_route_pos_pack.py, plain and under AddressSanitizer + UBSan.
#include <cstdint>
#include <cstdio>

#include "../../wepp_amd/csrc/route_pos.hpp"

using namespace wepp;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

int main() {
    static_assert(RT_LEN_SAT == (1u << RT_LEN_BITS) - 1u, "the saturated value is the field's largest");
    const uint32_t lens[] = {0u, 1u, RT_LEN_SAT - 1u};
    const uint32_t nests[] = {0u, 255u};
    for (uint32_t len : lens)
        for (uint32_t nest : nests) {
            uint32_t l = ~0u, n = ~0u;
            if (len >= RT_LEN_SAT) continue;        // (a field of one bit holds 0 only)
            CHECK(rt_pos_unpack(rt_pos_pack(len, nest), l, n));
            CHECK(l == len && n == nest);
        }
    // at and above the field's largest value: saturated, recognised, the nesting depth intact, the length a lower bound
    const uint32_t over[] = {RT_LEN_SAT, RT_LEN_SAT + 1u, 1u << 24, (1u << 25) - 1u, 0xFFFFFFFFu};
    for (uint32_t len : over)
        for (uint32_t nest : nests) {
            uint32_t l = 0, n = ~0u;
            CHECK(!rt_pos_unpack(rt_pos_pack(len, nest), l, n));
            CHECK(l == RT_LEN_SAT && l <= len && n == nest);
            CHECK(rt_pos_pack(len, nest) == rt_pos_pack(RT_LEN_SAT, nest));
        }
    // the last head slot of a slice holds 0: no events, no depth
    {
        uint32_t l = ~0u, n = ~0u;
        CHECK(rt_pos_unpack(0u, l, n) && l == 0 && n == 0);
    }
    // the two fields do not overlap
    for (uint32_t nest = 0; nest < 256; nest++) {
        uint32_t l = ~0u, n = ~0u;
        rt_pos_unpack(rt_pos_pack(RT_LEN_SAT - 1u, nest), l, n);
        CHECK(l == RT_LEN_SAT - 1u && n == nest);
    }
    if (fails) return 1;
    std::printf("ok %u\n", RT_LEN_BITS);
    return 0;
}
