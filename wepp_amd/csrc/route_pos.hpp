// route_pos.hpp -- the word k_route classifies a (read, position) by: per head slot of every slice of the walk arena,
// the events of the position's list (its length without the sentinel) and the position's nesting depth in ONE dword,
// where the kernel used to gather ix_nest[p], ix_head[p].off and ix_head[p + 1].off from two arrays of the arena.
// The table is derived on the device at upload (route_kernels.hip: k_route_pos); the flat image does not hold it.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define WEPP_RT_HD __host__ __device__
#else
#define WEPP_RT_HD
#endif

namespace wepp {

#ifndef WEPP_RT_LEN_BITS
#define WEPP_RT_LEN_BITS 24
#endif
// bits of the length field; the nesting depth (a byte, flatmat.hpp: ix_nest) sits above it.  A list of a tree of up to
// 2^25 nodes can outgrow 24 bits: the field SATURATES at its largest value, and a saturated field sends the lookup to
// the exact list heads, so what k_route counts stays exact at any width (tests build with 3 bits to take that path).
constexpr uint32_t RT_LEN_BITS = WEPP_RT_LEN_BITS;
static_assert(RT_LEN_BITS >= 1 && RT_LEN_BITS <= 24, "length and a byte of nesting depth share a dword");
constexpr uint32_t RT_LEN_SAT = (1u << RT_LEN_BITS) - 1u;

WEPP_RT_HD inline uint32_t rt_pos_pack(uint32_t len, uint32_t nest) {
    return (len < RT_LEN_SAT ? len : RT_LEN_SAT) | ((nest & 0xFFu) << RT_LEN_BITS);
}
// false: the length is saturated -- `len` is a lower bound only, the exact one is in the list heads
WEPP_RT_HD inline bool rt_pos_unpack(uint32_t word, uint32_t& len, uint32_t& nest) {
    len = word & RT_LEN_SAT;
    nest = (word >> RT_LEN_BITS) & 0xFFu;
    return len != RT_LEN_SAT;
}

}  // namespace wepp
