// wf_cq_sizes.hpp -- the sizes that the constant-Q read kernel (wf_cq.hpp) and the host builder of its tables
// (wf_measure_tables.cpp) must agree on.  Constants only: plain C++, no HIP.
#pragma once
#include <cstdint>

#include "wf_hip.h"

namespace wf {

constexpr uint32_t WF_CQ_THREADS = 1024;
constexpr uint32_t WF_CQ_WAVES = WF_CQ_THREADS / 64;
// the host's table per bin, in doubles: [0..3] the 64-frame steps of carrier and window phasor (re, im each), [4] 4 / L_b,
// [5] L_b, [6..7] unused, then per lane l < 64 the values at n = l: carrier re, im, window phasor re, im
constexpr uint32_t WF_CQ_BIN_HEAD = 8;
constexpr uint32_t WF_CQ_BIN_DOUBLES = WF_CQ_BIN_HEAD + 64 * 4;
// the schedule, in words: [0 .. WF_CQ_WAVES] where each wave's list starts in the order (the last: its end), then the order
constexpr uint32_t WF_CQ_SCHED_WORDS = WF_CQ_WAVES + 1 + WF_HIP_CQ_BINS;

} // namespace wf
