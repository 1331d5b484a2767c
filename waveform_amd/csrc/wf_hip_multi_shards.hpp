// wf_hip_multi_shards.hpp -- what wf_hip_multi.cpp lends the group's entry points that live in other translation units
// (wf_hip_multi_pcm.cpp).  Host code only.
#pragma once
#include <functional>

#include "wf_hip.h"

namespace wf::multi {

// fn(shard handle, local first, local count, offset of the shard's part in the range) for every shard the global range
// [first, first+count) overlaps, each on its device's own thread, concurrently; WF_HIP_ERR_INVALID for a range outside the
// group.  The first failure wins and its text becomes the group's last error.
int for_each_shard(wf_hip_multi *m, uint32_t first, uint32_t count, const std::function<int(wf_hip *, uint32_t, uint32_t, uint32_t)> &fn);
// the group's last error := msg; returns code
int fail(wf_hip_multi *m, int code, const char *msg);

} // namespace wf::multi
