// wf_hip_multi_pcm.cpp -- wf_hip_multi_push_pcm: wf_hip_push_pcm over the shards of a multi-device group (include/wf_hip.h).
// Host code only.  A translation unit of its own because wf_hip_multi.cpp is also built over a host-only mock of the
// wf_hip_* entry points it calls (tests/mock), which has no wf_hip_push_pcm.
#include "wf_hip.h"
#include "wf_hip_multi_shards.hpp"
#include "wf_pcm_formats.hpp"

int wf_hip_multi_push_pcm(wf_hip_multi *m, uint32_t first, uint32_t count, const wf_hip_pcm *pcm)
{
    if(m == nullptr)
        return WF_HIP_ERR_INVALID;
    if(pcm == nullptr || pcm->data == nullptr)
        return wf::multi::fail(m, WF_HIP_ERR_INVALID, "pcm or pcm->data is NULL");
    if(pcm->memory != WF_HIP_PCM_HOST || pcm->frames_per_stream != nullptr)
        return wf::multi::fail(m, WF_HIP_ERR_INVALID, "a group takes WF_HIP_PCM_HOST packets without frames_per_stream");
    if(!wf::pcm_format_valid(pcm->format) || pcm->channels < 1 || pcm->channels > 8)
        return wf::multi::fail(m, WF_HIP_ERR_INVALID, "bad format or channel count");
    // the channel pick is every shard's own check, made before it enqueues anything; a bad one fails on every shard alike
    const size_t block = (size_t)pcm->channels * pcm->frames * wf::pcm_sample_bytes(pcm->format);
    return wf::multi::for_each_shard(m, first, count, [pcm, block](wf_hip *h, uint32_t lf, uint32_t lc, uint32_t off) {
        wf_hip_pcm p = *pcm;
        p.data = static_cast<const unsigned char *>(pcm->data) + (size_t)off * block;
        return wf_hip_push_pcm(h, lf, lc, &p);
    });
}
