// wf_pcm_formats.hpp -- the facts of wf_hip_pcm.format (include/wf_hip.h), once: which values are formats, a sample's bytes, the
// layout, the sample kind and the alignment device data needs.  Plain C++ (no HIP): wf_hip.hip and wf_hip_multi_pcm.cpp use it,
// and tests/test_wire_cpu.py compiles it on its own.
//   1..4   wf_hip_pcm_format, interleaved (u8, s16, s32, f32)      5..8   the same, planar   (+4)
//   16..20 wf_hip_wire_format, interleaved (s24, s24_be, s16_be, mu-law, A-law)   24..28 the same, planar (+8)
// Every other value is no format: pcm_format_valid is false and the other functions return 0 / false.
#pragma once
#include <cstdint>
#include "wf_hip.h"

namespace wf {

constexpr bool pcm_format_valid(uint32_t format)
{
    return (format >= WF_HIP_PCM_U8 && format <= WF_HIP_PCM_F32_PLANAR) || (format >= WF_HIP_WIRE_S24 && format <= WF_HIP_WIRE_ALAW) ||
           (format >= WF_HIP_WIRE_S24_PLANAR && format <= WF_HIP_WIRE_ALAW_PLANAR);
}

// [frames][channels] (true) or [channels][frames]
constexpr bool pcm_is_interleaved(uint32_t format)
{
    return pcm_format_valid(format) && (format <= WF_HIP_PCM_F32 || (format >= WF_HIP_WIRE_S24 && format <= WF_HIP_WIRE_ALAW));
}

// the sample type: the interleaved format's value (WF_HIP_PCM_U8 .. WF_HIP_PCM_F32, WF_HIP_WIRE_S24 .. WF_HIP_WIRE_ALAW); 0: no format
constexpr uint32_t pcm_sample_kind(uint32_t format)
{
    return !pcm_format_valid(format)         ? 0u
           : pcm_is_interleaved(format)      ? format
           : format <= WF_HIP_PCM_F32_PLANAR ? format - 4u
                                             : format - 8u;
}

constexpr uint32_t pcm_sample_bytes(uint32_t format)
{
    switch(pcm_sample_kind(format)) {
    case WF_HIP_PCM_U8:
    case WF_HIP_WIRE_ULAW:
    case WF_HIP_WIRE_ALAW: return 1u;
    case WF_HIP_PCM_S16:
    case WF_HIP_WIRE_S16_BE: return 2u;
    case WF_HIP_WIRE_S24:
    case WF_HIP_WIRE_S24_BE: return 3u;
    case WF_HIP_PCM_S32:
    case WF_HIP_PCM_F32: return 4u;
    default: return 0u;
    }
}

// what WF_HIP_PCM_DEVICE data must be aligned to: the sample's natural alignment (a packed 24-bit sample has none)
constexpr uint32_t pcm_device_alignment(uint32_t format)
{
    const uint32_t bytes = pcm_sample_bytes(format);
    return bytes == 3u ? 1u : bytes;
}

} // namespace wf
