// wf_ring_view.hpp -- how the measurement kernels (wf_signal.hpp, wf_pitch.hpp, wf_stereo.hpp, wf_cq.hpp, wf_scope.hpp, wf_gonio.hpp, wf_sono.hpp, wf_bits.hpp, wf_thd.hpp and wf_imd.hpp through wf_thd_spectrum.hpp, wf_delay.hpp, wf_onset.hpp, wf_tempo.hpp, wf_hum.hpp, wf_xfer_sums.hpp for wf_xfer.hpp and wf_impulse.hpp, wf_click.hpp, and the
// loudness push kernel of wf_loudness.hpp) see the audio rings: the four words every one of them takes, where a stream's newest
// frames start and where a channel's ring lies.  Filled by ring_view() in wf_hip_measure.hip.  How each kernel fetches its window
// from there is its own business; wf_ring_stage.hpp is how wf_scope.hpp, wf_gonio.hpp and wf_bits.hpp copy theirs into LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace wf {

struct RingView {
    const float *ring;       // d_ring: [n_streams][cap_ch][ring_stride]
    const uint32_t *wpos;    // [n_streams] write positions, as of the pushes issued so far
    uint32_t ring_cap;       // frames per ring: a power of two
    uint32_t ring_stride;    // floats between consecutive rings: ring_cap + padding, a multiple of 4
};

// (the two below take the view by value: a copy of kernel arguments stays kernel arguments to the compiler, which a `this`
// pointer into them does not)

// Where the newest `frames` (<= ring_cap) frames of `stream` start, unmasked: frame i of the window is at ring position
// (start + i) & (ring_cap - 1).  The write position is a uint32 count of every frame ever pushed and wraps at 2^32; so does the
// subtraction, also where wpos < frames, and neither harms: the capacity divides 2^32, so the mask gives the same position.
__device__ __forceinline__ uint32_t window_start(const RingView v, uint32_t stream, uint32_t frames) { return v.wpos[stream] - frames; }

// the ring of channel `ch` of `stream` in a batch of `channels` captured channels
__device__ __forceinline__ const float *channel_ring(const RingView v, uint32_t stream, uint32_t ch, uint32_t channels)
{
    return v.ring + ((size_t)stream * channels + ch) * v.ring_stride;
}

} // namespace wf
