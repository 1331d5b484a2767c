// wf_wave_reduce.hpp -- the butterfly over the 64 lanes of a wavefront that the small kernels reduce with (device code only;
// hipcc): every lane ends with the same value, every lane combines the same pairs, so the order of the additions is fixed by
// the lane numbers alone and the same inputs give the same bits.
//
// The order of the six exchanges is part of a float sum's result.  WAVE_DOWN (lane distance 32, 16 .. 1) is what the RMS
// producer, the signal statistics and the band levels have always used; the loudness producer has always gone the other way
// (WAVE_UP: 1, 2 .. 32), and its readings are pinned bit for bit, so the direction is the call site's to state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wf_dev_guard.hpp"

namespace wf {

enum WaveOrder { WAVE_DOWN, WAVE_UP };

// T: float, double or uint32_t
template<WaveOrder ORDER = WAVE_DOWN, class T> __device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for(int i = 0; i < 6; ++i)
        v += __shfl_xor(v, ORDER == WAVE_DOWN ? 32 >> i : 1 << i, 64);
    return v;
}

template<WaveOrder ORDER = WAVE_DOWN> __device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for(int i = 0; i < 6; ++i)
        v = __builtin_fmaxf(v, __shfl_xor(v, ORDER == WAVE_DOWN ? 32 >> i : 1 << i, 64));
    return v;
}

} // namespace wf
