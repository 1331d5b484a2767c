// wf_wave_reduce.hpp -- the butterfly over the 64 lanes of a wavefront that the small kernels and every measurement kernel reduce
// with (device code only; hipcc): every lane ends with the same value, every lane combines the same pairs, so the order of the
// additions is fixed by the lane numbers alone and the same inputs give the same bits.
//
// The order of the exchanges is part of a float sum's result.  WAVE_DOWN (lane distance 32, 16 .. 1) is what the RMS producer and
// every measurement read kernel use; the loudness producer has always gone the other way (WAVE_UP: 1, 2 .. 32), and its readings
// are pinned bit for bit, so the direction is the call site's to state.  LANES < 64 reduces within aligned groups of LANES lanes
// (the oscilloscope's sixteen lanes per column).
//
// Users among the measurement kernels: wf_loudness.hpp, wf_peaks.hpp, wf_signal.hpp, wf_pitch.hpp, wf_bands.hpp, wf_scope.hpp,
// wf_gonio.hpp, wf_bits.hpp, wf_thd.hpp, wf_imd.hpp, wf_delay.hpp, wf_xfer_sums.hpp with wf_xfer.hpp and wf_impulse.hpp, wf_click.hpp, wf_hum.hpp.  The
// tick path (wf_kernels.hpp, wf_big.hpp, wf_meter.hpp) keeps reductions of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wf_dev_guard.hpp"

namespace wf {

enum WaveOrder { WAVE_DOWN, WAVE_UP };

// the exchanges of a group of LANES lanes: how many, and the lane distance of the i-th
template<int LANES> __device__ __forceinline__ constexpr int wave_steps()
{
    static_assert(LANES >= 2 && LANES <= 64 && (LANES & (LANES - 1)) == 0);
    return __builtin_ctz(LANES);
}
template<WaveOrder ORDER, int LANES> __device__ __forceinline__ constexpr int wave_step(int i)
{
    return ORDER == WAVE_DOWN ? (LANES / 2) >> i : 1 << i;
}

// The exchanges one after another, for kernels that reduce several values side by side: body(other) is one exchange, and other(v)
// is v of the lane it pairs this one with, so the shuffles of a step are in flight together
template<WaveOrder ORDER = WAVE_DOWN, int LANES = 64, class Body> __device__ __forceinline__ void wave_butterfly(Body body)
{
#pragma unroll
    for(int i = 0; i < wave_steps<LANES>(); ++i)
        body([i](auto v) { return __shfl_xor(v, wave_step<ORDER, LANES>(i), 64); });
}

// v = op(v, the other lane's v) over the exchanges.  T: a number, or a struct of two (a value and its index), which travel together
template<WaveOrder ORDER = WAVE_DOWN, int LANES = 64, class T, class Op> __device__ __forceinline__ T wave_reduce(T v, Op op)
{
#pragma unroll
    for(int i = 0; i < wave_steps<LANES>(); ++i) {
        if constexpr(__is_class(T)) {
            T o;
            auto &[oa, ob] = o;
            const auto &[a, b] = v;
            oa = __shfl_xor(a, wave_step<ORDER, LANES>(i), 64);
            ob = __shfl_xor(b, wave_step<ORDER, LANES>(i), 64);
            v = op(v, o);
        } else
            v = op(v, __shfl_xor(v, wave_step<ORDER, LANES>(i), 64));
    }
    return v;
}

// T: float, double or uint32_t
template<WaveOrder ORDER = WAVE_DOWN, class T> __device__ __forceinline__ T wave_sum(T v)
{
    return wave_reduce<ORDER>(v, [](T a, T b) { return a + b; });
}

// Or, maxima and minima.  Floating point: the builtins (the device's fmax / fmin are these), so a NaN loses to a number.  Integers: the
// comparisons as the kernels have always written them -- which operand a tie returns decides nothing, but the compiler keeps the
// operand order.
#define WF_WAVE_FOLD(name, T, expr)                                                                       \
    template<WaveOrder ORDER = WAVE_DOWN, int LANES = 64> __device__ __forceinline__ T name(T v)            \
    {                                                                                                     \
        return wave_reduce<ORDER, LANES>(v, [](T a, T b) { return expr; });                                 \
    }
WF_WAVE_FOLD(wave_or, uint32_t, a | b)
WF_WAVE_FOLD(wave_max, float, __builtin_fmaxf(a, b))
WF_WAVE_FOLD(wave_min, float, __builtin_fminf(a, b))
WF_WAVE_FOLD(wave_max, double, __builtin_fmax(a, b))
WF_WAVE_FOLD(wave_min, double, __builtin_fmin(a, b))
WF_WAVE_FOLD(wave_max, uint32_t, a > b ? a : b)
WF_WAVE_FOLD(wave_min, uint32_t, b < a ? b : a)
WF_WAVE_FOLD(wave_max, uint64_t, b > a ? b : a)
WF_WAVE_FOLD(wave_min, uint64_t, b < a ? b : a)
#undef WF_WAVE_FOLD

// of two (value, index) candidates of an argmax: the larger value, and the lower index of equal values (a NaN never wins).  Also
// what folds the waves' candidates behind the butterfly.
__device__ __forceinline__ void argmax_better(double &v, uint32_t &k, double ov, uint32_t ok)
{
    if(ov > v || (ov == v && ok < k)) {
        v = ov;
        k = ok;
    }
}

// (the exchanges written out, not wave_reduce over a struct of the two: the compiler orders the tie's two comparisons by how the
// pair reaches it, and the kernels' text is compared from change to change)
__device__ __forceinline__ void wave_argmax(double &v, uint32_t &k)
{
#pragma unroll
    for(int i = 0; i < wave_steps<64>(); ++i) {
        const double ov = __shfl_xor(v, wave_step<WAVE_DOWN, 64>(i), 64);
        const uint32_t ok = __shfl_xor(k, wave_step<WAVE_DOWN, 64>(i), 64);
        argmax_better(v, k, ov, ok);
    }
}

// a 32- or 64-bit value that every lane holds alike, moved to scalar registers: what is decided from it branches for the whole
// wavefront
template<class T> __device__ __forceinline__ T wave_uniform(T v)
{
    static_assert(sizeof(T) == 4 || sizeof(T) == 8);
    uint32_t w[sizeof(T) / 4];
    __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
    for(uint32_t i = 0; i < sizeof(T) / 4; ++i)
        w[i] = __builtin_amdgcn_readfirstlane(w[i]);
    __builtin_memcpy(&v, w, sizeof(T));
    return v;
}

} // namespace wf
