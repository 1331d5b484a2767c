// wf_thd_spectrum.hpp -- the head that the read kernels of WF_HIP_OUT_THD (wf_thd.hpp) and WF_HIP_OUT_IMD (wf_imd.hpp) share
// (device code only; hipcc; holds no kernel): the newest P frames of a stream's captured channels through the periodic 7-term
// Blackman-Harris taper, one complex float64 transform in LDS (wf_fft64_lds.hpp) and the power of every bin of either channel
// (the definition is in include/wf_hip.h, "distortion": window, taper, spectrum).  Also dB(x, y) of that definition and the
// workgroup both kernels run as.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_ring_view.hpp"
#include "wf_wave_reduce.hpp"
#include "wf_fft64_lds.hpp"

namespace wf {

constexpr uint32_t WF_THD_THREADS = 512;
constexpr uint32_t WF_THD_WAVES = WF_THD_THREADS / 64;
static_assert(WF_THD_THREADS * 16 == WF_HIP_THD_MAX_WINDOW, "one thread per 16 frames of the largest window");
static_assert(2 * WF_HIP_THD_LOBE + 1 <= 64, "a region is summed by the lanes of one wavefront");

// dB(x, y) of the definition: -inf where the numerator is 0, else +inf where the denominator is 0
__device__ __forceinline__ double thd_db(double num, double den)
{
    if(num == 0.0)
        return -INFINITY;
    if(den == 0.0)
        return INFINITY;
    return 10.0 * log10(num / den);
}

// Called by all WF_THD_THREADS threads of a workgroup, lds: P double2 of dynamic LDS.  On return slot fft64_at(k, a.log2p - 4) holds
// (p_0[k], p_1[k]) for 1 <= k < P / 2, behind a barrier.  Args: rings, window [P], tw [P / 2], first, P, log2p (ThdArgs, ImdArgs)
template<int CH, class Args> __device__ __forceinline__ void thd_spectrum(double2 *lds, const Args &a, uint32_t t)
{
    __shared__ uint32_t live[WF_THD_WAVES]; // (bit c: the wave has loaded a non-zero sample of channel c)
    const uint32_t lane = t & 63u, wave = t >> 6;
    const uint32_t stream = a.first + blockIdx.x;
    const uint32_t P = a.P, cb = a.log2p - 4u, M = P / 2u;
    const uint32_t mask = a.rings.ring_cap - 1u;
    const uint32_t s = window_start(a.rings, stream, P);
    const float *r0 = channel_ring(a.rings, stream, 0, CH);
    const float *r1 = channel_ring(a.rings, stream, CH - 1, CH);

    // load: the 16-point transform of frames c' + m P/16 in registers; then the passes.  With two channels the load also notes
    // which of them hold anything but zeros (`live`: the OR of the samples' magnitude bits, per wave, handed over before the
    // passes' first barrier and read behind their last)
    uint32_t any0 = 0, any1 = 0;
    fft64_load16(lds, a.tw, t, P, cb, [&](uint32_t i) {
        const uint32_t pos = (s + i) & mask;
        const double w = a.window[i];
        const float x0 = r0[pos], x1 = CH == 2 ? r1[pos] : 0.f;
        any0 |= __float_as_uint(x0) & 0x7fffffffu;
        any1 |= __float_as_uint(x1) & 0x7fffffffu;
        return make_double2(w * (double)x0, w * (double)x1);
    });
    if(CH == 2) {
        const bool w0 = __ballot(any0 != 0u) != 0ull, w1 = __ballot(any1 != 0u) != 0ull;
        if(lane == 0u)
            live[wave] = (w0 ? 1u : 0u) | (w1 ? 2u : 0u);
    }
    fft64_passes<WF_THD_THREADS>(lds, a.tw, t, P, cb, fft64_block_sync{});
    uint32_t alive = 3u;
    if(CH == 2) {
        alive = 0u;
#pragma unroll
        for(uint32_t w = 0; w < WF_THD_WAVES; ++w)
            alive |= live[w];
    }

    // bins: X_0 = (Z[k] + conj Z[P-k]) / 2, X_1 = (Z[k] - conj Z[P-k]) / 2j; slot k: |X_0|^2, |X_1|^2.  One channel: X_0 = Z
    for(uint32_t k = 1u + t; k < M; k += WF_THD_THREADS) {
        const uint32_t ia = fft64_at(k, cb);
        const double2 za = lds[ia];
        if(CH == 2) {
            const double2 zb = lds[fft64_at(P - k, cb)];
            const double lr = 0.5 * (za.x + zb.x), li = 0.5 * (za.y - zb.y);
            const double rr = 0.5 * (za.y + zb.y), ri = -0.5 * (za.x - zb.x);
            // (an all-zero channel is exact silence: the shared transform's rounding would leave it some 1e-32 of the other's power)
            lds[ia] = make_double2((alive & 1u) ? lr * lr + li * li : 0.0, (alive & 2u) ? rr * rr + ri * ri : 0.0);
        } else
            lds[ia] = make_double2(za.x * za.x + za.y * za.y, 0.0);
    }
    __syncthreads();
}

} // namespace wf
