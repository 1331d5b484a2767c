// wf_xfer.hpp -- gfx950 read kernel of WF_HIP_OUT_XFER (device code only; hipcc; included by wf_hip_measure.hip alone).
//
// Not in the reference: the transfer function of a dual-channel analyser, the gain, phase and coherence per bin of captured
// channel 0 (measured) against channel 1 (reference), averaged over the K half-overlapped segments of P frames in the rings, with
// the integer delay between the channels found by the floored PHAT of the averaged cross spectrum and taken out (the definition is
// in include/wf_hip.h, "transfer function").  wf_hip_read launches it on the handle's stream, behind every push issued so far, and
// copies the result back; nothing runs while the output is not read and nothing is kept between reads.
//
// One workgroup of WF_XFER_THREADS per stream; dynamic LDS is `z`, one region of P complex float64 for the transforms, and `ya`,
// half a region and a slot for the weighted cross spectrum (16 B x (3 P / 2 + 1): 48 KB at P = 2048; the registers, not the LDS,
// keep it to two workgroups a CU).  The transform is wf_fft64_lds.hpp's, unchanged; every phase has consecutive lanes on
// consecutive bins.
//   span, pass, lag, again   wf_xfer_sums.hpp's xfer_sums, which WF_HIP_OUT_IMPULSE's kernel (wf_impulse.hpp) shares: the span
//              check -- the zero record and out where it says so --, the sums of the K segments in 16 doubles a thread, the lag by
//              the floored PHAT and the second pass where the lag is not 0.
//   record     max Sxx by butterflies and a hand-over; every thread the three fields of its own bins; the weighted mean of the
//              coherence by wave sums, added up by thread 0 in wave order; index 0 and the indices from M up as zeros.
// The order of every sum and every max follows from P and K alone; there are no atomics and no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_xfer_sums.hpp"

namespace wf {

struct XferArgs {
    RingView rings;
    wf_hip_xfer *out;        // [count] the entry of stream `first`
    const double *window;    // [P] periodic Hann
    const double2 *tw;       // [P / 2] e^(-j 2 pi m / P)
    uint32_t first;          // first stream read
    uint32_t P;              // segment frames: a power of two, 64 <= P <= min(ring_cap / 8, WF_HIP_XFER_MAX_WINDOW)
    uint32_t log2p;
    uint32_t K;              // segments: (K - 1) P / 2 + 2 P + P / 2 - 1 < ring_cap
};

static_assert(sizeof(wf_hip_xfer) == 12336 && offsetof(wf_hip_xfer, phase) == offsetof(wf_hip_xfer, gain_db) + WF_HIP_XFER_BINS * sizeof(float) &&
                  offsetof(wf_hip_xfer, coherence) == offsetof(wf_hip_xfer, phase) + WF_HIP_XFER_BINS * sizeof(float),
              "the three curves are 3 x WF_HIP_XFER_BINS consecutive floats");

// grid: one workgroup per stream of [first, first + gridDim.x); dynamic LDS: (P + P / 2 + 1) * sizeof(double2)
__global__ __launch_bounds__(WF_XFER_THREADS, 2) void xfer_read_kernel(const XferArgs a)
{
    extern __shared__ __align__(16) double2 xfer_lds[];
    // the cross-wave hand-overs, each written once
    __shared__ double max_x[WF_XFER_WAVES];
    __shared__ double coh_num[WF_XFER_WAVES], coh_den[WF_XFER_WAVES];

    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t stream = a.first + blockIdx.x;
    const uint32_t P = a.P, M = P / 2u, H = P / 2u, K = a.K;
    double2 *z = xfer_lds, *ya = xfer_lds + P;
    const uint32_t wpos = a.rings.wpos[stream];
    wf_hip_xfer *out = a.out + blockIdx.x;
    float *const curves = &out->gain_db[0]; // gain_db, phase, coherence: 3 x WF_HIP_XFER_BINS consecutive floats

    // the running sums of this thread's bins k = 1 + t + u WF_XFER_THREADS, the lag and r[lag]
    double sxx[WF_XFER_OWN], syy[WF_XFER_OWN], sxr[WF_XFER_OWN], sxi[WF_XFER_OWN];
    int32_t n0;
    double peak;
    // silence in either channel, a NaN or an infinity: the zero record (uniform)
    if(!xfer_sums(a, z, ya, stream, sxx, syy, sxr, sxi, n0, peak)) {
        for(uint32_t i = t; i < 3u * WF_HIP_XFER_BINS; i += WF_XFER_THREADS)
            curves[i] = 0.f;
        if(t == 0u) {
            out->valid = 0u;
            out->window = P;
            out->hop = H;
            out->segments = K;
            out->lag = 0;
            out->newest = 0u;
            out->lag_peak = out->mean_coherence = 0.f;
            out->reserved[0] = out->reserved[1] = out->reserved[2] = out->reserved[3] = 0u;
        }
        return;
    }

    // record
    double mx = 0.0;
#pragma unroll
    for(uint32_t u = 0; u < WF_XFER_OWN; ++u)
        mx = fmax(mx, sxx[u]);
    mx = wave_max(mx);
    if(lane == 0u)
        max_x[wave] = mx;
    __syncthreads();
    mx = max_x[0];
#pragma unroll
    for(uint32_t w = 1; w < WF_XFER_WAVES; ++w)
        mx = fmax(mx, max_x[w]);
    const double dead = WF_HIP_STEREO_DEAD_RATIO * mx;

    double num = 0.0, den = 0.0;
#pragma unroll
    for(uint32_t u = 0; u < WF_XFER_OWN; ++u) {
        const uint32_t k = 1u + t + u * WF_XFER_THREADS;
        if(k < M) {
            float gain = 0.f, phase = 0.f, coh = 0.f;
            if(sxx[u] > dead) {
                den += sxx[u];
                if(syy[u] == 0.0)
                    gain = -INFINITY;
                else {
                    const double m2 = sxr[u] * sxr[u] + sxi[u] * sxi[u];
                    const double c = fmin(m2 / (sxx[u] * syy[u]), 1.0);
                    num += sxx[u] * c;
                    gain = (float)(10.0 * log10(m2 / (sxx[u] * sxx[u])));
                    phase = (float)atan2(sxi[u] / sxx[u], sxr[u] / sxx[u]);
                    coh = (float)c;
                }
            }
            curves[k] = gain;
            curves[WF_HIP_XFER_BINS + k] = phase;
            curves[2u * WF_HIP_XFER_BINS + k] = coh;
        }
    }
    // index 0 and the indices from M up: zeros on every read (the block is reused, and a slice may be its first read)
    for(uint32_t i = t; i < WF_HIP_XFER_BINS; i += WF_XFER_THREADS)
        if(i == 0u || i >= M)
            curves[i] = curves[WF_HIP_XFER_BINS + i] = curves[2u * WF_HIP_XFER_BINS + i] = 0.f;
    num = wave_sum(num);
    den = wave_sum(den);
    if(lane == 0u) {
        coh_num[wave] = num;
        coh_den[wave] = den;
    }
    __syncthreads();
    if(t == 0u) {
        num = coh_num[0];
        den = coh_den[0];
#pragma unroll
        for(uint32_t w = 1; w < WF_XFER_WAVES; ++w) {
            num += coh_num[w];
            den += coh_den[w];
        }
        out->valid = 1u;
        out->window = P;
        out->hop = H;
        out->segments = K;
        out->lag = n0;
        out->newest = wpos / H;
        out->lag_peak = (float)peak;
        out->mean_coherence = den > 0.0 ? (float)(num / den) : 0.f;
        out->reserved[0] = out->reserved[1] = out->reserved[2] = out->reserved[3] = 0u;
    }
}

} // namespace wf
