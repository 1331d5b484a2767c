// wf_stereo.hpp -- gfx950 read kernel of WF_HIP_OUT_STEREO (device code only; hipcc; included by wf_hip_measure.hip alone).
//
// Not in the reference: correlation, coherence, phase and balance between captured channels 0 and 1 in each of the 31
// third-octave bands, from one complex float64 transform of the newest P frames of both rings (the definition is in
// include/wf_hip.h, "stereo image").  wf_hip_read launches it on the handle's stream, behind every push issued so far, and
// copies the result back; nothing runs while the output is not read.
//
// One workgroup of WF_STEREO_THREADS per stream; the transform lives in LDS as P complex float64 (16 B each: 64 KB at P = 4096,
// the whole of what a workgroup gets without asking, so nothing else is kept in LDS).  The transform itself -- the 16-point load
// in registers, the passes of two radix-2 stages, the swizzled LDS addressing -- is wf_fft64_lds.hpp's, shared with the sonogram
// (wf_sono.hpp); here all 256 threads share one transform and __syncthreads orders its phases.  Behind it:
//   bins    thread per pair (k, P - k): Z[k] and Z[P - k] become |L|^2, |R|^2 in slot k and L conj(R) in slot P - k.
//   bands   wavefront w takes bands w, w + 4, ...; its lanes stride over the band's bins, each with four float64 sums, reduced
//           by the fixed butterfly of wf_wave_reduce.hpp; the four fields leave from lane 0.
// The order of every sum follows from P and the edges alone; there are no atomics and no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_ring_view.hpp"
#include "wf_wave_reduce.hpp"
#include "wf_fft64_lds.hpp"

namespace wf {

struct StereoArgs {
    RingView rings;          // (two captured channels)
    wf_hip_stereo *out;      // [count] the entry of stream `first`
    const double *window;    // [P] periodic Hann
    const double2 *tw;       // [P / 2] e^(-j 2 pi m / P)
    const double *edges;     // [WF_HIP_NUM_BANDS + 1] band edges in bins of P, ascending
    uint32_t first;          // first stream read
    uint32_t P;              // window frames: a power of two, 64 <= P <= min(ring_cap, WF_HIP_STEREO_MAX_WINDOW)
    uint32_t log2p;
    uint32_t covered;        // wf_hip_stereo::covered, the same for every stream
};

constexpr uint32_t WF_STEREO_THREADS = 256;
constexpr uint32_t WF_STEREO_WAVES = WF_STEREO_THREADS / 64;
static_assert(WF_STEREO_THREADS * 16 == WF_HIP_STEREO_MAX_WINDOW, "one thread per 16 frames of the largest window");

// grid: one workgroup per stream of [first, first + gridDim.x); dynamic LDS: P * sizeof(double2)
__global__ __launch_bounds__(WF_STEREO_THREADS) void stereo_read_kernel(const StereoArgs a)
{
    extern __shared__ __align__(16) double2 stereo_lds[];
    double2 *lds = stereo_lds;

    const uint32_t t = threadIdx.x;
    const uint32_t stream = a.first + blockIdx.x;
    const uint32_t P = a.P, cb = a.log2p - 4u;
    const uint32_t mask = a.rings.ring_cap - 1u;
    const uint32_t s = window_start(a.rings, stream, P);
    const float *r0 = channel_ring(a.rings, stream, 0, 2);
    const float *r1 = channel_ring(a.rings, stream, 1, 2);

    // load: the 16-point transform of frames c' + m P/16 in registers; then the passes
    fft64_load16(lds, a.tw, t, P, cb, [&](uint32_t i) {
        const uint32_t pos = (s + i) & mask;
        const double w = a.window[i];
        return make_double2(w * (double)r0[pos], w * (double)r1[pos]);
    });
    fft64_passes<WF_STEREO_THREADS>(lds, a.tw, t, P, cb, fft64_block_sync{});

    // bins: L = (Z[k] + conj Z[P-k]) / 2, R = (Z[k] - conj Z[P-k]) / 2j; slot k: |L|^2, |R|^2; slot P - k: L conj(R)
    const uint32_t M = P / 2u;
    for(uint32_t k = 1u + t; k < M; k += WF_STEREO_THREADS) {
        const uint32_t ia = fft64_at(k, cb), ib = fft64_at(P - k, cb);
        const double2 za = lds[ia], zb = lds[ib];
        const double lr = 0.5 * (za.x + zb.x), li = 0.5 * (za.y - zb.y);
        const double rr = 0.5 * (za.y + zb.y), ri = -0.5 * (za.x - zb.x);
        lds[ia] = make_double2(lr * lr + li * li, rr * rr + ri * ri);
        lds[ib] = make_double2(lr * rr + li * ri, li * rr - lr * ri);
    }
    __syncthreads();

    // bands
    const uint32_t lane = t & 63u, wave = t >> 6;
    wf_hip_stereo *out = a.out + blockIdx.x;
    for(uint32_t b = wave; b < WF_HIP_NUM_BANDS; b += WF_STEREO_WAVES) {
        const double lo = a.edges[b], hi = a.edges[b + 1u];
        // the bins that can overlap [lo, hi], generously: a bin outside it has the weight 0 and adds nothing
        const double f0 = floor(lo - 0.5), f1 = ceil(hi + 0.5) + 1.0;
        const uint32_t k0 = f0 > 1.0 ? (f0 < (double)M ? (uint32_t)f0 : M) : 1u;
        const uint32_t k1 = f1 < (double)M ? (f1 > 0.0 ? (uint32_t)f1 : 0u) : M;
        double sa = 0.0, sb = 0.0, xr = 0.0, xi = 0.0;
        for(uint32_t k = k0 + lane; k < k1; k += 64u) {
            const double2 p = lds[fft64_at(k, cb)], c = lds[fft64_at(P - k, cb)];
            const double kk = (double)k;
            const double w = fmax(fmin(kk + 0.5, hi) - fmax(kk - 0.5, lo), 0.0);
            sa = fma(w, p.x, sa);
            sb = fma(w, p.y, sb);
            xr = fma(w, c.x, xr);
            xi = fma(w, c.y, xi);
        }
        sa = wave_sum(sa);
        sb = wave_sum(sb);
        xr = wave_sum(xr);
        xi = wave_sum(xi);
        // a channel WF_HIP_STEREO_DEAD_RATIO under the other is what the transform's rounding leaves of a dead one: it counts as 0
        const double sa0 = sa;
        sa = sa > sb * WF_HIP_STEREO_DEAD_RATIO ? sa : 0.0;
        sb = sb > sa0 * WF_HIP_STEREO_DEAD_RATIO ? sb : 0.0;
        if(lane == 0u) {
            float corr = 0.f, coh = 0.f, ph = 0.f, bal = 0.f;
            if(sa > 0.0 && sb > 0.0) {
                const double d = sqrt(sa * sb);
                const double c = xr / d, g = sqrt(xr * xr + xi * xi) / d;
                corr = (float)(c < -1.0 ? -1.0 : c > 1.0 ? 1.0 : c);
                coh = (float)(g > 1.0 ? 1.0 : g);
                ph = (float)(atan2(xi, xr) * (180.0 / 3.141592653589793));
                if(ph == -180.f)
                    ph = 180.f;
                bal = (float)(10.0 * log10(sb / sa));
            } else
                bal = sa > 0.0 ? -INFINITY : sb > 0.0 ? INFINITY : 0.f;
            out->correlation[b] = corr;
            out->coherence[b] = coh;
            out->phase_deg[b] = ph;
            out->balance_db[b] = bal;
        }
    }
    if(t == 0u) {
        out->covered = a.covered;
        out->window = P;
    }
}

} // namespace wf
