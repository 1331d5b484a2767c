// wf_xfer_sums.hpp -- the head that the read kernels of WF_HIP_OUT_XFER (wf_xfer.hpp) and WF_HIP_OUT_IMPULSE (wf_impulse.hpp) share
// (device code only; hipcc): the span check, the averaged auto and cross spectra of the K half-overlapped segments of P frames in
// the rings of the two captured channels, and the integer delay between them by the floored PHAT of the cross spectrum, taken out
// by a second pass (the definition is in include/wf_hip.h, "transfer function").  Both outputs are defined on these sums, and both
// records carry lag, lag_peak and mean_coherence bit for bit, so the operations and their order are written once, here.
//
// One workgroup of WF_XFER_THREADS per stream calls xfer_sums, every thread of it; dynamic LDS is `z`, one region of P complex
// float64 for the transforms, and `ya`, half a region and a slot for the weighted cross spectrum.  The transform is
// wf_fft64_lds.hpp's, unchanged; every phase has consecutive lanes on consecutive bins.
//   span       every thread strides over the span of both channels: whether a channel holds anything but zeros and whether any
//              sample's exponent is all ones (a NaN or an infinity), as bits per wave; `false` where either says so: the caller
//              writes its zero record and leaves.
//   pass       the K segments oldest first, one transform of w (x_0 + j x_1(. - n)) each: thread t separates the channels of its
//              own bins k = 1 + t + 256 u, u < 4, as wf_stereo.hpp does it and adds |X_1|^2, |X_0|^2 and X_0 conj X_1 to 16 doubles
//              it keeps in registers.  A barrier in front of every segment: the region's readers are done before rows fall into it.
//              While it loads, every thread notes whether a channel of the segment holds anything but zeros and whether the two
//              differ in any bit, handed over per wave in front of the transform's barriers: a segment with a silent channel, or with
//              both channels the same, takes its spectra from Z[k] alone, and is then exact where the definition is.
//   lag        behind the pass with n = 0: g = max |Sxy| by wave butterflies and one hand-over; ya[k] = A[k], ya[0] = ya[M] = 0; one
//              transform of the Hermitian extension Y[k] = A[k], Y[P - k] = conj A[k], fetched from ya while the rows fall
//              into z, so that they cannot race; r[n] = Re y[-n] / (2 (M - 1)); the argmax as wf_delay.hpp's, argmax_better with the
//              index n + L: the larger |r| wins and the lower lag a tie.  No cross power at all: lag 0, no transform.
//   again      the pass once more with n = n0 where that is not 0 (uniform: every thread holds the same n0).
// The order of every sum and every max follows from P and K alone; there are no atomics and no scratch.  The caller's first access
// to z or ya behind the call needs a barrier in front of it: the last segment's readers may still be at work.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_ring_view.hpp"
#include "wf_wave_reduce.hpp"
#include "wf_fft64_lds.hpp"
#include "wf_phat.hpp"

namespace wf {

constexpr uint32_t WF_XFER_THREADS = 256;
constexpr uint32_t WF_XFER_WAVES = WF_XFER_THREADS / 64;
constexpr uint32_t WF_XFER_OWN = 4; // bins per thread at the cap
static_assert(WF_XFER_THREADS * WF_XFER_OWN == WF_HIP_XFER_MAX_WINDOW / 2 && WF_HIP_XFER_BINS == WF_HIP_XFER_MAX_WINDOW / 2,
              "every bin of the largest window has a thread and an index");
static_assert(WF_XFER_THREADS * 16 >= WF_HIP_XFER_MAX_WINDOW, "a thread per 16 frames of the largest window");

// Args: rings, window ([P] periodic Hann), tw ([P / 2] e^(-j 2 pi m / P)), P, log2p, K as XferArgs has them.  The sums of thread
// t's bins k = 1 + t + u WF_XFER_THREADS < M come back in sxx, syy, sxr + j sxi = Sxy, the lag in n0 and r[n0] in peak
template<class Args>
__device__ __forceinline__ bool xfer_sums(const Args &a, double2 *z, double2 *ya, uint32_t stream, double (&sxx)[WF_XFER_OWN], double (&syy)[WF_XFER_OWN],
                                          double (&sxr)[WF_XFER_OWN], double (&sxi)[WF_XFER_OWN], int32_t &n0, double &peak)
{
    // the cross-wave hand-overs, each written once
    __shared__ uint32_t seen[WF_XFER_WAVES]; // (bit c: a non-zero sample of channel c; bit 2: a NaN or an infinity)
    __shared__ uint32_t seg[WF_XFER_WAVES];  // (of the segment in hand; bit c: a non-zero sample of channel c; bit 2: the channels differ)
    __shared__ double max_g[WF_XFER_WAVES];
    __shared__ double arg_v[WF_XFER_WAVES];
    __shared__ uint32_t arg_k[WF_XFER_WAVES];

    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t P = a.P, cb = a.log2p - 4u, M = P / 2u, H = P / 2u, L = P / 4u, K = a.K;
    const uint32_t mask = a.rings.ring_cap - 1u;
    const uint32_t wpos = a.rings.wpos[stream];
    const uint32_t E = wpos - (wpos & (H - 1u)) - L; // where the newest segment of channel 0 ends; uint32 arithmetic that wraps with the counter
    const float *r0 = channel_ring(a.rings, stream, 0, 2);
    const float *r1 = channel_ring(a.rings, stream, 1, 2);

    // span: E - (K - 1) H - P - L .. E + L - 1 of both channels
    {
        const uint32_t span = (K - 1u) * H + P + 2u * L, s = E + L - span;
        uint32_t any0 = 0, any1 = 0, top = 0;
        for(uint32_t i = t; i < span; i += WF_XFER_THREADS) {
            const uint32_t pos = (s + i) & mask;
            const uint32_t b0 = __float_as_uint(r0[pos]), b1 = __float_as_uint(r1[pos]);
            any0 |= b0 & 0x7fffffffu;
            any1 |= b1 & 0x7fffffffu;
            top |= (uint32_t)((b0 & 0x7f800000u) == 0x7f800000u) | (uint32_t)((b1 & 0x7f800000u) == 0x7f800000u);
        }
        const bool w0 = __ballot(any0 != 0u) != 0ull, w1 = __ballot(any1 != 0u) != 0ull, wt = __ballot(top != 0u) != 0ull;
        if(lane == 0u)
            seen[wave] = (w0 ? 1u : 0u) | (w1 ? 2u : 0u) | (wt ? 4u : 0u);
    }
    __syncthreads();
    uint32_t all = 0u;
#pragma unroll
    for(uint32_t w = 0; w < WF_XFER_WAVES; ++w)
        all |= seen[w];

    // silence in either channel, a NaN or an infinity: the zero record (uniform: `all` is)
    if(all != 3u)
        return false;

    // pass: the sums over the K segments, oldest first, with channel 1 read n frames earlier
    const auto pass = [&](uint32_t n) __attribute__((always_inline)) {
#pragma unroll
        for(uint32_t u = 0; u < WF_XFER_OWN; ++u)
            sxx[u] = syy[u] = sxr[u] = sxi[u] = 0.0;
#pragma unroll 1
        for(uint32_t j = 0; j < K; ++j) {
            const uint32_t s0 = E - (K - 1u - j) * H - P, s1 = s0 - n; // the segment's first frame in either ring, unmasked
            __syncthreads(); // whoever read the region last is done with it, and with the segment's flags
            uint32_t any0 = 0, any1 = 0, differ = 0;
            fft64_load16(z, a.tw, t, P, cb, [&](uint32_t i) {
                const double w = a.window[i];
                const float x0 = r0[(s0 + i) & mask], x1 = r1[(s1 + i) & mask];
                const uint32_t b0 = __float_as_uint(x0), b1 = __float_as_uint(x1);
                any0 |= b0 & 0x7fffffffu;
                any1 |= b1 & 0x7fffffffu;
                differ |= b0 ^ b1;
                return make_double2(w * (double)x0, w * (double)x1);
            });
            {
                const bool w0 = __ballot(any0 != 0u) != 0ull, w1 = __ballot(any1 != 0u) != 0ull, wd = __ballot(differ != 0u) != 0ull;
                if(lane == 0u)
                    seg[wave] = (w0 ? 1u : 0u) | (w1 ? 2u : 0u) | (wd ? 4u : 0u);
            }
            fft64_passes<WF_XFER_THREADS>(z, a.tw, t, P, cb, fft64_block_sync{});
            uint32_t f = 0u;
#pragma unroll
            for(uint32_t w = 0; w < WF_XFER_WAVES; ++w)
                f |= seg[w];
            // X_0 = (Z[k] + conj Z[P-k]) / 2, X_1 = (Z[k] - conj Z[P-k]) / 2j -- two values that reach the same number by different
            // butterflies, so the separation leaves the transform's rounding where separate transforms leave none.  Three kinds of
            // segment therefore take their spectra from Z[k] alone (uniform: f is): channel 0 all +-0, Z = j X_1 and X_0 = 0 exactly;
            // channel 1 all +-0, Z = X_0; both channels the same bits, Z = (1 + j) X and X_0 = X_1 = Z (1 - j) / 2.  Products and
            // sums as they are written, none fused: spectra of the same bits give Sxx = Syy = Re Sxy and Im Sxy = 0 to the bit
#pragma unroll
            for(uint32_t u = 0; u < WF_XFER_OWN; ++u) {
#pragma clang fp contract(off)
                const uint32_t k = 1u + t + u * WF_XFER_THREADS;
                if(k < M) {
                    const double2 p = z[fft64_at(k, cb)], q = z[fft64_at(P - k, cb)];
                    double yr = 0.5 * (p.x + q.x), yi = 0.5 * (p.y - q.y);
                    double xr = 0.5 * (p.y + q.y), xi = -0.5 * (p.x - q.x);
                    if((f & 1u) == 0u) {
                        yr = yi = 0.0;
                        xr = p.y;
                        xi = -p.x;
                    } else if((f & 2u) == 0u) {
                        xr = xi = 0.0;
                        yr = p.x;
                        yi = p.y;
                    } else if((f & 4u) == 0u) {
                        xr = yr = 0.5 * (p.x + p.y);
                        xi = yi = 0.5 * (p.y - p.x);
                    }
                    sxx[u] += xr * xr + xi * xi;
                    syy[u] += yr * yr + yi * yi;
                    sxr[u] += xr * yr + xi * yi;
                    sxi[u] += xr * yi - xi * yr;
                }
            }
        }
    };
    pass(0u);

    // lag: the floored PHAT of G = Sxy
    n0 = 0;
    peak = 0.0;
    double g = 0.0;
#pragma unroll
    for(uint32_t u = 0; u < WF_XFER_OWN; ++u)
        g = fmax(g, sqrt(sxr[u] * sxr[u] + sxi[u] * sxi[u])); // (0 for a bin there is none of)
    g = wave_max(g);
    if(lane == 0u)
        max_g[wave] = g;
    __syncthreads();
    g = max_g[0];
#pragma unroll
    for(uint32_t w = 1; w < WF_XFER_WAVES; ++w)
        g = fmax(g, max_g[w]);
    if(g > 0.0) { // (uniform; no cross power in any bin: lag 0, and the sums stand)
        const double floor_g = WF_DELAY_BETA * g;
#pragma unroll
        for(uint32_t u = 0; u < WF_XFER_OWN; ++u) {
            const uint32_t k = 1u + t + u * WF_XFER_THREADS;
            if(k < M) {
                const double d = fmax(sqrt(sxr[u] * sxr[u] + sxi[u] * sxi[u]), floor_g);
                ya[k] = make_double2(sxr[u] / d, sxi[u] / d);
            }
        }
        if(t == 0u)
            ya[0] = ya[M] = make_double2(0.0, 0.0);
        __syncthreads(); // ya is written, and every thread is behind its last read of z
        fft64_load16(z, a.tw, t, P, cb, [&](uint32_t i) { // Y[i] = ya[i] up to M, conj ya[P - i] beyond
            const double2 c = ya[i <= M ? i : P - i];
            return make_double2(c.x, i <= M ? c.y : -c.y);
        });
        fft64_passes<WF_XFER_THREADS>(z, a.tw, t, P, cb, fft64_block_sync{});
        const double r_norm = 2.0 * (double)(M - 1u);
        const auto R = [&](int32_t n) { return z[fft64_at((uint32_t)(-n) & (P - 1u), cb)].x / r_norm; }; // Re y[(-n) mod P]

        // argmax of |r[n]|, -L <= n <= L, by the index n + L: the larger value, the lower lag of equal values
        double best = -1.0;
        uint32_t kbest = 0u;
        for(uint32_t i = t; i <= 2u * L; i += WF_XFER_THREADS) {
            const double v = fabs(R((int32_t)i - (int32_t)L));
            if(v > best) {
                best = v;
                kbest = i;
            }
        }
        wave_argmax(best, kbest);
        if(lane == 0u) {
            arg_v[wave] = best;
            arg_k[wave] = kbest;
        }
        __syncthreads();
        best = arg_v[0];
        kbest = arg_k[0];
#pragma unroll
        for(uint32_t w = 1; w < WF_XFER_WAVES; ++w)
            argmax_better(best, kbest, arg_v[w], arg_k[w]);
        n0 = (int32_t)kbest - (int32_t)L;
        peak = R(n0); // (the pass that may follow starts with a barrier)
        if(n0 != 0)   // (uniform; at lag 0 the sums of the first pass are the result)
            pass((uint32_t)n0);
    }
    return true;
}

} // namespace wf
