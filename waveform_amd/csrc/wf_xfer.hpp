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
//   span       every thread strides over the span of both channels: whether a channel holds anything but zeros and whether any
//              sample's exponent is all ones (a NaN or an infinity), as bits per wave; the zero record and out where either says so.
//   pass       the K segments oldest first, one transform of w (x_0 + j x_1(. - n)) each: thread t separates the channels of its
//              own bins k = 1 + t + 256 u, u < 4, as wf_stereo.hpp does it and adds |X_1|^2, |X_0|^2 and X_0 conj X_1 to 16 doubles
//              it keeps in registers.  A barrier in front of every segment: the region's readers are done before rows fall into it.
//              While it loads, every thread notes whether a channel of the segment holds anything but zeros and whether the two
//              differ in any bit, handed over per wave in front of the transform's barriers: a segment with a silent channel, or with
//              both channels the same, takes its spectra from Z[k] alone, and is then exact where the definition is.
//   lag        behind the pass with n = 0: g = max |Sxy| by wave butterflies and one hand-over; ya[k] = A[k], ya[0] = ya[M] = 0; one
//              transform of the Hermitian extension Y[k] = A[k], Y[P - k] = conj A[k], fetched from ya while the rows fall
//              into z, so that they cannot race; r[n] = Re y[-n] / (2 (M - 1)); the argmax as wf_delay.hpp's, thd_better with the
//              index n + L: the larger |r| wins and the lower lag a tie.  No cross power at all: lag 0, no transform.
//   again      the pass once more with n = n0 where that is not 0 (uniform: every thread holds the same n0).
//   record     max Sxx by butterflies and a hand-over; every thread the three fields of its own bins; the weighted mean of the
//              coherence by wave sums, added up by thread 0 in wave order; index 0 and the indices from M up as zeros.
// The order of every sum and every max follows from P and K alone; there are no atomics and no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_ring_view.hpp"
#include "wf_wave_reduce.hpp"
#include "wf_fft64_lds.hpp"
#include "wf_thd.hpp"   // thd_better, thd_wave_argmax
#include "wf_delay.hpp" // delay_wave_max, WF_DELAY_BETA

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

constexpr uint32_t WF_XFER_THREADS = 256;
constexpr uint32_t WF_XFER_WAVES = WF_XFER_THREADS / 64;
constexpr uint32_t WF_XFER_OWN = 4; // bins per thread at the cap
static_assert(WF_XFER_THREADS * WF_XFER_OWN == WF_HIP_XFER_MAX_WINDOW / 2 && WF_HIP_XFER_BINS == WF_HIP_XFER_MAX_WINDOW / 2,
              "every bin of the largest window has a thread and an index");
static_assert(WF_XFER_THREADS * 16 >= WF_HIP_XFER_MAX_WINDOW, "a thread per 16 frames of the largest window");
static_assert(sizeof(wf_hip_xfer) == 12336 && offsetof(wf_hip_xfer, phase) == offsetof(wf_hip_xfer, gain_db) + WF_HIP_XFER_BINS * sizeof(float) &&
                  offsetof(wf_hip_xfer, coherence) == offsetof(wf_hip_xfer, phase) + WF_HIP_XFER_BINS * sizeof(float),
              "the three curves are 3 x WF_HIP_XFER_BINS consecutive floats");

// grid: one workgroup per stream of [first, first + gridDim.x); dynamic LDS: (P + P / 2 + 1) * sizeof(double2)
__global__ __launch_bounds__(WF_XFER_THREADS, 2) void xfer_read_kernel(const XferArgs a)
{
    extern __shared__ __align__(16) double2 xfer_lds[];
    // the cross-wave hand-overs, each written once
    __shared__ uint32_t seen[WF_XFER_WAVES]; // (bit c: a non-zero sample of channel c; bit 2: a NaN or an infinity)
    __shared__ uint32_t seg[WF_XFER_WAVES];  // (of the segment in hand; bit c: a non-zero sample of channel c; bit 2: the channels differ)
    __shared__ double max_g[WF_XFER_WAVES], max_x[WF_XFER_WAVES];
    __shared__ double arg_v[WF_XFER_WAVES];
    __shared__ uint32_t arg_k[WF_XFER_WAVES];
    __shared__ double coh_num[WF_XFER_WAVES], coh_den[WF_XFER_WAVES];

    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t stream = a.first + blockIdx.x;
    const uint32_t P = a.P, cb = a.log2p - 4u, M = P / 2u, H = P / 2u, L = P / 4u, K = a.K;
    double2 *z = xfer_lds, *ya = xfer_lds + P;
    const uint32_t mask = a.rings.ring_cap - 1u;
    const uint32_t wpos = a.rings.wpos[stream];
    const uint32_t E = wpos - (wpos & (H - 1u)) - L; // where the newest segment of channel 0 ends; uint32 arithmetic that wraps with the counter
    const float *r0 = channel_ring(a.rings, stream, 0, 2);
    const float *r1 = channel_ring(a.rings, stream, 1, 2);
    wf_hip_xfer *out = a.out + blockIdx.x;
    float *const curves = &out->gain_db[0]; // gain_db, phase, coherence: 3 x WF_HIP_XFER_BINS consecutive floats

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
    if(all != 3u) {
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

    // the running sums of this thread's bins k = 1 + t + u WF_XFER_THREADS
    double sxx[WF_XFER_OWN], syy[WF_XFER_OWN], sxr[WF_XFER_OWN], sxi[WF_XFER_OWN];
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
    int32_t n0 = 0;
    double peak = 0.0;
    double g = 0.0;
#pragma unroll
    for(uint32_t u = 0; u < WF_XFER_OWN; ++u)
        g = fmax(g, sqrt(sxr[u] * sxr[u] + sxi[u] * sxi[u])); // (0 for a bin there is none of)
    g = delay_wave_max(g);
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
        thd_wave_argmax(best, kbest);
        if(lane == 0u) {
            arg_v[wave] = best;
            arg_k[wave] = kbest;
        }
        __syncthreads();
        best = arg_v[0];
        kbest = arg_k[0];
#pragma unroll
        for(uint32_t w = 1; w < WF_XFER_WAVES; ++w)
            thd_better(best, kbest, arg_v[w], arg_k[w]);
        n0 = (int32_t)kbest - (int32_t)L;
        peak = R(n0); // (the pass that may follow starts with a barrier)
        if(n0 != 0)   // (uniform; at lag 0 the sums of the first pass are the result)
            pass((uint32_t)n0);
    }

    // record
    double mx = 0.0;
#pragma unroll
    for(uint32_t u = 0; u < WF_XFER_OWN; ++u)
        mx = fmax(mx, sxx[u]);
    mx = delay_wave_max(mx);
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
