// wf_delay.hpp -- gfx950 read kernel of WF_HIP_OUT_DELAY (device code only; hipcc; included by wf_hip_measure.hip alone).
//
// Not in the reference: the delay finder, by how many frames one captured channel lags the other and whether one of them is
// inverted, from the floored-PHAT cross-correlation of the newest P frames of both rings (the definition is in include/wf_hip.h,
// "inter-channel delay").  wf_hip_read launches it on the handle's stream, behind every push issued so far, and copies the result
// back; nothing runs while the output is not read.
//
// One workgroup of WF_DELAY_THREADS per stream and two regions of P complex float64 in dynamic LDS, `za` and `zb` (2 x 16 B per
// frame: 128 KB at P = 4096, one workgroup to a CU).  Both transforms are wf_fft64_lds.hpp's, unchanged; every phase has
// consecutive lanes on consecutive bins and goes through fft64_at, whole 16-byte slots.
//   load       za = the 16-point transforms of w (x_0 + j x_1); per wave, whether a channel holds anything but zeros and whether
//              any sample's exponent is all ones (a NaN or an infinity), as bits handed over before the passes' first barrier.
//   passes     za = Z, the transform of both channels at once.
//   pairs      thread per pair (k, P - k): the channels separated as wf_stereo.hpp does it, G[k] = X_0 conj X_1 into slot k of za;
//              g = max |G|, E_0, E_1 by wave butterflies and one hand-over, summed by every thread in wave order.
//   spectrum   zb = Y with Y[k] = A[k] + j G[k] / g, Y[P - k] = conj A[k] + j conj G[k] / g, Y[0] = Y[M] = 0.  G enters divided by
//              its own maximum, so that both halves of Y are of order 1 whatever the level of the audio and neither drowns the
//              other in the transform's rounding; C[n] gets the g back.
//   transform  fft64_load16 fetches from zb and stores its rows into za (G is spent by then): the fetch reads one region and the
//              row stores fall into the other, so they cannot race.  za = y, and R[n] = Re y[-n] / (2 (M - 1)),
//              C[n] = g Im y[-n] / (2 sqrt(E_0 E_1)).
//   argmax     threads stride over the 2 L + 1 lags from -L up; argmax_better with the index n + L: the larger |R| wins and the lower
//              lag a tie.  Then the largest |R| more than two lags away from it.
//   fraction   zb still holds Y, which the transform only read: A[k] = (Y[k] + conj Y[P - k]) / 2 comes back from it to one
//              rounding of a value <= 1 (this is the choice "keep A in the second region"), u[k] = |A[k]|, and the rotation
//              e^(j 2 pi ((k n0) mod P) / P) from the twiddle table by symmetry.  atan2 in float64.
//   record     thread 0 the fields, lanes 0 .. 64 the curve.
// The order of every sum and every max follows from P alone; there are no atomics and no scratch, and the hand-overs are all the
// static LDS there is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_ring_view.hpp"
#include "wf_wave_reduce.hpp"
#include "wf_fft64_lds.hpp"
#include "wf_phat.hpp"

namespace wf {

struct DelayArgs {
    RingView rings;
    wf_hip_delay *out;       // [count] the entry of stream `first`
    const double *window;    // [P] periodic Hann
    const double2 *tw;       // [P / 2] e^(-j 2 pi m / P)
    double sample_rate;
    uint32_t first;          // first stream read
    uint32_t P;              // window frames: a power of two, 128 <= P <= min(ring_cap, WF_HIP_DELAY_MAX_WINDOW)
    uint32_t log2p;
};

constexpr uint32_t WF_DELAY_THREADS = 256;
constexpr uint32_t WF_DELAY_WAVES = WF_DELAY_THREADS / 64;
static_assert(WF_DELAY_THREADS * 16 == WF_HIP_DELAY_MAX_WINDOW, "one thread per 16 frames of the largest window");
static_assert(WF_HIP_DELAY_CURVE <= WF_DELAY_THREADS && (WF_HIP_DELAY_CURVE & 1) == 1, "a lane per curve entry, the peak in the middle");

// grid: one workgroup per stream of [first, first + gridDim.x); dynamic LDS: 2 * P * sizeof(double2)
__global__ __launch_bounds__(WF_DELAY_THREADS) void delay_read_kernel(const DelayArgs a)
{
    extern __shared__ __align__(16) double2 delay_lds[];
    // the cross-wave hand-overs
    __shared__ uint32_t seen[WF_DELAY_WAVES]; // (bit c: a non-zero sample of channel c; bit 2: a NaN or an infinity)
    __shared__ double sum_g[WF_DELAY_WAVES], sum_e0[WF_DELAY_WAVES], sum_e1[WF_DELAY_WAVES];
    __shared__ double arg_v[WF_DELAY_WAVES], second_v[WF_DELAY_WAVES];
    __shared__ uint32_t arg_k[WF_DELAY_WAVES];
    __shared__ double reg_num[WF_DELAY_WAVES], reg_den[WF_DELAY_WAVES];

    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t stream = a.first + blockIdx.x;
    const uint32_t P = a.P, cb = a.log2p - 4u, M = P / 2u, L = P / 4u;
    double2 *za = delay_lds, *zb = delay_lds + P;
    const uint32_t mask = a.rings.ring_cap - 1u;
    const uint32_t s = window_start(a.rings, stream, P);
    const float *r0 = channel_ring(a.rings, stream, 0, 2);
    const float *r1 = channel_ring(a.rings, stream, 1, 2);
    wf_hip_delay *out = a.out + blockIdx.x;

    // load and passes: Z = DFT(w (x_0 + j x_1))
    uint32_t any0 = 0, any1 = 0, top = 0;
    fft64_load16(za, a.tw, t, P, cb, [&](uint32_t i) {
        const uint32_t pos = (s + i) & mask;
        const double w = a.window[i];
        const float x0 = r0[pos], x1 = r1[pos];
        const uint32_t b0 = __float_as_uint(x0), b1 = __float_as_uint(x1);
        any0 |= b0 & 0x7fffffffu;
        any1 |= b1 & 0x7fffffffu;
        top |= (uint32_t)((b0 & 0x7f800000u) == 0x7f800000u) | (uint32_t)((b1 & 0x7f800000u) == 0x7f800000u);
        return make_double2(w * (double)x0, w * (double)x1);
    });
    {
        const bool w0 = __ballot(any0 != 0u) != 0ull, w1 = __ballot(any1 != 0u) != 0ull, wt = __ballot(top != 0u) != 0ull;
        if(lane == 0u)
            seen[wave] = (w0 ? 1u : 0u) | (w1 ? 2u : 0u) | (wt ? 4u : 0u);
    }
    fft64_passes<WF_DELAY_THREADS>(za, a.tw, t, P, cb, fft64_block_sync{});
    uint32_t all = 0u;
#pragma unroll
    for(uint32_t w = 0; w < WF_DELAY_WAVES; ++w)
        all |= seen[w];

    // pairs: X_0 = (Z[k] + conj Z[P-k]) / 2, X_1 = (Z[k] - conj Z[P-k]) / 2j; slot k: G[k] = X_0 conj X_1
    double g = 0.0, e0 = 0.0, e1 = 0.0;
    for(uint32_t k = 1u + t; k < M; k += WF_DELAY_THREADS) {
        const uint32_t ia = fft64_at(k, cb);
        const double2 p = za[ia], q = za[fft64_at(P - k, cb)];
        const double lr = 0.5 * (p.x + q.x), li = 0.5 * (p.y - q.y);
        const double rr = 0.5 * (p.y + q.y), ri = -0.5 * (p.x - q.x);
        const double gr = lr * rr + li * ri, gi = li * rr - lr * ri;
        g = fmax(g, sqrt(gr * gr + gi * gi));
        e0 += lr * lr + li * li;
        e1 += rr * rr + ri * ri;
        za[ia] = make_double2(gr, gi);
    }
    g = wave_max(g);
    e0 = wave_sum(e0);
    e1 = wave_sum(e1);
    if(lane == 0u) {
        sum_g[wave] = g;
        sum_e0[wave] = e0;
        sum_e1[wave] = e1;
    }
    __syncthreads();
    g = sum_g[0];
    e0 = sum_e0[0];
    e1 = sum_e1[0];
#pragma unroll
    for(uint32_t w = 1; w < WF_DELAY_WAVES; ++w) {
        g = fmax(g, sum_g[w]);
        e0 += sum_e0[w];
        e1 += sum_e1[w];
    }

    // silence in either channel, a NaN or an infinity, or no cross-power at all: the zero record (uniform: `all` and g are)
    if(all != 3u || !(g > 0.0 && g < INFINITY)) {
        if(t < WF_HIP_DELAY_CURVE)
            out->curve[t] = 0.f;
        if(t == 0u) {
            out->delay_frames = 0.0;
            out->delay_ms = out->peak = out->corr = out->corr_zero = out->ambiguity = 0.f;
            out->lag = out->polarity = 0;
            out->valid = 0u;
            out->window = P;
            out->reserved = 0u;
            out->reserved2[0] = out->reserved2[1] = out->reserved2[2] = 0u;
        }
        return;
    }

    // spectrum: Y = A + j G / g on the bins, its mirror image on the other half
    const double floor_g = WF_DELAY_BETA * g;
    for(uint32_t k = 1u + t; k < M; k += WF_DELAY_THREADS) {
        const double2 G = za[fft64_at(k, cb)];
        const double d = fmax(sqrt(G.x * G.x + G.y * G.y), floor_g);
        const double ar = G.x / d, ai = G.y / d, hr = G.x / g, hi = G.y / g;
        zb[fft64_at(k, cb)] = make_double2(ar - hi, ai + hr);
        zb[fft64_at(P - k, cb)] = make_double2(ar + hi, hr - ai);
    }
    if(t == 0u)
        zb[fft64_at(0u, cb)] = zb[fft64_at(M, cb)] = make_double2(0.0, 0.0);
    __syncthreads();

    // transform: y = DFT(Y), from zb into za
    fft64_load16(za, a.tw, t, P, cb, [&](uint32_t i) { return zb[fft64_at(i, cb)]; });
    fft64_passes<WF_DELAY_THREADS>(za, a.tw, t, P, cb, fft64_block_sync{});
    const double r_norm = 2.0 * (double)(M - 1u);
    const auto y_at = [&](int32_t n) { return za[fft64_at((uint32_t)(-n) & (P - 1u), cb)]; }; // y[(-n) mod P]
    const auto R = [&](int32_t n) { return y_at(n).x / r_norm; };

    // argmax of |R[n]|, -L <= n <= L, by the index n + L: the larger value, the lower lag of equal values
    double best = -1.0;
    uint32_t kbest = 0u;
    for(uint32_t i = t; i <= 2u * L; i += WF_DELAY_THREADS) {
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
    for(uint32_t w = 1; w < WF_DELAY_WAVES; ++w)
        argmax_better(best, kbest, arg_v[w], arg_k[w]);
    const int32_t n0 = (int32_t)kbest - (int32_t)L;

    // the second peak: the largest |R| more than two lags from n0
    double second = 0.0;
    for(uint32_t i = t; i <= 2u * L; i += WF_DELAY_THREADS) {
        const uint32_t dist = i > kbest ? i - kbest : kbest - i;
        if(dist > 2u)
            second = fmax(second, fabs(R((int32_t)i - (int32_t)L)));
    }
    second = wave_max(second);
    if(lane == 0u)
        second_v[wave] = second;

    // fraction: the slope of the phase that is left with the integer lag taken out
    const double2 y0 = y_at(n0);
    const double peak = y0.x / r_norm;
    const double pol = peak > 0.0 ? 1.0 : -1.0;
    const uint32_t n0p = (uint32_t)n0 & (P - 1u);
    double num = 0.0, den = 0.0;
    for(uint32_t k = 1u + t; k < M; k += WF_DELAY_THREADS) {
        const double2 p = zb[fft64_at(k, cb)], q = zb[fft64_at(P - k, cb)];
        const double ar = 0.5 * (p.x + q.x), ai = 0.5 * (p.y - q.y);
        const double u = sqrt(ar * ar + ai * ai);
        const uint32_t m = (k * n0p) & (P - 1u); // (< 2^23: no overflow)
        const double2 c = a.tw[m & (M - 1u)];    // e^(+j 2 pi m / P) = conj tw[m], m < M; -conj tw[m - M] beyond
        const double sg = m < M ? pol : -pol;
        const double cr = sg * c.x, ci = -sg * c.y;
        const double phi = atan2(ar * ci + ai * cr, ar * cr - ai * ci);
        const double kk = (double)k;
        num += u * kk * phi;
        den += u * kk * kk;
    }
    num = wave_sum(num);
    den = wave_sum(den);
    if(lane == 0u) {
        reg_num[wave] = num;
        reg_den[wave] = den;
    }
    __syncthreads();

    if(t < WF_HIP_DELAY_CURVE)
        out->curve[t] = (float)R(n0 - (int32_t)(WF_HIP_DELAY_CURVE / 2) + (int32_t)t);
    if(t == 0u) {
        num = reg_num[0];
        den = reg_den[0];
        second = second_v[0];
#pragma unroll
        for(uint32_t w = 1; w < WF_DELAY_WAVES; ++w) {
            num += reg_num[w];
            den += reg_den[w];
            second = fmax(second, second_v[w]);
        }
        double f = den == 0.0 ? 0.0 : -((double)P / (2.0 * 3.14159265358979323846)) * num / den;
        f = fmin(fmax(f, -0.5), 0.5);
        const double c_norm = 2.0 * sqrt(e0 * e1);
        const double frames = (double)n0 + f;
        out->delay_frames = frames;
        out->delay_ms = (float)(1000.0 * frames / a.sample_rate);
        out->peak = (float)peak;
        out->corr = (float)(g * y0.y / c_norm);
        out->corr_zero = (float)(g * y_at(0).y / c_norm);
        out->ambiguity = best > 0.0 ? (float)(second / best) : 0.f;
        out->lag = n0;
        out->polarity = (int32_t)pol;
        out->valid = 1u;
        out->window = P;
        out->reserved = 0u;
        out->reserved2[0] = out->reserved2[1] = out->reserved2[2] = 0u;
    }
}

} // namespace wf
