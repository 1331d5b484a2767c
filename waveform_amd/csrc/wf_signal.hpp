// wf_signal.hpp -- gfx950 read kernel of WF_HIP_OUT_SIGNAL (device code only; hipcc; included by wf_hip_measure.hip alone).
//
// Not in the reference: level, DC, clipping and stereo phase of the newest W = fft_size frames in each captured channel's
// ring (the definition is in include/wf_hip.h).  wf_hip_read launches it on the handle's stream, behind every push issued so
// far, and copies the result back; nothing runs while the output is not read.
//
// One workgroup of WF_SIGNAL_THREADS per stream.  The window is at most two contiguous runs of the ring (the wrap splits it):
// [s, min(s + W, cap)) and [0, s + W - cap).  Each run goes through in 16-B loads over its 16-B aligned body, four per
// channel in flight per lane, and element by element over the at most 3 frames before and after the body (a ragged push
// leaves the window at any alignment; every ring starts 16-B aligned: ring_stride is a multiple of 4 floats).  Channel 1's
// ring is read at the same offsets, so a lane holds l and r of the same frames.  Each lane sums in float64 -- S1, S2 per
// channel, Slr, sum (l + r)^2, sum (l - r)^2 (Smid and Sside times 4: scaling by a power of two commutes with rounding) --
// and keeps max |x| and the clip count per channel.  A butterfly over the wavefront, then the waves' partials in LDS added
// by one thread in wave order: the order of every addition is fixed by the window's position, never by timing, and there
// are no atomics, so the same ring contents read bit-identically.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_ring_view.hpp"
#include "wf_wave_reduce.hpp"

namespace wf {

struct SignalArgs {
    RingView rings;
    wf_hip_signal *out;      // [count] the entry of stream `first`
    uint32_t first;          // first stream read
    uint32_t W;              // window frames, <= ring_cap
};

constexpr uint32_t WF_SIGNAL_THREADS = 256;
constexpr uint32_t WF_SIGNAL_WAVES = WF_SIGNAL_THREADS / 64;
constexpr uint32_t WF_SIGNAL_UNROLL = 4; // float4 loads per channel in flight per lane
constexpr int WF_SIGNAL_OCC = 8;         // waves per SIMD

// one lane's partial sums (CH = 1: the stereo members stay unused and are dropped by the compiler)
template<int CH> struct SignalAcc {
    double s1[CH], s2[CH];
    double slr, sum2, dif2;  // sum l r, sum (l + r)^2, sum (l - r)^2
    float mx[CH];
    uint32_t clip[CH];
};

template<int CH>
__device__ __forceinline__ void signal_add(SignalAcc<CH> &a, float l, float r)
{
    const double dl = l;
    a.s1[0] += dl;
    a.s2[0] = __builtin_fma(dl, dl, a.s2[0]);
    a.mx[0] = __builtin_fmaxf(a.mx[0], __builtin_fabsf(l));
    a.clip[0] += __builtin_fabsf(l) >= WF_HIP_FULL_SCALE ? 1u : 0u;
    if constexpr(CH == 2) {
        const double dr = r;
        a.s1[1] += dr;
        a.s2[1] = __builtin_fma(dr, dr, a.s2[1]);
        a.mx[1] = __builtin_fmaxf(a.mx[1], __builtin_fabsf(r));
        a.clip[1] += __builtin_fabsf(r) >= WF_HIP_FULL_SCALE ? 1u : 0u;
        a.slr = __builtin_fma(dl, dr, a.slr);
        const double m = dl + dr, d = dl - dr; // exact
        a.sum2 = __builtin_fma(m, m, a.sum2);
        a.dif2 = __builtin_fma(d, d, a.dif2);
    }
}

template<int CH>
__device__ __forceinline__ void signal_add4(SignalAcc<CH> &a, const float4 &l, const float4 &r)
{
    signal_add<CH>(a, l.x, r.x);
    signal_add<CH>(a, l.y, r.y);
    signal_add<CH>(a, l.z, r.z);
    signal_add<CH>(a, l.w, r.w);
}

// ring positions [b0, b1) of both channels, b0 <= b1 <= ring_cap
template<int CH>
__device__ __forceinline__ void signal_run(SignalAcc<CH> &a, const float *r0, const float *r1, uint32_t b0, uint32_t b1)
{
    const uint32_t t = threadIdx.x;
    const uint32_t h = ((b0 + 3u) & ~3u) < b1 ? ((b0 + 3u) & ~3u) : b1; // end of the head
    const uint32_t e = (b1 & ~3u) > h ? (b1 & ~3u) : h;                 // end of the body
    const uint32_t nh = h - b0, nt = b1 - e;                            // at most 3 each
    if(t < nh)
        signal_add<CH>(a, r0[b0 + t], CH == 2 ? r1[b0 + t] : 0.f);
    else if(t - nh < nt)
        signal_add<CH>(a, r0[e + t - nh], CH == 2 ? r1[e + t - nh] : 0.f);
    const float4 *p0 = reinterpret_cast<const float4 *>(r0 + h);
    const float4 *p1 = reinterpret_cast<const float4 *>(r1 + h);
    const uint32_t n4 = (e - h) / 4u;
    constexpr uint32_t T = WF_SIGNAL_THREADS;
    uint32_t i = t;
    constexpr uint32_t U = WF_SIGNAL_UNROLL;
    for(; i + (U - 1u) * T < n4; i += U * T) {
        float4 l[U], r[U];
#pragma unroll
        for(uint32_t u = 0; u < U; ++u) {
            l[u] = p0[i + u * T];
            r[u] = CH == 2 ? p1[i + u * T] : l[u];
        }
#pragma unroll
        for(uint32_t u = 0; u < U; ++u)
            signal_add4<CH>(a, l[u], r[u]);
    }
    for(; i < n4; i += T)
        signal_add4<CH>(a, p0[i], CH == 2 ? p1[i] : p0[i]);
}

__device__ __forceinline__ float signal_db(double ratio, double scale)
{
    return ratio > 0.0 ? (float)(scale * log10(ratio)) : -INFINITY;
}

// grid: one workgroup per stream of [first, first + gridDim.x)
template<int CH>
__global__ __launch_bounds__(WF_SIGNAL_THREADS, WF_SIGNAL_OCC) void signal_read_kernel(const SignalArgs a)
{
    constexpr int ND = CH == 2 ? 7 : 2; // doubles reduced: s1[], s2[] (, slr, sum2, dif2)
    __shared__ double lds_d[WF_SIGNAL_WAVES][ND];
    __shared__ float lds_m[WF_SIGNAL_WAVES][CH];
    __shared__ uint32_t lds_c[WF_SIGNAL_WAVES][CH];

    const uint32_t stream = a.first + blockIdx.x;
    const uint32_t ring_cap = a.rings.ring_cap;
    const uint32_t s = window_start(a.rings, stream, a.W) & (ring_cap - 1u);
    const float *r0 = channel_ring(a.rings, stream, 0, CH);
    const float *r1 = CH == 2 ? channel_ring(a.rings, stream, 1, CH) : r0;

    SignalAcc<CH> acc;
#pragma unroll
    for(int c = 0; c < CH; ++c) {
        acc.s1[c] = 0.0;
        acc.s2[c] = 0.0;
        acc.mx[c] = 0.f;
        acc.clip[c] = 0u;
    }
    acc.slr = acc.sum2 = acc.dif2 = 0.0;
    const uint32_t end = s + a.W; // <= 2 ring_cap
    signal_run<CH>(acc, r0, r1, s, end < ring_cap ? end : ring_cap);
    if(end > ring_cap)
        signal_run<CH>(acc, r0, r1, 0u, end - ring_cap);

    double d[ND];
#pragma unroll
    for(int c = 0; c < CH; ++c) {
        d[2 * c] = acc.s1[c];
        d[2 * c + 1] = acc.s2[c];
    }
    if constexpr(CH == 2) {
        d[4] = acc.slr;
        d[5] = acc.sum2;
        d[6] = acc.dif2;
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for(int k = 0; k < ND; ++k)
        d[k] = wave_sum(d[k]);
    float mx[CH];
    uint32_t clip[CH];
#pragma unroll
    for(int c = 0; c < CH; ++c) {
        mx[c] = acc.mx[c];
        clip[c] = acc.clip[c];
        wave_butterfly([&](auto other) {
            mx[c] = __builtin_fmaxf(mx[c], other(mx[c]));
            clip[c] += other(clip[c]);
        });
    }
    if(lane == 0) {
#pragma unroll
        for(int k = 0; k < ND; ++k)
            lds_d[wave][k] = d[k];
#pragma unroll
        for(int c = 0; c < CH; ++c) {
            lds_m[wave][c] = mx[c];
            lds_c[wave][c] = clip[c];
        }
    }
    __syncthreads();
    // the totals: thread k adds quantity k over the waves in wave order
    __shared__ double tot_d[ND];
    __shared__ float tot_m[CH];
    __shared__ uint32_t tot_c[CH];
    const uint32_t t = threadIdx.x;
    if(t < (uint32_t)ND) {
        double v = lds_d[0][t];
        for(uint32_t w = 1; w < WF_SIGNAL_WAVES; ++w)
            v += lds_d[w][t];
        tot_d[t] = v;
    } else if(t - ND < (uint32_t)CH) {
        const uint32_t c = t - ND;
        float m = lds_m[0][c];
        uint32_t n = lds_c[0][c];
        for(uint32_t w = 1; w < WF_SIGNAL_WAVES; ++w) {
            m = __builtin_fmaxf(m, lds_m[w][c]);
            n += lds_c[w][c];
        }
        tot_m[c] = m;
        tot_c[c] = n;
    }
    __syncthreads();
    // thread j < 12 writes word j of the wf_hip_signal (one logarithm per thread: the epilogue stays small)
    if(t >= sizeof(wf_hip_signal) / 4u)
        return;
    const double W = (double)a.W;
    double ratio = 0.0, scale = 10.0; // a dB field: scale log10(ratio), -INFINITY where ratio is 0
    bool db = true;
    uint32_t bits = 0u;               // the other fields
    if(t < 8u) {                      // ch[t / 4]
        const uint32_t c = t >> 2, f = t & 3u;
        if(c < (uint32_t)CH) {
            if(f == 0u)
                ratio = tot_d[2 * c + 1] / W;
            else if(f == 1u) {
                ratio = (double)tot_m[c];
                scale = 20.0;
            } else {
                db = false;
                bits = f == 2u ? __float_as_uint((float)(tot_d[2 * c] / W)) : tot_c[c];
            }
        } else if(f >= 2u)
            db = false; // dc 0, clipped 0 (the dB fields: ratio 0, -INFINITY)
    } else if constexpr(CH == 2) {
        const double l2 = tot_d[1], r2 = tot_d[3];
        if(t == 8u) {
            db = false;
            const double c = l2 > 0.0 && r2 > 0.0 ? tot_d[4] / sqrt(l2 * r2) : 0.0;
            bits = __float_as_uint((float)(c < -1.0 ? -1.0 : c > 1.0 ? 1.0 : c));
        } else if(t == 9u) {
            if(l2 > 0.0 && r2 > 0.0)
                ratio = r2 / l2;
            else {
                db = false;
                bits = __float_as_uint(l2 > 0.0 ? -INFINITY : r2 > 0.0 ? INFINITY : 0.f);
            }
        } else
            ratio = 0.25 * tot_d[t == 10u ? 5 : 6] / W;
    } else
        db = t >= 10u; // one channel: correlation 0, balance 0, mid and side -INFINITY
    if(db)
        bits = __float_as_uint(signal_db(ratio, scale));
    reinterpret_cast<uint32_t *>(a.out + blockIdx.x)[t] = bits;
}

} // namespace wf
