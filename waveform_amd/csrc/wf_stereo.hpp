// wf_stereo.hpp -- gfx950 read kernel of WF_HIP_OUT_STEREO (device code only; hipcc; included by wf_hip_measure.hip alone).
//
// Not in the reference: correlation, coherence, phase and balance between captured channels 0 and 1 in each of the 31
// third-octave bands, from one complex float64 transform of the newest P frames of both rings (the definition is in
// include/wf_hip.h, "stereo image").  wf_hip_read launches it on the handle's stream, behind every push issued so far, and
// copies the result back; nothing runs while the output is not read.
//
// One workgroup of WF_STEREO_THREADS per stream; the transform lives in LDS as P complex float64 (16 B each: 64 KB at P = 4096,
// the whole of what a workgroup gets without asking, so nothing else is kept in LDS).  Decimation in time, natural order out:
//   load    thread c' takes the 16 frames c' + m P/16, m = 0 .. 15, of both rings (consecutive lanes on consecutive frames),
//           windows them and runs their 16-point transform in registers: the first four radix-2 stages, which in LDS would
//           be the ones with strides of 1 to 8 elements.  The result is block c = bitrev(c') of 16 consecutive elements.
//   passes  radix-2 stages two at a time (one read and one write of LDS per two stages), butterflies j, j + q, j + 2q, j + 3q
//           with q = 16, 64, 256, 1024; a last single stage when log2 P is odd.  Twiddles from the host's table [P / 2].
//   bins    thread per pair (k, P - k): Z[k] and Z[P - k] become |L|^2, |R|^2 in slot k and L conj(R) in slot P - k.
//   bands   wavefront w takes bands w, w + 4, ...; its lanes stride over the band's bins, each with four float64 sums, reduced
//           by the fixed butterfly of wf_wave_reduce.hpp; the four fields leave from lane 0.
// The order of every sum follows from P and the edges alone; there are no atomics and no scratch.
//
// LDS addressing.  Element i lives in 16-byte slot i ^ (bitrev(i >> 4) & 15): inside its aligned row of 16 slots (256 B, all 64
// banks) it is moved by the low bits of the number c' of the thread that produced the row.  Every later access has lanes on
// consecutive i with q >= 16, so 16 lanes cover one row whatever its permutation: ds_read_b128 / ds_write_b128 without
// conflicts.  The load phase's stores, where lane c' writes row bitrev(c') -- rows 1 KB apart at P = 4096, which unpermuted is
// one bank group for every lane -- fall on slot u ^ (c' & 15): eight consecutive lanes, eight different slots.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_ring_view.hpp"
#include "wf_wave_reduce.hpp"

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

__device__ __forceinline__ double2 stereo_mul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 stereo_add(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 stereo_sub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }

// two radix-2 stages of a decimation-in-time transform on x[j], x[j + q], x[j + 2q], x[j + 3q]: w1 = W_2q^j, w2 = W_4q^j
// (W_4q^(j + q) is w2 times -j)
__device__ __forceinline__ void stereo_bfly4(double2 &x0, double2 &x1, double2 &x2, double2 &x3, double2 w1, double2 w2)
{
    const double2 t1 = stereo_mul(w1, x1), t3 = stereo_mul(w1, x3);
    const double2 a0 = stereo_add(x0, t1), a1 = stereo_sub(x0, t1), a2 = stereo_add(x2, t3), a3 = stereo_sub(x2, t3);
    const double2 t2 = stereo_mul(w2, a2), v = stereo_mul(w2, a3);
    const double2 t4 = make_double2(v.y, -v.x);
    x0 = stereo_add(a0, t2);
    x2 = stereo_sub(a0, t2);
    x1 = stereo_add(a1, t4);
    x3 = stereo_sub(a1, t4);
}

// the slot of element i (cb = log2 P - 4 bits of row number)
__device__ __forceinline__ uint32_t stereo_at(uint32_t i, uint32_t cb) { return i ^ ((__brev(i >> 4) >> (32u - cb)) & 15u); }

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

    // load: the 16-point transform of frames c' + m P/16 in registers
    const uint32_t n16 = P >> 4;
    if(t < n16) {
        double2 x[16];
#pragma unroll
        for(uint32_t u = 0; u < 16; ++u) { // x[u]: frame number bitrev4(u) of the sixteen
            const uint32_t m = ((u & 1u) << 3) | ((u & 2u) << 1) | ((u & 4u) >> 1) | ((u & 8u) >> 3);
            const uint32_t i = t + m * n16;
            const uint32_t pos = (s + i) & mask;
            const double w = a.window[i];
            x[u] = make_double2(w * (double)r0[pos], w * (double)r1[pos]);
        }
        const double2 one = make_double2(1.0, 0.0);
#pragma unroll
        for(uint32_t g = 0; g < 4; ++g)
            stereo_bfly4(x[4 * g], x[4 * g + 1], x[4 * g + 2], x[4 * g + 3], one, one);
#pragma unroll
        for(uint32_t j = 0; j < 4; ++j)
            stereo_bfly4(x[j], x[j + 4], x[j + 8], x[j + 12], a.tw[2u * j * n16], a.tw[j * n16]);
        const uint32_t row = (__brev(t) >> (32u - cb)) << 4, swz = t & 15u;
#pragma unroll
        for(uint32_t u = 0; u < 16; ++u)
            lds[row + (u ^ swz)] = x[u];
    }

    // passes: stages of half-length q and 2q together
    uint32_t q = 16;
    for(; 4u * q <= P; q *= 4u) {
        __syncthreads();
        const uint32_t step = P / (4u * q);
        for(uint32_t u = t; u < P / 4u; u += WF_STEREO_THREADS) {
            const uint32_t j = u & (q - 1u), base = ((u - j) << 2) + j;
            const uint32_t i0 = stereo_at(base, cb), i1 = stereo_at(base + q, cb), i2 = stereo_at(base + 2u * q, cb),
                           i3 = stereo_at(base + 3u * q, cb);
            const double2 w2 = a.tw[j * step], w1 = a.tw[2u * j * step];
            double2 x0 = lds[i0], x1 = lds[i1], x2 = lds[i2], x3 = lds[i3];
            stereo_bfly4(x0, x1, x2, x3, w1, w2);
            lds[i0] = x0;
            lds[i1] = x1;
            lds[i2] = x2;
            lds[i3] = x3;
        }
    }
    if(2u * q == P) { // log2 P odd: the last stage alone
        __syncthreads();
        for(uint32_t j = t; j < q; j += WF_STEREO_THREADS) {
            const uint32_t i0 = stereo_at(j, cb), i1 = stereo_at(j + q, cb);
            const double2 x0 = lds[i0], v = stereo_mul(a.tw[j], lds[i1]);
            lds[i0] = stereo_add(x0, v);
            lds[i1] = stereo_sub(x0, v);
        }
    }
    __syncthreads();

    // bins: L = (Z[k] + conj Z[P-k]) / 2, R = (Z[k] - conj Z[P-k]) / 2j; slot k: |L|^2, |R|^2; slot P - k: L conj(R)
    const uint32_t M = P / 2u;
    for(uint32_t k = 1u + t; k < M; k += WF_STEREO_THREADS) {
        const uint32_t ia = stereo_at(k, cb), ib = stereo_at(P - k, cb);
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
            const double2 p = lds[stereo_at(k, cb)], c = lds[stereo_at(P - k, cb)];
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
