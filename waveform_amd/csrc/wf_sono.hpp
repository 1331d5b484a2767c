// wf_sono.hpp -- gfx950 read kernel of WF_HIP_OUT_SONO (device code only; hipcc; included by wf_hip_measure.hip alone).
//
// Not in the reference: a spectrogram of every stream's newest audio, T columns of WF_HIP_SONO_WINDOW frames a hop of
// WF_HIP_SONO_HOP apart, each reduced to 64 bands of an eighth of an octave, the columns anchored to the stream's sample counter
// (the definition is in include/wf_hip.h, "sonogram").  wf_hip_read launches it on the handle's stream, behind every push issued
// so far, and copies the result back; nothing runs while the output is not read and nothing is kept between reads.
//
// One wavefront per column: P / 16 = 64 lanes, so the 16-point load of wf_fft64_lds.hpp fills every lane, and the column's
// transform lives in 16 KB of LDS as P complex float64.  A workgroup of 256 threads takes four consecutive columns of one
// stream in 64 KB of dynamic LDS (two workgroups to a CU); the grid is (ceil(T / 4), streams).  The waves of a workgroup share
// nothing but the L1 hits on the three quarters of a window that neighbouring columns have in common: every ordering point is
// wave-wide (fft64_wave_sync), there is no workgroup barrier in the kernel, and a wave whose column is >= T skips the transform
// without holding anyone up.  (T = ring_cap / 256 - 4 is a multiple of four for every ring the library makes, a power of two of
// at least 2048 frames: in practice no wave is without a column, and the early exit is a guard.)
//   load    lane c' takes frames c' + 64 m of the column from the rings, at positions masked by the capacity, windows them
//           (both captured channels as one complex signal, as the stereo image does) and runs their 16-point transform.
//   passes  three passes of two radix-2 stages (q = 16, 64, 256).
//   bins    lane per pair (k, P - k): slot k becomes |L[k]|^2, |R[k]|^2 (one channel: |X[k]|^2, 0).
//   bands   lane b takes band b: the bins that overlap it, ascending, each with its share as the weight, one fma per bin and
//           channel (at most 45 bins at any sample rate; a wave-wide reduction per band would cost 64 x 12 exchanges of
//           float64 for sums this short).  The lane then holds cell b: the 64 lanes store a column's row of each channel as
//           256 consecutive bytes.
// Columns T .. 63, which no wave transforms, are written as -INFINITY on every read by all threads of the stream's
// workgroups in turn (the block is reused, and a slice may be its first read); so is channel 1 of a capture of one channel, by
// the lanes that write channel 0.  The header words leave from thread 0 of the stream's first workgroup.  The order of every
// sum follows from P and the edges alone; there are no atomics and no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_ring_view.hpp"
#include "wf_fft64_lds.hpp"

namespace wf {

struct SonoArgs {
    RingView rings;
    wf_hip_sono *out;        // [count] the entry of stream `first`
    const double *window;    // [P] periodic Hann
    const double2 *tw;       // [P / 2] e^(-j 2 pi m / P)
    const double *edges;     // [WF_HIP_SONO_BANDS + 1] band edges in bins of P, ascending
    uint32_t first;          // first stream read
    uint32_t columns;        // T <= WF_HIP_SONO_COLUMNS: (T - 1) H + P + H - 1 < ring_cap
    uint32_t first_covered, end_covered;
};

constexpr uint32_t WF_SONO_P = WF_HIP_SONO_WINDOW, WF_SONO_H = WF_HIP_SONO_HOP;
constexpr uint32_t WF_SONO_WAVES = 4;                      // columns per workgroup
constexpr uint32_t WF_SONO_THREADS = 64 * WF_SONO_WAVES;
constexpr uint32_t WF_SONO_CB = 6;                         // log2 P - 4
constexpr size_t WF_SONO_LDS_BYTES = (size_t)WF_SONO_WAVES * WF_SONO_P * sizeof(double2);
static_assert(WF_SONO_P == 16u << WF_SONO_CB && WF_SONO_P / 16 == 64, "one lane per 16 frames of a column");
static_assert(WF_HIP_SONO_BANDS == 64, "one lane per band");
static_assert((WF_SONO_H & (WF_SONO_H - 1)) == 0, "the hop divides 2^32");

// grid: (ceil(T / WF_SONO_WAVES), streams of [first, first + gridDim.y)); dynamic LDS: WF_SONO_LDS_BYTES
template<int CH> __global__ __launch_bounds__(WF_SONO_THREADS) void sono_read_kernel(const SonoArgs a)
{
    extern __shared__ __align__(16) double2 sono_lds[];

    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t stream = a.first + blockIdx.y;
    wf_hip_sono *out = a.out + blockIdx.y;
    const uint32_t T = a.columns;
    const uint32_t wpos = a.rings.wpos[stream];

    // columns T .. 63 of both channels: the threads of the stream's workgroups in turn
    constexpr uint32_t cells = WF_HIP_SONO_COLUMNS * WF_HIP_SONO_BANDS; // of one channel
    float *const db = &out->db[0][0][0];
    for(uint32_t i = T * WF_HIP_SONO_BANDS + blockIdx.x * WF_SONO_THREADS + t; i < cells; i += gridDim.x * WF_SONO_THREADS) {
        db[i] = -INFINITY;
        db[cells + i] = -INFINITY;
    }
    if(blockIdx.x == 0 && t == 0) {
        out->columns = T;
        out->newest = wpos / WF_SONO_H;
        out->first_covered = a.first_covered;
        out->end_covered = a.end_covered;
        out->window = WF_SONO_P;
        out->hop = WF_SONO_H;
        out->reserved[0] = 0;
        out->reserved[1] = 0;
    }

    const uint32_t age = blockIdx.x * WF_SONO_WAVES + wave;
    if(age >= T)
        return; // (no workgroup barrier follows)

    // the column's first frame, unmasked: uint32 arithmetic that wraps with the counter; the capacity and H divide 2^32
    const uint32_t mask = a.rings.ring_cap - 1u;
    const uint32_t s = wpos - (wpos & (WF_SONO_H - 1u)) - age * WF_SONO_H - WF_SONO_P;
    const float *r0 = channel_ring(a.rings, stream, 0, CH);
    const float *r1 = channel_ring(a.rings, stream, CH - 1, CH);
    double2 *lds = sono_lds + wave * WF_SONO_P;
    constexpr uint32_t P = WF_SONO_P, cb = WF_SONO_CB, M = P / 2u;

    fft64_load16(lds, a.tw, lane, P, cb, [&](uint32_t i) {
        const uint32_t pos = (s + i) & mask;
        const double w = a.window[i];
        if constexpr(CH == 2)
            return make_double2(w * (double)r0[pos], w * (double)r1[pos]);
        else
            return make_double2(w * (double)r0[pos], 0.0);
    });
    fft64_passes<64>(lds, a.tw, lane, P, cb, fft64_wave_sync{});

    // bins: L = (Z[k] + conj Z[P-k]) / 2, R = (Z[k] - conj Z[P-k]) / 2j; slot k: |L|^2, |R|^2.  Slot P - k is read by this lane alone
    for(uint32_t k = 1u + lane; k < M; k += 64u) {
        const uint32_t ia = fft64_at(k, cb);
        const double2 za = lds[ia];
        if constexpr(CH == 2) {
            const double2 zb = lds[fft64_at(P - k, cb)];
            const double lr = 0.5 * (za.x + zb.x), li = 0.5 * (za.y - zb.y);
            const double rr = 0.5 * (za.y + zb.y), ri = -0.5 * (za.x - zb.x);
            lds[ia] = make_double2(lr * lr + li * li, rr * rr + ri * ri);
        } else
            lds[ia] = make_double2(za.x * za.x + za.y * za.y, 0.0);
    }
    fft64_wave_sync{}();

    // bands: lane b sums band b
    const double lo = a.edges[lane], hi = a.edges[lane + 1u];
    // the bins that can overlap [lo, hi], generously: a bin outside it has the weight 0 and adds nothing
    const double f0 = floor(lo - 0.5), f1 = ceil(hi + 0.5) + 1.0;
    const uint32_t k0 = f0 > 1.0 ? (f0 < (double)M ? (uint32_t)f0 : M) : 1u;
    const uint32_t k1 = f1 < (double)M ? (f1 > 0.0 ? (uint32_t)f1 : 0u) : M;
    double sa = 0.0, sb = 0.0;
    for(uint32_t k = k0; k < k1; ++k) {
        const double2 p = lds[fft64_at(k, cb)];
        const double kk = (double)k;
        const double w = fmax(fmin(kk + 0.5, hi) - fmax(kk - 0.5, lo), 0.0);
        sa = fma(w, p.x, sa);
        if constexpr(CH == 2)
            sb = fma(w, p.y, sb);
    }
    if constexpr(CH == 2) {
        // a channel WF_HIP_STEREO_DEAD_RATIO under the other is what the transform's rounding leaves of a dead one: it counts as 0
        const double sa0 = sa;
        sa = sa > sb * WF_HIP_STEREO_DEAD_RATIO ? sa : 0.0;
        sb = sb > sa0 * WF_HIP_STEREO_DEAD_RATIO ? sb : 0.0;
    }
    // a sine of amplitude A reads 20 log10 A: the periodic Hann's coherent gain 1/2 and its noise bandwidth of 1.5 bins
    constexpr double scale = 32.0 / (3.0 * (double)P * (double)P);
    out->db[0][age][lane] = sa > 0.0 ? (float)(10.0 * log10(sa * scale)) : -INFINITY;
    out->db[1][age][lane] = sb > 0.0 ? (float)(10.0 * log10(sb * scale)) : -INFINITY;
}

} // namespace wf
