// wf_onset_column.hpp -- the head that the kernels of WF_HIP_OUT_ONSET (wf_onset.hpp) and WF_HIP_OUT_TEMPO (wf_tempo.hpp) share
// (device code only; hipcc; it holds no kernel): one spectral column of the onset strength, by one wavefront.
//   onset_band          lane b's band of the sonogram's filterbank: its edges and the bins that can overlap it
//   onset_column_level  the column that starts at counter frame s through the periodic Hann window and the transform of P = 1024
//                       points in the wave's 16 KB of LDS (wf_fft64_lds.hpp, wave-wide ordering points), the bins, the band sums:
//                       lane b returns S[b] = log1p(100 sqrt(B[b] scale)) / ln 10
//   onset_column_flux   lane b: d = max(S[b] - S_before[b], 0) into the wave's transform region, which is dead by then; lanes 0, 1, 2
//                       add up the groups low, mid, high in ascending band order; every lane returns the three sums
// Both kernels call these with the same arguments for the same column, so that a column's strength is the same bits in both
// outputs.  Neither function holds a workgroup barrier.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_fft64_lds.hpp"

namespace wf {

constexpr uint32_t WF_ONSET_P = WF_HIP_ONSET_WINDOW, WF_ONSET_H = WF_HIP_ONSET_HOP;
constexpr uint32_t WF_ONSET_WAVES = 4;                     // spectral columns per round
constexpr uint32_t WF_ONSET_THREADS = 64 * WF_ONSET_WAVES;
constexpr uint32_t WF_ONSET_CB = 6;                        // log2 P - 4
constexpr double WF_ONSET_KNEE = 100.0;
constexpr uint32_t WF_ONSET_LOW_END = 16, WF_ONSET_MID_END = 40; // the groups: bands [0, 16), [16, 40), [40, 64)
static_assert(WF_ONSET_P == WF_HIP_SONO_WINDOW && WF_ONSET_H == WF_HIP_SONO_HOP && WF_HIP_ONSET_BANDS == WF_HIP_SONO_BANDS,
              "the sonogram's columns and tables");
static_assert(WF_ONSET_P == 16u << WF_ONSET_CB && WF_ONSET_P / 16 == 64, "one lane per 16 frames of a column");
static_assert(WF_HIP_ONSET_BANDS == 64, "one lane per band");
static_assert((WF_ONSET_H & (WF_ONSET_H - 1)) == 0, "the hop divides 2^32");

struct OnsetBand {
    double lo, hi;   // the band's edges in bins of P
    uint32_t k0, k1; // the bins [k0, k1) that can overlap [lo, hi], generously (a bin outside it has the weight 0 and adds nothing)
};

// edges: [WF_HIP_ONSET_BANDS + 1] band edges in bins of P, ascending
__device__ inline OnsetBand onset_band(const double *edges, uint32_t lane)
{
    constexpr uint32_t M = WF_ONSET_P / 2u;
    OnsetBand b;
    b.lo = edges[lane];
    b.hi = edges[lane + 1u];
    const double f0 = floor(b.lo - 0.5), f1 = ceil(b.hi + 0.5) + 1.0;
    b.k0 = f0 > 1.0 ? (f0 < (double)M ? (uint32_t)f0 : M) : 1u;
    b.k1 = f1 < (double)M ? (f1 > 0.0 ? (uint32_t)f1 : 0u) : M;
    return b;
}

// lds: the wave's [P] double2; r0, r1: the rings of the stream's first and last captured channel; s: the column's first frame,
// unmasked; mask: ring_cap - 1
template<int CH>
__device__ inline double onset_column_level(double2 *lds, const float *r0, const float *r1, const double *window, const double2 *tw, uint32_t s,
                                            uint32_t mask, uint32_t lane, const OnsetBand &band)
{
    constexpr uint32_t P = WF_ONSET_P, cb = WF_ONSET_CB, M = P / 2u;
    // the sonogram's factor (a sine of amplitude A reads A^2) over the captured channels
    constexpr double scale = 32.0 / (3.0 * (double)P * (double)P * (double)CH);
    constexpr double ln10 = 2.302585092994045684;
    const double lo = band.lo, hi = band.hi;
    fft64_load16(lds, tw, lane, P, cb, [&](uint32_t i) {
        const uint32_t pos = (s + i) & mask;
        const double w = window[i];
        if constexpr(CH == 2)
            return make_double2(w * (double)r0[pos], w * (double)r1[pos]);
        else
            return make_double2(w * (double)r0[pos], 0.0);
    });
    fft64_passes<64>(lds, tw, lane, P, cb, fft64_wave_sync{});

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

    // bands: lane b sums band b of each channel, ascending
    double sa = 0.0, sb = 0.0;
    for(uint32_t k = band.k0; k < band.k1; ++k) {
        const double2 p = lds[fft64_at(k, cb)];
        const double kk = (double)k;
        const double w = fmax(fmin(kk + 0.5, hi) - fmax(kk - 0.5, lo), 0.0);
        sa = fma(w, p.x, sa);
        if constexpr(CH == 2)
            sb = fma(w, p.y, sb);
    }
    return log1p(WF_ONSET_KNEE * sqrt((sa + sb) * scale)) / ln10;
}

// lds: the wave's transform region (dead: the workgroup barrier behind onset_column_level has been passed)
__device__ inline void onset_column_flux(double2 *lds, uint32_t lane, double s_cur, double s_before, double &low, double &mid, double &high)
{
    const double d = fmax(s_cur - s_before, 0.0);
    double *const dl = reinterpret_cast<double *>(lds);
    dl[lane] = d;
    fft64_wave_sync{}();
    double sum = 0.0;
    if(lane < 3u) {
        const uint32_t b0 = lane == 0u ? 0u : (lane == 1u ? WF_ONSET_LOW_END : WF_ONSET_MID_END);
        const uint32_t b1 = lane == 0u ? WF_ONSET_LOW_END : (lane == 1u ? WF_ONSET_MID_END : (uint32_t)WF_HIP_ONSET_BANDS);
        for(uint32_t b = b0; b < b1; ++b)
            sum += dl[b];
    }
    low = __shfl(sum, 0);
    mid = __shfl(sum, 1);
    high = __shfl(sum, 2);
}

} // namespace wf
