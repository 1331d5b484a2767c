// wf_onset.hpp -- gfx950 read kernel of WF_HIP_OUT_ONSET (device code only; hipcc; included by wf_hip_measure.hip alone).
//
// Not in the reference: the onset strength of every stream's newest audio -- the positive change of a compressed band level
// from one sonogram column to the next, in total and in three frequency groups -- and the onsets picked from the four curves by
// one fixed rule (the definition is in include/wf_hip.h, "onsets").  wf_hip_read launches it on the handle's stream, behind every
// push issued so far, and copies the result back; nothing runs while the output is not read and nothing is kept between reads.
//
// One workgroup of 256 threads per stream, one wavefront per spectral column.  A column's level and flux are the functions of
// wf_onset_column.hpp, the head this kernel shares with WF_HIP_OUT_TEMPO's (wf_tempo.hpp).  The columns are the sonogram's (wf_sono.hpp): the
// same window, the same transform of P = 1024 points in 16 KB of LDS with wave-wide ordering points (wf_fft64_lds.hpp, unchanged),
// the same bins and the same band sums, so that lane b ends up holding band b.  The Ts = T + 1 spectral columns go oldest first in
// rounds of four, wave w of round r on column 4 r + w:
//   level     lane b: S[b] = log1p(100 sqrt(B[b] scale)) / ln 10, written to the round's table in LDS (four columns, and in front of
//             them the last column of the round before)
//   barrier
//   flux      lane b: d = max(S[b] - S_before[b], 0) into the wave's own transform region, which is dead by now; lanes 0, 1, 2 add
//             up the groups low, mid, high in ascending band order; lane 0 rounds the four strengths to float32 into the entry's
//             image in LDS, at the column's age
//   barrier   (the table may be written again), and wave 3 leaves its S as the column before the next round's
// Unlike the sonogram kernel this one has workgroup barriers, and every wave reaches every one of them: a wave without a column
// in the last round (Ts = 129: one active wave of four) skips the work between the barriers, not the barriers; there is no
// return in front of a barrier.  The oldest spectral column has no predecessor and yields no strength.
// After the last round thread a < 128 picks age a from the float32 strengths in LDS -- comparisons, float64 additions and one
// division, nothing that could be contracted --, the 512 floats of the entry leave as two coalesced stores per thread, the 128
// flag bytes as 32 words, and thread 0 counts the onsets and writes the header.  Ages >= T are written as zeros on every read
// (the block is reused, and a slice may be its first read).  No atomics and no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_ring_view.hpp"
#include "wf_onset_column.hpp"

namespace wf {

struct OnsetArgs {
    RingView rings;
    wf_hip_onset *out;       // [count] the entry of stream `first`
    const double *window;    // [P] periodic Hann
    const double2 *tw;       // [P / 2] e^(-j 2 pi m / P)
    const double *edges;     // [WF_HIP_ONSET_BANDS + 1] band edges in bins of P, ascending
    uint32_t first;          // first stream read
    uint32_t spectral;       // Ts, 2 <= Ts <= WF_HIP_ONSET_COLUMNS + 1: Ts H + P <= ring_cap
};

constexpr uint32_t WF_ONSET_A = WF_HIP_ONSET_COLUMNS;      // ages of an entry
constexpr uint32_t WF_ONSET_BEFORE = 6, WF_ONSET_AFTER = 3, WF_ONSET_MEAN = 16; // the picking windows
constexpr double WF_ONSET_MARGIN = 2.0;
// dynamic LDS: the four transforms, the round's table of S (five columns), the entry's 4 x 128 strengths, its 128 flag bytes
constexpr size_t WF_ONSET_LDS_BYTES = (size_t)WF_ONSET_WAVES * WF_ONSET_P * sizeof(double2) + (WF_ONSET_WAVES + 1) * 64 * sizeof(double) +
                                      4 * WF_ONSET_A * sizeof(float) + WF_ONSET_A;
static_assert(WF_ONSET_A <= WF_ONSET_THREADS && 4 * WF_ONSET_A == 2 * WF_ONSET_THREADS, "one thread per age; two floats per thread");
static_assert(sizeof(wf_hip_onset) == 2240 && offsetof(wf_hip_onset, group) == WF_ONSET_A * sizeof(float) &&
                  offsetof(wf_hip_onset, flags) == 4 * WF_ONSET_A * sizeof(float),
              "the strengths are the entry's first 512 floats, the flags behind them");

// grid: the streams of [first, first + gridDim.x); dynamic LDS: WF_ONSET_LDS_BYTES
template<int CH> __global__ __launch_bounds__(WF_ONSET_THREADS) void onset_read_kernel(const OnsetArgs a)
{
    extern __shared__ __align__(16) double2 onset_lds[];
    constexpr uint32_t P = WF_ONSET_P, H = WF_ONSET_H, A = WF_ONSET_A;
    double *const stab = reinterpret_cast<double *>(onset_lds + WF_ONSET_WAVES * P); // [5][64]: row 0 the column before the round's
    float *const str = reinterpret_cast<float *>(stab + (WF_ONSET_WAVES + 1) * 64);  // [4][A]: total, low, mid, high by age
    uint8_t *const fl = reinterpret_cast<uint8_t *>(str + 4 * A);                    // [A]

    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t stream = a.first + blockIdx.x;
    wf_hip_onset *out = a.out + blockIdx.x;
    const uint32_t Ts = a.spectral, T = Ts - 1u;
    const uint32_t wpos = a.rings.wpos[stream];

    // ages >= T stay 0 (the first barrier of round 0 lies between these stores and every strength's)
    str[t] = 0.f;
    str[t + WF_ONSET_THREADS] = 0.f;

    const uint32_t mask = a.rings.ring_cap - 1u;
    const uint32_t newest_end = wpos - (wpos & (H - 1u)); // where column `newest` ends; uint32 arithmetic that wraps with the counter
    const float *r0 = channel_ring(a.rings, stream, 0, CH);
    const float *r1 = channel_ring(a.rings, stream, CH - 1, CH);
    double2 *lds = onset_lds + wave * P;

    const OnsetBand band = onset_band(a.edges, lane);

    const uint32_t rounds = (Ts + WF_ONSET_WAVES - 1u) / WF_ONSET_WAVES;
    for(uint32_t r = 0; r < rounds; ++r) {
        const uint32_t j = r * WF_ONSET_WAVES + wave; // oldest first
        const bool active = j < Ts;                   // (uniform across the wave)
        const uint32_t age = Ts - 1u - j;             // of spectral column j; the strength against its predecessor has the same age
        double s_cur = 0.0;
        if(active) {
            const uint32_t s = newest_end - age * H - P; // the column's first frame, unmasked
            s_cur = onset_column_level<CH>(lds, r0, r1, a.window, a.tw, s, mask, lane, band);
            stab[(1u + wave) * 64u + lane] = s_cur;
        }
        __syncthreads(); // the round's table is written (and every lane of this wave is done with its transform region)

        if(active && j >= 1u) {
            double low, mid, high;
            onset_column_flux(lds, lane, s_cur, stab[wave * 64u + lane], low, mid, high);
            if(lane == 0u) { // (age < T: j >= 1)
                str[age] = (float)((low + mid) + high);
                str[A + age] = (float)low;
                str[2u * A + age] = (float)mid;
                str[3u * A + age] = (float)high;
            }
        }
        __syncthreads(); // the table has been read
        if(wave == WF_ONSET_WAVES - 1u && active)
            stab[lane] = s_cur; // the column before the next round's (read behind that round's first barrier)
    }
    // (the last round's second barrier: every strength is in LDS)

    // picking: thread a picks age a of the four curves; the column m hops older has the age a + m
    if(t < A) {
        uint32_t f = 0u;
        if(t >= WF_ONSET_AFTER && t + WF_ONSET_MEAN < T) {
            f = 0x80u;
#pragma unroll
            for(uint32_t g = 0; g < 4u; ++g) {
                const float *o = str + g * A;
                const float v = o[t];
                bool on = true;
                for(uint32_t m = 1; m <= WF_ONSET_BEFORE; ++m)
                    on = on && v > o[t + m];
                for(uint32_t m = 1; m <= WF_ONSET_AFTER; ++m)
                    on = on && v >= o[t - m];
                double sum = (double)o[t + WF_ONSET_MEAN];
                for(uint32_t i = 1; i < WF_ONSET_MEAN + WF_ONSET_AFTER + 1u; ++i) // oldest first
                    sum += (double)o[t + WF_ONSET_MEAN - i];
                on = on && (double)v >= sum / (double)(WF_ONSET_MEAN + WF_ONSET_AFTER + 1u) + WF_ONSET_MARGIN;
                f |= on ? 1u << g : 0u;
            }
        }
        fl[t] = (uint8_t)f;
    }
    __syncthreads();

    float *const dst = &out->strength[0]; // strength[A], group[3][A]: 4 A consecutive floats
    dst[t] = str[t];
    dst[t + WF_ONSET_THREADS] = str[t + WF_ONSET_THREADS];
    if(t < A / 4u)
        reinterpret_cast<uint32_t *>(out->flags)[t] = reinterpret_cast<const uint32_t *>(fl)[t];
    if(t == 0u) {
        uint32_t onsets = 0u, last = 0xFFFFFFFFu;
        for(uint32_t i = A; i-- > 0u;) // oldest first: the newest one found last
            if(fl[i] & 1u) {
                ++onsets;
                last = i;
            }
        out->columns = T;
        out->newest = wpos / H;
        out->decided_first = WF_ONSET_AFTER;
        out->decided_end = T > WF_ONSET_MEAN + WF_ONSET_AFTER ? T - WF_ONSET_MEAN : 0u;
        out->window = P;
        out->hop = H;
        out->onsets = onsets;
        out->last_age = last;
        out->last_frame = onsets ? newest_end - last * H - 3u * P / 8u : 0u;
        out->last_strength = onsets ? str[last] : 0.f;
        for(uint32_t i = 0; i < 6u; ++i)
            out->reserved[i] = 0u;
    }
}

} // namespace wf
