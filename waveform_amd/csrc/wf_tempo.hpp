// wf_tempo.hpp -- gfx950 read kernels of WF_HIP_OUT_TEMPO (device code only; hipcc; included by wf_hip_measure.hip alone).
//
// Not in the reference: the tempo and the beat phase of every stream, from the onset strength of WF_HIP_OUT_ONSET over up to 2048
// columns (the definition is in include/wf_hip.h, "tempo").  wf_hip_read launches both kernels on the handle's stream, A then B,
// behind every push issued so far; nothing runs while the output is not read and nothing is kept between reads.
//
// A, tempo_columns_kernel<CH>: the strength columns, spread over the grid.  The onset kernel walks its 129 spectral columns inside
// one workgroup per stream; at 2049 that would be 513 serial rounds and a batch of 64 streams would leave most of the chip idle.
// Here a workgroup of 256 threads takes a chunk of up to 64 strength columns of one stream, oldest first in rounds of four, one
// wavefront per spectral column, through the functions of wf_onset_column.hpp -- the onset kernel's, so that a column is the same
// bits in both outputs.  A chunk of c strengths computes c + 1 spectral columns; its oldest serves only as the predecessor of the
// next (the chunk before computes it once more as its newest).  T = 507 leaves a last chunk of 59, whose last round is not full:
// as in wf_onset.hpp every wave reaches every barrier, a wave without a column skips the work between the barriers, and there is
// no return in front of one.  Lane 0 of a wave stores the float32 total strength of its column at its age in a scratch block of
// WF_HIP_TEMPO_COLUMNS floats per stream.  Dynamic LDS: the four transforms and the round's table of S, 66.5 KB.
//
// B, tempo_read_kernel: the rule, one workgroup of WF_HIP_TEMPO_LAGS = 576 threads per stream, every sum in the order of the
// definition.  The float64 arithmetic of this kernel is not contracted (no fused multiply-add): the restatement forms every
// product and every sum on its own, and comparisons decide lag, lag2 and beat_age.
//   copy       the strengths from the scratch block to the entry (zeros from age T on) and, as float64 and oldest first, to LDS
//   mean       thread 0 alone adds o[0 .. T-1] oldest first, and finds the largest strength and whether all are finite
//   centre     e[n] = o[n] - mean
//   acf        thread L < 2 lag_hi + 2: r[L], a serial ascending sum; e[n] is a broadcast and e[n - L] consecutive words
//   salience   thread L in [lag_lo, lag_hi]: c[L]
//   picks      thread 0 alone: the argmax, the parabola, the second candidate, each a serial ascending scan
//   phase      thread k < ceil(period): phi[k], a serial sum in ascending j; thread 0 alone picks beat_age and writes the header
// An entry that is not valid leaves as the definition says: the strengths and the seven words that need no curve, zeros elsewhere.
// Static LDS, 26 KB.  No atomics and no scratch memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_ring_view.hpp"
#include "wf_onset_column.hpp"

namespace wf {

struct TempoColumnsArgs {
    RingView rings;
    float *strength;         // [n_streams][WF_HIP_TEMPO_COLUMNS] the scratch block, by age
    const double *window;    // [P] periodic Hann
    const double2 *tw;       // [P / 2] e^(-j 2 pi m / P)
    const double *edges;     // [WF_HIP_ONSET_BANDS + 1] band edges in bins of P, ascending
    uint32_t first;          // first stream read
    uint32_t columns;        // T, 1 <= T <= WF_HIP_TEMPO_COLUMNS: (T + 1) H + P <= ring_cap
};

struct TempoArgs {
    RingView rings;
    const float *strength;   // the scratch block
    wf_hip_tempo *out;       // [count] the entry of stream `first`
    const double *prior;     // [WF_HIP_TEMPO_MAX_LAG + 1] w[L]
    double beats;            // 60 sr / H: bpm(L) = beats / L
    uint32_t first;
    uint32_t columns;        // T
    uint32_t lag_lo, lag_hi; // lag_lo + 2 <= lag_hi <= min(T / 4, WF_HIP_TEMPO_MAX_LAG)
};

constexpr uint32_t WF_TEMPO_CHUNK = 64;                    // strength columns of a workgroup of kernel A
constexpr uint32_t WF_TEMPO_T = WF_HIP_TEMPO_COLUMNS;
constexpr uint32_t WF_TEMPO_THREADS = WF_HIP_TEMPO_LAGS;   // of kernel B: one thread per lag
constexpr uint32_t WF_TEMPO_PHASES = WF_HIP_TEMPO_MAX_LAG + 1; // ceil(period) <= lag_hi + 1
// dynamic LDS of kernel A: the four transforms, the round's table of S (five columns)
constexpr size_t WF_TEMPO_LDS_BYTES = (size_t)WF_ONSET_WAVES * WF_ONSET_P * sizeof(double2) + (WF_ONSET_WAVES + 1) * 64 * sizeof(double);
static_assert(WF_HIP_TEMPO_WINDOW == WF_HIP_ONSET_WINDOW && WF_HIP_TEMPO_HOP == WF_HIP_ONSET_HOP, "the onset detector's columns");
static_assert(WF_TEMPO_THREADS % 64 == 0 && WF_TEMPO_THREADS <= 1024 && 2 * WF_HIP_TEMPO_MAX_LAG + 2 <= WF_TEMPO_THREADS, "one thread per lag");
static_assert(WF_HIP_TEMPO_MAX_LAG <= WF_TEMPO_T / 4, "2 lag_hi + 1 < T at the cap");
static_assert(sizeof(wf_hip_tempo) == 10592 && offsetof(wf_hip_tempo, acf) == WF_TEMPO_T * sizeof(float) &&
                  offsetof(wf_hip_tempo, bpm) == (WF_TEMPO_T + WF_HIP_TEMPO_LAGS) * sizeof(float),
              "the strengths are the entry's first 2048 floats, the autocorrelation behind them");

// grid: (chunks of WF_TEMPO_CHUNK strength columns, the streams of [first, first + gridDim.y)); dynamic LDS: WF_TEMPO_LDS_BYTES
template<int CH> __global__ __launch_bounds__(WF_ONSET_THREADS) void tempo_columns_kernel(const TempoColumnsArgs a)
{
    extern __shared__ __align__(16) double2 tempo_lds[];
    constexpr uint32_t P = WF_ONSET_P, H = WF_ONSET_H;
    double *const stab = reinterpret_cast<double *>(tempo_lds + WF_ONSET_WAVES * P); // [5][64]: row 0 the column before the round's

    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t stream = a.first + blockIdx.y;
    const uint32_t T = a.columns;
    // strength n (oldest first) is spectral column n + 1 against column n; this chunk: strengths [n0, n0 + c)
    const uint32_t n0 = blockIdx.x * WF_TEMPO_CHUNK; // (< T: the grid has ceil(T / 64) chunks)
    const uint32_t c = T - n0 < WF_TEMPO_CHUNK ? T - n0 : WF_TEMPO_CHUNK;
    const uint32_t wpos = a.rings.wpos[stream];
    const uint32_t mask = a.rings.ring_cap - 1u;
    const uint32_t newest_end = wpos - (wpos & (H - 1u)); // where column `newest` ends; uint32 arithmetic that wraps with the counter
    const float *r0 = channel_ring(a.rings, stream, 0, CH);
    const float *r1 = channel_ring(a.rings, stream, CH - 1, CH);
    double2 *lds = tempo_lds + wave * P;
    float *const dst = a.strength + (size_t)stream * WF_TEMPO_T;
    const OnsetBand band = onset_band(a.edges, lane);

    const uint32_t rounds = (c + 1u + WF_ONSET_WAVES - 1u) / WF_ONSET_WAVES;
    for(uint32_t r = 0; r < rounds; ++r) {
        const uint32_t i = r * WF_ONSET_WAVES + wave; // the chunk's spectral column, oldest first: column n0 + i of the T + 1
        const bool active = i <= c;                   // (uniform across the wave)
        const uint32_t age = T - (n0 + i);            // of spectral column n0 + i (the newest has age 0); as a strength: n0 + i - 1
        double s_cur = 0.0;
        if(active) {
            const uint32_t s = newest_end - age * H - P; // the column's first frame, unmasked
            s_cur = onset_column_level<CH>(lds, r0, r1, a.window, a.tw, s, mask, lane, band);
            stab[(1u + wave) * 64u + lane] = s_cur;
        }
        __syncthreads(); // the round's table is written (and every lane of this wave is done with its transform region)

        if(active && i >= 1u) {
            double low, mid, high;
            onset_column_flux(lds, lane, s_cur, stab[wave * 64u + lane], low, mid, high);
            if(lane == 0u)
                dst[age] = (float)((low + mid) + high); // (age < T: i >= 1)
        }
        __syncthreads(); // the table has been read
        if(wave == WF_ONSET_WAVES - 1u && active)
            stab[lane] = s_cur; // the column before the next round's (read behind that round's first barrier)
    }
}

// grid: the streams of [first, first + gridDim.x)
__global__ __launch_bounds__(WF_TEMPO_THREADS) void tempo_read_kernel(const TempoArgs a)
{
#pragma clang fp contract(off)
    constexpr uint32_t P = WF_ONSET_P, H = WF_ONSET_H;
    __shared__ double e[WF_TEMPO_T];            // oldest first: the strengths, then less their mean
    __shared__ double rr[WF_HIP_TEMPO_LAGS];    // r[L], then acf[L]
    __shared__ double cc[WF_TEMPO_PHASES + 1];  // c[L]
    __shared__ double phi[WF_TEMPO_PHASES];
    __shared__ double s_mean, s_period;
    __shared__ uint32_t s_valid, s_phases;

    const uint32_t t = threadIdx.x;
    const uint32_t stream = a.first + blockIdx.x;
    wf_hip_tempo *out = a.out + blockIdx.x;
    const uint32_t T = a.columns, lo = a.lag_lo, hi = a.lag_hi;
    const uint32_t n_lags = 2u * hi + 2u; // (<= WF_HIP_TEMPO_LAGS, and 2 hi + 1 <= T / 2 + 1 < T)
    const float *src = a.strength + (size_t)stream * WF_TEMPO_T;
    const uint32_t wpos = a.rings.wpos[stream];
    const uint32_t newest_end = wpos - (wpos & (H - 1u));

    // copy: ages >= T are written as zeros on every read (the block is reused, and a slice may be its first read)
    for(uint32_t age = t; age < WF_TEMPO_T; age += WF_TEMPO_THREADS) {
        const float v = age < T ? src[age] : 0.f;
        out->strength[age] = v;
        if(age < T)
            e[T - 1u - age] = (double)v;
    }
    __syncthreads();

    if(t == 0u) { // mean: one thread, oldest first
        double sum = 0.0;
        float largest = (float)e[0];
        bool finite = true;
        for(uint32_t n = 0; n < T; ++n) {
            const double v = e[n];
            sum += v;
            finite = finite && fabs(v) <= 3.4028234663852886e38; // (false for a NaN)
            largest = (float)v > largest ? (float)v : largest;
        }
        s_mean = sum / (double)T;
        s_valid = finite && largest >= (float)WF_HIP_TEMPO_MARGIN ? 1u : 0u;
        out->strength_max = largest; // (put right below if the entry is not valid)
    }
    __syncthreads();
    const double mean = s_mean;
    for(uint32_t n = t; n < T; n += WF_TEMPO_THREADS)
        e[n] = e[n] - mean;
    __syncthreads();

    // acf: a thread per lag
    if(t < n_lags) {
        double r = 0.0;
        for(uint32_t n = t; n < T; ++n)
            r += e[n] * e[n - t];
        rr[t] = r / (double)(T - t);
    }
    __syncthreads();
    const double r0 = rr[0];
    const bool valid = s_valid != 0u && r0 > 0.0; // (uniform across the workgroup)
    __syncthreads();                              // (rr[0] has been read by everyone)
    const double acf = valid && t < n_lags ? rr[t] / r0 : 0.0;
    rr[t] = acf;
    out->acf[t] = (float)acf;
    __syncthreads();

    // salience
    if(t <= hi + 1u)
        cc[t] = valid && t >= lo && t <= hi ? (rr[t] + 0.5 * rr[2u * t]) * a.prior[t] : 0.0;
    __syncthreads();

    if(t == 0u) { // picks: one thread, ascending lags
        uint32_t lag = lo;
        double period = 0.0;
        if(valid) {
            for(uint32_t L = lo + 1u; L <= hi; ++L)
                lag = cc[L] > cc[lag] ? L : lag;
            double p = 0.0;
            if(lag > lo && lag < hi) {
                const double x = cc[lag - 1u], y = cc[lag], z = cc[lag + 1u];
                const double den = x - 2.0 * y + z;
                p = den < 0.0 ? 0.5 * (x - z) / den : 0.0;
            }
            const double at = (double)lag + p;
            period = rint(at * 16.0) / 16.0;
            uint32_t lag2 = 0u;
            const uint32_t clear = lag / 16u > 2u ? lag / 16u : 2u;
            for(uint32_t L = lo + 1u; L < hi; ++L) {
                const uint32_t dist = L > lag ? L - lag : lag - L;
                if(cc[L] > cc[L - 1u] && cc[L] >= cc[L + 1u] && dist > clear && (lag2 == 0u || cc[L] > cc[lag2]))
                    lag2 = L;
            }
            out->bpm = (float)(a.beats / at);
            out->period = (float)period;
            out->confidence = (float)rr[lag];
            out->salience = (float)cc[lag];
            out->bpm2 = lag2 ? (float)(a.beats / (double)lag2) : 0.f;
            out->salience2 = lag2 ? (float)cc[lag2] : 0.f;
            out->ambiguity = lag2 && cc[lag] > 0.0 ? (float)(cc[lag2] / cc[lag]) : 0.f;
            out->strength_mean = (float)mean;
            out->lag = lag;
            out->lag2 = lag2;
            out->period_frames = (uint32_t)(period * (double)H);
        } else {
            out->bpm = out->period = out->confidence = out->salience = out->bpm2 = out->salience2 = out->ambiguity = 0.f;
            out->strength_max = out->strength_mean = 0.f;
            out->lag = out->lag2 = out->period_frames = 0u;
        }
        s_period = period;
        s_phases = valid ? (uint32_t)ceil(period) : 0u; // (<= lag_hi + 1)
        out->valid = valid ? 1u : 0u;
        out->columns = T;
        out->newest = wpos / H;
        out->lag_lo = lo;
        out->lag_hi = hi;
        out->window = P;
        out->hop = H;
        out->reserved[0] = out->reserved[1] = 0u;
    }
    __syncthreads();

    // phase: a thread per age of the newest beat
    const uint32_t phases = s_phases;
    if(t < phases) {
        const double period = s_period;
        double sum = 0.0;
        for(uint32_t j = 0;; ++j) {
            const uint32_t back = t + (uint32_t)rint((double)j * period); // (period >= lag_lo >= 1: the walk ends)
            if(back > T - 1u)
                break;
            sum += e[T - 1u - back];
        }
        phi[t] = sum;
    }
    __syncthreads();
    if(t == 0u) {
        uint32_t beat = 0u;
        for(uint32_t k = 1; k < phases; ++k)
            beat = phi[k] > phi[beat] ? k : beat;
        const uint32_t last = newest_end - beat * H - 3u * P / 8u;
        out->beat_age = valid ? beat : 0u;
        out->last_beat_frame = valid ? last : 0u;
        out->next_beat_frame = valid ? last + (uint32_t)(s_period * (double)H) : 0u;
    }
}

} // namespace wf
