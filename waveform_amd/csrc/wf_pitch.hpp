// wf_pitch.hpp -- gfx950 read kernel of WF_HIP_OUT_PITCH (device code only; hipcc; included by wf_hip_measure.hip alone).
//
// Not in the reference: the fundamental frequency of the newest P = min(fft_size, 4096) frames in each stream's rings by YIN
// (de Cheveigne and Kawahara 2002, steps 1 to 5; the definition is in include/wf_hip.h, "pitch").  wf_hip_read launches it on
// the handle's stream, behind every push issued so far, and copies the result back; nothing runs while the output is not read.
//
// One workgroup of WF_PITCH_THREADS per stream, in three phases:
//   stage   the window leaves the ring (positions (wpos - P + i) mod capacity, 4-byte loads, consecutive lanes on consecutive
//           frames: 32 KB per stream against the H^2 multiply-adds below, so nothing wider is needed) and goes into LDS as the
//           mixed float64 signal x[i].  Element i lives at double i + i / 8: lanes that read a stride of 8 doubles then fall on
//           a stride of 9, which is conflict-free for ds_read_b64 (odd, so the 32 lanes of a half-wave cover all 32 bank pairs).
//   lags    the hot loop, compute-bound: thread t owns the WF_PITCH_LAGS = 8 consecutive lags 1 + 8 t .. 8 + 8 t and walks j from
//           0 to H - 1 with the window x[j + tau] of its lags in registers.  Each j costs one broadcast read of x[j], one read of
//           the sample that enters the window and 17 float64 FMAs: r(tau) += x[j] x[j + tau] and e(tau) += x[j + tau]^2 for the 8
//           lags, and e(0) += x[j]^2, which every thread keeps for itself.  So r(tau) and e(tau) are direct sums, in the order
//           of j, by one thread: the order is the same for every lag and every launch, which is what makes d(tau) exactly 0 where
//           x[j + tau] == x[j] for every j (a constant, a whole-sample period) -- a prefix sum of squares would not.
//   search  d(tau) stays in the registers of the thread that owns the lag.  Its running sum is a scan in a fixed order: 8 serial
//           additions per thread, a shuffle scan over the wavefront, the waves' totals added in wave order.  d'(tau) goes to LDS
//           (over the signal, behind a barrier) for the neighbours the search and the parabola need.  "The first lag under the
//           threshold", "the end of the descent from it" and "the smallest d', lower lag on ties" are min-reductions over
//           (value, lag) keys; thread 0 interpolates and writes the 16 bytes.
// No atomics, no scratch; the same ring contents read bit-identically.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_ring_view.hpp"
#include "wf_wave_reduce.hpp"

namespace wf {

struct PitchArgs {
    RingView rings;
    wf_hip_pitch *out;       // [count] the entry of stream `first`
    double sample_rate;
    uint32_t first;          // first stream read
    uint32_t P;              // window frames: a multiple of 16, 64 <= P <= min(ring_cap, WF_HIP_PITCH_MAX_WINDOW)
};

constexpr uint32_t WF_PITCH_THREADS = 256;
constexpr uint32_t WF_PITCH_WAVES = WF_PITCH_THREADS / 64;
constexpr uint32_t WF_PITCH_LAGS = 8; // consecutive lags per thread: THREADS x LAGS = the 2048 lags of the largest window
constexpr int WF_PITCH_OCC = 4;       // waves per SIMD: four workgroups of 37 KB in a CU's 160 KB of LDS
// the signal's LDS image: P frames and the zeros the last block of j reads ahead of the window, padded by one double in 8
constexpr uint32_t WF_PITCH_X = WF_HIP_PITCH_MAX_WINDOW + 3 * WF_PITCH_LAGS;
constexpr uint32_t WF_PITCH_LDS = WF_PITCH_X + WF_PITCH_X / 8 + 1;
static_assert(WF_PITCH_THREADS * WF_PITCH_LAGS == WF_HIP_PITCH_MAX_WINDOW / 2, "one thread per 8 lags of the largest window");
static_assert(WF_HIP_PITCH_MIN_LAG >= 1 && WF_HIP_PITCH_MIN_LAG <= WF_PITCH_LAGS, "the search starts inside thread 0's lags");

__device__ __forceinline__ uint32_t pitch_at(uint32_t i) { return i + (i >> 3); }

// a (value, lag) key orders by value, then by lag: the smallest key is the smallest value at its lowest lag
struct PitchKey {
    double v;
    uint32_t lag;
};

__device__ __forceinline__ PitchKey pitch_min(PitchKey a, PitchKey b)
{
    return (b.v < a.v || (b.v == a.v && b.lag < a.lag)) ? b : a;
}

__device__ __forceinline__ PitchKey pitch_wave_min(PitchKey k)
{
    return wave_reduce(k, [](PitchKey a, PitchKey b) { return pitch_min(a, b); });
}

// the 8 steps j = j0 .. j0 + 7 of one thread's lags tau0 .. tau0 + 7
__device__ __forceinline__ void pitch_block(const double *lds, uint32_t j0, uint32_t tau0, double (&win)[2 * WF_PITCH_LAGS],
                                            double (&r)[WF_PITCH_LAGS], double (&e)[WF_PITCH_LAGS], double &e0)
{
    constexpr uint32_t L = WF_PITCH_LAGS;
    double xj[L];
#pragma unroll
    for(uint32_t u = 0; u < L; ++u) {
        xj[u] = lds[pitch_at(j0 + u)];                         // the same address in every lane: a broadcast
        win[L + u] = lds[pitch_at(j0 + tau0 + L + u)];         // <= H - 1 + H + 2 L - 1 < WF_PITCH_X
    }
#pragma unroll
    for(uint32_t u = 0; u < L; ++u) { // j = j0 + u
        e0 = __builtin_fma(xj[u], xj[u], e0);
#pragma unroll
        for(uint32_t k = 0; k < L; ++k) {
            r[k] = __builtin_fma(xj[u], win[u + k], r[k]);
            e[k] = __builtin_fma(win[u + k], win[u + k], e[k]);
        }
    }
#pragma unroll
    for(uint32_t k = 0; k < L; ++k)
        win[k] = win[L + k];
}

// grid: one workgroup per stream of [first, first + gridDim.x)
template<int CH>
__global__ __launch_bounds__(WF_PITCH_THREADS, WF_PITCH_OCC) void pitch_read_kernel(const PitchArgs a)
{
    __shared__ double lds[WF_PITCH_LDS];           // the signal, then d'(0 .. H)
    __shared__ double lds_tot[WF_PITCH_WAVES];     // the waves' sums of d
    __shared__ PitchKey lds_key[WF_PITCH_WAVES];   // the waves' smallest d'
    __shared__ uint32_t lds_idx[2][WF_PITCH_WAVES]; // the waves' first lag under the threshold / end of the descent

    constexpr uint32_t L = WF_PITCH_LAGS;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t stream = a.first + blockIdx.x;
    const uint32_t P = a.P, H = P / 2u;
    const uint32_t mask = a.rings.ring_cap - 1u;
    const uint32_t s = window_start(a.rings, stream, P);
    const float *r0 = channel_ring(a.rings, stream, 0, CH);
    const float *r1 = CH == 2 ? channel_ring(a.rings, stream, 1, CH) : r0;

    // ---- stage: x[i], i < P, and zeros up to the end of the image
    for(uint32_t i = t; i < WF_PITCH_X; i += WF_PITCH_THREADS) {
        double x = 0.0;
        if(i < P) {
            const uint32_t p = (s + i) & mask;
            x = (double)r0[p];
            if constexpr(CH == 2)
                x = (x + (double)r1[p]) * 0.5; // exact
        }
        lds[pitch_at(i)] = x;
    }
    __syncthreads();

    // ---- lags: r(tau) and e(tau) of tau = tau0 + k, and e(0)
    const uint32_t tau0 = 1u + L * t;
    double r[L], e[L], e0 = 0.0;
#pragma unroll
    for(uint32_t k = 0; k < L; ++k)
        r[k] = e[k] = 0.0;
    if(tau0 <= H) {
        double win[2 * L]; // win[k] = x[j0 + tau0 + k]
#pragma unroll
        for(uint32_t k = 0; k < L; ++k)
            win[k] = lds[pitch_at(tau0 + k)];
        for(uint32_t j0 = 0; j0 < H; j0 += L) // (H is a multiple of 8)
            pitch_block(lds, j0, tau0, win, r, e, e0);
    }

    // ---- d(tau), its running sum, d'(tau)
    double d[L], run[L], mine = 0.0;
#pragma unroll
    for(uint32_t k = 0; k < L; ++k) {
        const double v = (e0 + e[k]) - 2.0 * r[k];
        d[k] = tau0 + k <= H && v > 0.0 ? v : 0.0;
        mine += d[k];
        run[k] = mine;
    }
    double incl = mine; // inclusive scan over the wavefront, lane order
#pragma unroll
    for(int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_up(incl, off, 64);
        if(lane >= (uint32_t)off)
            incl += o;
    }
    if(lane == 63u)
        lds_tot[wave] = incl;
    __syncthreads(); // (also: every thread has left the signal)
    double before = 0.0, total = 0.0;
    for(uint32_t w = 0; w < WF_PITCH_WAVES; ++w) {
        if(w == wave)
            before = total;
        total += lds_tot[w];
    }
    const double lower = __shfl_up(incl, 1, 64);
    before += lane ? lower : 0.0; // the sum of d over the lags below tau0
    double dp[L];
#pragma unroll
    for(uint32_t k = 0; k < L; ++k) {
        const double c = before + run[k];
        dp[k] = c > 0.0 ? d[k] * (double)(tau0 + k) / c : 1.0;
        if(tau0 + k <= H)
            lds[tau0 + k] = dp[k];
    }
    if(t == 0u)
        lds[0] = 1.0;

    // ---- search over [WF_HIP_PITCH_MIN_LAG, H - 1]
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    uint32_t first = NONE;
    PitchKey best{INFINITY, NONE};
#pragma unroll
    for(uint32_t k = 0; k < L; ++k) {
        const uint32_t tau = tau0 + k;
        if(tau >= WF_HIP_PITCH_MIN_LAG && tau < H) {
            if(dp[k] < WF_HIP_PITCH_THRESHOLD && first == NONE)
                first = tau;
            best = pitch_min(best, PitchKey{dp[k], tau});
        }
    }
    first = wave_min(first);
    best = pitch_wave_min(best);
    if(lane == 0u) {
        lds_idx[0][wave] = first;
        lds_key[wave] = best;
    }
    __syncthreads(); // (d' is in LDS)
    first = lds_idx[0][0];
    best = lds_key[0];
    for(uint32_t w = 1; w < WF_PITCH_WAVES; ++w) {
        first = lds_idx[0][w] < first ? lds_idx[0][w] : first;
        best = pitch_min(best, lds_key[w]);
    }
    uint32_t lag = best.lag;
    const uint32_t voiced = first != NONE ? 1u : 0u;
    if(voiced) { // the end of the descent: the first tau >= first with tau == H - 1 or not d'(tau + 1) < d'(tau)
        uint32_t stop = NONE;
        const double next = tau0 + L <= H ? lds[tau0 + L] : 0.0;
#pragma unroll
        for(uint32_t k = 0; k < L; ++k) {
            const uint32_t tau = tau0 + k;
            const double after = k + 1u < L ? dp[(k + 1u) % L] : next;
            if(tau >= first && tau < H && stop == NONE && (tau == H - 1u || !(after < dp[k])))
                stop = tau;
        }
        stop = wave_min(stop);
        if(lane == 0u)
            lds_idx[1][wave] = stop;
        __syncthreads(); // (voiced is the same in every thread)
        lag = lds_idx[1][0];
        for(uint32_t w = 1; w < WF_PITCH_WAVES; ++w)
            lag = lds_idx[1][w] < lag ? lds_idx[1][w] : lag;
    }
    if(t != 0u)
        return;

    // ---- interpolation
    wf_hip_pitch out{0.f, 0.f, 0u, 0u};
    if(total > 0.0) { // (else: digital silence, a constant: nothing to report)
        const double pa = lds[lag - 1u], pb = lds[lag], pc = lds[lag + 1u];
        const double den = pa - 2.0 * pb + pc;
        double p = 0.0;
        if(den > 0.0) {
            p = 0.5 * (pa - pc) / den;
            p = p < -0.5 ? -0.5 : p > 0.5 ? 0.5 : p;
        }
        const double clarity = 1.0 - pb;
        out.hz = (float)(a.sample_rate / ((double)lag + p));
        out.clarity = (float)(clarity < 0.0 ? 0.0 : clarity > 1.0 ? 1.0 : clarity);
        out.lag = lag;
        out.voiced = voiced;
    }
    a.out[blockIdx.x] = out;
}

} // namespace wf
