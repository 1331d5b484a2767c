// wf_impulse.hpp -- gfx950 read kernel of WF_HIP_OUT_IMPULSE (device code only; hipcc; included by wf_hip_measure.hip alone).
//
// Not in the reference: the fourth view of a dual-channel analyser, the response of captured channel 0 (measured) against channel 1
// (reference) over time -- the impulse response, its energy-time curve and the up to eight strongest arrivals (the definition is in
// include/wf_hip.h, "impulse response").  It stands on the sums of WF_HIP_OUT_XFER, taken by the same code (wf_xfer_sums.hpp), so
// the fields the two records share are the same bits.  wf_hip_read launches it on the handle's stream, behind every push issued so
// far, and copies the result back; nothing runs while the output is not read and nothing is kept between reads.
//
// One workgroup of WF_XFER_THREADS per stream; dynamic LDS as the transfer function's, `z` (P complex float64) and `ya` (half a
// region and a slot): 48 KB at P = 2048.
//   head       xfer_sums: the span check -- the zero record and out where it says so --, the sums of this thread's four bins, the lag.
//   response   max Sxx by butterflies and a hand-over; lambda; every thread Hr of its own bins to ya, ya[0] = ya[M] = 0; on the
//              way the weighted mean of the coherence, operation for operation as wf_xfer.hpp's record takes it.
//   ir         one transform of the Hermitian extension of ya, fetched while the rows fall into z; thread t reads
//              h[i - L] = Re y[(L - i) mod P] / P for i = t + 256 j, j < 8, writes ir[i] (consecutive lanes, consecutive floats), keeps
//              the eight float64 values in registers for direct_db and adds their squares up.
//   envelope   a barrier, then one transform of the one-sided spectrum 4 w[2 k] ya[k] -- T[k] = 1 - cos(2 pi k / M) is twice the Hann
//              table's entry 2 k --, 0 outside 1 <= k < M.  Behind it ya is free and holds exactly P doubles and two: env[i], which
//              the candidates' neighbours are read from.  etc_db[i]; the peak by wave_argmax and argmax_better.
//   arrivals   every thread holds env of its own indices that are candidates at or above the -30 dB rule, -1 otherwise; a round
//              strikes those within the guard of the arrival just taken and takes the block's argmax, up to seven times, one
//              barrier and one hand-over slot a round; thread 0 writes each arrival as it is taken.
//   record     the sums of h^2, all of it and around the peak, by wave sums added up by thread 0 in wave order; the scalars.
// The order of every sum and every max follows from P and K alone; there are no atomics and no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_xfer_sums.hpp"

namespace wf {

struct ImpulseArgs {
    RingView rings;
    wf_hip_impulse *out;     // [count] the entry of stream `first`
    const double *window;    // [P] periodic Hann
    const double2 *tw;       // [P / 2] e^(-j 2 pi m / P)
    double sample_rate;
    uint32_t first;          // first stream read
    uint32_t P;              // segment frames: a power of two, 64 <= P <= min(ring_cap / 8, WF_HIP_XFER_MAX_WINDOW)
    uint32_t log2p;
    uint32_t K;              // segments: (K - 1) P / 2 + 2 P + P / 2 - 1 < ring_cap
};

constexpr uint32_t WF_IMPULSE_OWN = WF_HIP_IMPULSE_FRAMES / WF_XFER_THREADS; // indices of ir and etc_db per thread
constexpr uint32_t WF_IMPULSE_WORDS = sizeof(wf_hip_impulse) / sizeof(uint32_t);
static_assert(WF_HIP_IMPULSE_FRAMES == WF_HIP_XFER_MAX_WINDOW && WF_IMPULSE_OWN * WF_XFER_THREADS == WF_HIP_IMPULSE_FRAMES,
              "every index of the largest window has a thread");
static_assert(sizeof(wf_hip_impulse) == 16576 && offsetof(wf_hip_impulse, arrivals) == 64 &&
                  offsetof(wf_hip_impulse, ir) == 64 + WF_HIP_IMPULSE_ARRIVALS * sizeof(wf_hip_impulse_arrival) &&
                  offsetof(wf_hip_impulse, etc_db) == offsetof(wf_hip_impulse, ir) + WF_HIP_IMPULSE_FRAMES * sizeof(float),
              "16 words of scalars, the arrivals, then the two curves");
static_assert(offsetof(wf_hip_impulse, window) == 4 && offsetof(wf_hip_impulse, hop) == 8 && offsetof(wf_hip_impulse, segments) == 12,
              "the words of the zero record that are not 0");
static_assert(2 * WF_HIP_IMPULSE_DIRECT + 1 <= WF_XFER_THREADS, "at most one index around the peak to a thread");

// grid: one workgroup per stream of [first, first + gridDim.x); dynamic LDS: (P + P / 2 + 1) * sizeof(double2)
__global__ __launch_bounds__(WF_XFER_THREADS, 2) void impulse_read_kernel(const ImpulseArgs a)
{
    extern __shared__ __align__(16) double2 impulse_lds[];
    // the cross-wave hand-overs, each written once
    __shared__ double max_x[WF_XFER_WAVES];
    __shared__ double coh_num[WF_XFER_WAVES], coh_den[WF_XFER_WAVES];
    __shared__ double sum_e[WF_XFER_WAVES], sum_d[WF_XFER_WAVES];
    __shared__ double arg_v[WF_HIP_IMPULSE_ARRIVALS][WF_XFER_WAVES]; // (a slot per round: the peak, then the arrivals)
    __shared__ uint32_t arg_k[WF_HIP_IMPULSE_ARRIVALS][WF_XFER_WAVES];

    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t stream = a.first + blockIdx.x;
    const uint32_t P = a.P, cb = a.log2p - 4u, M = P / 2u, H = P / 2u, L = P / 4u, K = a.K;
    double2 *z = impulse_lds, *ya = impulse_lds + P;
    const uint32_t wpos = a.rings.wpos[stream];
    wf_hip_impulse *out = a.out + blockIdx.x;

    // the running sums of this thread's bins k = 1 + t + u WF_XFER_THREADS, the lag and r[lag]
    double sxx[WF_XFER_OWN], syy[WF_XFER_OWN], sxr[WF_XFER_OWN], sxi[WF_XFER_OWN];
    int32_t n0;
    double peak;
    // silence in either channel, a NaN or an infinity: the zero record (uniform)
    if(!xfer_sums(a, z, ya, stream, sxx, syy, sxr, sxi, n0, peak)) {
        uint32_t *words = reinterpret_cast<uint32_t *>(out);
        for(uint32_t i = t; i < WF_IMPULSE_WORDS; i += WF_XFER_THREADS)
            words[i] = i == 1u ? P : i == 2u ? H : i == 3u ? K : 0u;
        return;
    }

    // response: lambda from max Sxx
    double mx = 0.0;
#pragma unroll
    for(uint32_t u = 0; u < WF_XFER_OWN; ++u)
        mx = fmax(mx, sxx[u]);
    mx = wave_max(mx);
    if(lane == 0u)
        max_x[wave] = mx;
    __syncthreads();
    mx = max_x[0];
#pragma unroll
    for(uint32_t w = 1; w < WF_XFER_WAVES; ++w)
        mx = fmax(mx, max_x[w]);
    const double dead = WF_HIP_STEREO_DEAD_RATIO * mx, lambda = WF_HIP_IMPULSE_REG * mx;

    // the weighted mean of the coherence over the live bins, as wf_xfer.hpp's record takes it
    double num = 0.0, den = 0.0;
#pragma unroll
    for(uint32_t u = 0; u < WF_XFER_OWN; ++u) {
        const uint32_t k = 1u + t + u * WF_XFER_THREADS;
        if(k < M) {
            if(sxx[u] > dead) {
                den += sxx[u];
                if(syy[u] != 0.0) {
                    const double m2 = sxr[u] * sxr[u] + sxi[u] * sxi[u];
                    const double c = fmin(m2 / (sxx[u] * syy[u]), 1.0);
                    num += sxx[u] * c;
                }
            }
        }
    }
    num = wave_sum(num);
    den = wave_sum(den);
    if(lane == 0u) {
        coh_num[wave] = num;
        coh_den[wave] = den;
    }
    // Hr[k] = Sxy[k] / (Sxx[k] + lambda) (0 where a reference that lies in the slack alone leaves the divisor 0)
#pragma unroll
    for(uint32_t u = 0; u < WF_XFER_OWN; ++u) {
        const uint32_t k = 1u + t + u * WF_XFER_THREADS;
        if(k < M) {
            const double d = sxx[u] + lambda;
            ya[k] = d > 0.0 ? make_double2(sxr[u] / d, sxi[u] / d) : make_double2(0.0, 0.0);
        }
    }
    if(t == 0u)
        ya[0] = ya[M] = make_double2(0.0, 0.0);
    __syncthreads(); // ya is written, and every thread is behind its last read of z

    // ir: h[n] = Re y[(-n) mod P] / P of the Hermitian extension's transform
    fft64_load16(z, a.tw, t, P, cb, [&](uint32_t i) { // Y[i] = ya[i] up to M, conj ya[P - i] beyond
        const double2 c = ya[i <= M ? i : P - i];
        return make_double2(c.x, i <= M ? c.y : -c.y);
    });
    fft64_passes<WF_XFER_THREADS>(z, a.tw, t, P, cb, fft64_block_sync{});
    const double inv_p = 1.0 / (double)P; // (a power of two: the product is the quotient)
    double hreg[WF_IMPULSE_OWN];
    double e = 0.0;
#pragma unroll
    for(uint32_t j = 0; j < WF_IMPULSE_OWN; ++j) {
        const uint32_t i = t + j * WF_XFER_THREADS;
        hreg[j] = 0.0;
        if(i < P) {
            hreg[j] = z[fft64_at((L - i) & (P - 1u), cb)].x * inv_p;
            e += hreg[j] * hreg[j];
        }
        out->ir[i] = (float)hreg[j]; // (the indices from P up: zeros on every read)
    }
    e = wave_sum(e);
    if(lane == 0u)
        sum_e[wave] = e;
    __syncthreads(); // every thread is behind its reads of z

    // envelope: a[n] of the one-sided spectrum 2 T[k] Hr[k]
    fft64_load16(z, a.tw, t, P, cb, [&](uint32_t i) {
        if(i == 0u || i >= M)
            return make_double2(0.0, 0.0);
        const double2 c = ya[i];
        const double s = 4.0 * a.window[2u * i];
        return make_double2(s * c.x, s * c.y);
    });
    fft64_passes<WF_XFER_THREADS>(z, a.tw, t, P, cb, fft64_block_sync{});
    double *env = reinterpret_cast<double *>(ya); // [P]: the load's barrier has passed, ya is free
    double best = -1.0;
    uint32_t kbest = 0u;
#pragma unroll
    for(uint32_t j = 0; j < WF_IMPULSE_OWN; ++j) {
        const uint32_t i = t + j * WF_XFER_THREADS;
        float db = 0.f;
        if(i < P) {
            const double2 c = z[fft64_at((L - i) & (P - 1u), cb)];
            const double ar = c.x * inv_p, ai = c.y * inv_p;
            const double ev = sqrt(ar * ar + ai * ai);
            env[i] = ev;
            db = ev == 0.0 ? -INFINITY : (float)(20.0 * log10(ev));
            if(ev > best) {
                best = ev;
                kbest = i;
            }
        }
        out->etc_db[i] = db;
    }
    wave_argmax(best, kbest);
    if(lane == 0u) {
        arg_v[0][wave] = best;
        arg_k[0][wave] = kbest;
    }
    __syncthreads(); // env is written
    best = arg_v[0][0];
    kbest = arg_k[0][0];
#pragma unroll
    for(uint32_t w = 1; w < WF_XFER_WAVES; ++w)
        argmax_better(best, kbest, arg_v[0][w], arg_k[0][w]);
    const double epk = best;
    const uint32_t ipk = kbest;

    // what thread 0 needs of both records that follow
    const auto head = [&](uint32_t count) {
        double cn = coh_num[0], cd = coh_den[0];
#pragma unroll
        for(uint32_t w = 1; w < WF_XFER_WAVES; ++w) {
            cn += coh_num[w];
            cd += coh_den[w];
        }
        out->valid = 1u;
        out->window = P;
        out->hop = H;
        out->segments = K;
        out->lag = n0;
        out->newest = wpos / H;
        out->lag_peak = (float)peak;
        out->mean_coherence = cd > 0.0 ? (float)(cn / cd) : 0.f;
        out->count = count;
        out->reserved[0] = out->reserved[1] = 0u;
    };
    uint32_t *const arrival_words = reinterpret_cast<uint32_t *>(&out->arrivals[0]);
    constexpr uint32_t ARRIVAL_WORDS = sizeof(wf_hip_impulse_arrival) / sizeof(uint32_t);

    // no response at all (uniform): a measured channel that is +-0 under every segment
    if(epk == 0.0) {
#pragma unroll
        for(uint32_t j = 0; j < WF_IMPULSE_OWN; ++j) {
            const uint32_t i = t + j * WF_XFER_THREADS;
            if(i < P)
                out->ir[i] = 0.f; // (+0 where the transform left -0)
        }
        if(t < WF_HIP_IMPULSE_ARRIVALS * ARRIVAL_WORDS)
            arrival_words[t] = 0u;
        if(t == 0u) {
            head(0u);
            out->peak_index = 0u;
            out->peak_db = out->delay_ms = out->energy_db = out->direct_db = 0.f;
        }
        return;
    }

    // direct: the sum of h^2 within WF_HIP_IMPULSE_DIRECT indices of the peak
    double dsum = 0.0;
#pragma unroll
    for(uint32_t j = 0; j < WF_IMPULSE_OWN; ++j) {
        const uint32_t i = t + j * WF_XFER_THREADS;
        const uint32_t dist = i > ipk ? i - ipk : ipk - i;
        if(i < P && dist <= WF_HIP_IMPULSE_DIRECT)
            dsum += hreg[j] * hreg[j];
    }
    dsum = wave_sum(dsum);
    if(lane == 0u)
        sum_d[wave] = dsum; // (read behind the first round's barrier)

    // an arrival at index i into slot `slot` (thread 0); its position in frames behind the reference
    const auto arrival = [&](uint32_t slot, uint32_t i) {
        const double c = env[i];
        double frac = 0.0;
        if(i >= 1u && i + 1u < P) {
            const double l = env[i - 1u], r = env[i + 1u];
            const double curv = (l - c) + (r - c);
            if(curv < 0.0)
                frac = fmin(fmax(0.5 * (l - r) / curv, -0.5), 0.5);
        }
        const double frames = (double)(n0 + (int32_t)i - (int32_t)L) + frac;
        out->arrivals[slot].frames = (float)frames;
        out->arrivals[slot].level_db = (float)(20.0 * log10(c / epk));
        out->arrivals[slot].polarity = z[fft64_at((L - i) & (P - 1u), cb)].x >= 0.0 ? 1 : -1;
        out->arrivals[slot].reserved = 0u;
        return frames;
    };
    double peak_frames = 0.0;
    if(t == 0u)
        peak_frames = arrival(0u, ipk);

    // the candidates of this thread's indices: interior local maxima at or above the -30 dB rule
    const double least = WF_HIP_IMPULSE_ARRIVAL_RATIO * epk;
    double cand[WF_IMPULSE_OWN];
#pragma unroll
    for(uint32_t j = 0; j < WF_IMPULSE_OWN; ++j) {
        const uint32_t i = t + j * WF_XFER_THREADS;
        cand[j] = -1.0;
        if(i >= 1u && i + 1u < P) {
            const double ev = env[i];
            if(ev > env[i - 1u] && ev >= env[i + 1u] && ev >= least)
                cand[j] = ev;
        }
    }
    uint32_t count = 1u, last = ipk;
#pragma unroll 1
    for(uint32_t r = 1; r < WF_HIP_IMPULSE_ARRIVALS; ++r) {
        best = -1.0;
        kbest = 0u;
#pragma unroll
        for(uint32_t j = 0; j < WF_IMPULSE_OWN; ++j) {
            const uint32_t i = t + j * WF_XFER_THREADS;
            const uint32_t dist = i > last ? i - last : last - i;
            if(dist <= WF_HIP_IMPULSE_GUARD)
                cand[j] = -1.0;
            if(cand[j] > best) { // (ascending i: the lower index of equal values)
                best = cand[j];
                kbest = i;
            }
        }
        wave_argmax(best, kbest);
        if(lane == 0u) {
            arg_v[r][wave] = best;
            arg_k[r][wave] = kbest;
        }
        __syncthreads();
        best = arg_v[r][0];
        kbest = arg_k[r][0];
#pragma unroll
        for(uint32_t w = 1; w < WF_XFER_WAVES; ++w)
            argmax_better(best, kbest, arg_v[r][w], arg_k[r][w]);
        if(best < 0.0) // (uniform) no candidate is left
            break;
        if(t == 0u)
            arrival(count, kbest);
        last = kbest;
        ++count;
    }

    // record
    if(t == 0u) {
        for(uint32_t i = count * ARRIVAL_WORDS; i < WF_HIP_IMPULSE_ARRIVALS * ARRIVAL_WORDS; ++i)
            arrival_words[i] = 0u; // (the slots not used: zeros on every read)
        double es = sum_e[0], ds = sum_d[0];
#pragma unroll
        for(uint32_t w = 1; w < WF_XFER_WAVES; ++w) {
            es += sum_e[w];
            ds += sum_d[w];
        }
        head(count);
        out->peak_index = ipk;
        out->peak_db = (float)(20.0 * log10(epk));
        out->delay_ms = (float)(peak_frames * 1000.0 / a.sample_rate);
        out->energy_db = (float)thd_db(es, 1.0);
        out->direct_db = (float)thd_db(ds, 1.0);
    }
}

} // namespace wf
