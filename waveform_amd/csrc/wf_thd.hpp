// wf_thd.hpp -- gfx950 read kernel of WF_HIP_OUT_THD (device code only; hipcc; included by wf_hip_measure.hip alone).
//
// Not in the reference: the distortion analyser, per captured channel the fundamental of a test tone, its harmonics 2 .. 10, THD,
// THD+N, SNR, SFDR and the noise floor, from one complex float64 transform of the newest P frames of the rings through a 7-term
// Blackman-Harris taper (the definition is in include/wf_hip.h, "distortion").  wf_hip_read launches it on the handle's stream,
// behind every push issued so far, and copies the result back; nothing runs while the output is not read.
//
// One workgroup of WF_THD_THREADS per stream; the transform lives in LDS as P complex float64 (16 B each: 128 KB at P = 8192, one
// workgroup to a CU).  The transform itself is wf_fft64_lds.hpp's, shared with the stereo image and the sonogram, as are its
// swizzled slots: every phase below has consecutive lanes on consecutive bins and reads whole 16-byte slots, so 16 lanes cover one
// 256-byte row whatever its permutation and no read conflicts.  The load, the transform and the bins' powers are
// wf_thd_spectrum.hpp's, the head shared with the intermodulation analyser (wf_imd.hpp):
//   bins       thread per pair (k, P - k): slot k becomes (p_0[k], p_1[k]), as wf_stereo.hpp does it; a channel whose window is
//              all zeros, which the load has noted, reads 0 exactly.
// then per channel
//   argmax     threads stride over [2H + 1, M - H - 1]; a wave butterfly and a hand-over of eight (value, bin) pairs through LDS,
//              every thread scanning them in wave order: the larger value wins and the lower bin a tie, so k0 is uniform.
//   fundamental lanes 0 .. 16 of every wave take the bins k0 - H .. k0 + H, and every wave forms the same F and f0.
//   harmonics  wave w takes harmonic 2 + w (wave 0 also the tenth): its region's sum and bin go to LDS.
//   residue    threads stride over (H, M), classify each bin against the fundamental's and the in-band harmonics' regions and
//              accumulate D, N, n and the spur; wave butterflies, the eight waves' parts through LDS, summed by thread 0 in
//              wave order, which writes the fields.
// The order of every sum follows from P, k0 and the k_h alone; there are no atomics and no scratch, and the hand-over is all the
// static LDS there is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_thd_spectrum.hpp"

namespace wf {

struct ThdArgs {
    RingView rings;
    wf_hip_thd *out;         // [count] the entry of stream `first`
    const double *window;    // [P] periodic 7-term Blackman-Harris
    const double2 *tw;       // [P / 2] e^(-j 2 pi m / P)
    double S;                // P sum w^2 / 4
    double sample_rate;
    uint32_t first;          // first stream read
    uint32_t P;              // window frames: a power of two, 512 <= P <= min(ring_cap, WF_HIP_THD_MAX_WINDOW)
    uint32_t log2p;
};
static_assert(WF_HIP_THD_HARMONICS <= 2 * WF_THD_WAVES, "at most two harmonics to a wavefront");

// grid: one workgroup per stream of [first, first + gridDim.x); dynamic LDS: P * sizeof(double2)
template<int CH> __global__ __launch_bounds__(WF_THD_THREADS) void thd_read_kernel(const ThdArgs a)
{
    extern __shared__ __align__(16) double2 thd_lds[];
    double2 *lds = thd_lds;
    // the cross-wave hand-over
    __shared__ double arg_v[WF_THD_WAVES];
    __shared__ uint32_t arg_k[WF_THD_WAVES];
    __shared__ double harm_p[WF_HIP_THD_HARMONICS];
    __shared__ uint32_t harm_k[WF_HIP_THD_HARMONICS]; // (~0: not in band)
    __shared__ double res_d[WF_THD_WAVES], res_n[WF_THD_WAVES], res_v[WF_THD_WAVES];
    __shared__ uint32_t res_cnt[WF_THD_WAVES], res_k[WF_THD_WAVES];

    constexpr uint32_t H = WF_HIP_THD_LOBE, NH = WF_HIP_THD_HARMONICS;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t P = a.P, cb = a.log2p - 4u, M = P / 2u;

    // load, transform and bins: slot k becomes (p_0[k], p_1[k])
    thd_spectrum<CH>(lds, a, t);

    wf_hip_thd *out = a.out + blockIdx.x;
#pragma unroll
    for(int c = 0; c < CH; ++c) {
        // p[k], 1 <= k < M, of this channel (a whole slot is read: 16 lanes, one row)
        const auto p = [&](uint32_t k) {
            const double2 v = lds[fft64_at(k, cb)];
            return c == 0 ? v.x : v.y;
        };

        // argmax over [2H + 1, M - H - 1]
        double best = 0.0;
        uint32_t k0 = 2u * H + 1u;
        for(uint32_t k = 2u * H + 1u + t; k <= M - H - 1u; k += WF_THD_THREADS) {
            const double v = p(k);
            if(v > best) {
                best = v;
                k0 = k;
            }
        }
        wave_argmax(best, k0);
        if(lane == 0u) {
            arg_v[wave] = best;
            arg_k[wave] = k0;
        }
        __syncthreads();
        best = arg_v[0];
        k0 = arg_k[0];
#pragma unroll
        for(uint32_t w = 1; w < WF_THD_WAVES; ++w)
            argmax_better(best, k0, arg_v[w], arg_k[w]);

        // fundamental: every wave sums the same 2H + 1 bins in the same order
        double F, f0;
        {
            const uint32_t k = k0 - H + lane; // (k0 - H >= H + 1, k0 + H <= M - 1)
            const double v = lane <= 2u * H ? p(k) : 0.0;
            F = wave_sum(v);
            f0 = wave_sum((double)k * v) / F;
        }
        const bool valid = F > 0.0 && F < INFINITY; // (false for a NaN)

        // harmonics: one region per wave
        for(uint32_t h = 2u + wave; h < 2u + NH; h += WF_THD_WAVES) {
            uint32_t kh = ~0u;
            if(valid) {
                const uint32_t r = (uint32_t)floor((double)h * f0 + 0.5); // (<= 10 (M + H): no overflow)
                if(r + H <= M - 1u && r > H) // (r >= 2 (k0 - H) > H always: stated for the index below)
                    kh = r;
            }
            const uint32_t k = kh - H + lane;
            const double v = (kh != ~0u && lane <= 2u * H) ? p(k) : 0.0;
            const double hp = wave_sum(v);
            if(lane == 0u) {
                harm_p[h - 2u] = hp;
                harm_k[h - 2u] = kh;
            }
        }
        __syncthreads();

        // residue: D over H < k < M outside the fundamental's region, N and n outside the harmonics' as well, the spur
        uint32_t hk[NH];
#pragma unroll
        for(uint32_t i = 0; i < NH; ++i)
            hk[i] = harm_k[i];
        double D = 0.0, N = 0.0, sv = -1.0;
        uint32_t n = 0, ks = ~0u;
        for(uint32_t k = H + 1u + t; k < M; k += WF_THD_THREADS) {
            if(k + H >= k0 && k <= k0 + H)
                continue;
            const double v = p(k);
            D += v;
            if(v > sv) {
                sv = v;
                ks = k;
            }
            bool harmonic = false;
#pragma unroll
            for(uint32_t i = 0; i < NH; ++i)
                harmonic = harmonic || (hk[i] != ~0u && k + H >= hk[i] && k <= hk[i] + H);
            if(!harmonic) {
                N += v;
                ++n;
            }
        }
        D = wave_sum(D);
        N = wave_sum(N);
        n = wave_sum(n);
        wave_argmax(sv, ks);
        if(lane == 0u) {
            res_d[wave] = D;
            res_n[wave] = N;
            res_v[wave] = sv;
            res_cnt[wave] = n;
            res_k[wave] = ks;
        }
        __syncthreads();

        if(t == 0u) {
            wf_hip_thd_channel r{};
            if(valid) {
                D = res_d[0];
                N = res_n[0];
                n = res_cnt[0];
                sv = res_v[0];
                ks = res_k[0];
#pragma unroll
                for(uint32_t w = 1; w < WF_THD_WAVES; ++w) {
                    D += res_d[w];
                    N += res_n[w];
                    n += res_cnt[w];
                    argmax_better(sv, ks, res_v[w], res_k[w]);
                }
                double hsum = 0.0;
                uint32_t bits = 0;
#pragma unroll
                for(uint32_t i = 0; i < NH; ++i) {
                    const bool in_band = hk[i] != ~0u;
                    r.harmonic_db[i] = in_band ? (float)thd_db(harm_p[i], F) : -INFINITY;
                    if(in_band) {
                        hsum += harm_p[i];
                        bits |= 1u << i;
                    }
                }
                const double Ns = N * (double)(M - 3u * H - 2u) / (double)n;
                const double thdn = thd_db(D, F);
                r.fundamental_hz = f0 * a.sample_rate / (double)P;
                r.fundamental_db = (float)thd_db(F, a.S);
                r.thd_db = bits ? (float)thd_db(hsum, F) : -INFINITY;
                r.thdn_db = (float)thdn;
                r.snr_db = (float)thd_db(F, Ns);
                r.noise_db = (float)thd_db(Ns, 2.0 * a.S);
                r.sfdr_db = (float)thd_db(p(k0), sv);
                r.spur_hz = (float)((double)ks * a.sample_rate / (double)P);
                r.enob = (float)((-thdn - 1.76) / 6.02);
                r.fundamental_bin = k0;
                r.spur_bin = ks;
                r.harmonics = bits;
                r.valid = 1u;
            }
            out->ch[c] = r;
        }
    }
    if(t == 0u) {
        if(CH == 1)
            out->ch[1] = wf_hip_thd_channel{};
        out->window = P;
        out->reserved[0] = out->reserved[1] = out->reserved[2] = 0u;
    }
}

} // namespace wf
