// wf_imd.hpp -- gfx950 read kernel of WF_HIP_OUT_IMD (device code only; hipcc; included by wf_hip_measure.hip alone).
//
// Not in the reference: the two-tone intermodulation analyser, per captured channel the two tones of a twin-tone stimulus, their
// twenty sum and difference products of orders 2 .. 5, the figures of three standards (total IMD, the difference-frequency
// distortion of IEC 60268-3, the modulation distortion of the DIN / SMPTE method), total distortion + noise and the noise floor,
// from the spectrum of the distortion analyser (the definition is in include/wf_hip.h, "intermodulation").  wf_hip_read launches it
// on the handle's stream, behind every push issued so far, and copies the result back; nothing runs while the output is not read.
//
// One workgroup of WF_THD_THREADS per stream; the load, the transform in P complex float64 of dynamic LDS and the bins' powers are
// wf_thd_spectrum.hpp's, the head shared with wf_thd.hpp, whose tables these are too.  Behind it, per channel:
//   tones      two argmax searches as wf_thd.hpp's one: threads stride over [2H + 1, M - H - 1], the second search passing over the
//              bins within 2H of the first's; a wave butterfly and a hand-over of eight (value, bin) pairs through LDS, every
//              thread scanning them in wave order.  Lanes 0 .. 16 of every wave take a tone's bins, and every wave forms the same
//              F and f of both.
//   regions    the twenty products and the harmonics 2 .. 5 of either tone, 28 regions: wave w takes the regions w, w + 8 ..., one
//              a round; the region's sum and bin (~0: not clear, not in band) go to LDS.
//   residue    threads stride over (H, M), pass over the tones' regions, classify each of their bins against the 28 regions (a
//              region can hold one bin of a thread at most: found by division, not by search) and accumulate D, I, N and n; wave
//              butterflies, the eight waves' parts through LDS, summed in wave order by wave 0, which writes the fields: a
//              channel's 33 levels are a log10 each, so lane i forms and stores the i-th rather than thread 0 all of them in
//              turn (with that tail, and the record's registers costing a workgroup per CU at P = 4096, a read of 4096 streams took
//              1.9 and 1.3 times as long at P = 4096 and 8192), and one more lane the frequencies and the integers.
// The order of every sum follows from P, the two bins and the regions' bins alone; there are no atomics and no scratch, and the
// hand-over is all the static LDS there is.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_thd_spectrum.hpp"

namespace wf {

struct ImdArgs {
    RingView rings;
    wf_hip_imd *out;         // [count] the entry of stream `first`
    const double *window;    // [P] periodic 7-term Blackman-Harris: the distortion analyser's tables
    const double2 *tw;       // [P / 2] e^(-j 2 pi m / P)
    double S;                // P sum w^2 / 4
    double sample_rate;
    uint32_t first;          // first stream read
    uint32_t P;              // window frames: a power of two, 512 <= P <= min(ring_cap, WF_HIP_THD_MAX_WINDOW)
    uint32_t log2p;
};

constexpr uint32_t WF_IMD_HARMONICS = 4;                                            // h = 2 .. 5 of either tone
constexpr uint32_t WF_IMD_REGIONS = WF_HIP_IMD_PRODUCTS + 2 * WF_IMD_HARMONICS;     // products first
static_assert(WF_HIP_IMD_PRODUCTS == 20, "orders 2 .. 5: 2 (1 + 2 + 3 + 4) products, and the masks below");
constexpr uint32_t WF_IMD_ORDER_MASK[4] = {0x3u, 0x3cu, 0xfc0u, 0xff000u};          // the products q of order 2 .. 5
constexpr uint32_t WF_IMD_MOD_MASK = 0x30cfu;                                       // q of f_hi -+ n f_lo, n = 1 .. 4
// a channel's levels are its float32 fields, LV of them in a row from lo_db to product_db[19]: level i is the i-th
constexpr uint32_t WF_IMD_LEVELS = 13 + WF_HIP_IMD_PRODUCTS;
static_assert(offsetof(wf_hip_imd_channel, hi_db) == offsetof(wf_hip_imd_channel, lo_db) + 4 &&
              offsetof(wf_hip_imd_channel, ratio_db) == offsetof(wf_hip_imd_channel, lo_db) + 8 &&
              offsetof(wf_hip_imd_channel, imd_db) == offsetof(wf_hip_imd_channel, lo_db) + 12 &&
              offsetof(wf_hip_imd_channel, order_db) == offsetof(wf_hip_imd_channel, lo_db) + 16 &&
              offsetof(wf_hip_imd_channel, dfd2_db) == offsetof(wf_hip_imd_channel, lo_db) + 32 &&
              offsetof(wf_hip_imd_channel, dfd3_db) == offsetof(wf_hip_imd_channel, lo_db) + 36 &&
              offsetof(wf_hip_imd_channel, mod_db) == offsetof(wf_hip_imd_channel, lo_db) + 40 &&
              offsetof(wf_hip_imd_channel, tdn_db) == offsetof(wf_hip_imd_channel, lo_db) + 44 &&
              offsetof(wf_hip_imd_channel, noise_db) == offsetof(wf_hip_imd_channel, lo_db) + 48 &&
              offsetof(wf_hip_imd_channel, product_db) == offsetof(wf_hip_imd_channel, lo_db) + 52 &&
              offsetof(wf_hip_imd_channel, lo_bin) == offsetof(wf_hip_imd_channel, lo_db) + 4 * WF_IMD_LEVELS,
              "the order of the levels in wf_hip_imd_channel");
static_assert(WF_IMD_LEVELS < 64 && sizeof(wf_hip_imd_channel) / 4 <= 64, "a channel's levels and its words: a lane each");

// grid: one workgroup per stream of [first, first + gridDim.x); dynamic LDS: P * sizeof(double2)
template<int CH> __global__ __launch_bounds__(WF_THD_THREADS) void imd_read_kernel(const ImdArgs a)
{
    extern __shared__ __align__(16) double2 imd_lds[];
    double2 *lds = imd_lds;
    // the cross-wave hand-over ([2]: one per search, so that the second needs no barrier before it writes)
    __shared__ double arg_v[2][WF_THD_WAVES];
    __shared__ uint32_t arg_k[2][WF_THD_WAVES];
    __shared__ double reg_p[WF_IMD_REGIONS];
    __shared__ uint32_t reg_k[WF_IMD_REGIONS]; // (~0: not clear, not in band)
    __shared__ double res_d[WF_THD_WAVES], res_i[WF_THD_WAVES], res_n[WF_THD_WAVES];
    __shared__ uint32_t res_cnt[WF_THD_WAVES];

    constexpr uint32_t H = WF_HIP_THD_LOBE, NQ = WF_HIP_IMD_PRODUCTS, NR = WF_IMD_REGIONS, LV = WF_IMD_LEVELS;
    constexpr uint32_t WORDS = sizeof(wf_hip_imd_channel) / 4u;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t P = a.P, cb = a.log2p - 4u, M = P / 2u;

    // load, transform and bins: slot k becomes (p_0[k], p_1[k])
    thd_spectrum<CH>(lds, a, t);

    wf_hip_imd *out = a.out + blockIdx.x;
#pragma unroll
    for(int c = 0; c < CH; ++c) {
        // p[k], 1 <= k < M, of this channel (a whole slot is read: 16 lanes, one row)
        const auto p = [&](uint32_t k) {
            const double2 v = lds[fft64_at(k, cb)];
            return c == 0 ? v.x : v.y;
        };
        // |k - centre| <= reach (no operand below 0)
        const auto within = [](uint32_t k, uint32_t centre, uint32_t reach) { return k + reach >= centre && k <= centre + reach; };
        // the argmax over [2H + 1, M - H - 1], with `second` outside 2H of `first`: uniform
        const auto strongest = [&](const uint32_t slot, const bool second, const uint32_t first, double &best, uint32_t &kb) {
            best = 0.0;
            kb = 2u * H + 1u;
            for(uint32_t k = 2u * H + 1u + t; k <= M - H - 1u; k += WF_THD_THREADS) {
                if(second && within(k, first, 2u * H))
                    continue;
                const double v = p(k);
                if(v > best) {
                    best = v;
                    kb = k;
                }
            }
            wave_argmax(best, kb);
            if(lane == 0u) {
                arg_v[slot][wave] = best;
                arg_k[slot][wave] = kb;
            }
            __syncthreads();
            best = arg_v[slot][0];
            kb = arg_k[slot][0];
#pragma unroll
            for(uint32_t w = 1; w < WF_THD_WAVES; ++w)
                argmax_better(best, kb, arg_v[slot][w], arg_k[slot][w]);
        };
        // a tone's region: every wave sums the same 2H + 1 bins in the same order (k0 - H >= H + 1, k0 + H <= M - 1)
        const auto tone = [&](const uint32_t k0, double &F, double &f) {
            const uint32_t k = k0 - H + lane;
            const double v = lane <= 2u * H ? p(k) : 0.0;
            F = wave_sum(v);
            f = wave_sum((double)k * v) / F;
        };

        double va, vb, Fa, fa, Fb, fb;
        uint32_t ka, kb;
        strongest(0, false, 0u, va, ka);
        tone(ka, Fa, fa);
        strongest(1, true, ka, vb, kb);
        tone(kb, Fb, fb);
        const bool one = Fa > 0.0 && Fa < INFINITY; // (false for a NaN)
        const bool two = one && vb > 0.0 && Fb < INFINITY && !(Fb < WF_HIP_IMD_MIN_RATIO * Fa);
        const bool a_low = fa < fb; // (the regions share no bin, so the two never meet)
        const uint32_t klo = a_low ? ka : kb, khi = a_low ? kb : ka;
        const double flo = a_low ? fa : fb, fhi = a_low ? fb : fa;
        const double Flo = a_low ? Fa : Fb, Fhi = a_low ? Fb : Fa;

        // products and harmonics: one region per wave and round
        for(uint32_t r = wave; r < NR; r += WF_THD_WAVES) {
            const bool product = r < NQ;
            double f;
            if(product) { // pair j = q / 2 of order o, the m-th of its order
                const uint32_t j = r >> 1, o = j < 1u ? 2u : j < 3u ? 3u : j < 6u ? 4u : 5u;
                const uint32_t m = j - (o - 1u) * (o - 2u) / 2u + 1u, n = o - m;
                f = (r & 1u) ? (double)m * fhi + (double)n * flo : fabs((double)m * fhi - (double)n * flo);
            } else {
                const uint32_t i = r - NQ;
                f = (double)(2u + (i & 3u)) * ((i >> 2) ? fhi : flo);
            }
            uint32_t kr = ~0u;
            if(two) {
                const uint32_t q = (uint32_t)floor(f + 0.5); // (0 <= f <= 5 (M + H): no overflow)
                bool ok = q + H <= M - 1u && q > H;          // (a harmonic's q >= 2 (2H + 1 - H) > H always: stated for the index below)
                if(product)
                    ok = ok && q >= 2u * H + 1u && !within(q, klo, 2u * H) && !within(q, khi, 2u * H);
                if(ok)
                    kr = q;
            }
            const uint32_t k = kr - H + lane;
            const double v = (kr != ~0u && lane <= 2u * H) ? p(k) : 0.0;
            const double rp = wave_sum(v);
            if(lane == 0u) {
                reg_p[r] = rp;
                reg_k[r] = kr;
            }
        }
        __syncthreads();

        // residue: D over H < k < M outside the tones' regions; of these bins I in a clear product's region, N and n in no region.
        // A thread's bins lie WF_THD_THREADS apart and a region is 2H + 1 wide, so a region holds at most one of them, the last at
        // or below its upper end: the thread's bin j is classified in bit j of `in_i` (products) and `in_h` (harmonics), region by
        // region, and the sums follow in ascending k
        static_assert(2 * WF_HIP_THD_LOBE + 1 <= WF_THD_THREADS && WF_HIP_THD_MAX_WINDOW / 2 <= 32 * WF_THD_THREADS);
        const uint32_t k_first = H + 1u + t;
        uint32_t in_i = 0, in_h = 0, bits = 0;
#pragma unroll 1
        for(uint32_t i = 0; i < NR; ++i) {
            const uint32_t kr = reg_k[i];
            if(kr == ~0u)
                continue;
            if(i < NQ)
                bits |= 1u << i;
            if(kr + H < k_first)
                continue;
            const uint32_t j = (kr + H - k_first) / WF_THD_THREADS; // (k_first + j THREADS <= kr + H <= M - 1)
            if(k_first + j * WF_THD_THREADS + H >= kr)
                (i < NQ ? in_i : in_h) |= 1u << j;
        }
        double D = 0.0, I = 0.0, N = 0.0;
        uint32_t n = 0;
        for(uint32_t k = k_first, j = 0; k < M; k += WF_THD_THREADS, ++j) {
            if(within(k, klo, H) || within(k, khi, H))
                continue;
            const double v = p(k);
            D += v;
            if(in_i >> j & 1u)
                I += v;
            else if(!(in_h >> j & 1u)) {
                N += v;
                ++n;
            }
        }
        D = wave_sum(D);
        I = wave_sum(I);
        N = wave_sum(N);
        n = wave_sum(n);
        if(lane == 0u) {
            res_d[wave] = D;
            res_i[wave] = I;
            res_n[wave] = N;
            res_cnt[wave] = n;
        }
        __syncthreads();

        // the fields, by wave 0: the channel's 33 levels are one log10 each, so lane i forms the i-th of them, in the struct's order,
        // rather than one thread all of them in turn; lane LV the frequencies and the integers.  Every lane sums the waves' parts
        // alike, in wave order
        if(wave == 0u) {
            uint32_t *words = reinterpret_cast<uint32_t *>(&out->ch[c]);
            if(!two) { // every field 0 but `tones`
                if(lane < WORDS)
                    words[lane] = lane == offsetof(wf_hip_imd_channel, tones) / 4u ? (one ? 1u : 0u) : 0u;
            } else {
                D = res_d[0];
                I = res_i[0];
                N = res_n[0];
                n = res_cnt[0];
#pragma unroll
                for(uint32_t w = 1; w < WF_THD_WAVES; ++w) {
                    D += res_d[w];
                    I += res_i[w];
                    N += res_n[w];
                    n += res_cnt[w];
                }
                const double T = Flo + Fhi;
                // the sums over products that the levels 4 .. 7 (an order's) and 10 (the modulation's) need: q ascending, the clear ones
                const uint32_t pick = (lane >= 4u && lane < 8u ? WF_IMD_ORDER_MASK[lane & 3u] : lane == 10u ? WF_IMD_MOD_MASK : 0u) & bits;
                double psum = 0.0;
#pragma unroll 1
                for(uint32_t q = 0; q < NQ; ++q)
                    if(pick >> q & 1u)
                        psum += reg_p[q];
                const double den = sqrt(Flo) + sqrt(Fhi);
                const double Ns = n ? N * (double)(M - 5u * H - 3u) / (double)n : 0.0;
                // level i = scale log10(num / den), or -inf where it is not defined
                double num = 0.0, under = T, scale = 10.0;
                bool defined = true;
                if(lane >= LV - NQ && lane < LV) { // product_db[q]
                    const uint32_t q = lane - (LV - NQ);
                    num = reg_p[q];
                    defined = bits >> q & 1u;
                } else if(lane >= 4u && lane < 8u) { // order_db[o - 2]
                    num = psum;
                    defined = pick != 0u;
                } else {
                    switch(lane) {
                    case 0: num = Flo, under = a.S; break;                           // lo_db
                    case 1: num = Fhi, under = a.S; break;                           // hi_db
                    case 2: num = Fhi, under = Flo; break;                           // ratio_db
                    case 3: num = I, defined = bits != 0u; break;                    // imd_db
                    case 8: num = sqrt(reg_p[0]), under = den, scale = 20.0, defined = bits & 1u; break; // dfd2_db
                    case 9:                                                          // dfd3_db
                        num = ((bits & 4u) ? sqrt(reg_p[2]) : 0.0) + ((bits & 16u) ? sqrt(reg_p[4]) : 0.0);
                        under = den, scale = 20.0, defined = bits & 20u;
                        break;
                    case 10: num = psum, under = Fhi; break;                         // mod_db
                    case 11: num = D; break;                                         // tdn_db
                    case 12: num = Ns, under = 2.0 * a.S; break;                     // noise_db
                    default: break;
                    }
                }
                float level = -INFINITY;
                if(defined) // (dB(x, y) of the definition)
                    level = num == 0.0 ? -INFINITY : under == 0.0 ? INFINITY : (float)(scale * log10(num / under));
                if(lane < LV)
                    words[offsetof(wf_hip_imd_channel, lo_db) / 4u + lane] = __float_as_uint(level);
                else if(lane == LV) {
                    wf_hip_imd_channel &r = out->ch[c];
                    r.lo_hz = flo * a.sample_rate / (double)P;
                    r.hi_hz = fhi * a.sample_rate / (double)P;
                    r.lo_bin = klo;
                    r.hi_bin = khi;
                    r.products = bits;
                    r.tones = 2u;
                    r.valid = 1u;
                    r.reserved[0] = r.reserved[1] = 0u;
                }
            }
        }
    }
    if(CH == 1 && t < WORDS)
        reinterpret_cast<uint32_t *>(&out->ch[1])[t] = 0u;
    if(t == 0u) {
        out->window = P;
        out->reserved[0] = out->reserved[1] = out->reserved[2] = 0u;
    }
}

} // namespace wf
