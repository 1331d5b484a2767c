// wf_click.hpp -- gfx950 read kernel of WF_HIP_OUT_CLICK (device code only; hipcc; included by wf_hip_measure.hip alone).
//
// Not in the reference: the click detector of a restoration or QC suite, per captured channel the clicks, pops and splices of the
// newest P = min(fft_size, 8192) frames of the ring -- the frames a linear predictor of order 16, fitted to the window itself,
// cannot account for -- as a count, a rate and the up to eight strongest events (the definition is in include/wf_hip.h, "clicks").
// wf_hip_read launches it on the handle's stream, behind every push issued so far, and copies the result back; nothing runs while
// the output is not read.
//
// One workgroup of WF_CLICK_THREADS per stream and captured channel (blockIdx.x = entry * CH + channel); the ring is read once.
//   load       frame i of the window at x[i] in dynamic LDS, consecutive lanes consecutive words of the ring, eight fetches in flight.  A = the largest
//              |x| as an integer maximum of the patterns without their sign, the NaN / infinity verdict from the exponent bits:
//              no float operation sees a sample before the verdict.
//   r[0..16]   thread t keeps 17 running fma sums over the frames t, t + 256, ..., each with its 17 lagged operands from LDS (a
//              product of two float32 is exact in float64, so the fused sum is the plain one); wave_sum (lane distance 32 .. 1);
//              the four waves' sums in order, by every thread.
//   Levinson   every thread, redundantly: r, a and the step's copy stay in registers (both loops unrolled), no broadcast and no
//              divergence.  Contraction is off here and in the residual: the definition rounds every product on its own.
//   residual   a thread per frame, strided like the sums: d[n] = (float) |e[n]| into LDS behind the window.
//   medians    a wavefront per block of 256 (the last up to 511) judged frames, up to 8 patterns per lane: the element of rank
//              len / 2 bit by bit from bit 30 down, a ballot and a popcount per slot and bit; all of it wave-uniform.  A window of
//              one block has two more waves select the medians of its halves.
//   g          the same selection over all judged frames across the workgroup, the thread's up to 32 patterns in registers over the
//              31 rounds: a wave's count per bit by ballots, the four counts through LDS (two buffers by turns, one barrier per bit).
//   hits       s_b by thread b; d[n] / s_b > 16 by ballot into a bitmap of 64-bit words; the largest ratio per lane, then per
//              wave, then of the four.  A hit starts an event if the 32 bits below it are clear (a thread per word); an event's
//              number is the count of starts up to its hit.  Per event, integer LDS atomics: the largest ratio as the pattern of
//              a positive double, the last hit, then the first hit whose ratio is that largest.  Words without a hit are skipped.
//   list       a thread per event (at most 248: starts lie more than 32 frames apart); eight rounds of wave_argmax /
//              argmax_better over ((double) strength_db, start), the winner writes its slot and leaves.
//   leave      the channel's 224 bytes from an image in LDS; channel 0's workgroup writes the tail, and with CH == 1 the zero ch[1].
// No float atomics: every float sum has the order above, every other accumulation is an integer count, a maximum or a minimum.
// Measured on an MI355X (tools/click_bench.py, profiles/click_kernel_stats.json; 4096 stereo streams, the read's 1.9 MB copy into
// page-locked memory included): noise 980 us, a sine with a click 1002 us, silence 272 us at P = 4096; 2277, 2307 and 597 us at
// P = 8192, against 2361 and 4890 us for copying the windows to the host.  (With the window fetched a word at a time and g's patterns
// read from LDS in every round: 1187, 1212, 305 and 3031, 3098, 737 us.)  The kernel's own time without the copy, and its phases
// alone: unmeasured.  100 VGPRs, 98 SGPRs, no scratch, no spills, no static LDS; 65536 + 9040 bytes of dynamic LDS at the cap.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_ring_view.hpp"
#include "wf_wave_reduce.hpp"

namespace wf {

struct ClickArgs {
    RingView rings;
    wf_hip_click *out;       // [count] the entry of stream `first` (16-byte aligned: a hipMalloc'ed block of 464-byte entries)
    double sample_rate;
    uint32_t first;          // first stream read
    uint32_t P;              // window: WF_CLICK_MIN_WINDOW <= P <= min(ring_cap, WF_HIP_CLICK_MAX_WINDOW)
};

constexpr uint32_t WF_CLICK_THREADS = 256;
constexpr uint32_t WF_CLICK_WAVES = WF_CLICK_THREADS / 64;
constexpr uint32_t WF_CLICK_MIN_WINDOW = 256;
constexpr uint32_t WF_CLICK_ORDER = WF_HIP_CLICK_ORDER;
constexpr uint32_t WF_CLICK_BLOCK = 256;                                                           // B
constexpr uint32_t WF_CLICK_MAX_BLOCKS = (WF_HIP_CLICK_MAX_WINDOW - WF_CLICK_ORDER) / WF_CLICK_BLOCK; // 31
constexpr uint32_t WF_CLICK_MAX_WORDS = WF_HIP_CLICK_MAX_WINDOW / 64;                              // of the hit bitmap
constexpr uint32_t WF_CLICK_CH_WORDS = sizeof(wf_hip_click_channel) / 4;
static_assert(sizeof(wf_hip_click_event) == 24 && sizeof(wf_hip_click_channel) == 224 && sizeof(wf_hip_click) == 464);
static_assert(offsetof(wf_hip_click_channel, ev) == 32 && offsetof(wf_hip_click, window) == 448);
static_assert(WF_CLICK_ORDER == 16 && WF_HIP_CLICK_GAP == 32 && WF_HIP_CLICK_MAX_EVENTS == 8);
static_assert(WF_CLICK_MAX_BLOCKS <= 32 && WF_CLICK_MAX_WORDS <= WF_CLICK_THREADS);
// (starts lie at least WF_HIP_CLICK_GAP + 1 frames apart: a thread per event)
static_assert((WF_HIP_CLICK_MAX_WINDOW - WF_CLICK_ORDER + WF_HIP_CLICK_GAP) / (WF_HIP_CLICK_GAP + 1) <= WF_CLICK_THREADS);

// what follows the window and the residual in dynamic LDS
struct ClickWork {
    double wsum[WF_CLICK_WAVES][WF_CLICK_ORDER + 1];   // the waves' sums of r
    double sb[32];                                     // s_b
    double pk[WF_CLICK_WAVES];                         // the waves' largest ratio
    double arg_v[2][WF_CLICK_WAVES];                   // the list's rounds, two buffers by turns
    unsigned long long hits[WF_CLICK_MAX_WORDS];       // frame n: bit n & 63 of word n / 64
    unsigned long long starts[WF_CLICK_MAX_WORDS];
    unsigned long long ev_max[WF_CLICK_THREADS];       // per event: the largest ratio, as the pattern of a positive double
    uint32_t ev_start[WF_CLICK_THREADS], ev_end[WF_CLICK_THREADS], ev_peak[WF_CLICK_THREADS];
    uint32_t pre[WF_CLICK_MAX_WORDS];                  // starts in the words below
    uint32_t med[32];                                  // m_b, as patterns
    uint32_t cnt[2][WF_CLICK_WAVES];                   // g's rounds, two buffers by turns
    uint32_t arg_k[2][WF_CLICK_WAVES];
    uint32_t amax[WF_CLICK_WAVES], bad[WF_CLICK_WAVES], nhit[WF_CLICK_WAVES];
    uint32_t image[WF_CLICK_CH_WORDS];                 // the channel as it leaves
};
static_assert(offsetof(ClickWork, hits) % 8 == 0 && offsetof(ClickWork, ev_max) % 8 == 0 && sizeof(ClickWork) == 9040);

// floats per LDS array: P rounded up to whole wavefronts
__host__ __device__ inline uint32_t click_lds_stride(uint32_t P) { return (P + 63u) & ~63u; }
__host__ __device__ inline size_t click_lds_bytes(uint32_t P) { return (size_t)2 * click_lds_stride(P) * sizeof(float) + sizeof(ClickWork); }

// e[n] = x[n] - sum_k a[k] x[n - k], k ascending, every product and every sum rounded on its own (n >= WF_CLICK_ORDER)
__device__ __forceinline__ double click_residual(const float *x, const double (&a)[WF_CLICK_ORDER + 1], uint32_t n)
{
#pragma clang fp contract(off)
    double acc = 0.0;
#pragma unroll
    for(uint32_t k = 1; k <= WF_CLICK_ORDER; ++k)
        acc = acc + a[k] * (double)x[n - k];
    return (double)x[n] - acc;
}

// Levinson-Durbin on r with r[0] (1 + 1e-9): a[1..16] and the error power E; every product and every sum rounded on its own
__device__ __forceinline__ void click_levinson(const double (&r)[WF_CLICK_ORDER + 1], double (&a)[WF_CLICK_ORDER + 1], double &E)
{
#pragma clang fp contract(off)
    E = r[0] * (1.0 + 1e-9);
    a[0] = 0.0;
#pragma unroll
    for(uint32_t i = 1; i <= WF_CLICK_ORDER; ++i) {
        double acc = r[i];
#pragma unroll
        for(uint32_t j = 1; j < i; ++j)
            acc = acc - a[j] * r[i - j];
        const double k = acc / E;
        double next[WF_CLICK_ORDER + 1];
#pragma unroll
        for(uint32_t j = 1; j < i; ++j)
            next[j] = a[j] - k * a[i - j];
#pragma unroll
        for(uint32_t j = 1; j < i; ++j)
            a[j] = next[j];
        a[i] = k;
        E = E * (1.0 - k * k);
    }
}

// the record of a channel that cannot be judged: all zero, the dB fields -INFINITY
__device__ __forceinline__ void click_leave_invalid(uint32_t *out_ch, uint32_t t)
{
    if(t < WF_CLICK_CH_WORDS)
        out_ch[t] = (t >= offsetof(wf_hip_click_channel, peak_db) / 4u && t <= offsetof(wf_hip_click_channel, prediction_gain_db) / 4u) ? 0xff800000u : 0u;
}

// grid: one workgroup per stream of [first, first + gridDim.x / CH) and captured channel; dynamic LDS: click_lds_bytes(P)
template<int CH>
__global__ __launch_bounds__(WF_CLICK_THREADS) void click_read_kernel(const ClickArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float click_lds[]; // x[S], d[S], then the ClickWork
    constexpr uint32_t p = WF_CLICK_ORDER;
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const uint32_t entry = blockIdx.x / (uint32_t)CH, c = blockIdx.x % (uint32_t)CH;
    const uint32_t stream = a.first + entry;
    const uint32_t P = a.P;
    const uint32_t S = click_lds_stride(P);
    float *x = click_lds;
    float *d = click_lds + S;
    uint32_t *xb = reinterpret_cast<uint32_t *>(x);
    const uint32_t *db = reinterpret_cast<const uint32_t *>(d);
    ClickWork &w = *reinterpret_cast<ClickWork *>(click_lds + 2u * (size_t)S);
    uint32_t *out_words = reinterpret_cast<uint32_t *>(a.out + entry);
    uint32_t *out_ch = out_words + c * WF_CLICK_CH_WORDS;

    // the tail, and the channel a capture of one does not have
    if(c == 0u) {
        if(t < 4u)
            out_words[offsetof(wf_hip_click, window) / 4u + t] = t == 0u ? P : t == 1u ? p : 0u;
        if(CH == 1 && t >= 64u && t < 64u + WF_CLICK_CH_WORDS)
            out_words[WF_CLICK_CH_WORDS + t - 64u] = 0u;
    }

    // load
    const uint32_t start = window_start(a.rings, stream, P);
    const uint32_t mask = a.rings.ring_cap - 1u;
    const uint32_t *ring = reinterpret_cast<const uint32_t *>(channel_ring(a.rings, stream, c, CH));
    uint32_t amax = 0u;
    bool bad = false;
    for(uint32_t base = t; base < S; base += 8u * WF_CLICK_THREADS) {
        uint32_t u[8]; // (eight fetches in flight before the first is used)
#pragma unroll
        for(uint32_t j = 0; j < 8u; ++j) {
            const uint32_t i = base + j * WF_CLICK_THREADS;
            u[j] = i < P ? ring[(start + i) & mask] : 0u;
        }
#pragma unroll
        for(uint32_t j = 0; j < 8u; ++j) {
            const uint32_t i = base + j * WF_CLICK_THREADS;
            const uint32_t m = u[j] & 0x7fffffffu;
            if(i < S)
                xb[i] = u[j];
            amax = amax > m ? amax : m;
            bad = bad || m >= 0x7f800000u;
        }
    }
    if(t < WF_CLICK_CH_WORDS)
        w.image[t] = 0u;
    amax = wave_max(amax);
    const bool wave_bad = __ballot(bad) != 0ull;
    if(lane == 0u) {
        w.amax[wave] = amax;
        w.bad[wave] = wave_bad ? 1u : 0u;
    }
    __syncthreads();
    uint32_t any_bad = 0u;
    amax = 0u;
    for(uint32_t k = 0; k < WF_CLICK_WAVES; ++k) {
        any_bad |= w.bad[k];
        amax = amax > w.amax[k] ? amax : w.amax[k];
    }
    if(__builtin_amdgcn_readfirstlane(any_bad) != 0u) { // (the same in every wave: no barrier is left behind)
        click_leave_invalid(out_ch, t);
        return;
    }
    const double A = (double)__uint_as_float(amax);

    // r[k], k = 0 .. p: the thread's strided partial in ascending n, the wave butterfly, the waves in order
    double r[p + 1];
    {
        double acc[p + 1];
#pragma unroll
        for(uint32_t k = 0; k <= p; ++k)
            acc[k] = 0.0;
        for(uint32_t n = t; n < P; n += WF_CLICK_THREADS) {
            const double xn = (double)x[n];
#pragma unroll
            for(uint32_t k = 0; k <= p; ++k) {
                const double xk = n >= k ? (double)x[n >= k ? n - k : 0u] : 0.0;
                acc[k] = __builtin_fma(xn, xk, acc[k]);
            }
        }
#pragma unroll
        for(uint32_t k = 0; k <= p; ++k) {
            const double s = wave_sum<WAVE_DOWN>(acc[k]);
            if(lane == 0u)
                w.wsum[wave][k] = s;
        }
        __syncthreads();
#pragma unroll
        for(uint32_t k = 0; k <= p; ++k)
            r[k] = ((w.wsum[0][k] + w.wsum[1][k]) + w.wsum[2][k]) + w.wsum[3][k];
    }
    if(__builtin_amdgcn_readfirstlane(r[0] == 0.0 ? 1u : 0u) != 0u) { // (every thread holds the same r)
        click_leave_invalid(out_ch, t);
        return;
    }

    double lp[p + 1], E;
    click_levinson(r, lp, E);

    // the residual
    for(uint32_t n = t; n < S; n += WF_CLICK_THREADS)
        d[n] = (n >= p && n < P) ? (float)__builtin_fabs(click_residual(x, lp, n)) : 0.0f;
    __syncthreads();

    // the block medians
    const uint32_t judged = P - p;
    const uint32_t nb = judged / WF_CLICK_BLOCK > 0u ? judged / WF_CLICK_BLOCK : 1u;
    // (a lone block has no neighbours: the medians of its two halves, behind it in med[], stand in for them at half their weight)
    const uint32_t half = p + judged / 2u;
    for(uint32_t b = wave; b < (nb == 1u ? 3u : nb); b += WF_CLICK_WAVES) {
        const uint32_t lo = nb == 1u ? (b == 2u ? half : p) : p + b * WF_CLICK_BLOCK;
        const uint32_t len = (nb == 1u ? (b == 1u ? half : P) : b == nb - 1u ? P : lo + WF_CLICK_BLOCK) - lo; // <= 511
        uint32_t v[8];
#pragma unroll
        for(uint32_t j = 0; j < 8u; ++j) {
            const uint32_t i = lane + 64u * j;
            v[j] = i < len ? db[lo + i] : 0xffffffffu; // (above every pattern of a |e|)
        }
        uint32_t rank = len / 2u, prefix = 0u;
        for(int bit = 30; bit >= 0; --bit) {
            uint32_t zeros = 0u;
#pragma unroll
            for(uint32_t j = 0; j < 8u; ++j)
                zeros += (uint32_t)__popcll(__ballot(((v[j] ^ prefix) >> bit) == 0u));
            if(rank >= zeros) {
                rank -= zeros;
                prefix |= 1u << bit;
            }
        }
        if(lane == 0u)
            w.med[b] = prefix;
    }

    // g: the same over all judged frames
    uint32_t g_bits = 0u;
    {
        uint32_t rank = judged / 2u;
        uint32_t v[WF_CLICK_MAX_WORDS / WF_CLICK_WAVES]; // the thread's patterns stay in registers over the 31 rounds
#pragma unroll
        for(uint32_t j = 0; j < WF_CLICK_MAX_WORDS / WF_CLICK_WAVES; ++j) {
            const uint32_t n = 64u * wave + j * WF_CLICK_THREADS + lane;
            v[j] = (n >= p && n < P) ? db[n] : 0xffffffffu;
        }
        for(int bit = 30; bit >= 0; --bit) {
            uint32_t zeros = 0u;
#pragma unroll
            for(uint32_t j = 0; j < WF_CLICK_MAX_WORDS / WF_CLICK_WAVES; ++j)
                if(64u * wave + j * WF_CLICK_THREADS < S) // (wave-uniform; a pattern beyond P counts nowhere either way)
                    zeros += (uint32_t)__popcll(__ballot(((v[j] ^ g_bits) >> bit) == 0u));
            uint32_t *cnt = w.cnt[bit & 1];
            if(lane == 0u)
                cnt[wave] = zeros;
            __syncthreads();
            const uint32_t all = __builtin_amdgcn_readfirstlane(cnt[0] + cnt[1] + cnt[2] + cnt[3]);
            if(rank >= all) {
                rank -= all;
                g_bits |= 1u << bit;
            }
        }
    }
    const double g = (double)__uint_as_float(g_bits);

    // s_b (the medians are behind g's barriers)
    if(t < nb) {
        double m = (double)__uint_as_float(w.med[t]);
        if(t > 0u)
            m = __builtin_fmax(m, (double)__uint_as_float(w.med[t - 1u]));
        if(t + 1u < nb)
            m = __builtin_fmax(m, (double)__uint_as_float(w.med[t + 1u]));
        if(nb == 1u)
            m = __builtin_fmax(m, 0.5 * (double)__builtin_fmaxf(__uint_as_float(w.med[1]), __uint_as_float(w.med[2])));
        m = __builtin_fmax(m, 0.25 * g);
        m = __builtin_fmax(m, 0x1p-24 * A);
        w.sb[t] = 1.4826 * m;
    }
    w.ev_max[t] = 0ull;
    w.ev_start[t] = 0u;
    w.ev_end[t] = 0u;
    w.ev_peak[t] = 0xffffffffu;
    __syncthreads();

    // the hits
    const uint32_t words = S / 64u;
    auto ratio_of = [&](uint32_t n) {
        const uint32_t b = (n - p) / WF_CLICK_BLOCK;
        return (double)d[n] / w.sb[b < nb ? b : nb - 1u];
    };
    {
        double pk = 0.0;
        uint32_t nhit = 0u;
        for(uint32_t base = 64u * wave; base < S; base += WF_CLICK_THREADS) {
            const uint32_t n = base + lane;
            const double ratio = (n >= p && n < P) ? ratio_of(n) : 0.0;
            const unsigned long long H = __ballot(ratio > WF_HIP_CLICK_THRESHOLD);
            if(lane == 0u)
                w.hits[base / 64u] = H;
            nhit += (uint32_t)__popcll(H);
            pk = __builtin_fmax(pk, ratio);
        }
        pk = wave_max(pk);
        if(lane == 0u) {
            w.pk[wave] = pk;
            w.nhit[wave] = nhit;
        }
    }
    __syncthreads();
    // a hit with no hit in the WF_HIP_CLICK_GAP frames below it starts an event
    if(t < words) {
        const unsigned long long H = w.hits[t], below = t > 0u ? w.hits[t - 1u] : 0ull;
        unsigned long long shadow = 0ull;
#pragma unroll
        for(uint32_t j = 1; j <= WF_HIP_CLICK_GAP; ++j)
            shadow |= (H << j) | (below >> (64u - j));
        w.starts[t] = H & ~shadow;
    }
    __syncthreads();
    if(t < words) {
        uint32_t n = 0u;
        for(uint32_t k = 0; k < t; ++k)
            n += (uint32_t)__popcll(w.starts[k]);
        w.pre[t] = n;
    }
    __syncthreads();
    const uint32_t events = __builtin_amdgcn_readfirstlane(w.pre[words - 1u] + (uint32_t)__popcll(w.starts[words - 1u]));
    const uint32_t hit_frames = w.nhit[0] + w.nhit[1] + w.nhit[2] + w.nhit[3];
    const double top = __builtin_fmax(__builtin_fmax(w.pk[0], w.pk[1]), __builtin_fmax(w.pk[2], w.pk[3]));

    // per event: the largest ratio and the last hit, then the first hit of that ratio
    for(int pass = 0; pass < 2; ++pass) {
        for(uint32_t base = 64u * wave; base < S; base += WF_CLICK_THREADS) {
            const uint32_t word = base / 64u;
            const unsigned long long H = w.hits[word];
            if(__builtin_amdgcn_readfirstlane((uint32_t)(H != 0ull)) == 0u)
                continue;
            if((H >> lane) & 1ull) {
                const uint32_t n = base + lane;
                const unsigned long long Sw = w.starts[word];
                const uint32_t ev = w.pre[word] + (uint32_t)__popcll(Sw & ((2ull << lane) - 1ull)) - 1u; // < events <= 248
                const unsigned long long rb = (unsigned long long)__double_as_longlong(ratio_of(n));
                if(pass == 0) {
                    __hip_atomic_fetch_max(&w.ev_max[ev], rb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_max(&w.ev_end[ev], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if((Sw >> lane) & 1ull)
                        w.ev_start[ev] = n;
                } else if(rb == w.ev_max[ev])
                    __hip_atomic_fetch_min(&w.ev_peak[ev], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __syncthreads();
    }

    // the list: strength_db descending, then start ascending
    const uint32_t listed = events < WF_HIP_CLICK_MAX_EVENTS ? events : WF_HIP_CLICK_MAX_EVENTS;
    float strength = 0.0f;
    double mine = -INFINITY;
    uint32_t my_start = 0xffffffffu;
    if(t < events) {
        strength = (float)(20.0 * log10(__longlong_as_double((long long)w.ev_max[t])));
        mine = (double)strength;
        my_start = w.ev_start[t];
    }
    for(uint32_t round = 0; round < listed; ++round) {
        double best = mine;
        uint32_t kbest = my_start;
        wave_argmax(best, kbest);
        if(lane == 0u) {
            w.arg_v[round & 1u][wave] = best;
            w.arg_k[round & 1u][wave] = kbest;
        }
        __syncthreads();
        best = w.arg_v[round & 1u][0];
        kbest = w.arg_k[round & 1u][0];
#pragma unroll
        for(uint32_t k = 1; k < WF_CLICK_WAVES; ++k)
            argmax_better(best, kbest, w.arg_v[round & 1u][k], w.arg_k[round & 1u][k]);
        if(t < events && my_start == kbest && mine == best) { // (starts differ: one thread)
            const uint32_t peak = w.ev_peak[t];
            uint32_t *ev = w.image + offsetof(wf_hip_click_channel, ev) / 4u + round * (uint32_t)(sizeof(wf_hip_click_event) / 4u);
            ev[0] = my_start;
            ev[1] = w.ev_end[t] - my_start + 1u;
            ev[2] = peak;
            ev[3] = start + my_start;
            ev[4] = __float_as_uint(strength);
            ev[5] = __float_as_uint((float)click_residual(x, lp, peak));
            mine = -INFINITY;
            my_start = 0xffffffffu;
        }
    }
    if(t == 0u) {
        w.image[0] = 1u;
        w.image[1] = events;
        w.image[2] = hit_frames;
        w.image[3] = listed;
        w.image[4] = __float_as_uint((float)((double)events * a.sample_rate / (double)judged));
        w.image[5] = __float_as_uint((float)(20.0 * log10(top)));
        w.image[6] = __float_as_uint((float)(20.0 * log10(1.4826 * g)));
        w.image[7] = __float_as_uint((float)(10.0 * log10(r[0] / E)));
    }
    __syncthreads();
    if(t < WF_CLICK_CH_WORDS)
        out_ch[t] = w.image[t];
}

} // namespace wf
