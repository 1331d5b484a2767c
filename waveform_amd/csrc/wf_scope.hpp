// wf_scope.hpp -- gfx950 read kernel of WF_HIP_OUT_SCOPE (device code only; hipcc; included by wf_hip_measure.hip alone).
//
// Not in the reference: a triggered oscilloscope trace, the smallest and largest sample per display column of a view of V = P / 2
// frames that starts at the last rising 50 % crossing of the newest P = min(fft_size, 8192) frames in each captured channel's ring
// (the definition is in include/wf_hip.h, "oscilloscope").  wf_hip_read launches it on the handle's stream, behind every push
// issued so far, and copies the result back; nothing runs while the output is not read.
//
// One workgroup of WF_SCOPE_THREADS per stream; the ring is read once.
//   stage    wf_ring_stage.hpp's ring_stage_window<CH>: the at most two contiguous runs of the window into dynamic LDS, 16-B words
//            over the aligned body, four per channel in flight per lane, element by element over the at most 3 frames around it;
//            frame i of channel c at x[c][o + i], o = (window start) & 3.
//   level    t = x_0 + x_1 in float64 (exact), its minimum and maximum by a butterfly over the wavefront and the waves' partials
//            in wave order; level and hysteresis from them, one IEEE operation and one exact scaling each.
//   scan     frames 0 .. P - V in groups of 64, a wavefront per group: two ballots give the group's LOW and HIGH masks L and H.
//            With C = L | H the triggers of a group are (((L << 1) | armed_in) + ~C) & H -- the carry of the addition runs through
//            the frames of neither class to the next classified one -- and armed_in of group g is whether the last classified frame
//            of the nearest earlier group that has one is LOW: thread g finds that group with a count of leading zeros over the ballots
//            of the groups' summaries.  The two largest triggers are the two highest bits of the last non-empty trigger masks.
//   trace    sixteen lanes per column (a column is at most 16 frames), sixteen columns per pass: consecutive lanes read consecutive
//            frames, a butterfly over the sixteen, and the result goes into the entry's image in LDS, which was zeroed before -- the
//            columns past K and the channel that was not captured read 0 without a memset per read.  The image leaves as 16-B words.
// No atomics, no static LDS, no scratch; nothing depends on timing, so the same ring contents read bit-identically.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_ring_view.hpp"
#include "wf_ring_stage.hpp"
#include "wf_wave_reduce.hpp"

namespace wf {

struct ScopeArgs {
    RingView rings;          // (ring_cap a multiple of 4)
    wf_hip_scope *out;       // [count] the entry of stream `first` (16-byte aligned: a hipMalloc'ed block of 4128-byte entries)
    uint32_t first;          // first stream read
    uint32_t P, V, K;        // window <= min(ring_cap, WF_HIP_SCOPE_MAX_WINDOW), view P / 2, columns min(WF_HIP_SCOPE_COLUMNS, V) >= 1
};

constexpr uint32_t WF_SCOPE_THREADS = 256;
constexpr uint32_t WF_SCOPE_WAVES = WF_SCOPE_THREADS / 64;
constexpr uint32_t WF_SCOPE_UNROLL = 4;       // float4 loads per channel in flight per lane
constexpr int WF_SCOPE_OCC = 4;               // waves per SIMD the registers allow; the LDS allows two workgroups per CU at the cap
constexpr uint32_t WF_SCOPE_LANES = 16;       // lanes per column: ceil(V / K) <= 16
constexpr uint32_t WF_SCOPE_MAX_GROUPS = 128; // 64-frame groups of frames 0 .. P - V: at most 4097 frames, 65 groups
static_assert(WF_HIP_SCOPE_MAX_WINDOW - WF_HIP_SCOPE_MAX_WINDOW / 2 + 1 <= 64 * WF_SCOPE_MAX_GROUPS);
static_assert((WF_HIP_SCOPE_MAX_WINDOW / 2 + WF_HIP_SCOPE_COLUMNS - 1) / WF_HIP_SCOPE_COLUMNS <= WF_SCOPE_LANES);
static_assert(sizeof(wf_hip_scope) % 16 == 0 && WF_SCOPE_MAX_GROUPS <= WF_SCOPE_THREADS);

// what follows the staged windows in dynamic LDS
struct ScopeWork {
    uint32_t image[sizeof(wf_hip_scope) / 4]; // the entry as it leaves
    unsigned long long low[WF_SCOPE_MAX_GROUPS], high[WF_SCOPE_MAX_GROUPS], trig[WF_SCOPE_MAX_GROUPS];
    double tmin[WF_SCOPE_WAVES], tmax[WF_SCOPE_WAVES];
    unsigned long long some[2], last_low[2], fired[2]; // per 64 groups: has classified frames, the last of them is LOW, has triggers
};
static_assert(offsetof(ScopeWork, low) % 16 == 0);

__host__ __device__ constexpr size_t scope_lds_bytes(uint32_t channels, uint32_t P)
{
    return (size_t)channels * ring_stage_stride(P) * sizeof(float) + sizeof(ScopeWork);
}
static_assert(2 * scope_lds_bytes(2, WF_HIP_SCOPE_MAX_WINDOW) <= WF_LDS_PER_CU, "two workgroups to a CU at the cap");

// index of the highest set bit of a mask that has one
__device__ __forceinline__ uint32_t scope_top(unsigned long long m) { return 63u - (uint32_t)__builtin_clzll(m); }

// grid: one workgroup per stream of [first, first + gridDim.x); dynamic LDS: scope_lds_bytes(CH, P)
template<int CH>
__global__ __launch_bounds__(WF_SCOPE_THREADS, WF_SCOPE_OCC) void scope_read_kernel(const ScopeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float scope_x[]; // [CH][S], then the ScopeWork
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const uint32_t stream = a.first + blockIdx.x;
    const uint32_t P = a.P, V = a.V, K = a.K;
    const uint32_t S = ring_stage_stride(P);
    ScopeWork &w = *reinterpret_cast<ScopeWork *>(scope_x + (size_t)CH * S);
    const uint32_t ring_cap = a.rings.ring_cap;
    const uint32_t s = window_start(a.rings, stream, P) & (ring_cap - 1u);
    const uint32_t o = s & 3u;
    const float *r0 = channel_ring(a.rings, stream, 0, CH);
    const float *r1 = CH == 2 ? channel_ring(a.rings, stream, 1, CH) : r0;
    const float *x0 = scope_x + o, *x1 = x0 + S; // x_c[i]

    ring_stage_window<CH, WF_SCOPE_THREADS, WF_SCOPE_UNROLL>(scope_x, S, r0, r1, s, P, ring_cap);
    for(uint32_t i = t; i < sizeof(wf_hip_scope) / 4u; i += WF_SCOPE_THREADS)
        w.image[i] = 0u;
    __syncthreads();

    // level and hysteresis
    double tmin, tmax;
    {
        const double t0 = CH == 2 ? (double)x0[0] + (double)x1[0] : (double)x0[0];
        tmin = tmax = t0;
        for(uint32_t i = t; i < P; i += WF_SCOPE_THREADS) {
            const double v = CH == 2 ? (double)x0[i] + (double)x1[i] : (double)x0[i];
            tmin = __builtin_fmin(tmin, v);
            tmax = __builtin_fmax(tmax, v);
        }
        wave_butterfly([&](auto other) {
            tmin = __builtin_fmin(tmin, other(tmin));
            tmax = __builtin_fmax(tmax, other(tmax));
        });
        if(lane == 0) {
            w.tmin[wave] = tmin;
            w.tmax[wave] = tmax;
        }
        __syncthreads();
        tmin = w.tmin[0];
        tmax = w.tmax[0];
        for(uint32_t k = 1; k < WF_SCOPE_WAVES; ++k) {
            tmin = __builtin_fmin(tmin, w.tmin[k]);
            tmax = __builtin_fmax(tmax, w.tmax[k]);
        }
    }
    const double level = (tmax + tmin) * 0.5;
    const double hyst = (tmax - tmin) * 0.125;
    const bool flat = tmax == tmin;

    // the classes of frames 0 .. P - V, a group of 64 per wavefront and step
    const uint32_t last = P - V;
    const uint32_t groups = last / 64u + 1u;
    for(uint32_t g = wave; g < groups; g += WF_SCOPE_WAVES) {
        const uint32_t i = 64u * g + lane;
        bool lo = false, hi = false;
        if(i <= last && !flat) {
            const double tv = CH == 2 ? (double)x0[i] + (double)x1[i] : (double)x0[i];
            const double u = tv - level;
            lo = u <= -hyst;
            hi = u >= 0.0;
        }
        const unsigned long long L = __ballot(lo), H = __ballot(hi);
        if(lane == 0) {
            w.low[g] = L;
            w.high[g] = H;
        }
    }
    __syncthreads();
    // thread g takes group g: first the groups' summaries ...
    unsigned long long L = 0, H = 0;
    if(t < WF_SCOPE_MAX_GROUPS) { // (whole wavefronts)
        if(t < groups) {
            L = w.low[t];
            H = w.high[t];
        }
        const unsigned long long C = L | H;
        const unsigned long long some = __ballot(C != 0), last_low = __ballot(C != 0 && ((L >> scope_top(C | 1ull)) & 1ull) != 0);
        if(lane == 0) {
            w.some[wave] = some;
            w.last_low[wave] = last_low;
        }
    }
    __syncthreads();
    // ... then whether it starts armed, and its triggers
    if(t < WF_SCOPE_MAX_GROUPS) {
        const unsigned long long below = (1ull << lane) - 1ull;
        bool armed = false;
        if(w.some[wave] & below)
            armed = ((w.last_low[wave] >> scope_top(w.some[wave] & below)) & 1ull) != 0;
        else if(wave == 1u && w.some[0] != 0)
            armed = ((w.last_low[0] >> scope_top(w.some[0])) & 1ull) != 0;
        const unsigned long long T = (((L << 1) | (armed ? 1ull : 0ull)) + ~(L | H)) & H;
        w.trig[t] = T;
        const unsigned long long fired = __ballot(T != 0);
        if(lane == 0)
            w.fired[wave] = fired;
    }
    __syncthreads();
    // the two largest triggers (every thread, the same for all)
    uint32_t start = last, triggered = 0u, period = 0u;
    float frac = 0.f;
    {
        unsigned long long f1 = w.fired[1], f0 = w.fired[0];
        if((f1 | f0) != 0) {
            uint32_t g = f1 != 0 ? 64u + scope_top(f1) : scope_top(f0);
            unsigned long long T = w.trig[g];
            start = 64u * g + scope_top(T);
            triggered = 1u;
            T &= ~(1ull << scope_top(T));
            if(T == 0) { // the trigger before lies in an earlier group, if there is one
                if(g >= 64u)
                    f1 &= ~(1ull << (g - 64u));
                else
                    f0 &= ~(1ull << g);
                if((f1 | f0) != 0) {
                    g = f1 != 0 ? 64u + scope_top(f1) : scope_top(f0);
                    T = w.trig[g];
                }
            }
            if(T != 0)
                period = start - (64u * g + scope_top(T));
            const double ta = CH == 2 ? (double)x0[start - 1u] + (double)x1[start - 1u] : (double)x0[start - 1u]; // (start >= 1)
            const double tb = CH == 2 ? (double)x0[start] + (double)x1[start] : (double)x0[start];
            const double ua = ta - level, ub = tb - level;
            const double den = ua - ub;
            frac = (float)(ua / den);
        }
    }

    // the trace: column c = 16 pass + t / 16 takes view frames [c V / K, (c + 1) V / K), lane r of its sixteen the r-th of them
    {
        const uint32_t r = t & (WF_SCOPE_LANES - 1u);
        constexpr uint32_t PER_PASS = WF_SCOPE_THREADS / WF_SCOPE_LANES;
        for(uint32_t c = t / WF_SCOPE_LANES; c < ((K + PER_PASS - 1u) & ~(PER_PASS - 1u)); c += PER_PASS) {
            const uint32_t cc = c < K ? c : K - 1u; // (whole wavefronts in the butterfly)
            const uint32_t f0 = cc * V / K, f1 = (cc + 1u) * V / K; // f0 < f1 <= f0 + 16 (K V <= 2^20)
            const uint32_t f = start + (f0 + r < f1 ? f0 + r : f0);
#pragma unroll
            for(int ch = 0; ch < CH; ++ch) {
                float lo = (ch ? x1 : x0)[f], hi = lo;
                wave_butterfly<WAVE_DOWN, WF_SCOPE_LANES>([&](auto other) {
                    lo = __builtin_fminf(lo, other(lo));
                    hi = __builtin_fmaxf(hi, other(hi));
                });
                if(r == 0u && c < K) {
                    w.image[(0 + ch) * WF_HIP_SCOPE_COLUMNS + c] = __float_as_uint(lo);
                    w.image[(2 + ch) * WF_HIP_SCOPE_COLUMNS + c] = __float_as_uint(hi);
                }
            }
        }
    }
    if(t < 8u) {
        const uint32_t word = t == 0u ? P : t == 1u ? V : t == 2u ? K : t == 3u ? start : t == 4u ? triggered : t == 5u ? period
                            : t == 6u ? __float_as_uint(frac) : 0u;
        w.image[offsetof(wf_hip_scope, window) / 4u + t] = word;
    }
    __syncthreads();
    const uint4 *src = reinterpret_cast<const uint4 *>(w.image);
    uint4 *dst = reinterpret_cast<uint4 *>(a.out + blockIdx.x);
    for(uint32_t i = t; i < sizeof(wf_hip_scope) / 16u; i += WF_SCOPE_THREADS)
        dst[i] = src[i];
}

} // namespace wf
