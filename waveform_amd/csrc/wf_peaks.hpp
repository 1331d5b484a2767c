// wf_peaks.hpp -- gfx950 read kernel of WF_HIP_OUT_PEAKS (device code only; hipcc; included by wf_hip_measure.hip alone).
//
// Not in the reference: the WF_HIP_MAX_PEAKS strongest local maxima of every m_decibels row, with the parabola through
// each maximum and its two neighbours (the definition is in include/wf_hip.h).  wf_hip_read launches it on the handle's
// stream, behind every tick issued so far, and copies the result back; nothing runs while the output is not read.
//
// One wavefront per row.  The row streams through in chunks of 64 x float4 (256 bins), WF_PEAKS_GROUP chunks loaded
// together and the next group in flight while the current one is searched.  A bin's neighbours inside the chunk come from
// the lanes beside it (shuffles); the chunk boundaries take the last bin of the previous chunk and the first of the next.
// Every lane keeps its own 8 best candidates in registers as 64-bit keys -- order-preserving float bits of the value in
// the high word, ~k in the low word, so a larger key is the stronger peak and, among equal values, the lower bin -- and
// 8 rounds of a wave-wide 64-bit max merge them.  No scratch, no LDS, no atomics: the output is a function of the row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_wave_reduce.hpp"

namespace wf {

struct PeaksArgs {
    const float *rows;  // the first row read: [n_rows][M]
    wf_hip_peaks *out;  // [n_rows]
    uint32_t n_rows;
    uint32_t M;         // bins per row (fft_size / 2; a multiple of 8)
    float floor_db;     // cfg.floor_db: a candidate lies above it
    double hz_per_bin;  // sample_rate / fft_size
};

constexpr int WF_PEAKS_GROUP = 3;    // chunks loaded together (3 KiB per wavefront in flight; 4 would spill at 8 waves per SIMD)
constexpr int WF_PEAKS_WAVES = 4;    // rows per workgroup

__device__ __forceinline__ uint32_t peaks_ordered(float v)
{
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float peaks_unordered(uint32_t u)
{
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// the key of bin k (0: not a candidate); keys of candidates are never 0 (~k of k < 2^31 sets the low word's top bit)
__device__ __forceinline__ uint64_t peaks_key(float prev, float v, float next, uint32_t k, uint32_t M, float floor_db)
{
    const bool cand = (k - 1u) < (M - 2u) && v > prev && v >= next && v > floor_db;
    return cand ? ((uint64_t)peaks_ordered(v + 0.0f) << 32) | (uint32_t)~k : 0ull; // (+ 0.0f: -0 ranks as the equal +0)
}

// sorted descending; x enters at its place and the smallest drops out
__device__ __forceinline__ void peaks_insert(uint64_t (&best)[WF_HIP_MAX_PEAKS], uint64_t x)
{
#pragma unroll
    for(int i = 0; i < WF_HIP_MAX_PEAKS; ++i) {
        const bool gt = x > best[i];
        const uint64_t lo = gt ? best[i] : x;
        best[i] = gt ? x : best[i];
        x = lo;
    }
}

__device__ __forceinline__ float peaks_lane_bits(float v, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

__global__ __launch_bounds__(64 * WF_PEAKS_WAVES, 8) void peaks_read_kernel(PeaksArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t row = blockIdx.x * WF_PEAKS_WAVES + (threadIdx.x >> 6);
    if(row >= a.n_rows)
        return; // (wave-uniform)
    const float *d = a.rows + (size_t)row * a.M;
    const float4 *d4 = reinterpret_cast<const float4 *>(d);
    const uint32_t n4 = a.M / 4u;
    const uint32_t nch = (n4 + 63u) / 64u;

    uint64_t best[WF_HIP_MAX_PEAKS];
#pragma unroll
    for(int i = 0; i < WF_HIP_MAX_PEAKS; ++i)
        best[i] = 0ull;

    float4 cur[WF_PEAKS_GROUP], nxt[WF_PEAKS_GROUP];
#pragma unroll
    for(int u = 0; u < WF_PEAKS_GROUP; ++u) {
        const uint32_t i = (uint32_t)u * 64u + lane;
        cur[u] = i < n4 ? d4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float carry = 0.f; // the bin before the chunk (chunk 0: bin -1, never a neighbour of a candidate)
    for(uint32_t g = 0; g < nch; g += WF_PEAKS_GROUP) {
#pragma unroll
        for(int u = 0; u < WF_PEAKS_GROUP; ++u) {
            const uint32_t i = (g + WF_PEAKS_GROUP + (uint32_t)u) * 64u + lane;
            nxt[u] = i < n4 ? d4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for(int u = 0; u < WF_PEAKS_GROUP; ++u) {
            if(g + (uint32_t)u >= nch)
                break; // (wave-uniform)
            const float4 v = cur[u];
            // the first bin of the next chunk (past the row's end it is never a neighbour of a candidate)
            const float after = peaks_lane_bits(u + 1 < WF_PEAKS_GROUP ? cur[(u + 1) % WF_PEAKS_GROUP].x : nxt[0].x, 0);
            float left = __shfl_up(v.w, 1, 64);
            float right = __shfl_down(v.x, 1, 64);
            if(lane == 0)
                left = carry;
            if(lane == 63)
                right = after;
            const uint32_t k = (g + (uint32_t)u) * 256u + lane * 4u;
            // two candidates are never adjacent, so each pair of bins holds at most one of them
            const uint64_t k01 = peaks_key(left, v.x, v.y, k, a.M, a.floor_db) | peaks_key(v.x, v.y, v.z, k + 1u, a.M, a.floor_db);
            const uint64_t k23 = peaks_key(v.y, v.z, v.w, k + 2u, a.M, a.floor_db) | peaks_key(v.z, v.w, right, k + 3u, a.M, a.floor_db);
            peaks_insert(best, k01);
            peaks_insert(best, k23);
            carry = peaks_lane_bits(v.w, 63);
        }
#pragma unroll
        for(int u = 0; u < WF_PEAKS_GROUP; ++u)
            cur[u] = nxt[u];
    }

    // merge: round r takes the largest head of the 64 lists; lane r keeps it
    uint64_t mine = 0ull;
    uint32_t count = 0;
#pragma unroll
    for(int r = 0; r < WF_HIP_MAX_PEAKS; ++r) {
        const uint64_t m = wave_max(best[0]);
        if(m == 0ull)
            break; // (wave-uniform)
        if(lane == (uint32_t)r)
            mine = m;
        ++count;
        if(best[0] == m) { // (one lane: the keys of different bins differ)
#pragma unroll
            for(int i = 0; i + 1 < WF_HIP_MAX_PEAKS; ++i)
                best[i] = best[i + 1];
            best[WF_HIP_MAX_PEAKS - 1] = 0ull;
        }
    }

    wf_hip_peaks *o = a.out + row;
    if(lane < WF_HIP_MAX_PEAKS) {
        float hz = 0.f, db = -INFINITY;
        if(lane < count) {
            // the parabola through the three dB values, in float64 (exact differences of the float32 inputs)
            const uint32_t k = ~(uint32_t)mine;
            const double b = peaks_unordered((uint32_t)(mine >> 32));
            const double l = d[k - 1], r = d[k + 1];
            const double den = (l - b) + (r - b); // < 0: l < b and r <= b
            const double p = 0.5 * (l - r) / den;
            hz = (float)(((double)k + p) * a.hz_per_bin);
            db = (float)(b - 0.25 * (l - r) * p);
        }
        o->peak[lane].hz = hz;
        o->peak[lane].db = db;
    }
    if(lane == 0) {
        o->count = count;
        o->reserved = 0u;
    }
}

} // namespace wf
