// wf_ring_stage.hpp -- a window of the audio rings as contiguous runs, and its copy into LDS (device code only; hipcc).  Next to
// wf_ring_view.hpp, which says where a window starts; used by wf_scope.hpp, wf_gonio.hpp and wf_bits.hpp.  (wf_signal.hpp walks the
// same two runs and sums them where these stage them; its loop is its own.)
//
// A window of P <= ring_cap frames that starts at ring position s is at most two contiguous runs of the ring, [s, min(s + P, cap))
// and [0, s + P - cap): the wrap splits it.  Each run is staged in 16-B loads over its 16-B aligned body, UNROLL per channel in
// flight per lane, and element by element over the at most 3 frames before and after the body (a ragged push leaves the window at
// any alignment; every ring starts 16-B aligned: ring_stride is a multiple of 4 floats).  Frame i of channel c lands at
// x[c S + o + i], o = s & 3: the ring's 16-B groups stay 16-B groups in LDS in both runs (the capacity is a multiple of 4), so the
// body is stored as 16-B words.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace wf {

// the LDS of a gfx950 compute unit: what the staged windows and a kernel's working set behind them are sized against
constexpr size_t WF_LDS_PER_CU = 160 * 1024;

// floats between the channels' windows in LDS: P + 3 (the window starts up to 3 floats in), rounded up to 16 bytes
__host__ __device__ constexpr uint32_t ring_stage_stride(uint32_t P) { return (P + 6u) & ~3u; }

// ring positions [b0, b1) of every channel, b0 <= b1 <= ring_cap, to LDS index (ring position + d), d + b0 a multiple of 4 wherever
// b0 is; every one of the workgroup's THREADS threads calls it
template<int CH, uint32_t THREADS, uint32_t UNROLL>
__device__ __forceinline__ void ring_stage(float *x, uint32_t S, const float *r0, const float *r1, uint32_t b0, uint32_t b1, uint32_t d)
{
    const uint32_t t = threadIdx.x;
    const uint32_t h = ((b0 + 3u) & ~3u) < b1 ? ((b0 + 3u) & ~3u) : b1; // end of the head
    const uint32_t e = (b1 & ~3u) > h ? (b1 & ~3u) : h;                 // end of the body
    const uint32_t nh = h - b0, nt = b1 - e;                            // at most 3 each
    static_assert(THREADS >= 6, "a thread per frame of the head and the tail");
    if(t < nh) {
        x[b0 + t + d] = r0[b0 + t];
        if constexpr(CH == 2)
            x[S + b0 + t + d] = r1[b0 + t];
    } else if(t - nh < nt) {
        x[e + t - nh + d] = r0[e + t - nh];
        if constexpr(CH == 2)
            x[S + e + t - nh + d] = r1[e + t - nh];
    }
    const float4 *p0 = reinterpret_cast<const float4 *>(r0 + h);
    const float4 *p1 = reinterpret_cast<const float4 *>(r1 + h);
    float4 *q0 = reinterpret_cast<float4 *>(x + (h + d)); // (h + d: a multiple of 4, as S is)
    float4 *q1 = reinterpret_cast<float4 *>(x + S + (h + d));
    const uint32_t n4 = (e - h) / 4u;
    constexpr uint32_t T = THREADS, U = UNROLL;
    uint32_t i = t;
    for(; i + (U - 1u) * T < n4; i += U * T) {
        float4 l[U], r[U];
#pragma unroll
        for(uint32_t u = 0; u < U; ++u) {
            l[u] = p0[i + u * T];
            if constexpr(CH == 2)
                r[u] = p1[i + u * T];
        }
#pragma unroll
        for(uint32_t u = 0; u < U; ++u) {
            q0[i + u * T] = l[u];
            if constexpr(CH == 2)
                q1[i + u * T] = r[u];
        }
    }
    for(; i < n4; i += T) {
        q0[i] = p0[i];
        if constexpr(CH == 2)
            q1[i] = p1[i];
    }
}

// the window of P frames at ring position s of every channel into x, S = ring_stage_stride(P) floats per channel (r1 is unread
// with CH == 1); a barrier between it and the first read of x is the caller's
template<int CH, uint32_t THREADS, uint32_t UNROLL>
__device__ __forceinline__ void ring_stage_window(float *x, uint32_t S, const float *r0, const float *r1, uint32_t s, uint32_t P, uint32_t ring_cap)
{
    const uint32_t o = s & 3u;
    const uint32_t end = s + P; // <= 2 ring_cap
    ring_stage<CH, THREADS, UNROLL>(x, S, r0, r1, s, end < ring_cap ? end : ring_cap, o - s);
    if(end > ring_cap)
        ring_stage<CH, THREADS, UNROLL>(x, S, r0, r1, 0u, end - ring_cap, o + (ring_cap - s));
}

} // namespace wf
