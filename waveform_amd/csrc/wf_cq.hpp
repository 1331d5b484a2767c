// wf_cq.hpp -- gfx950 read kernel of WF_HIP_OUT_CQ (device code only; hipcc; included by wf_hip_measure.hip alone).
//
// Not in the reference: a constant-Q spectrum, one level per semitone from C0 to B9, of the newest frames in each captured
// channel's ring (the definition is in include/wf_hip.h, "constant-Q spectrum").  Bin b correlates the newest L_b frames with a
// Hann-windowed carrier at f_b, L_b = Q periods: long in the bass, short in the treble.  wf_hip_read launches it on the handle's
// stream, behind every push issued so far, and copies the result back; nothing runs while the output is not read.
//
// One workgroup of WF_CQ_THREADS per stream.
//   stage   the newest Lmax frames of every channel go from the ring into dynamic LDS as float32, element i = frame
//           wpos - Lmax + i (the wrap and any alignment a ragged push left are taken by the index mask), CH * Lmax * 4 bytes:
//           128 KB at the cap with two channels, so one workgroup has a CU to itself.
//   bins    a wavefront takes a whole bin, both channels at once; which bins in which order is the host's table (`sched`), made
//           so that the sixteen waves' sums of ceil(L_b / 64) are level.  Lane l takes n = l, l + 64, ... of the bin's window
//           (consecutive lanes on consecutive floats: LDS reads without bank conflicts).  The carrier e^(-j w_b n) and the
//           window's phasor e^(j 2 pi n / L_b) start from the host's exact float64 value of n = l and advance by one complex
//           multiplication with the host's e^(.. 64) per iteration: at most 256 steps from an exact value.  Per iteration
//           w = 0.5 - 0.5 Re(phasor), p = w carrier, and four fused multiply-adds into S(l), S(r).
//   finish  the fixed butterfly of wf_wave_reduce.hpp over the four sums; lane c writes 20 log10(4 |S_c| / L_b) of channel c.
// Sixteen waves give every SIMD four rotation chains to interleave: the rotation is a serial float64 dependency, and with the
// CU's LDS taken by one workgroup nothing else would hide it.  Waves share nothing after the staging barrier, so the order of
// every sum follows from L_b and the lane alone; there are no atomics, no static LDS and no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_cq_sizes.hpp" // WF_CQ_THREADS, WF_CQ_WAVES and the sizes of the host's tables
#include "wf_ring_view.hpp"
#include "wf_wave_reduce.hpp"

namespace wf {

struct CqArgs {
    RingView rings;
    wf_hip_cq *out;          // [count] the entry of stream `first`
    const double *tab;       // [end_covered][WF_CQ_BIN_DOUBLES], 16-byte aligned
    const uint32_t *sched;   // [WF_CQ_SCHED_WORDS]: bins < end_covered, each once
    uint32_t first;          // first stream read
    uint32_t Lmax;           // frames staged: a multiple of 64, <= min(ring_cap, WF_HIP_CQ_MAX_WINDOW); every L_b <= Lmax
    uint32_t end_covered, first_resolved;
};

// a times b
__device__ __forceinline__ double2 cq_mul(double2 a, double2 b)
{
    return make_double2(__builtin_fma(a.x, b.x, -(a.y * b.y)), __builtin_fma(a.x, b.y, a.y * b.x));
}

// grid: one workgroup per stream of [first, first + gridDim.x); dynamic LDS: CH * Lmax * sizeof(float)
template<int CH>
__global__ __launch_bounds__(WF_CQ_THREADS) void cq_read_kernel(const CqArgs a)
{
    extern __shared__ float cq_x[]; // [CH][Lmax]
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const uint32_t stream = a.first + blockIdx.x;
    const uint32_t mask = a.rings.ring_cap - 1u;
    const uint32_t s = window_start(a.rings, stream, a.Lmax);
    const float *r0 = channel_ring(a.rings, stream, 0, CH);
    for(uint32_t i = t; i < a.Lmax; i += WF_CQ_THREADS) {
        const uint32_t at = (s + i) & mask;
        cq_x[i] = r0[at];
        if constexpr(CH == 2)
            cq_x[a.Lmax + i] = r0[a.rings.ring_stride + at];
    }
    // what no wave computes: the uncovered bins and the channel that was not captured read -INFINITY; the geometry
    uint32_t *words = reinterpret_cast<uint32_t *>(a.out + blockIdx.x);
    if(t < 2u * WF_HIP_CQ_BINS) {
        if(t >= (uint32_t)CH * WF_HIP_CQ_BINS || t % WF_HIP_CQ_BINS >= a.end_covered)
            words[t] = __float_as_uint(-INFINITY);
    } else if(t < 2u * WF_HIP_CQ_BINS + 4u) {
        const uint32_t f = t - 2u * WF_HIP_CQ_BINS;
        words[t] = f == 0u ? a.end_covered : f == 1u ? a.first_resolved : f == 2u ? a.Lmax : 0u;
    }
    __syncthreads();

    for(uint32_t k = a.sched[wave]; k < a.sched[wave + 1u]; ++k) {
        const uint32_t b = a.sched[WF_CQ_WAVES + 1u + k];
        const double *tb = a.tab + (size_t)b * WF_CQ_BIN_DOUBLES;
        const double2 cstep = make_double2(tb[0], tb[1]), hstep = make_double2(tb[2], tb[3]);
        const uint32_t L = (uint32_t)tb[5];
        const double2 *start = reinterpret_cast<const double2 *>(tb + WF_CQ_BIN_HEAD) + 2u * lane;
        double2 c = start[0], h = start[1];
        const float *x0 = cq_x + (a.Lmax - L); // the bin's window: the newest L frames
        const float *x1 = x0 + a.Lmax;
        double2 s0 = make_double2(0.0, 0.0), s1 = s0;
        for(uint32_t n = lane; n < L; n += 64u) {
            const double w = __builtin_fma(-0.5, h.x, 0.5);
            const double pr = w * c.x, pi = w * c.y;
            const double l = (double)x0[n];
            s0.x = __builtin_fma(l, pr, s0.x);
            s0.y = __builtin_fma(l, pi, s0.y);
            if constexpr(CH == 2) {
                const double r = (double)x1[n];
                s1.x = __builtin_fma(r, pr, s1.x);
                s1.y = __builtin_fma(r, pi, s1.y);
            }
            c = cq_mul(c, cstep);
            h = cq_mul(h, hstep);
        }
        s0.x = wave_sum(s0.x);
        s0.y = wave_sum(s0.y);
        if constexpr(CH == 2) {
            s1.x = wave_sum(s1.x);
            s1.y = wave_sum(s1.y);
        }
        if(lane < (uint32_t)CH) {
            const double2 v = (CH == 2 && lane == 1u) ? s1 : s0;
            const double amp = tb[4] * sqrt(__builtin_fma(v.x, v.x, v.y * v.y));
            a.out[blockIdx.x].db[lane][b] = amp > 0.0 ? (float)(20.0 * log10(amp)) : -INFINITY;
        }
    }
}

} // namespace wf
