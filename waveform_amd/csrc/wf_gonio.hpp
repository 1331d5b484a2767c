// wf_gonio.hpp -- gfx950 read kernel of WF_HIP_OUT_GONIO (device code only; hipcc; included by wf_hip_measure.hip alone).
//
// Not in the reference: a stereo vectorscope (goniometer), the mid/side Lissajous picture of the newest P = min(fft_size, 8192)
// frames of captured channels 0 and 1 as a 64 x 64 image of frame counts, magnified by a power of two so that the loudest sample
// lies between half and full deflection (the definition is in include/wf_hip.h, "vectorscope").  wf_hip_read launches it on the
// handle's stream, behind every push issued so far, and copies the result back; nothing runs while the output is not read.
//
// One workgroup of WF_GONIO_THREADS per stream; the ring is read once.
//   stage    wf_ring_stage.hpp's ring_stage_window<2>: the at most two contiguous runs of the window into dynamic LDS, 16-B words over the
//            aligned body, element by element over the at most 3 frames around it; frame i of channel c at x[c][o + i].
//   pass one the largest |sample| as an integer maximum over the samples' bits less their sign (the order of non-negative floats
//            is the order of their bits: nothing depends on how the hardware treats denormals), max |mid| and max |side| in
//            float64, and the two phase counts from the sign bits; a butterfly over the wavefront, the waves' partials through LDS,
//            combined by every thread in wave order.  The exponent e follows from the bits of the peak.
//   pass two (skipped when the peak is 0: the entry is known, all P frames in cell [32][32])
//            a wavefront per 64 consecutive frames, lane j the j-th of them: u, v, the cell.  The count goes into the entry's
//            image in LDS with integer LDS atomic adds, two uint16 cells to the word (a count is at most P <= 8192 < 2^16, so the
//            halves never carry into each other): an add of 1 or of 1 << 16.  (The compiler fuses the scaling by 2^-e with the
//            addition of 1.0 into one fma; the product is exact, so the fused operation rounds what the addition alone rounds.)
//   leave    the non-zero cells are counted from the finished image, the eight scalars join it, and it leaves as 16-B words: no
//            memset per read, no global atomics.
// Contention of the count.  Same-address LDS atomics of one wavefront are serialised, and the usual inputs pile the frames into
// few cells (a mono source: one column; a one-sided one: a diagonal; a source with one loud click: the centre).  Of the two ways
// out, combining within the wavefront was taken, not a sub-image per wavefront: a sub-image only separates the waves from each
// other, and it is the 64 lanes of ONE wave that collide; it would also add 24 KB of LDS (four packed images) and take the
// workgroups per CU at the cap from two to one.  The combination: lanes hold consecutive frames, so audio below a few kHz puts
// neighbouring lanes into the same cell.  A lane whose cell equals its lower neighbour's hands its count over: one ballot of the
// run heads, each head finds the next head with a count of trailing zeros and adds the length of its run.  A constant, a slow
// wave or a window that sits in one cell costs one atomic per wavefront and step; white noise costs what it cost before (its
// lanes rarely collide: the picture has hundreds of cells).  Measured on an MI355X (tools/gonio_bench.py,
// profiles/gonio_kernel_stats.json; 4096 streams, the read's 33.7 MB copy into page-locked memory included, which is about
// 590 us of each figure): noise 688 us, a mono source 699 us, silence 664 us at P = 4096; 759, 802 and 699 us at P = 8192.  The
// kernel without the hand-over, and the kernel's own time without the copy: unmeasured.
// No float atomics, no static LDS, no scratch; the only accumulation is integer counting, which commutes, so the same ring
// contents read bit-identically.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "wf_hip.h"
#include "wf_ring_view.hpp"
#include "wf_ring_stage.hpp"
#include "wf_wave_reduce.hpp"

namespace wf {

struct GonioArgs {
    RingView rings;
    wf_hip_gonio *out;       // [count] the entry of stream `first` (16-byte aligned: a hipMalloc'ed block of 8224-byte entries)
    uint32_t first;          // first stream read
    uint32_t P;              // window <= min(ring_cap, WF_HIP_GONIO_MAX_WINDOW), >= 1
};

constexpr uint32_t WF_GONIO_THREADS = 256;
constexpr uint32_t WF_GONIO_WAVES = WF_GONIO_THREADS / 64;
constexpr uint32_t WF_GONIO_UNROLL = 4;                  // float4 loads per channel in flight per lane
constexpr int WF_GONIO_OCC = 4;                         // waves per SIMD the registers allow; the LDS allows two workgroups per CU at the cap
constexpr uint32_t WF_GONIO_CELLS = WF_HIP_GONIO_GRID * WF_HIP_GONIO_GRID;
static_assert(WF_GONIO_THREADS == 256 && sizeof(wf_hip_gonio) % 16 == 0 && offsetof(wf_hip_gonio, window) == WF_GONIO_CELLS * 2);
static_assert(sizeof(wf_hip_gonio) - offsetof(wf_hip_gonio, window) == 32 && WF_HIP_GONIO_MAX_WINDOW < 65536);

// what follows the staged windows in dynamic LDS
struct GonioWork {
    uint32_t image[sizeof(wf_hip_gonio) / 4]; // the entry as it leaves: two cells to the word, then the scalars
    double mid[WF_GONIO_WAVES], side[WF_GONIO_WAVES];
    uint32_t peak[WF_GONIO_WAVES], in_phase[WF_GONIO_WAVES], out_phase[WF_GONIO_WAVES], occupied[WF_GONIO_WAVES];
};
static_assert(offsetof(GonioWork, mid) % 8 == 0);

__host__ __device__ constexpr size_t gonio_lds_bytes(uint32_t P) { return (size_t)2 * ring_stage_stride(P) * sizeof(float) + sizeof(GonioWork); }
static_assert(2 * gonio_lds_bytes(WF_HIP_GONIO_MAX_WINDOW) <= WF_LDS_PER_CU, "two workgroups to a CU at the cap");

// the cell index of a coordinate: min and max in floating point before the conversion, so no index leaves the grid
__device__ __forceinline__ uint32_t gonio_index(double u)
{
    const double g = __builtin_floor((u + 1.0) * (WF_HIP_GONIO_GRID / 2));
    return (uint32_t)(int)__builtin_fmin(__builtin_fmax(g, 0.0), (double)(WF_HIP_GONIO_GRID - 1));
}

// grid: one workgroup per stream of [first, first + gridDim.x); dynamic LDS: gonio_lds_bytes(P)
__global__ __launch_bounds__(WF_GONIO_THREADS, WF_GONIO_OCC) void gonio_read_kernel(const GonioArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float gonio_x[]; // [2][S], then the GonioWork
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const uint32_t stream = a.first + blockIdx.x;
    const uint32_t P = a.P;
    const uint32_t S = ring_stage_stride(P);
    GonioWork &w = *reinterpret_cast<GonioWork *>(gonio_x + (size_t)2 * S);
    const uint32_t ring_cap = a.rings.ring_cap;
    const uint32_t s = window_start(a.rings, stream, P) & (ring_cap - 1u);
    const uint32_t o = s & 3u;
    const float *r0 = channel_ring(a.rings, stream, 0, 2);
    const float *r1 = channel_ring(a.rings, stream, 1, 2);
    const float *x0 = gonio_x + o, *x1 = x0 + S; // x_c[i]

    ring_stage_window<2, WF_GONIO_THREADS, WF_GONIO_UNROLL>(gonio_x, S, r0, r1, s, P, ring_cap);
    for(uint32_t i = t; i < sizeof(wf_hip_gonio) / 4u; i += WF_GONIO_THREADS)
        w.image[i] = 0u;
    __syncthreads();

    // pass one: the peaks and the phase counts
    uint32_t peak = 0u, in_phase = 0u, out_phase = 0u;
    double mid = 0.0, side = 0.0;
    for(uint32_t i = t; i < P; i += WF_GONIO_THREADS) {
        const float l = x0[i], r = x1[i];
        const uint32_t lb = __float_as_uint(l), rb = __float_as_uint(r);
        const uint32_t la = lb & 0x7fffffffu, ra = rb & 0x7fffffffu;
        peak = peak > la ? peak : la;
        peak = peak > ra ? peak : ra;
        const double dl = (double)l, dr = (double)r;
        side = __builtin_fmax(side, __builtin_fabs((dr - dl) * 0.5));
        mid = __builtin_fmax(mid, __builtin_fabs((dl + dr) * 0.5));
        const bool both = la != 0u && ra != 0u; // neither is a zero
        const bool same = ((lb ^ rb) >> 31) == 0u;
        in_phase += both && same ? 1u : 0u;
        out_phase += both && !same ? 1u : 0u;
    }
    wave_butterfly([&](auto other) {
        const uint32_t p = other(peak);
        peak = peak > p ? peak : p;
        mid = __builtin_fmax(mid, other(mid));
        side = __builtin_fmax(side, other(side));
    });
    in_phase = wave_sum(in_phase);
    out_phase = wave_sum(out_phase);
    if(lane == 0) {
        w.peak[wave] = peak;
        w.mid[wave] = mid;
        w.side[wave] = side;
        w.in_phase[wave] = in_phase;
        w.out_phase[wave] = out_phase;
    }
    __syncthreads();
    peak = w.peak[0];
    mid = w.mid[0];
    side = w.side[0];
    in_phase = w.in_phase[0];
    out_phase = w.out_phase[0];
    for(uint32_t k = 1; k < WF_GONIO_WAVES; ++k) {
        peak = peak > w.peak[k] ? peak : w.peak[k];
        mid = __builtin_fmax(mid, w.mid[k]);
        side = __builtin_fmax(side, w.side[k]);
        in_phase += w.in_phase[k];
        out_phase += w.out_phase[k];
    }
    // A = f 2^e, 0.5 <= f < 1: e = (biased exponent) - 126; a denormal peak lies far below the clamp
    int e = 0;
    if(peak != 0u) {
        const int biased = (int)(peak >> 23);
        e = biased == 0 ? WF_HIP_GONIO_MIN_EXP : biased - 126;
        e = e < WF_HIP_GONIO_MIN_EXP ? WF_HIP_GONIO_MIN_EXP : e;
    }

    // pass two: the count
    if(peak != 0u) { // (the same for every thread)
        const double scale = __longlong_as_double((long long)(1023 - e) << 52); // 2^-e (e <= 129)
        for(uint32_t base = 64u * wave; base < P; base += WF_GONIO_THREADS) {
            const uint32_t i = base + lane;
            const bool valid = i < P; // (the valid lanes are the lowest)
            uint32_t cell = 0xffffffffu;
            if(valid) {
                const double dl = (double)x0[i], dr = (double)x1[i];
                const double u = (dr - dl) * 0.5 * scale, v = (dl + dr) * 0.5 * scale;
                cell = gonio_index(v) * WF_HIP_GONIO_GRID + gonio_index(u);
            }
            const uint32_t below = __shfl_up(cell, 1, 64);
            const bool head = valid && (lane == 0u || cell != below);
            const unsigned long long heads = __ballot(head);
            const uint32_t n_valid = (uint32_t)__popcll(__ballot(valid));
            if(head) { // the run ends in front of the next head, or with the valid lanes
                const unsigned long long above = heads & ~((2ull << lane) - 1ull);
                const uint32_t next = above != 0 ? (uint32_t)__builtin_ctzll(above) : n_valid;
                __hip_atomic_fetch_add(&w.image[cell >> 1], (next - lane) << (16u * (cell & 1u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    } else if(t == 0u)
        w.image[(WF_GONIO_CELLS / 2u + WF_HIP_GONIO_GRID / 2u) / 2u] = P; // cell [32][32]: an even cell, the low half
    __syncthreads();

    uint32_t occupied = 0u;
    for(uint32_t i = t; i < WF_GONIO_CELLS / 2u; i += WF_GONIO_THREADS) {
        const uint32_t c = w.image[i];
        occupied += ((c & 0xffffu) != 0u ? 1u : 0u) + ((c >> 16) != 0u ? 1u : 0u);
    }
    occupied = wave_sum(occupied);
    if(lane == 0)
        w.occupied[wave] = occupied;
    __syncthreads();
    if(t < 8u) {
        occupied = w.occupied[0];
        for(uint32_t k = 1; k < WF_GONIO_WAVES; ++k)
            occupied += w.occupied[k];
        const uint32_t word = t == 0u ? P : t == 1u ? (uint32_t)-e : t == 2u ? peak : t == 3u ? __float_as_uint((float)mid)
                            : t == 4u ? __float_as_uint((float)side) : t == 5u ? in_phase : t == 6u ? out_phase : occupied;
        w.image[offsetof(wf_hip_gonio, window) / 4u + t] = word;
    }
    __syncthreads();
    const uint4 *src = reinterpret_cast<const uint4 *>(w.image);
    uint4 *dst = reinterpret_cast<uint4 *>(a.out + blockIdx.x);
    for(uint32_t i = t; i < sizeof(wf_hip_gonio) / 16u; i += WF_GONIO_THREADS)
        dst[i] = src[i];
}

} // namespace wf
