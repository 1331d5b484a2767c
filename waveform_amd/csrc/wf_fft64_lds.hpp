// wf_fft64_lds.hpp -- the complex float64 transform in LDS that the read kernels of WF_HIP_OUT_STEREO (wf_stereo.hpp: one
// transform per workgroup of 256 threads), WF_HIP_OUT_SONO (wf_sono.hpp: one per wavefront), WF_HIP_OUT_THD and WF_HIP_OUT_IMD (wf_thd_spectrum.hpp for wf_thd.hpp and wf_imd.hpp: one
// per workgroup of 512 threads, up to P = 8192), WF_HIP_OUT_DELAY (wf_delay.hpp: two per workgroup of 256 threads, one behind
// the other in two regions), WF_HIP_OUT_ONSET and WF_HIP_OUT_TEMPO (wf_onset_column.hpp for wf_onset.hpp and wf_tempo.hpp: one per wavefront and round, as the sonogram's), WF_HIP_OUT_XFER
// (wf_xfer.hpp by wf_xfer_sums.hpp: up to 65 per workgroup of 256 threads, one behind the other in one region),
// WF_HIP_OUT_IMPULSE (wf_impulse.hpp: the same and two more) and WF_HIP_OUT_HUM (wf_hum.hpp: up to 32 of 512 or 1024 points per
// workgroup of 256 threads, one behind the other in one region) share (device code only; hipcc).
//
// P complex float64 (16 B each), P a power of two >= 64, decimation in time, natural order out:
//   load    thread c' < P / 16 takes the 16 elements c' + m P/16, m = 0 .. 15 (consecutive lanes on consecutive elements) from
//           the caller's fetch and runs their 16-point transform in registers: the first four radix-2 stages, which in LDS would
//           be the ones with strides of 1 to 8 elements.  The result is block c = bitrev(c') of 16 consecutive elements.
//   passes  radix-2 stages two at a time (one read and one write of LDS per two stages), butterflies j, j + q, j + 2q, j + 3q
//           with q = 16, 64, 256, 1024; a last single stage when log2 P is odd.  Twiddles from the host's table [P / 2].
// THREADS threads share one transform and `sync` orders their LDS phases: fft64_block_sync for a workgroup, fft64_wave_sync for
// the 64 lanes of one wavefront, whose LDS operations execute in program order, so that no hardware barrier is needed, only the
// compiler's promise not to move LDS accesses across the phase boundary -- other wavefronts of the workgroup then never wait
// for this one and may leave early.
//
// LDS addressing.  Element i lives in 16-byte slot i ^ (bitrev(i >> 4) & 15): inside its aligned row of 16 slots (256 B, all 64
// banks) it is moved by the low bits of the number c' of the thread that produced the row.  Every later access has lanes on
// consecutive i with q >= 16, so 16 lanes cover one row whatever its permutation: ds_read_b128 / ds_write_b128 without
// conflicts.  The load phase's stores, where lane c' writes row bitrev(c') -- rows 1 KB apart at P = 4096, which unpermuted is
// one bank group for every lane -- fall on slot u ^ (c' & 15): eight consecutive lanes, eight different slots.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wf {

__device__ __forceinline__ double2 fft64_mul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 fft64_add(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 fft64_sub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }

// two radix-2 stages of a decimation-in-time transform on x[j], x[j + q], x[j + 2q], x[j + 3q]: w1 = W_2q^j, w2 = W_4q^j
// (W_4q^(j + q) is w2 times -j)
__device__ __forceinline__ void fft64_bfly4(double2 &x0, double2 &x1, double2 &x2, double2 &x3, double2 w1, double2 w2)
{
    const double2 t1 = fft64_mul(w1, x1), t3 = fft64_mul(w1, x3);
    const double2 a0 = fft64_add(x0, t1), a1 = fft64_sub(x0, t1), a2 = fft64_add(x2, t3), a3 = fft64_sub(x2, t3);
    const double2 t2 = fft64_mul(w2, a2), v = fft64_mul(w2, a3);
    const double2 t4 = make_double2(v.y, -v.x);
    x0 = fft64_add(a0, t2);
    x2 = fft64_sub(a0, t2);
    x1 = fft64_add(a1, t4);
    x3 = fft64_sub(a1, t4);
}

// the slot of element i (cb = log2 P - 4 bits of row number)
__device__ __forceinline__ uint32_t fft64_at(uint32_t i, uint32_t cb) { return i ^ ((__brev(i >> 4) >> (32u - cb)) & 15u); }

// how the threads of one transform order their LDS phases
struct fft64_block_sync {
    __device__ __forceinline__ void operator()() const { __syncthreads(); }
};
struct fft64_wave_sync {
    __device__ __forceinline__ void operator()() const
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
};

// load: thread t (of the transform's own) < P / 16 fetches elements t + m P/16 through fetch(i) and leaves their 16-point
// transform in its row of `lds`
template<class Fetch> __device__ __forceinline__ void fft64_load16(double2 *lds, const double2 *tw, uint32_t t, uint32_t P, uint32_t cb, Fetch fetch)
{
    const uint32_t n16 = P >> 4;
    if(t < n16) {
        double2 x[16];
#pragma unroll
        for(uint32_t u = 0; u < 16; ++u) { // x[u]: element number bitrev4(u) of the sixteen
            const uint32_t m = ((u & 1u) << 3) | ((u & 2u) << 1) | ((u & 4u) >> 1) | ((u & 8u) >> 3);
            x[u] = fetch(t + m * n16);
        }
        const double2 one = make_double2(1.0, 0.0);
#pragma unroll
        for(uint32_t g = 0; g < 4; ++g)
            fft64_bfly4(x[4 * g], x[4 * g + 1], x[4 * g + 2], x[4 * g + 3], one, one);
#pragma unroll
        for(uint32_t j = 0; j < 4; ++j)
            fft64_bfly4(x[j], x[j + 4], x[j + 8], x[j + 12], tw[2u * j * n16], tw[j * n16]);
        const uint32_t row = (__brev(t) >> (32u - cb)) << 4, swz = t & 15u;
#pragma unroll
        for(uint32_t u = 0; u < 16; ++u)
            lds[row + (u ^ swz)] = x[u];
    }
}

// passes: what is left of the transform behind fft64_load16, and the ordering point behind the last stage
template<uint32_t THREADS, class Sync> __device__ __forceinline__ void fft64_passes(double2 *lds, const double2 *tw, uint32_t t, uint32_t P, uint32_t cb, Sync sync)
{
    // stages of half-length q and 2q together
    uint32_t q = 16;
    for(; 4u * q <= P; q *= 4u) {
        sync();
        const uint32_t step = P / (4u * q);
        for(uint32_t u = t; u < P / 4u; u += THREADS) {
            const uint32_t j = u & (q - 1u), base = ((u - j) << 2) + j;
            const uint32_t i0 = fft64_at(base, cb), i1 = fft64_at(base + q, cb), i2 = fft64_at(base + 2u * q, cb),
                           i3 = fft64_at(base + 3u * q, cb);
            const double2 w2 = tw[j * step], w1 = tw[2u * j * step];
            double2 x0 = lds[i0], x1 = lds[i1], x2 = lds[i2], x3 = lds[i3];
            fft64_bfly4(x0, x1, x2, x3, w1, w2);
            lds[i0] = x0;
            lds[i1] = x1;
            lds[i2] = x2;
            lds[i3] = x3;
        }
    }
    if(2u * q == P) { // log2 P odd: the last stage alone
        sync();
        for(uint32_t j = t; j < q; j += THREADS) {
            const uint32_t i0 = fft64_at(j, cb), i1 = fft64_at(j + q, cb);
            const double2 x0 = lds[i0], v = fft64_mul(tw[j], lds[i1]);
            lds[i0] = fft64_add(x0, v);
            lds[i1] = fft64_sub(x0, v);
        }
    }
    sync();
}

} // namespace wf
