// wf_dev_helpers.hpp -- the small device helpers every kernel header shares: 16-byte loads and stores and their non-temporal
// forms, separately rounded products and sums (mul_unfused, meter_ema), the wavefront helpers (wave_arrive, seg_prefix_scan),
// the LDS accessors all exchange traffic goes through, dbfs and mag2.  Compiled by hipcc and, for tests/emu, by g++.
#pragma once
#include "wf_fft_core.hpp"

namespace wf {

// ---- small helpers ------------------------------------------------------------------------
WF_DEV f4 ld4(const float *p) { return *reinterpret_cast<const f4 *>(p); }
WF_DEV f2 ld2(const float *p) { return *reinterpret_cast<const f2 *>(p); }
WF_DEV void st4(float *p, f4 v) { *reinterpret_cast<f4 *>(p) = v; }
// Streaming accesses.  Measured on MI355X (cfg3, interleaved A/B on one box): the m_decibels rows -- output nothing on the
// device reads again -- stored with the non-temporal hint +1.8 % (they stop displacing the rings from the 256 MB Infinity
// Cache).  The smoothing state is read once and written once per tick: the hint on its stores alone +-0, on its loads
// alone +-0, on both +3.7 % (0.701 -> 0.727; 16384 streams 0.69 -> 0.72-0.75) -- then only the rings, whose consecutive
// windows overlap by 80 %, compete for the cache.  On the window loads themselves the hint costs 2 %: they are plain ld4.
// So: rows through store_row<.., NT = true>, the state through ld_state / st_state, everything else plain (EXPERIMENTS.md,
// "Retired build switches").
#if defined(__HIPCC__)
WF_DEV f4 ld4_nt(const float *p)
{
    typedef float v4f __attribute__((ext_vector_type(4)));
    const v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(p));
    return f4{v.x, v.y, v.z, v.w};
}
WF_DEV void st4_nt(float *p, f4 v)
{
    typedef float v4f __attribute__((ext_vector_type(4)));
    __builtin_nontemporal_store(v4f{v.x, v.y, v.z, v.w}, reinterpret_cast<v4f *>(p));
}
#else // the g++ wavefront emulator (tests/emu): plain accesses
WF_DEV f4 ld4_nt(const float *p) { return ld4(p); }
WF_DEV void st4_nt(float *p, f4 v) { st4(p, v); }
#endif

// m_tsmooth_buf is read once and written once per tick: both with the hint
WF_DEV f4 ld_state(const float *p) { return ld4_nt(p); }
WF_DEV void st_state(float *p, f4 v) { st4_nt(p, v); }

// Products and sums that must be rounded on their own, as the reference's scalar code rounds them.  HIP compiles device code
// with -ffp-contract=fast, and __fmul_rn / __fadd_rn are plain operators to the optimiser: `__fadd_rn(__fmul_rn(a, b), c)`
// becomes one fma.  Harmless within a tolerance -- except where the sum cancels: the level meter's smoothing starts from
// m_meter_buf = DB_MIN (a quirk of the reference: -758.6 taken as a linear level), and on the tick where g * old + g2 * new
// first turns positive a fused product moved the level by 7e-4 dB (fuzz seed 14562 of an extended sweep).
WF_DEV float mul_unfused(float a, float b)
{
#pragma clang fp contract(off)
    return a * b;
}
WF_DEV float add_unfused(float a, float b)
{
#pragma clang fp contract(off)
    return a + b;
}
// (g * old) + (g2 * cur), three roundings (reference src/source_generic.cpp:255)
WF_DEV float meter_ema(float g, float old, float g2, float cur)
{
#pragma clang fp contract(off)
    const float x = g * old;
    const float y = g2 * cur;
    return x + y;
}

// The spectrum's temporal smoothing, mag = g * old + (1 - g) * mag (reference src/source_generic.cpp:124-132): the
// generic class's three roundings (two products, one sum) -- not fma(g, old, g2 * mag), two roundings, as the reference's own AVX2
// class contracts it (src/source_avx2.cpp:154)
WF_DEV float spectrum_ema(float g, float old, float g2, float cur) { return meter_ema(g, old, g2, cur); }

// ordering point between LDS operations of one wavefront (they execute in program order: a scheduling fence suffices)
#if defined(__HIPCC__)
WF_DEV void wait_vmem_all() { __builtin_amdgcn_s_waitcnt(0x0F70); } // vmcnt(0), the other counters untouched (gfx9 encoding)
WF_DEV void wave_fence() { __builtin_amdgcn_wave_barrier(); }
WF_DEV float wave_shfl_down(float v, int d) { return __shfl_down(v, d, 64); } // lane l gets lane l + d's value (its own past the wavefront)
// Segmented inclusive prefix sum over the lanes of a wavefront: lane l ends up with the sum of the lanes of its segment up to
// and including itself.  `info` bits 0..5 say which of the six steps of a wave-wide scan this lane takes (BarPieceTables::info:
// the lanes 1, 2, 4, 8 below it inside its row of 16, the last lane of the row before, lane 31).  Six DPP moves at VALU speed
// instead of six ds_bpermute round trips; a step not taken adds an exact 0 (the moved value is masked, not multiplied: whatever
// an unused lane holds stays out).
WF_DEV float seg_prefix_scan(float v, uint32_t info)
{
#define WF_SCAN_STEP(CTRL, ROWS, BIT)                                                                                      \
    {                                                                                                                      \
        const int o = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROWS, 0xf, true);                            \
        v += __int_as_float(o & __builtin_amdgcn_sbfe((int)info, BIT, 1));                                                 \
    }
    WF_SCAN_STEP(0x111, 0xf, 0) // row_shr:1
    WF_SCAN_STEP(0x112, 0xf, 1) // row_shr:2
    WF_SCAN_STEP(0x114, 0xf, 2) // row_shr:4
    WF_SCAN_STEP(0x118, 0xf, 3) // row_shr:8
    WF_SCAN_STEP(0x142, 0xa, 4) // row_bcast:15 into rows 1 and 3
    WF_SCAN_STEP(0x143, 0xc, 5) // row_bcast:31 into rows 2 and 3
#undef WF_SCAN_STEP
    return v;
}
// The arrival counters of the display phase (a wavefront has made its last reads of the exchange buffer / has left its part of the
// row): release on the count, acquire on the wait, at workgroup scope -- what the memory model asks for.  (Until round 5: relaxed
// operations between compiler barriers, leaning on gfx9 executing a wavefront's LDS operations in order; on LDS the ordered forms cost
// one s_waitcnt lgkmcnt(0) in front of the count.)
// a wavefront counts itself in (LDS atomic, workgroup scope); every lane gets the count before it
WF_DEV int wave_arrive(int *counter, int lane)
{
    int old = 0;
    asm volatile("" ::: "memory");
    if(lane == 0)
        old = __hip_atomic_fetch_add(counter, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
    old = __builtin_amdgcn_readfirstlane(old);
    asm volatile("" ::: "memory");
    return old;
}
#else
WF_DEV void wait_vmem_all() {}
WF_DEV void wave_fence() {}
WF_DEV float wave_shfl_down(float v, int) { return v; } // (the emulator does not run the bar reduction)
WF_DEV float seg_prefix_scan(float v, uint32_t) { return v; }
WF_DEV int wave_arrive(int *counter, int) { return __atomic_fetch_add(counter, 1, __ATOMIC_ACQ_REL); }
#endif

// All LDS traffic goes through these four helpers (ds_read_b64/b128, ds_write_b64/b128).
// WF_LDS_TRACE is defined only by the g++ wavefront emulator in tests/emu to record
// (address, width, direction) per access for the bank-conflict census; it is empty here.
#ifndef WF_LDS_TRACE
#define WF_LDS_TRACE(idx, bytes, is_write)
#endif
WF_DEV cf lds_ld2(const cf *lds, int idx) { WF_LDS_TRACE(idx, 8, 0); return lds[idx]; }
WF_DEV void lds_st2(cf *lds, int idx, cf a) { WF_LDS_TRACE(idx, 8, 1); lds[idx] = a; }
WF_DEV f4 lds_ld4(const cf *lds, int idx) { WF_LDS_TRACE(idx, 16, 0); return *reinterpret_cast<const f4 *>(lds + idx); }
WF_DEV void lds_st4(cf *lds, int idx, cf a, cf b) { WF_LDS_TRACE(idx, 16, 1); *reinterpret_cast<f4 *>(lds + idx) = f4{a.x, a.y, b.x, b.y}; }


WF_DEV uint32_t f32_bits(float v)
{
#if defined(__HIPCC__)
    return __float_as_uint(v);
#else
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return u;
#endif
}

// dbfs(), reference src/source.hpp:293-299: mag > 0 ? 20*log10f(mag) : DB_MIN.
// Device form: max(log2(m) * 20*log10(2), DB_MIN) on the hardware log2 (v_log_f32, <= 1 ulp of its result; relative
// error of the dB value <= ~2e-7).  log2(0) = -inf and log2(negative) = NaN both end at DB_MIN through the max, as the
// reference's test does; for every normal m > 0 the max is a no-op because 20*log10(FLT_MIN) == DB_MIN.  One stated
// deviation: v_log_f32 flushes denormal inputs, so magnitudes below FLT_MIN (1.2e-38, i.e. under -758 dBFS) read
// DB_MIN where the reference would read -759..-897 dB -- far below any displayable floor (>= -120 dB).
// (The host branch is the reference's own form: the g++ emulator runs it.)
WF_DEV float dbfs(float mag, float db_min)
{
#if defined(__HIPCC__)
    return fmaxf(__builtin_amdgcn_logf(mag) * 6.02059991327962390f, db_min);
#else
    return (mag > 0.0f) ? 20.0f * log10f(mag) : db_min;
#endif
}

// |2X| from its parts.  hypotf in the reference (:119); here sqrt(fma) on the hardware square root (1 ulp).
// (Squares of parts below ~1e-19 underflow where hypotf still answers -- the first ticks behind a reset through a narrow window:
// |X| ~ 1e-26, -520 dBFS, far below any displayable floor; the rescaling branch once kept for them, WF_MAG_SAFE, is retired.)
WF_DEV float mag2(float xr, float xi)
{
    const float s = fmaf(xi, xi, xr * xr);
#if defined(__HIPCC__)
    return __builtin_amdgcn_sqrtf(s);
#else
    return sqrtf(s);
#endif
}

// std::lerp as libstdc++ evaluates it (reference src/math_funcs.hpp:31-35)
WF_DEV float lerp_std(float a, float b, float t)
{
    if((a <= 0 && b >= 0) || (a >= 0 && b <= 0))
        return t * b + (1 - t) * a;
    if(t == 1)
        return b;
    const float x = a + t * (b - a);
    return ((t > 1) == (b > a)) ? (b < x ? x : b) : (b > x ? x : b);
}

} // namespace wf
