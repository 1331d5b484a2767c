// wf_tick_phases.hpp -- thread-level phases of the fused spectrum tick.
//
// One spectrum (= one channel of one stream, one call of the per-channel loop at
// reference src/source_generic.cpp:53-136) is processed by T threads in phases; a
// phase boundary is a point where threads exchange data through LDS:
//
//   P1  fetch the latest N samples of the channel ring (reference :55-59), multiply by
//       the window (:97-103), radix-R1 butterflies, twiddle            -> write ex1
//   P2  read ex1, radix-R2 butterflies, twiddle                         -> write ex2
//   P3  read ex2, radix-R3 butterflies                                  -> write ex3 (Z, four planes by k mod 4)
//   P4  read Z[k], Z[M-k]; real split; |X|*2/sum(w) (:110-119); slope (:121-122);
//       temporal smoothing incl. fast peaks (:124-132); dBFS (:144-159, src/source.hpp:293-299);
//       volume normalisation (:161-167); roll-off (:169-179)            -> HBM
//   then, for configurations that display bars or a curve, the render-time reduction of the row just produced
//   (render_bars / render_curve, src/source.cpp:1360-1425, 1500-1564): bars_reduce_row / curve_row, outputs_finish
//   (wf_tick_display.hpp).
// Here: Policy, P1-P4 of the power-of-two sizes, the row helpers, plan_stream and the silence helpers.  The argument structs
// are in wf_tick_args.hpp, the small helpers in wf_dev_helpers.hpp, the Bluestein fetch and epilogue in wf_bluestein.hpp, the
// mixed-radix epilogue in wf_mixed.hpp.
//
// Each P*_read / P*_write split below marks where a block barrier is needed when
// T > 64 (several wavefronts share the spectrum); with T == 64 program order inside
// the wavefront is enough.
#pragma once
#include "wf_fft_core.hpp"
#include "wf_tick_args.hpp"
#include "wf_dev_helpers.hpp"

namespace wf {

// ---- P1: fetch + window + pass 1 ---------------------------------------------------------------
// x      : base of this spectrum's ring
// start  : ring index of the first sample of the window
// ALIGNED: start % 4 == 0 (vector loads never straddle the ring wrap)
// p1_fetch copies this thread's share of the window into registers (the reference's peek_front into
// m_fft_input, :55-59) as smp[j][e] = x[start + 2*(j*M1 + B1*t) + e] and reports whether any of them is
// non-zero (the reference's silence scan, :63-72).
// Everything pass 1 and the real split need from HBM/L2, issued back to back so the latencies overlap:
//   smp   this thread's share of the window (the reference's peek_front into m_fft_input, :55-59):
//         smp[j][e] = x[start + 2*(j*M1 + B1*t) + e]
//   win   the window coefficients of the same samples (:97-103)
//   tw1   W_M^(n' k1) for this thread's n' (k1 = 1..R1-1)
//   wb    W_N^(4t+i), i = 0..3: the real-split twiddles of this thread's first bin group; the other groups
//         are wb * W_N^(4Tu) = wb * W_32^(u*64/P) (exact multiples of 1/32 turn)
// Prefetch policy.  Every thread owns <= 16 points, holds the window / twiddle operands from the start and prefetches the
// smoothing state (16 VGPRs at P = 16) and the slope table into registers while passes 2-3 run, or loads them in P4: Policy<G>::MODE.
template<class G> struct Policy {
    static_assert(G::P <= 32, "the phase functions keep a thread's operands in registers: at most 32 points per thread (two waves per SIMD)");
    // 1: state + slope into registers right after pass 1;
    // 0: everything requested at the start of P4, consumed after the real split.  Round 1 found 1 best for the one-wavefront
    // geometries (N = 1024: 68 vs 75 us, N = 2048: 72.3 vs 75 us) and, for N >= 4096, "touching" one dword per 64-byte line
    // of the state row behind pass 1 so that P4's loads are served from L2 (77.1-79.1 vs 79.3-80.4 us then); with the lanes and
    // the non-temporal row stores of round 2 the early requests only lengthen the fetch
    // burst's queue: mode 0 is +3 % at N = 4096, +1.7 % at 2048, +1..3 % at 8192 / 16384, +-0 at 32768 (interleaved A/B).
    // The 8-point geometry keeps 1 (its decimated epilogue takes the operands from registers).  The touch mode and a late form
    // of mode 1 (requested behind pass 3's stores) are retired: EXPERIMENTS.md, "Retired build switches".
    static constexpr int MODE = G::P <= 8 ? 1 : 0;
    static constexpr bool PREFETCH_STATE = (MODE == 1);
    static constexpr bool PREFETCH_SLOPE = (MODE == 1);
    // The slope factors m_slope_modifiers[k] = log10f(10 * powf(1000, k * slope / (M - 1))) (src/source.cpp:1283-1290) are, but for
    // the roundings of powf and log10f, 1 + 3 k slope / (M - 1): the geometries that request all of P4's operands first (MODE 0)
    // form them with one fma per bin instead of loading them -- four of the twelve requests of P4's burst and 16 registers across
    // the real split gone (N = 4096: 0.791 -> 0.803 of the HBM peak, interleaved, profiles/r04a_coef_early.txt); the factors
    // differ from the reference's table by at most 4e-7 relative (tests/test_cpu_units.py pins it), DESIGN.md section 5.
    static constexpr bool SLOPE_LINEAR = MODE == 0;
    // The display's per-thread tables (BarEntries) requested in front of P4 instead of behind its state stores: a load at the end
    // of the kernel waits out the whole loaded memory pipeline once more -- that wait, not the barrier or the shuffles, was the
    // bars tail (profiles/r04a_tail_cuts.txt).  Needs the registers SLOPE_LINEAR frees (without them: 128 VGPRs + 36 B of scratch).
    static constexpr bool BAR_COEF_EARLY = SLOPE_LINEAR && G::T >= 128;
};
// Pass-1 twiddle rows W_M^(n' k1), k1 = 1..R1-1: only the rows whose k1 is a power of two come from the table; the others
// are products of two of those (or of one and an earlier product): k1 = hi + lo with lo the lowest set bit.  At R1 = 8 that
// is 3 loaded rows and 4 complex multiplications per point instead of 7 loaded rows: 16 fewer VGPRs held through the fetch
// burst and 4 of its 23 sixteen-byte requests gone.  Accuracy: inputs are correctly rounded table entries (1/2 ulp each), a
// product adds one rounding: the worst row (k1 = 7 = (4 + 2) + 1) carries ~3.5 rounding units (2e-7 relative) instead of 1/2
// -- the size of the FFT's own round-off, an order of magnitude under the parity tolerance.  (Round 1 tried powers of the
// single row k1 = 1: up to 8e-7, rejected then.)
constexpr bool tw1_row_loaded(int k1) { return (k1 & (k1 - 1)) == 0; }

template<class G> struct P1Regs {
    float smp[G::R1][2 * G::B1];
    float win[G::R1][2 * G::B1];
    float tw1[G::R1][2 * G::B1];
    cf wb[4];
};

// window coefficients / pass-1 twiddles of row j of this thread
template<class G> WF_DEV void p1_load_window(const TickArgs &a, int t, int j, float (&win)[2 * G::B1])
{
    constexpr int B1 = G::B1, M1 = G::M1;
    const uint32_t s0 = 2u * (uint32_t)(j * M1 + B1 * t);
    if(B1 == 2) {
        const f4 w = ld4(a.window + s0);
        win[0] = w.x; win[1] = w.y; win[2 * B1 - 2] = w.z; win[2 * B1 - 1] = w.w;
    } else {
        const f2 w = ld2(a.window + s0);
        win[0] = w.x; win[1] = w.y;
    }
}
template<class G> WF_DEV void p1_load_tw1(const TickArgs &a, int t, int k1, float (&tw1)[2 * G::B1])
{
    constexpr int B1 = G::B1, M1 = G::M1;
    const float *tw = reinterpret_cast<const float *>(a.tw1 + k1 * M1 + B1 * t);
    if(B1 == 2) {
        const f4 w = ld4(tw);
        tw1[0] = w.x; tw1[1] = w.y; tw1[2 * B1 - 2] = w.z; tw1[2 * B1 - 1] = w.w;
    } else {
        const f2 w = ld2(tw);
        tw1[0] = w.x; tw1[1] = w.y;
    }
}

// returns whether any sample of this thread is non-zero (the reference's silence scan, :63-72)
// DEC > 0 (FFT sizes below the smallest geometry): the window is the first N >> DEC samples of a zero-padded N-point
// transform -- rows j >= R1 >> DEC of every thread are zeros and are not loaded -- and the real-split twiddles are those of
// the bins the small transform keeps, k = (4t + i) << DEC.
// TLDS: the window and pass-1 twiddle tables are not loaded here -- the workgroup stages them in LDS (p1_tables_to_lds).
template<class G, bool ALIGNED, int DEC = 0, bool TLDS = false>
WF_DEV bool p1_fetch(const TickArgs &a, int t, const float *x, uint32_t start, P1Regs<G> &r)
{
    constexpr int R1 = G::R1, B1 = G::B1, M1 = G::M1;
    constexpr int RV = R1 >> DEC; // rows that hold samples
    static_assert(RV >= 1, "zero-padding leaves at least one row of samples per thread");
    WF_UNROLL
    for(int j = 0; j < R1; ++j) {
        const uint32_t s0 = 2u * (uint32_t)(j * M1 + B1 * t);
        if(j >= RV) {
            WF_UNROLL
            for(int e = 0; e < 2 * B1; ++e) {
                r.smp[j][e] = 0.0f;
                r.win[j][e] = 0.0f;
            }
        } else if(ALIGNED) {
            if(B1 == 2) {
                const f4 q = ld4(x + ((start + s0) & a.ring_mask));
                r.smp[j][0] = q.x; r.smp[j][1] = q.y; r.smp[j][2 * B1 - 2] = q.z; r.smp[j][2 * B1 - 1] = q.w;
            } else {
                const f2 q = ld2(x + ((start + s0) & a.ring_mask));
                r.smp[j][0] = q.x; r.smp[j][1] = q.y;
            }
        } else {
            WF_UNROLL
            for(int e = 0; e < 2 * B1; ++e)
                r.smp[j][e] = *(x + ((start + s0 + (uint32_t)e) & a.ring_mask));
        }
    }
    WF_UNROLL
    for(int j = 0; j < R1; ++j) {
        if(j < RV && !TLDS)
            p1_load_window<G>(a, t, j, r.win[j]);
        if(j >= 1 && !TLDS && tw1_row_loaded(j))
            p1_load_tw1<G>(a, t, j, r.tw1[j]);
    }
    if(DEC == 0) {
        const f4 wa = ld4(reinterpret_cast<const float *>(a.tws + 4 * t));
        const f4 wc = ld4(reinterpret_cast<const float *>(a.tws + 4 * t + 2));
        r.wb[0] = cf{wa.x, wa.y}; r.wb[1] = cf{wa.z, wa.w}; r.wb[2] = cf{wc.x, wc.y}; r.wb[3] = cf{wc.z, wc.w};
    } else {
        WF_UNROLL
        for(int i = 0; i < 4; ++i) {
            const int k = ((4 * t + i) << DEC) & (G::M - 1); // threads beyond the kept bins read a valid entry they never use
            const f2 w = ld2(reinterpret_cast<const float *>(a.tws + k));
            r.wb[i] = cf{w.x, w.y};
        }
    }
    // x != 0.0f for any sample: OR the bit patterns, drop the sign bit (-0.0f == 0.0f); NaNs have non-zero bits
    uint32_t acc = 0;
    WF_UNROLL
    for(int j = 0; j < R1; ++j) {
        WF_UNROLL
        for(int e = 0; e < 2 * B1; ++e)
            acc |= f32_bits(r.smp[j][e]);
    }
    return (acc & 0x7fffffffu) != 0;
}

// window multiply (reference :97-103; the table is all ones for FFTWindow::NONE: x * 1.0f == x), butterflies over n1 (= j),
// twiddle by W_M^(n' k1): o[k1][b] = A'[k1][n' + b]
template<class G>
WF_DEV void p1_window_dft(P1Regs<G> &r, cf (&o)[G::R1][G::B1])
{
    constexpr int R1 = G::R1, B1 = G::B1;
    cf u[B1][R1];
    WF_UNROLL
    for(int j = 0; j < R1; ++j) {
        WF_UNROLL
        for(int e = 0; e < 2 * B1; ++e)
            r.smp[j][e] *= r.win[j][e];
        WF_UNROLL
        for(int b = 0; b < B1; ++b)
            u[b][j] = cf{r.smp[j][2 * b], r.smp[j][2 * b + 1]};
    }
    WF_UNROLL
    for(int b = 0; b < B1; ++b)
        dft_dif<R1>(u[b]);
    constexpr int LB = ilog2(R1);
    WF_UNROLL
    for(int k1 = 0; k1 < R1; ++k1) {
        if(k1 >= 1 && !tw1_row_loaded(k1)) { // row k1 = row (k1 minus its lowest set bit) times row (lowest set bit)
            const int lo = k1 & -k1, hi = k1 - lo;
            WF_UNROLL
            for(int b = 0; b < B1; ++b) {
                const cf w = cmul(cf{r.tw1[hi][2 * b], r.tw1[hi][2 * b + 1]}, cf{r.tw1[lo][2 * b], r.tw1[lo][2 * b + 1]});
                r.tw1[k1][2 * b] = w.x;
                r.tw1[k1][2 * b + 1] = w.y;
            }
        }
        WF_UNROLL
        for(int b = 0; b < B1; ++b)
            o[k1][b] = (k1 == 0) ? u[b][0] : cmul(u[b][brev(k1, LB)], cf{r.tw1[k1][2 * b], r.tw1[k1][2 * b + 1]});
    }
}
// store A'[k1][n'] into the exchange buffer
template<class G> WF_DEV void p1_store(int t, cf *lds, const cf (&o)[G::R1][G::B1])
{
    constexpr int R1 = G::R1, B1 = G::B1;
    const int np = B1 * t;
    WF_UNROLL
    for(int k1 = 0; k1 < R1; ++k1) {
        if(B1 == 2)
            lds_st4(lds, ex1_addr<G>(k1, np), o[k1][0], o[k1][B1 - 1]);
        else
            lds_st2(lds, ex1_addr<G>(k1, np), o[k1][0]);
    }
}
template<class G>
WF_DEV void p1_window_pass1(const TickArgs &a, int t, P1Regs<G> &r, cf *lds)
{
    (void)a;
    cf o[G::R1][G::B1];
    p1_window_dft<G>(r, o);
    p1_store<G>(t, lds, o);
}
// TLDS: the window (N floats) and the pass-1 twiddles (M complex) staged by the workgroup in LDS, in memory order:
// tab[0 .. M) = window as float pairs, tab[M .. 2M) = tw1.  This thread's operands, as p1_fetch would have loaded them.
template<class G> WF_DEV void p1_tables_from_lds(int t, const cf *tab, P1Regs<G> &r)
{
    constexpr int R1 = G::R1, B1 = G::B1, M1 = G::M1, M = G::M;
    WF_UNROLL
    for(int j = 0; j < R1; ++j) {
        if(B1 == 2) {
            const f4 w = lds_ld4(tab, j * M1 + B1 * t);
            r.win[j][0] = w.x; r.win[j][1] = w.y; r.win[j][2 * B1 - 2] = w.z; r.win[j][2 * B1 - 1] = w.w;
            if(j >= 1) {
                const f4 q = lds_ld4(tab, M + j * M1 + B1 * t);
                r.tw1[j][0] = q.x; r.tw1[j][1] = q.y; r.tw1[j][2 * B1 - 2] = q.z; r.tw1[j][2 * B1 - 1] = q.w;
            }
        } else {
            const cf w = lds_ld2(tab, j * M1 + t);
            r.win[j][0] = w.x; r.win[j][1] = w.y;
            if(j >= 1) {
                const cf q = lds_ld2(tab, M + j * M1 + t);
                r.tw1[j][0] = q.x; r.tw1[j][1] = q.y;
            }
        }
    }
}

// Issued as soon as pass 1 has freed its registers so that the HBM latency of the smoothing state (and the
// L2 latency of the slope table) is covered by passes 2 and 3 instead of being paid in P4.
template<class G> struct P4Regs {
    float st[Policy<G>::PREFETCH_STATE ? G::P : 1]; // m_tsmooth_buf of this thread's bins
    float sl[Policy<G>::PREFETCH_SLOPE ? G::P : 1]; // m_slope_modifiers of this thread's bins
    float unused[2];                                // (the retired touch mode's two dwords.  Never read or written; without them the register
                                                    // allocator names two registers of two N = 1024 kernels the other way round, and the
                                                    // retirement was held to byte-identical device code: goes with the next change that is not)
};
template<class G> WF_DEV void p4_prefetch(const TickArgs &a, int t, const float *ts, P4Regs<G> &q)
{
    constexpr int T = G::T, P = G::P;
    if(Policy<G>::PREFETCH_STATE && (a.mode & WF_MODE_TSMOOTH)) { // one scalar branch around all of the state loads
        constexpr int S = Policy<G>::PREFETCH_STATE ? 1 : 0;
        WF_UNROLL
        for(int u = 0; u < P / 4; ++u) {
            const f4 o = ld_state(ts + 4 * (t + T * u));
            q.st[S * (4 * u)] = o.x; q.st[S * (4 * u + 1)] = o.y; q.st[S * (4 * u + 2)] = o.z; q.st[S * (4 * u + 3)] = o.w;
        }
    }
    WF_UNROLL
    for(int u = 0; u < P / 4; ++u) {
        const int k0 = 4 * (t + T * u);
        if(Policy<G>::PREFETCH_SLOPE) {
            constexpr int S = Policy<G>::PREFETCH_SLOPE ? 1 : 0;
            const f4 o = ld4(a.slope + k0);
            q.sl[S * (4 * u)] = o.x; q.sl[S * (4 * u + 1)] = o.y; q.sl[S * (4 * u + 2)] = o.z; q.sl[S * (4 * u + 3)] = o.w;
        }
    }
}

// ---- P2: pass 2 ---------------------------------------------------------------------------------
template<class G> WF_DEV void p2_read(int t, const cf *lds, cf (&v)[G::P])
{
    constexpr int R2 = G::R2, R3 = G::R3, B2 = G::B2;
    if constexpr(G::H2 == 2) {
        // radix 32 with 16 points per thread (N = 32768): threads c and c + R1*R3 share column c = k1*R3 + n3.  Both read
        // the whole column; thread h keeps the half of the first radix-2 stage that feeds the outputs k2 = 2k' + h, as
        // pass 3 does: u[j] = (v[j] + sg * v[j+16]) * (h ? W_32^j : 1).
        constexpr int HALF = R2 / 2;
        static_assert(R2 == 32 || R2 == 16 || R2 == 8, "the shared second pass: radix 32 / 16 / 8 with 16 / 8 / 4 points per thread");
        const int c = t & (G::R1 * R3 - 1), h = t / (G::R1 * R3);
        const int k1 = c / R3, n3 = c % R3;
        const float hf = (float)h;
        const float sg = 1.0f - 2.0f * hf;
        WF_UNROLL
        for(int j = 0; j < HALF; ++j) {
            const cf lo = lds_ld2(lds, ex1_addr<G>(k1, j * R3 + n3));
            const cf hi = lds_ld2(lds, ex1_addr<G>(k1, (j + HALF) * R3 + n3));
            const cf e = cf{fmaf(sg, hi.x, lo.x), fmaf(sg, hi.y, lo.y)};
            v[j] = cmul(e, half_twiddle32(j * (32 / R2), hf)); // W_R2^j
        }
        return;
    }
    const int q0 = B2 * t;
    const int k1 = q0 / R3, n30 = q0 % R3;
    WF_UNROLL
    for(int n2 = 0; n2 < R2; ++n2) {
        const int base = ex1_addr<G>(k1, n2 * R3 + n30);
        if(B2 == 1) {
            v[n2] = lds_ld2(lds, base);
        } else {
            WF_UNROLL
            for(int b = 0; b < B2; b += 2) {
                const f4 q = lds_ld4(lds, base + b);
                v[b * R2 + n2] = cf{q.x, q.y};
                v[(b + 1) * R2 + n2] = cf{q.z, q.w};
            }
        }
    }
}

// tw2: the workgroup's LDS copy of the pass-2 twiddle table [R2][R3] (no vector-memory wait in the middle of the FFT,
// which would also wait for the state prefetch issued before it: loads return in order)
template<class G> WF_DEV void p2_pass2_write(const cf *tw2, int t, cf *lds, cf (&v)[G::P])
{
    constexpr int R1 = G::R1, R2 = G::R2, R3 = G::R3, B2 = G::B2;
    if constexpr(G::H2 == 2) {
        constexpr int HALF = R2 / 2, LBH = ilog2(HALF);
        const int c = t & (R1 * R3 - 1), h = t / (R1 * R3);
        const int k1 = c / R3, n3 = c % R3;
        cf u[HALF];
        WF_UNROLL
        for(int j = 0; j < HALF; ++j)
            u[j] = v[j];
        dft_dif<HALF>(u);
        WF_UNROLL
        for(int kk = 0; kk < HALF; ++kk) {
            const int k2 = 2 * kk + h;                 // this thread's outputs
            const cf w = lds_ld2(tw2, k2 * R3 + n3);   // W_(R2 R3)^(n3 k2); row 0 is all ones
            lds_st2(lds, ex2_addr<G>(k1 + R1 * k2, n3), cmul(u[brev(kk, LBH)], w));
        }
        return;
    }
    constexpr int LB = ilog2(R2);
    const int q0 = B2 * t;
    const int k1 = q0 / R3, n30 = q0 % R3;
    const int a20 = ex2_addr<G>(k1, n30);
    cf u[B2][R2];
    WF_UNROLL
    for(int b = 0; b < B2; ++b) {
        WF_UNROLL
        for(int n2 = 0; n2 < R2; ++n2)
            u[b][n2] = v[b * R2 + n2];
        dft_dif<R2>(u[b]);
    }
    WF_UNROLL
    for(int k2 = 0; k2 < R2; ++k2) {
        cf o[B2];
        if(k2 == 0) {
            WF_UNROLL
            for(int b = 0; b < B2; ++b)
                o[b] = u[b][0];
        } else if(B2 == 1) {
            const cf w = lds_ld2(tw2, k2 * R3 + n30);
            o[0] = cmul(u[0][brev(k2, LB)], w);
        } else {
            WF_UNROLL
            for(int b = 0; b < B2; b += 2) {
                const f4 w = lds_ld4(tw2, k2 * R3 + n30 + b);
                o[b] = cmul(u[b][brev(k2, LB)], cf{w.x, w.y});
                o[b + 1] = cmul(u[b + 1][brev(k2, LB)], cf{w.z, w.w});
            }
        }
        const int q = k1 + R1 * k2;
        if(B2 == 1) {
            // == ex2_addr<G>(q, n30): two distinct base registers per thread, the rest is an immediate offset
            lds_st2(lds, (a20 ^ ex2_xor<G>(k2)) + k2 * R1 * R3, o[0]);
        } else {
            WF_UNROLL
            for(int b = 0; b < B2; b += 2)
                lds_st4(lds, ex2_addr<G>(q, n30 + b), o[b], o[b + 1]);
        }
    }
}

// ---- P3: pass 3 ---------------------------------------------------------------------------------
template<class G> WF_DEV void p3_read(int t, const cf *lds, cf (&v)[G::P])
{
    constexpr int R3 = G::R3, B3 = G::B3, T = G::T;
    if constexpr(G::H3 == 2) {
        // radix 32 with 16 points per thread: threads q and q + R1*R2 share row q.  Both read the whole row; thread h
        // keeps the first radix-2 stage's half that feeds the outputs k3 = 2k' + h:
        //   h = 0: s[j] = v[j] + v[j+16]        h = 1: d[j] = (v[j] - v[j+16]) * W_32^j
        // written select-free: u[j] = (v[j] + sg * v[j+16]) * (h ? W_32^j : 1).
        constexpr int HALF = R3 / 2;
        const int q = t & (G::R1 * G::R2 - 1), h = t / (G::R1 * G::R2); // the two threads of row q sit in different wavefronts
        const float hf = (float)h;
        const float sg = 1.0f - 2.0f * hf;
        WF_UNROLL
        for(int j = 0; j < HALF; j += 2) {
            const f4 lo = lds_ld4(lds, ex2_addr<G>(q, j));
            const f4 hi = lds_ld4(lds, ex2_addr<G>(q, j + HALF));
            const cf e0 = cf{fmaf(sg, hi.x, lo.x), fmaf(sg, hi.y, lo.y)};
            const cf e1 = cf{fmaf(sg, hi.z, lo.z), fmaf(sg, hi.w, lo.w)};
            v[j] = cmul(e0, half_twiddle32(j * (32 / R3), hf)); // W_R3^j
            v[j + 1] = cmul(e1, half_twiddle32((j + 1) * (32 / R3), hf));
        }
        return;
    }
    WF_UNROLL
    for(int b = 0; b < B3; ++b) {
        const int q = t + T * b;
        WF_UNROLL
        for(int n3 = 0; n3 < R3; n3 += 2) {
            const f4 w = lds_ld4(lds, ex2_addr<G>(q, n3));
            v[b * R3 + n3] = cf{w.x, w.y};
            v[b * R3 + n3 + 1] = cf{w.z, w.w};
        }
    }
}

template<class G> WF_DEV void p3_pass3_write(int t, cf *lds, cf (&v)[G::P])
{
    constexpr int R1 = G::R1, R2 = G::R2, R3 = G::R3, B3 = G::B3, T = G::T;
    if constexpr(G::H3 == 2) {
        constexpr int HALF = R3 / 2, LBH = ilog2(HALF);
        static_assert((R1 * R2) % 4 == 0, "ex3 stride algebra");
        const int q = t & (R1 * R2 - 1), h = t / (R1 * R2);
        cf u[HALF];
        WF_UNROLL
        for(int j = 0; j < HALF; ++j)
            u[j] = v[j];
        dft_dif<HALF>(u);
        const int a3 = ex3_addr<G>(q + R1 * R2 * h); // == ex3_addr<G>(q + R1*R2*(2*kk + h)) - kk * ex3_step(2*R1*R2)
        WF_UNROLL
        for(int kk = 0; kk < HALF; ++kk)
            lds_st2(lds, a3 + kk * ex3_step<G>(2 * R1 * R2), u[brev(kk, LBH)]);
        return;
    }
    constexpr int LB = ilog2(R3);
    WF_UNROLL
    for(int b = 0; b < B3; ++b) {
        cf u[R3];
        WF_UNROLL
        for(int n3 = 0; n3 < R3; ++n3)
            u[n3] = v[b * R3 + n3];
        dft_dif<R3>(u);
        static_assert((R1 * R2) % 4 == 0, "ex3 stride algebra");
        const int q = t + T * b;
        const int a3 = ex3_addr<G>(q); // == ex3_addr<G>(q + R1*R2*k3) - k3 * ex3_step(R1*R2)
        WF_UNROLL
        for(int k3 = 0; k3 < R3; ++k3)
            lds_st2(lds, a3 + k3 * ex3_step<G>(R1 * R2), u[brev(k3, LB)]);
    }
}

// ---- P4: real split + epilogue ------------------------------------------------------------------
// Produces the smoothed linear magnitudes of bins 4g..4g+3 (g = t + T*u) in mag[u][0..3], updating the temporal-smoothing
// state on the way (reference :110-135).  The smoothing mode is a property of the configuration: the kernel branches on it
// once (a scalar branch) into a body compiled for it -- TS: m_tsmoothing != NONE, FPK: m_fast_peaks -- instead of testing
// mode bits per bin (which also made every conditionally loaded register a zero-initialised one).
//
// slope (reference :121-122) and temporal smoothing incl. fast peaks (:124-132) of bin group u; the slope table is all ones
// when m_slope <= 0.  st4v/sl4 are this group's m_tsmooth_buf / m_slope_modifiers values.
template<class G, bool TS, bool FPK>
WF_DEV void p4_slope_smooth_group(const TickArgs &a, int t, int u, float *ts, const float (&st4v)[4], const float (&sl4)[4],
                                  float (&mag)[G::P])
{
    constexpr int T = G::T;
    const int k0 = 4 * (t + T * u);
    WF_UNROLL
    for(int i = 0; i < 4; ++i)
        mag[4 * u + i] *= sl4[i];
    if(TS) {
        WF_UNROLL
        for(int i = 0; i < 4; ++i) {
            float old = st4v[i];
            if(FPK)
                old = fmaxf(mag[4 * u + i], old);
            // (g * oldval) + (g2 * mag) (reference :130); evaluated as fma(g, old, g2*mag) like the reference's own
            // AVX2 path (src/source_avx2.cpp:154) -- within 1 ulp of the generic path's separately rounded sum
            mag[4 * u + i] = spectrum_ema(a.g, old, a.g2, mag[4 * u + i]);
        }
        st_state(ts + k0, f4{mag[4 * u], mag[4 * u + 1], mag[4 * u + 2], mag[4 * u + 3]});
    }
}

struct NoMid { WF_DEV void operator()() const {} };
// mid(): called between the real split and the smoothing (whose state stores follow): where the kernel requests the display's
// tables -- in front of the stores in the memory pipeline, behind the registers' peak
template<class G, bool TS, bool FPK, class Mid = NoMid>
WF_DEV void p4_split_smooth_impl(const TickArgs &a, int t, const cf *lds, float *ts, const cf (&wb)[4], const P4Regs<G> &q,
                                 float (&mag)[G::P], Mid mid = Mid{})
{
    constexpr int M = G::M, T = G::T, P = G::P;
    // Threads that did not prefetch state/slope into registers earlier issue ALL of those loads now and consume them only
    // after the whole real split (two loops), so the split math covers their (L2) latency.
    constexpr bool LOAD_ALL_FIRST = !Policy<G>::PREFETCH_STATE;
    float st_all[LOAD_ALL_FIRST ? P : 4], sl_all[(LOAD_ALL_FIRST && !Policy<G>::SLOPE_LINEAR) ? P : 4];
    if(LOAD_ALL_FIRST) {
        WF_UNROLL
        for(int u = 0; u < P / 4; ++u) {
            const int k0 = 4 * (t + T * u);
            if(TS) {
                const f4 o = ld_state(ts + k0);
                st_all[4 * u] = o.x; st_all[4 * u + 1] = o.y; st_all[4 * u + 2] = o.z; st_all[4 * u + 3] = o.w;
            }
            if(!Policy<G>::SLOPE_LINEAR) {
                constexpr int S = Policy<G>::SLOPE_LINEAR ? 0 : 1;
                const f4 sv = ld4(a.slope + k0);
                sl_all[S * (4 * u)] = sv.x; sl_all[S * (4 * u + 1)] = sv.y; sl_all[S * (4 * u + 2)] = sv.z; sl_all[S * (4 * u + 3)] = sv.w;
            }
        }
    }
    // this group's state / slope operands, from wherever the policy put them
    auto group = [&](int u) {
        const int k0 = 4 * (t + T * u);
        float st4v[4] = {0.0f, 0.0f, 0.0f, 0.0f}, sl4[4];
        if(Policy<G>::PREFETCH_SLOPE) {
            WF_UNROLL
            for(int i = 0; i < 4; ++i)
                sl4[i] = q.sl[(Policy<G>::PREFETCH_SLOPE ? 1 : 0) * (4 * u + i)];
        } else if(LOAD_ALL_FIRST && Policy<G>::SLOPE_LINEAR) {
            WF_UNROLL // (formed, not loaded: Policy<G>::SLOPE_LINEAR)
            for(int i = 0; i < 4; ++i)
                sl4[i] = fmaf((float)(k0 + i), a.slope_step, 1.0f);
        } else if(LOAD_ALL_FIRST) {
            WF_UNROLL
            for(int i = 0; i < 4; ++i)
                sl4[i] = sl_all[(LOAD_ALL_FIRST ? 1 : 0) * (4 * u + i)];
        } else {
            const f4 o = ld4(a.slope + k0);
            sl4[0] = o.x; sl4[1] = o.y; sl4[2] = o.z; sl4[3] = o.w;
        }
        if(TS) {
            if(Policy<G>::PREFETCH_STATE) {
                WF_UNROLL
                for(int i = 0; i < 4; ++i)
                    st4v[i] = q.st[(Policy<G>::PREFETCH_STATE ? 1 : 0) * (4 * u + i)];
            } else if(LOAD_ALL_FIRST) {
                WF_UNROLL
                for(int i = 0; i < 4; ++i)
                    st4v[i] = st_all[(LOAD_ALL_FIRST ? 1 : 0) * (4 * u + i)];
            } else {
                const f4 o = ld_state(ts + k0);
                st4v[0] = o.x; st4v[1] = o.y; st4v[2] = o.z; st4v[3] = o.w;
            }
        }
        p4_slope_smooth_group<G, TS, FPK>(a, t, u, ts, st4v, sl4, mag);
    };
    // ---- loop 1: real split -> |2X| * coef/2 -------------------------------------------------------------------------
    // LDS addresses: bins advance by 4T per group, i.e. by T words inside every ex3 plane, so every group is the first
    // one's address plus a compile-time step.  Z[k0 + i] sits at aA[i]; the mirrored bins M - k0 - i at aB[i] - u*step,
    // except bin M - 0 = 0 for the very first bin of thread 0.
    int aA[4], aB[4];
    WF_UNROLL
    for(int i = 0; i < 4; ++i) {
        aA[i] = ex3_addr<G>(4 * t + i);
        aB[i] = ex3_addr<G>(M - 4 * t - i - 4 * T * (P / 4 - 1)); // the LAST group's address: offsets below stay non-negative
    }
    const int aB00 = ex3_addr<G>((M - 4 * t) & (M - 1));
    WF_UNROLL
    for(int u = 0; u < P / 4; ++u) {
        cf A[4];
        WF_UNROLL
        for(int i = 0; i < 4; ++i)
            A[i] = lds_ld2(lds, aA[i] + u * ex3_step<G>(4 * T));
        WF_UNROLL
        for(int i = 0; i < 4; ++i) {
            const cf W = mul_w32(wb[i], u * (64 / P)); // W_N^(k0 + i) = wb[i] * W_N^(4Tu)
            const cf B = lds_ld2(lds, (u == 0 && i == 0) ? aB00 : aB[i] + (P / 4 - 1 - u) * ex3_step<G>(4 * T));
            // 2X[k] = (A + conj B) - i W (A - conj B)
            const float er = A[i].x + B.x, ei = A[i].y - B.y;
            const float dr = A[i].x - B.x, di = A[i].y + B.y;
            const float pr = fmaf(W.x, dr, -(W.y * di)); // Re(W D)
            const float pi = fmaf(W.x, di, W.y * dr);    // Im(W D)
            const float xr = er + pi, xi = ei - pr;
            mag[4 * u + i] = mag2(xr, xi) * a.half_coef;
        }
        if(!LOAD_ALL_FIRST)
            group(u);
    }
    mid();
    // ---- loop 2: slope, temporal smoothing, state store ----------------------------------------------------------------
    if(LOAD_ALL_FIRST) {
        WF_UNROLL
        for(int u = 0; u < P / 4; ++u)
            group(u);
    }
}

template<class G, class Mid = NoMid>
WF_DEV void p4_split_smooth(const TickArgs &a, int t, const cf *lds, float *ts, const cf (&wb)[4], const P4Regs<G> &q, float (&mag)[G::P], Mid mid = Mid{})
{
    if(a.mode & WF_MODE_TSMOOTH) {
        if(a.mode & WF_MODE_FAST_PEAKS)
            p4_split_smooth_impl<G, true, true>(a, t, lds, ts, wb, q, mag, mid);
        else
            p4_split_smooth_impl<G, true, false>(a, t, lds, ts, wb, q, mag, mid);
    } else
        p4_split_smooth_impl<G, false, false>(a, t, lds, ts, wb, q, mag, mid);
}

// ---- decimated epilogue (DEC > 0): the N >> DEC point transform's bin o is bin o << DEC of the zero-padded one --------------
// Row geometry of the outputs: MO = M >> DEC bins, the first MO / 4 threads own four consecutive ones each.
template<int TT, int PP> struct RowG { static constexpr int T = TT, P = PP; };

template<class G, int DEC> WF_DEV void p4_prefetch_dec(const TickArgs &a, int t, const float *ts, P4Regs<G> &q)
{
    static_assert(Policy<G>::PREFETCH_STATE && Policy<G>::PREFETCH_SLOPE, "the decimated path runs on a one-wavefront geometry");
    constexpr int TO = (G::M >> DEC) / 4;
    const int tt = t < TO ? t : 0;
    if(a.mode & WF_MODE_TSMOOTH) {
        const f4 o = ld_state(ts + 4 * tt);
        q.st[0] = o.x; q.st[1] = o.y; q.st[2] = o.z; q.st[3] = o.w;
    }
    const f4 sv = ld4(a.slope + 4 * tt);
    q.sl[0] = sv.x; q.sl[1] = sv.y; q.sl[2] = sv.z; q.sl[3] = sv.w;
}

// Returns the four magnitudes by value (not through the caller's array): with the array written inside each of the three
// mode arms, ROCm 7.2's clang sinks the arms' last stores -- one into scratch, two into the state row -- into a single store
// through a pointer phi, a flat pointer its backend then fails to select ("Operand has incorrect register class").
template<class G, int DEC, bool TS, bool FPK>
WF_DEV f4 p4_split_smooth_dec_impl(const TickArgs &a, int t, const cf *lds, float *ts, const cf (&wb)[4], const P4Regs<G> &q)
{
    constexpr int M = G::M;
    float mag[4];
    WF_UNROLL
    for(int i = 0; i < 4; ++i) {
        const int k = (4 * t + i) << DEC;
        const cf A = lds_ld2(lds, ex3_addr<G>(k));
        const cf B = lds_ld2(lds, ex3_addr<G>((M - k) & (M - 1)));
        const cf W = wb[i];
        const float er = A.x + B.x, ei = A.y - B.y;
        const float dr = A.x - B.x, di = A.y + B.y;
        const float pr = fmaf(W.x, dr, -(W.y * di));
        const float pi = fmaf(W.x, di, W.y * dr);
        const float xr = er + pi, xi = ei - pr;
        float m = mag2(xr, xi) * a.half_coef;
        m *= q.sl[i];
        if(TS) {
            float old = q.st[i];
            if(FPK)
                old = fmaxf(m, old);
            m = spectrum_ema(a.g, old, a.g2, m);
        }
        mag[i] = m;
    }
    const f4 r = f4{mag[0], mag[1], mag[2], mag[3]};
    if(TS)
        st_state(ts + 4 * t, r);
    return r;
}
template<class G, int DEC>
WF_DEV void p4_split_smooth_dec(const TickArgs &a, int t, const cf *lds, float *ts, const cf (&wb)[4], const P4Regs<G> &q, float (&mag)[4])
{
    f4 r;
    if(a.mode & WF_MODE_TSMOOTH) {
        if(a.mode & WF_MODE_FAST_PEAKS)
            r = p4_split_smooth_dec_impl<G, DEC, true, true>(a, t, lds, ts, wb, q);
        else
            r = p4_split_smooth_dec_impl<G, DEC, true, false>(a, t, lds, ts, wb, q);
    } else
        r = p4_split_smooth_dec_impl<G, DEC, false, false>(a, t, lds, ts, wb, q);
    mag[0] = r.x; mag[1] = r.y; mag[2] = r.z; mag[3] = r.w;
}

// dB conversion + volume normalisation + roll-off of this thread's bins (reference :144-179); d[] is the
// final m_decibels content, stored by store_row()
// GUARD (rows shorter than T * P bins: the Bluestein path): groups of four bins at or beyond `nb` are skipped
template<class G, bool GUARD = false>
WF_DEV void p4_db(const TickArgs &a, int t, const float (&mag)[G::P], float (&d)[G::P], float vol_comp, int nb = 0, int kbase = 0)
{
    constexpr int T = G::T, P = G::P;
    // roll-off row: all of this thread's vectors requested before the first logarithm -- one round trip to L2 under the dB
    // math instead of one per group of four bins, each waited for on the spot
    f4 roll[P / 4];
    if(a.mode & WF_MODE_ROLLOFF) {
        WF_UNROLL
        for(int u = 0; u < P / 4; ++u) {
            const int k0 = 4 * (t + T * u);
            roll[u] = (GUARD && k0 >= nb) ? f4{0.0f, 0.0f, 0.0f, 0.0f} : ld4(a.rolloff + k0 + kbase);
        }
    }
    WF_UNROLL
    for(int u = 0; u < P / 4; ++u) {
        int k0 = 4 * (t + T * u);
        if(GUARD && k0 >= nb)
            continue;
        k0 += kbase; // rows longer than T * P bins are finished in parts (wf_big.hpp): the bin index of the whole row
        WF_UNROLL
        for(int i = 0; i < 4; ++i)
            d[4 * u + i] = dbfs(mag[4 * u + i], a.db_min);
        if(a.mode & WF_MODE_NORMALIZE) {
            WF_UNROLL
            for(int i = 0; i < 4; ++i)
                if(k0 + i >= 1) // the generic path starts at i = 1 (reference :165)
                    d[4 * u + i] += vol_comp;
        }
    }
    if(a.mode & WF_MODE_ROLLOFF) {
        WF_UNROLL
        for(int u = 0; u < P / 4; ++u) {
            const int k0 = 4 * (t + T * u);
            if(GUARD && k0 >= nb)
                continue;
            const float rr[4] = {roll[u].x, roll[u].y, roll[u].z, roll[u].w};
            WF_UNROLL
            for(int i = 0; i < 4; ++i)
                if(k0 + kbase + i >= 1) // reference :173
                    d[4 * u + i] = fmaxf(d[4 * u + i] - rr[i], a.db_min);
        }
    }
}

template<class G, bool GUARD = false, bool NT = false> WF_DEV void store_row(float *row, int t, const float (&d)[G::P], int nb = 0)
{
    constexpr int T = G::T, P = G::P;
    WF_UNROLL
    for(int u = 0; u < P / 4; ++u)
        if(!GUARD || 4 * (t + T * u) < nb) {
            if constexpr(NT)
                st4_nt(row + 4 * (t + T * u), f4{d[4 * u], d[4 * u + 1], d[4 * u + 2], d[4 * u + 3]});
            else
                st4(row + 4 * (t + T * u), f4{d[4 * u], d[4 * u + 1], d[4 * u + 2], d[4 * u + 3]});
        }
}
// ---- silence state machine helpers (reference :63-95, :138-139) ------------------------------------
// "outsilent": every value of the previously displayed row is <= floor - 10.  Each thread looks at the
// bins it owns in the P4 layout; the caller and-reduces over the spectrum's threads.
template<class G, bool GUARD = false> WF_DEV bool row_all_below(const float *row, int t, float limit, int nb = 0)
{
    constexpr int T = G::T, P = G::P;
    bool below = true;
    WF_UNROLL
    for(int u = 0; u < P / 4; ++u) {
        if(GUARD && 4 * (t + T * u) >= nb)
            continue;
        const f4 d = ld4(row + 4 * (t + T * u));
        below = below && !(d.x > limit) && !(d.y > limit) && !(d.z > limit) && !(d.w > limit);
    }
    return below;
}

// a skipped channel of a stream that is not silent: the reference's end-of-tick dB pass runs over its
// *stale* m_decibels row again; load that row as the "magnitudes"
template<class G, bool GUARD = false> WF_DEV void load_row(const float *row, int t, float (&mag)[G::P], int nb = 0)
{
    constexpr int T = G::T, P = G::P;
    WF_UNROLL
    for(int u = 0; u < P / 4; ++u) {
        if(GUARD && 4 * (t + T * u) >= nb)
            continue;
        const f4 d = ld4(row + 4 * (t + T * u));
        mag[4 * u] = d.x; mag[4 * u + 1] = d.y; mag[4 * u + 2] = d.z; mag[4 * u + 3] = d.w;
    }
}

template<class G, bool GUARD = false> WF_DEV void fill_row(float *row, int t, float v, int nb = 0)
{
    constexpr int T = G::T, P = G::P;
    WF_UNROLL
    for(int u = 0; u < P / 4; ++u)
        if(!GUARD || 4 * (t + T * u) < nb)
            st4(row + 4 * (t + T * u), f4{v, v, v, v});
}

// The per-stream decision of the channel loop, replayed from the per-channel facts.
//   last_silent : m_last_silent on entry
//   nz[c]       : channel c's window has a non-zero sample
//   below[c]    : the row the reference inspects for channel c (m_decibels[stereo ? c : 0] as left by the
//                 previous tick) is entirely <= floor - 10
// Outputs process[c] (run the FFT path for channel c) and the new m_last_silent.
struct StreamPlan { bool process0, process1; bool last_silent; };
WF_DEV StreamPlan plan_stream(bool last_silent, uint32_t cap_ch, bool stereo, bool nz0, bool nz1, bool below0, bool below1)
{
    StreamPlan p;
    p.process0 = p.process1 = false;
    bool ls = last_silent;
    uint32_t silent_channels = 0;
    // channel 0
    if(nz0) {
        ls = false;              // reference :68-69
        p.process0 = true;
    } else if(!ls) {             // :76-77
        if(below0) {             // :78-94
            if(++silent_channels >= cap_ch)
                ls = true;
        } else
            p.process0 = true;
    }
    // channel 1
    if(cap_ch > 1) {
        if(nz1) {
            ls = false;
            p.process1 = true;
        } else if(!ls) {
            // In mono display mode channel 1 inspects row 0, which channel 0 has just overwritten with linear
            // magnitudes (>= 0 > floor - 10) if it was processed in this tick.
            const bool outsilent = below1 && !(!stereo && p.process0);
            if(outsilent) {
                if(++silent_channels >= cap_ch)
                    ls = true;
            } else
                p.process1 = true;
        }
    }
    p.last_silent = ls;
    return p;
}

} // namespace wf
