// wf_tick_display.hpp -- the display phase of the fused tick: what render_bars / render_curve derive from the dB row a spectrum
// has just produced (reference src/source.cpp:1360-1425, 1500-1564) -- bars in the segment, piece and prefix-sum layouts, curves
// (Lanczos tables, Catmull-Rom on the fly), the Gaussian filter, the dB -> pixel mapping.  The tables it reads: BarArgs
// (wf_tick_args.hpp), built by wf_host_tables.cpp.
#pragma once
#include "wf_tick_phases.hpp"
#include "wf_dev_guard.hpp" // WF_BAR_STAMP exists under WF_PHASE_TIMING

#ifdef WF_PHASE_TIMING
#define WF_BAR_STAMP(i) do { if(t == 0 && b.clk) b.clk[i] = __builtin_readcyclecounter(); } while(0)
#else
#define WF_BAR_STAMP(i)
#endif

namespace wf {

// ---- bars (render_bars interpolation + dB -> pixel mapping, reference src/source.cpp:1500-1557) -------

// All T threads of a spectrum reduce the bars of one displayed row.
//   db   : the row's dB values in LDS (float[M]);  prod: LDS scratch for the products (capacity checked on the host)
//   sync : barrier over the spectrum's threads;  xor_sum(v, m): v + (v of lane ^ m) for m < 64 (wave shuffle)
// What a thread needs to know about "its" bar in the first pass of the first chunk (bar = t / lanes_per_bar).  Fetched at
// the very start of the kernel with the audio window, so that the bars phase at the end does not begin with a chain of
// dependent table loads.
struct BarPre { int off, len, count; int s0, s1; int glen; int lead; };
template<class G, bool PIECES = true, bool PS_OK = true> WF_DEV BarPre bars_preload(const BarArgs &b, int t)
{
    BarPre p{0, 0, 1, 0, 0, 0, -1};
    if(b.out != nullptr && !(PS_OK && b.ps_lanes > 0)) { // (the prefix-sum layout keeps everything in its lane table: bars_fetch_entries)
        if(PIECES && b.num_segs > 0 && b.piece_mode) {
            // glen: the scan flags and 1 + the slot this lane's piece total goes to.  One wavefront per spectrum: the slot is the
            // bar itself (lead / count); several: lane l of whichever wavefront arrives last finishes bar l from slots [s0, s1)
            p.glen = b.seg_group[t];
            if(G::T == 64) {
                p.lead = (int)((uint32_t)p.glen >> 8) - 1;
                if(p.lead >= 0)
                    p.count = b.count[p.lead];
            } else if((t & 63) < b.num_bars) {
                p.lead = t & 63;
                p.s0 = b.bar_seg[p.lead];
                p.s1 = b.bar_seg[p.lead + 1];
                p.count = b.count[p.lead];
            }
        } else if(b.num_segs > 0 && b.wave_local) { // the bar this thread leads, if any
            p.lead = b.lead_bar[t];
            p.s0 = t;
            p.s1 = b.lead_end[t]; // one past the last segment of this thread's bar
            if(p.lead >= 0)
                p.count = b.count[p.lead];
        } else if(b.num_segs > 0) { // bar t's segment range
            p.glen = b.seg_group[t];
            if(t < b.num_bars) {
                p.s0 = b.bar_seg[t];
                p.s1 = b.bar_seg[t + 1];
                p.count = b.count[t];
            }
        } else {
            const int bar = t / b.lanes_per_bar;
            if(bar < b.num_bars) {
                p.off = b.off[bar];
                p.len = b.off[bar + 1] - p.off;
                p.count = b.count[bar];
            }
        }
    }
    return p;
}

// The (coefficient, bin) pairs of this thread's segment: 16-byte loads, coalesced across the threads, requested before
// the dB math so that their L2 latency is off the critical path.
template<class G> struct BarEntries {
    static constexpr int CMAX = G::P / 4 + 2; // the host builds segments of at most 4 * CMAX entries; the prefix-sum layout's lane table is three words
    f4 coef[CMAX];
    int base;
};
template<class G, bool PS_OK = true, bool PS_ONLY = false> WF_DEV void bars_fetch_entries(const BarArgs &b, int t, BarEntries<G> &be, bool finisher = false)
{
    constexpr int T = G::T;
    be.base = 0;
    if constexpr(PS_ONLY) { // (the instantiation displays bars in the prefix-sum layout and nothing else: spectrum_tick_kernel<.., DISP = 1>)
        if(finisher) { // wave-uniform
            const float *p = b.ps_tab + (size_t)(t & 63) * 4;
            WF_UNROLL
            for(int c = 0; c < 3; ++c)
                be.coef[c] = ld4(p + c * 256);
        }
        return;
    }
    if constexpr(!PS_OK) { // (the instantiation never runs the prefix-sum layout -- the Bluestein / mixed-radix kernels at their register caps)
        if(b.out == nullptr || b.num_segs == 0)
            return;
        be.base = b.lane_base[t];
        WF_UNROLL
        for(int c = 0; c < BarEntries<G>::CMAX; ++c)
            if(c < b.lane_blocks) // uniform
                be.coef[c] = ld4(b.lane_coef + (c * T + t) * 4);
        return;
    }
    if(b.out == nullptr || (b.num_segs == 0 && b.ps_lanes == 0))
        return;
    // One loop for both layouts (two loops writing the one array left half of it in scratch: ROCm 7.2's SROA gives up on the phi).
    // Prefix-sum layout: the three 16-byte words of this lane's sub-band edge (BarPsTables), requested only by the wavefront that
    // finishes sub-bands (`finisher`, wave-uniform).
    const bool ps = b.ps_lanes > 0;
    const float *p = ps ? b.ps_tab + (size_t)(t & 63) * 4 : b.lane_coef + (size_t)t * 4;
    const int stride = ps ? 256 : T * 4;
    int n = ps ? (finisher ? 3 : 0) : b.lane_blocks;
#if defined(__HIPCC__)
    n = __builtin_amdgcn_readfirstlane(n);
#endif
    if(!ps)
        be.base = b.lane_base[t];
    WF_UNROLL
    for(int c = 0; c < BarEntries<G>::CMAX; ++c)
        if(c < n) // uniform
            be.coef[c] = ld4(p + c * stride);
}

// mean dB of output o -> pixel row (reference src/source.cpp:1548-1557 bars, :1411 curve):
// y = lerp(border_top, border_bottom, clamp(ceiling - v, 0, range) / range).  Straight-line code: the quotient is
// tt * (1 / range) corrected by one residual step (q + fma(-q, range, tt) * inv: the correctly rounded quotient but for
// rare last-bit ties), and std::lerp's case distinction on the signs of its end points is a property of the configuration
// (BarArgs::lerp_mixed) -- testing it per output cost a dozen scalar branches per point.
WF_DEV float map_output(const BarArgs &b, float v)
{
    float tt = b.ceiling - v; // reference src/source.cpp:1550
    tt = fminf(fmaxf(tt, 0.0f), b.dbrange);
    float q = tt * b.inv_dbrange;
    q = fmaf(fmaf(-q, b.dbrange, tt), b.inv_dbrange, q);
    if(b.lerp_mixed) // border_top <= 0 <= border_bottom (or the reverse): t * b + (1 - t) * a
        return q * b.border_bottom + (1.0f - q) * b.border_top;
    return lerp_std(b.border_top, b.border_bottom, q);
}
// stores incl. the mirrored image (:1559-1564, :1419-1424): outputs above the middle repeat the lower ones
WF_DEV void put_output(const BarArgs &b, float *row, int o, float y)
{
    row[o] = y;
    WF_UNROLL
    for(int j = 0; j < 8; ++j) // (constant indices: indexed by a run-time j the kernel's argument block went to scratch, 784 B per lane)
        if(j < b.out2_n) // uniform
            row[(long long)o + b.out2_delta[j]] = y;
}
WF_DEV void store_output(const BarArgs &b, int o, float y, float *out_row, float *dup_row)
{
    if(!b.mirror) {
        put_output(b, out_row, o, y);
        if(dup_row) put_output(b, dup_row, o, y);
        return;
    }
    const int half = b.num_bars / 2;
    const int img = 2 * half - o;
    const bool own = o <= half;
    const bool image = o < half && img > half && img < b.num_bars;
    if(o == half + 1 && b.pre_out != nullptr) { // (one lane per row; the caller has pointed pre_out at this row's entry: BarArgs::pre_out)
        b.pre_out[0] = y;
        if(dup_row) b.pre_out[1] = y; // (the second row of a single captured channel shown as stereo: the next entry)
    }
    if(own) {
        put_output(b, out_row, o, y);
        if(dup_row) put_output(b, dup_row, o, y);
    }
    if(image) {
        put_output(b, out_row, img, y);
        if(dup_row) put_output(b, dup_row, img, y);
    }
}
WF_DEV void emit_output(const BarArgs &b, int o, float v, float *out_row, float *dup_row)
{
    store_output(b, o, map_output(b, v), out_row, dup_row);
}

// the outputs (bars or curve points) thread t finishes: o = t + T*k, k < out_steps <= KMAX
template<class G> struct OutVals {
    static constexpr int KMAX = (G::T <= 64) ? 16 : 8; // 1024 outputs per row on one wavefront, 8 per thread otherwise
    float v[KMAX];
};

// curve points of this thread from the dB row parked in LDS.  Steps are taken four at a time: the (L2) table loads of a
// group are issued together; the tables are padded to whole groups with zero coefficients.
// (TT: threads that share the row -- G::T, or 2 * G::T when the threads of both spectra of a workgroup finish the one row a
// mono mixdown displays, BarArgs::both_subs)
template<class G, int TT = G::T> WF_DEV void curve_row(const BarArgs &b, bool has_row, const float *db, int t, OutVals<G> &ov)
{
    constexpr int T = TT, K = OutVals<G>::KMAX;
    static_assert(K % 4 == 0, "curve steps are processed in groups of four");
    WF_UNROLL
    for(int k = 0; k < K; ++k)
        ov.v[k] = 0.0f;
    WF_UNROLL
    for(int g = 0; g < K / 4; ++g) {
        if(4 * g < b.out_steps && has_row) { // the first condition is uniform
            f4 c0[4], c1[4];
            int base[4];
            WF_UNROLL
            for(int j = 0; j < 4; ++j) {
                const int o = (4 * g + j) * T + t;
                c0[j] = ld4(b.cur_coef + 8 * o);
                c1[j] = ld4(b.cur_coef + 8 * o + 4);
                base[j] = b.cur_base[o];
            }
            WF_UNROLL
            for(int j = 0; j < 4; ++j) {
                const float *p = db + base[j];
                // kernel_convolve (reference src/filter.hpp:160-169): sum += samples[i] * weight, ascending taps
                float sum = p[0] * c0[j].x;
                sum = fmaf(p[1], c0[j].y, sum);
                sum = fmaf(p[2], c0[j].z, sum);
                sum = fmaf(p[3], c0[j].w, sum);
                sum = fmaf(p[4], c1[j].x, sum);
                sum = fmaf(p[5], c1[j].y, sum);
                sum = fmaf(p[6], c1[j].z, sum);
                sum = fmaf(p[7], c1[j].w, sum);
                ov.v[4 * g + j] = sum;
            }
        }
    }
}

// make_catrom_kernel's weights for u = x - floor(x), tension 0.5, evaluated as the reference does: sum += row[k] * matrix[j][k]
// over row = {1, u, u*u, u*u*u}, separately rounded products and sums (the zero matrix entries add exact zeros)
struct CatromW { float w0, w1, w2, w3; };
WF_DEV CatromW catrom_weights(float u)
{
#pragma clang fp contract(off) // every product and sum rounded on its own, as the reference's table was computed
    const float u2 = u * u, u3 = u2 * u;
    CatromW c;
    c.w0 = ((u * -0.5f) + u2) + (u3 * -0.5f);          // {0, -t, 2t, -t}
    c.w1 = (1.0f + (u2 * -2.5f)) + (u3 * 1.5f);        // {1, 0, t-3, 2-t}
    c.w2 = ((u * 0.5f) + (u2 * 2.0f)) + (u3 * -1.5f);  // {0, t, 3-2t, t-2}
    c.w3 = (u2 * -0.5f) + (u3 * 0.5f);                 // {0, 0, -t, t}
    return c;
}
// one Catmull-Rom point: kernel_convolve (reference src/filter.hpp:160-169) over taps floor(x) - 1 .. floor(x) + 2.  The
// positions lie in [1, M - 1] (init_interp clamps them to [lowbin, highbin]), so only the taps at M and M + 1 can fall
// outside the row: the caller parks two zeros there (a dropped tap adds an exact 0).
WF_DEV float catrom_point(const float *db, float x)
{
#pragma clang fp contract(off)
    const float fl = __builtin_floorf(x);
    const CatromW c = catrom_weights(x - fl);
    const float *p = db + ((int)fl - 1);
    float sum = p[0] * c.w0;
    sum = sum + (p[1] * c.w1);
    sum = sum + (p[2] * c.w2);
    sum = sum + (p[3] * c.w3);
    return sum;
}
template<class G, int TT = G::T> WF_DEV void curve_row_catrom(const BarArgs &b, bool has_row, const float *db, int t, OutVals<G> &ov)
{
    constexpr int T = TT, K = OutVals<G>::KMAX;
    WF_UNROLL
    for(int k = 0; k < K; ++k)
        ov.v[k] = 0.0f;
    // (requesting the positions before the dB math, as the bars' entries are, measured 8 % slower: the loads queue ahead
    // of the row stores)
    WF_UNROLL
    for(int g = 0; g < K / 4; ++g) {
        if(4 * g < b.out_steps && has_row) { // the first condition is uniform
            float x[4];
            WF_UNROLL
            for(int j = 0; j < 4; ++j)
                x[j] = b.cur_x[(4 * g + j) * T + t];
            WF_UNROLL
            for(int j = 0; j < 4; ++j)
                ov.v[4 * g + j] = catrom_point(db, x[j]);
        }
    }
}

// Curves wider than KMAX points per thread: a run-time loop over the steps; every point is mapped and stored as soon as it
// is produced, or -- with the Gaussian filter on -- staged behind the dB row ([pad | points | pad | weights] from
// db + stage_off, sized on the host) and filtered in a second loop.
template<class G, int TT = G::T, class Sync>
WF_DEV void curve_row_stream(const BarArgs &b, bool has_row, const float *db, float *lds, int t, float *out_row, float *dup_row, Sync sync)
{
    constexpr int T = TT;
    const int n = b.num_bars;
    const bool filtered = b.gauss_radius > 0;
    const int pad = b.gauss_radius - 1, size = 2 * b.gauss_radius - 1;
    float *vp = lds + b.stage_off;
    float *wl = vp + n + 2 * pad;
    if(filtered && has_row) {
        for(int i = t; i < pad; i += T) {
            vp[i] = 0.0f;
            vp[pad + n + i] = 0.0f;
        }
        for(int i = t; i < size; i += T)
            wl[i] = b.gauss[i];
    }
    if(has_row) {
        for(int k = 0; k < b.out_steps; ++k) {
            const int o = k * T + t;
            float v;
            if(b.curve == 2) {
                v = catrom_point(db, b.cur_x[o]);
            } else {
                const f4 c0 = ld4(b.cur_coef + 8 * o), c1 = ld4(b.cur_coef + 8 * o + 4);
                const float *p = db + b.cur_base[o];
                v = p[0] * c0.x;
                v = fmaf(p[1], c0.y, v);
                v = fmaf(p[2], c0.z, v);
                v = fmaf(p[3], c0.w, v);
                v = fmaf(p[4], c1.x, v);
                v = fmaf(p[5], c1.y, v);
                v = fmaf(p[6], c1.z, v);
                v = fmaf(p[7], c1.w, v);
            }
            if(o < n) {
                if(filtered)
                    vp[pad + o] = v;
                else
                    emit_output(b, o, v, out_row, dup_row);
            }
        }
    }
    if(filtered) {
        sync();
        if(has_row) {
            for(int o = t; o < n; o += T) {
                float sum = 0.0f;
                for(int tap = 0; tap < size; ++tap)
                    sum = fmaf(vp[o + tap], wl[tap], sum);
                emit_output(b, o, sum / b.gauss_wsum[o], out_row, dup_row);
            }
        }
    }
}

// optional Gaussian filter across the row's outputs, then mapping + stores.  `lds` is the spectrum's LDS as floats; it may
// alias everything the row used before (the dB row, the partials) and is written only after a barrier.
// weighted_avg (reference src/filter.hpp:133-157) divides the tap sum by the sum of the weights whose taps fall inside the
// row.  Here the row is staged with radius-1 zeros on either side (a dropped tap adds an exact 0), the weights sit next
// to it, and the divisor of every output comes from a table the host accumulated in the reference's order -- so the
// inner loop is one LDS read and one FMA per tap, no bounds logic.
template<class G, int TT = G::T, class Sync>
WF_DEV void outputs_finish(const BarArgs &b, bool has_row, OutVals<G> &ov, float *lds, int t, float *out_row, float *dup_row, Sync sync)
{
    constexpr int T = TT, K = OutVals<G>::KMAX;
    static_assert(K % 4 == 0, "outputs are filtered in groups of four");
    const int n = b.num_bars;
    if(b.gauss_radius > 0) {
        const int pad = b.gauss_radius - 1, size = 2 * b.gauss_radius - 1;
        float *vp = lds;               // [pad | n | pad]
        float *wl = lds + n + 2 * pad; // [size]
        sync();
        // only the spectrum that has a row stages anything: in mono display channel 1's buffer is what channel 0 reads the
        // partner's magnitudes from, and on the one-wavefront geometries nothing orders that read before this point
        if(has_row) {
            for(int i = t; i < pad; i += T) {
                vp[i] = 0.0f;
                vp[pad + n + i] = 0.0f;
            }
            for(int i = t; i < size; i += T)
                wl[i] = b.gauss[i];
        }
        if(has_row) {
            WF_UNROLL
            for(int k = 0; k < K; ++k)
                if(k < b.out_steps && k * T + t < n)
                    vp[pad + k * T + t] = ov.v[k];
        }
        sync();
        if(has_row) {
            WF_UNROLL
            for(int g = 0; g < K / 4; ++g) {
                if(4 * g < b.out_steps) { // uniform
                    float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    int o[4];
                    float div[4];
                    WF_UNROLL
                    for(int j = 0; j < 4; ++j) {
                        o[j] = (4 * g + j) * T + t;
                        if(o[j] >= n)
                            o[j] = n - 1; // lanes past the end redo the last output; their result is not stored
                        div[j] = b.gauss_wsum[o[j]];
                    }
                    for(int tap = 0; tap < size; ++tap) {
                        const float w = wl[tap];
                        WF_UNROLL
                        for(int j = 0; j < 4; ++j)
                            sum[j] = fmaf(vp[o[j] + tap], w, sum[j]);
                    }
                    WF_UNROLL
                    for(int j = 0; j < 4; ++j)
                        ov.v[4 * g + j] = sum[j] / div[j];
                }
            }
        }
    }
    if(has_row) {
        float y[K];
        WF_UNROLL
        for(int k = 0; k < K; ++k)
            y[k] = map_output(b, ov.v[k]); // all of them, branch-free; the ones past the row are not stored
        WF_UNROLL
        for(int k = 0; k < K; ++k)
            if(k < b.out_steps && k * T + t < n)
                store_output(b, k * T + t, y[k], out_row, dup_row);
    }
}

// ---- bars, prefix-sum layout (BarPsTables, wf_host_tables.hpp) ---------------------------------------------------------------
// The tick of a bars display is as much bound by the vector units as by memory (cut-point builds, profiles/r05b_ps_cuts*.txt: 100
// more instructions per wavefront in the tail cost what they add to its ~1200, 8 %), so the layout is built around instruction
// count: every wavefront only parks its part of the row and the sums of its four-bin groups (12 additions, five 16-byte LDS
// stores); ONE wavefront finishes -- for both spectra of a workgroup where the sub-bands fit 32 lanes each -- and it alone forms
// the prefix sum, over 16-bin quads, in float64.
// A spectrum's LDS in this layout, as floats from `dbl`: [4 zeros | the row's M dB values | 4 zeros] (bins -4 .. M + 3: the taps
// kernel_convolve drops read an exact 0), then gs[M / 4] = the four-bin group sums, thread-major (group g = bin / 4 = t + T u of
// thread t, register group u, sits at t (P / 4) + u: one 16-byte store per thread), then qp[M / 16 + 1] doubles: the sum of all
// quads in front of quad Q (the last entry: the row's total).
WF_DEV float *ps_gs_area(float *dbl, int M) { return dbl + 8 + M; }
WF_DEV double *ps_qp_area(float *dbl, int M) { return reinterpret_cast<double *>(dbl + 8 + M + M / 4); }
template<class RG> WF_DEV void ps_park(float *dbl, int M, int t, const float (&d)[RG::P])
{
    constexpr int NG = RG::P / 4;
    static_assert(NG == 1 || NG == 2 || NG % 4 == 0, "group sums are stored as 4-, 8- or 16-byte words");
    store_row<RG>(dbl + 4, t, d);
    float *gs = ps_gs_area(dbl, M) + t * NG;
    float s[NG];
    WF_UNROLL
    for(int u = 0; u < NG; ++u)
        s[u] = (d[4 * u] + d[4 * u + 1]) + (d[4 * u + 2] + d[4 * u + 3]);
    if constexpr(NG == 1)
        gs[0] = s[0];
    else if constexpr(NG == 2)
        *reinterpret_cast<f2 *>(gs) = f2{s[0], s[1]};
    else {
        WF_UNROLL
        for(int u = 0; u < NG; u += 4)
            st4(gs + u, f4{s[u], s[u + 1], s[u + 2], s[u + 3]});
    }
    if(t == 0) {
        st4(dbl, f4{0.0f, 0.0f, 0.0f, 0.0f});
        st4(dbl + 4 + M, f4{0.0f, 0.0f, 0.0f, 0.0f});
    }
}
// Inclusive prefix of a double over the 64 lanes of a wavefront: the classic six DPP steps (row_shr 1, 2, 4, 8 inside rows of 16,
// row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3) on the two halves of the value; a lane without a source adds +0.0
WF_DEV double wave_scan_f64(double v)
{
#if defined(__HIPCC__)
#define WF_SCAN64_STEP(CTRL, ROWS)                                                                                         \
    {                                                                                                                      \
        const long long b = __double_as_longlong(v);                                                                       \
        const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, ROWS, 0xf, true);                     \
        const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROWS, 0xf, true);                              \
        v += __longlong_as_double(((long long)hi << 32) | (long long)(unsigned int)lo);                                    \
    }
    WF_SCAN64_STEP(0x111, 0xf)
    WF_SCAN64_STEP(0x112, 0xf)
    WF_SCAN64_STEP(0x114, 0xf)
    WF_SCAN64_STEP(0x118, 0xf)
    WF_SCAN64_STEP(0x142, 0xa)
    WF_SCAN64_STEP(0x143, 0xc)
#undef WF_SCAN64_STEP
#endif
    return v;
}
// the value of lane l ^ 1 (quad_perm:[1,0,3,2])
WF_DEV int lane_swap1(int v)
{
#if defined(__HIPCC__)
    return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true);
#else
    return v;
#endif
}
// The finishing wavefront of a spectrum: lane `ll` (i) adds the group sums of its share of the quads and leaves their float64
// prefix in LDS, (ii) evaluates one edge of sub-band ll / 2 -- the look-up at its position and the dot product of its window --;
// the edges meet on the even lane, the sub-bands of a bar by the segmented scan, and the lane that finishes a bar maps and stores
// it.  (`emit` false: the spectrum produced no row -- everything is computed on whatever the buffer holds and nothing is stored;
// the DPP steps must not sit under a divergent branch.)
template<class G, class RG> WF_DEV void ps_finish(const BarArgs &b, const BarEntries<G> &be, float *dbl, int M, int ll, bool emit, float *out_row, float *dup_row)
{
    constexpr int T = RG::T, NG = RG::P / 4;
    const float *gs = ps_gs_area(dbl, M);
    double *qp = ps_qp_area(dbl, M);
    // group g = t + T u is stored at t NG + u; the four groups of quad Q are four consecutive threads of one register group
    auto quad_groups = [&](int Q) { const int g0 = 4 * Q; return gs + (g0 & (T - 1)) * NG + g0 / T; };
    constexpr int QUADS = G::M / 16, NQ = (QUADS + 63) / 64;
    double run = 0.0, ex[NQ];
    WF_UNROLL
    for(int k = 0; k < NQ; ++k) {
        const int Q = ll * NQ + k;
        const float *p = quad_groups(Q < QUADS ? Q : 0);
        const float qt = (p[0] + p[NG]) + (p[2 * NG] + p[3 * NG]);
        ex[k] = run;
        run += (double)((QUADS % 64 == 0 || Q < QUADS) ? qt : 0.0f);
    }
    const double inc = wave_scan_f64(run), base = inc - run;
    WF_UNROLL
    for(int k = 0; k < NQ; ++k) {
        const int Q = ll * NQ + k;
        if(QUADS % 64 == 0 || Q < QUADS)
            qp[Q] = base + ex[k];
    }
    if(ll == 63)
        qp[QUADS] = inc;
    wave_fence(); // (LDS operations of a wavefront execute in order: the look-ups below see the prefix)
    const int q = (int)f32_bits(be.coef[2].x);
    const uint32_t info = f32_bits(be.coef[2].y);
    const float *pw = dbl + q + 1; // bins q - 3 .. q + 3 of the row parked from dbl + 4
    float w[7];
    WF_UNROLL
    for(int j = 0; j < 7; ++j)
        w[j] = pw[j];
    // PS[min(q + 4, M)]: the quads in front (float64), the groups of the quad in front, the bins of the group in front (the top
    // three of the window; a clamped position is a multiple of 16)
    const int x = q + 4 < M ? q + 4 : M;
    const int ng = (x >> 2) & 3, nb = x & 3;
    const float *pg = quad_groups(x >> 4);
    double f = qp[x >> 4];
    f += (double)(ng >= 1 ? pg[0] : 0.0f);
    f += (double)(ng >= 2 ? pg[NG] : 0.0f);
    f += (double)(ng >= 3 ? pg[2 * NG] : 0.0f);
    f += (double)(nb >= 1 ? w[6] : 0.0f);
    f += (double)(nb >= 2 ? w[5] : 0.0f);
    f += (double)(nb >= 3 ? w[4] : 0.0f);
    float e0 = w[0] * be.coef[0].x, e1 = w[1] * be.coef[0].y;
    e0 = fmaf(w[2], be.coef[0].z, e0);
    e1 = fmaf(w[3], be.coef[0].w, e1);
    e0 = fmaf(w[4], be.coef[1].x, e0);
    e1 = fmaf(w[5], be.coef[1].y, e1);
    e0 = fmaf(w[6], be.coef[1].z, e0);
    const float e = e0 + e1;
    // the high edge's prefix and window sum come over from the odd lane
    const long long fb = __builtin_bit_cast(long long, f);
    const long long ob = ((long long)lane_swap1((int)(fb >> 32)) << 32) | (long long)(unsigned int)lane_swap1((int)(fb & 0xffffffffll));
    const float oe = __builtin_bit_cast(float, lane_swap1(__builtin_bit_cast(int, e)));
    const double dp = __builtin_bit_cast(double, ob) - f;
    float sub = (ll & 1) ? 0.0f : fmaf(be.coef[1].w, (float)dp, e + oe);
    sub = seg_prefix_scan(sub, info);
    const int bar = (int)((info >> 8) & 0xffu) - 1;
    if(emit && bar >= 0)
        emit_output(b, bar, sub / (float)(info >> 16), out_row, dup_row);
}

// Called by every thread of the workgroup (sync may be a block barrier); `has_row` says whether this spectrum produced one.
// Returns true when the bars were left in `ov` for outputs_finish (one bar per thread, k = 0), false when they have already
// been mapped and stored (chunked path; no filter there).
// arrivals / arrive_last (piece mode, several wavefronts per spectrum): the spectrum's arrival counter in LDS and the value it
// reads once every wavefront of the spectrum has counted itself in for the last time
// PIECES == false: the instantiation never runs the wave-private layout (the Bluestein kernels, at their register cap: the host
// does not build it for them)
template<class G, bool PIECES = true, class Sync, class XorSum>
WF_DEV bool bars_reduce_row(const BarArgs &b, const BarPre &pre, const BarEntries<G> &be, bool has_row, float *db, float *prod, int t,
                            float *out_row, float *dup_row, OutVals<G> &ov, Sync sync, XorSum xor_sum, int *arrivals = nullptr, int arrive_last = 0)
{
    constexpr int T = G::T;
    auto emit = [&](int bar, float sum, int cnt) { emit_output(b, bar, sum / (float)cnt, out_row, dup_row); };
    if(b.num_segs > 0) {
        // A: every thread forms the dot product of its own segment (padded bins have coefficient 0) -- four
        // independent partial sums in entry order
        float part = 0.0f;
        if(has_row) {
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
            const float *p = db + be.base;
            WF_UNROLL
            for(int cc = 0; cc < BarEntries<G>::CMAX; ++cc) {
                if(cc < b.lane_blocks) { // uniform
                    const f4 w = be.coef[cc];
                    const f4 v = *reinterpret_cast<const f4 *>(p + 4 * cc);
                    a0 = fmaf(v.x, w.x, a0);
                    a1 = fmaf(v.y, w.y, a1);
                    a2 = fmaf(v.z, w.z, a2);
                    a3 = fmaf(v.w, w.w, a3);
                }
            }
            part = (a0 + a1) + (a2 + a3);
        }
        if(PIECES && b.piece_mode) {
            // Every segment read bins its own wavefront parked (LDS operations of a wave execute in order: no barrier in front
            // of them).  The partials of a piece are added over the lanes; its last lane holds the total.
            WF_BAR_STAMP(14);
            const uint32_t info = (uint32_t)pre.glen;
            part = seg_prefix_scan(part, info);
            const int slot = (int)(info >> 8) - 1;
            WF_BAR_STAMP(15);
            if constexpr(T == 64) {
                if(has_row && slot >= 0)
                    emit(slot, part, pre.count); // one wavefront: a bar is one piece
            } else {
                // the totals meet in LDS behind the row; a wavefront that has left its own counts itself in, and the one that
                // finds everybody else's count adds the pieces of every bar in slot order -- nobody waits for anybody
                if(has_row && slot >= 0)
                    prod[slot] = part;
                const int before = wave_arrive(arrivals, t & 63);
                if(before == arrive_last - 1 && has_row && pre.lead >= 0) {
                    float sum = 0.0f;
                    for(int k = pre.s0; k < pre.s1; ++k)
                        sum += prod[k];
                    emit(pre.lead, sum, pre.count);
                }
            }
            return false;
        }
        if(b.wave_local) {
            // every bar lives inside one wavefront: its partials are added by a segmented reduction over the lanes (six
            // shuffles; lane s ends up with the sum of segments [s, end of its bar)) -- no LDS round trip, no barrier
            WF_BAR_STAMP(14);
            WF_UNROLL
            for(int d = 1; d < 64; d *= 2) {
                const float o = wave_shfl_down(part, d);
                if(t + d < pre.s1)
                    part += o;
            }
            WF_BAR_STAMP(15);
            if(has_row && pre.lead >= 0)
                emit(pre.lead, part, pre.count);
            return false;
        }
        if(has_row)
            prod[t] = part; // parked behind the dB row
        sync();
        WF_BAR_STAMP(14);
        WF_BAR_STAMP(15);
        // B1: the partials of a bar are added in two levels -- groups of up to eight consecutive segments first (their
        // leaders read the eight values in one go), then one thread per bar adds its group sums in order.  A log-axis display
        // has bars of a few hundred bins = dozens of segments; one thread walking them alone was the longest chain of the phase.
        float *gsum = prod + T + 8; // behind the partials and the eight floats a leader may read past them
        if(has_row && pre.glen > 0) {
            float q[8];
            WF_UNROLL
            for(int j = 0; j < 8; ++j)
                q[j] = prod[t + j]; // inside the scratch for every t; entries past the group are not used
            float a0 = q[0], a1 = 0.0f;
            WF_UNROLL
            for(int j = 1; j < 8; ++j) {
                const float v = (j < pre.glen) ? q[j] : 0.0f;
                if(j & 1) a1 += v; else a0 += v;
            }
            gsum[t] = a0 + a1;
        }
        sync();
        // B2: one thread per bar
        WF_UNROLL
        for(int k = 0; k < OutVals<G>::KMAX; ++k)
            ov.v[k] = 0.0f;
        if(has_row && t < b.num_bars) {
            float a0 = 0.0f, a1 = 0.0f;
            int k = pre.s0;
            for(; k + 8 < pre.s1; k += 16) {
                a0 += gsum[k];
                a1 += gsum[k + 8];
            }
            if(k < pre.s1)
                a0 += gsum[k];
            ov.v[0] = (a0 + a1) / (float)pre.count;
        }
        return true;
    }
    // ---- tables larger than the scratch (very many bars): chunk by chunk, lanes_per_bar threads per bar ---------------
    const int lpb = b.lanes_per_bar;
    const int bars_per_pass = T / lpb;
    // With the Gaussian filter the bar means are parked in a staging area behind the product scratch (the host sized the
    // chunks around it) instead of being mapped at once; the filter runs when the last chunk is done.
    const bool filtered = b.gauss_radius > 0;
    const int gpad = b.gauss_radius - 1, gsize = 2 * b.gauss_radius - 1;
    float *vp = db + b.stage_off;                   // [gpad | num_bars | gpad]
    float *wl = vp + b.num_bars + 2 * gpad;         // [gsize]
    if(filtered && has_row) {
        for(int i = t; i < gpad; i += T) {
            vp[i] = 0.0f;
            vp[gpad + b.num_bars + i] = 0.0f;
        }
        for(int i = t; i < gsize; i += T)
            wl[i] = b.gauss[i];
    }
    for(int c = 0; c < b.num_chunks; ++c) {
        const bool single = (b.num_chunks == 1);
        const int bar_lo = single ? 0 : b.chunk[c], bar_hi = single ? b.num_bars : b.chunk[c + 1];
        const int e_lo = single ? 0 : b.off[bar_lo], e_hi = single ? b.entries : b.off[bar_hi];
        if(has_row) {
            for(int e = e_lo + t; e < e_hi; e += T)
                prod[e - e_lo] = db[b.bin[e]] * b.coef[e];
        }
        sync();
        for(int b0 = bar_lo; b0 < bar_hi; b0 += bars_per_pass) {
            const int bar = b0 + t / lpb;
            const int sub = t % lpb;
            const bool live = has_row && bar < bar_hi;
            const bool first_pass = (c == 0 && b0 == 0);
            float acc = 0.0f;
            int cnt = 1;
            if(live) {
                const int boff = first_pass ? pre.off : b.off[bar];
                const int n = first_pass ? pre.len : b.off[bar + 1] - boff;
                cnt = first_pass ? pre.count : b.count[bar];
                const int o = boff - e_lo;
                float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
                int k = sub;
                for(; k + 3 * lpb < n; k += 4 * lpb) {
                    a0 += prod[o + k];
                    a1 += prod[o + k + lpb];
                    a2 += prod[o + k + 2 * lpb];
                    a3 += prod[o + k + 3 * lpb];
                }
                for(; k < n; k += lpb)
                    a0 += prod[o + k];
                acc = (a0 + a1) + (a2 + a3);
            }
            for(int m = lpb >> 1; m >= 1; m >>= 1)
                acc = xor_sum(acc, m);
            if(live && sub == 0) {
                if(filtered)
                    vp[gpad + bar] = acc / (float)cnt;
                else
                    emit(bar, acc, cnt);
            }
        }
        if(c + 1 < b.num_chunks)
            sync(); // prod is reused by the next chunk
    }
    if(filtered) {
        // apply_filter / weighted_avg (reference src/filter.hpp:133-157, :171-180) as in outputs_finish, one output per
        // thread and round
        sync();
        if(has_row) {
            for(int o = t; o < b.num_bars; o += T) {
                float sum = 0.0f;
                for(int tap = 0; tap < gsize; ++tap)
                    sum = fmaf(vp[o + tap], wl[tap], sum);
                emit_output(b, o, sum / b.gauss_wsum[o], out_row, dup_row);
            }
        }
    }
    return false;
}

} // namespace wf
