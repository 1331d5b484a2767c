// wf_tick_plan.cpp -- see wf_tick_plan.hpp.  Plain C++ (g++): no HIP, no handle, no getenv.
#include "wf_tick_plan.hpp"

#include <algorithm>
#include <cmath>

#include "wf_geometry.hpp"
#include "wf_host_tables.hpp"

namespace wf {

namespace {

// sizes up to 16384 that are not powers of two: Bluestein over the container of geom_n / 2 points, or -- sizes with small prime
// factors -- the same instantiation's fetch and epilogue around a direct mixed-radix transform
void plan_in_lds(TransformPlan &t)
{
    t.family = Family::BLUESTEIN;
    uint32_t threads = 0, points = 0;
    uint64_t container = 0;
    dispatch_geometry(t.geom_n, [&](auto g) {
        using G = decltype(g);
        if constexpr(G::N >= 32768) { // (this container keeps 1024 threads of 16 points: a mixed-radix plan's last pass has one butterfly
                                      // per thread at most, and 39 sizes have no plan on 512 threads)
            threads = (uint32_t)GBig::T, points = (uint32_t)GBig::P, container = (uint64_t)GBig::M;
        } else if constexpr(G::N >= 1024) { // (the smallest container a size that is not a power of two ever gets: wf::bluestein_length)
            threads = (uint32_t)G::T, points = (uint32_t)G::P, container = (uint64_t)G::M;
        }
    });
    if(!threads)
        return;
    const int passes = plan_mixed_radix(t.n / 2, threads, t.radix, container);
    if(passes <= 0) {
        std::fill(t.radix, t.radix + 4, 0);
        return;
    }
    t.family = Family::MIXED_RADIX;
    t.passes = passes;
    // one-wavefront containers: plans made of small radices take the instantiation that carries only those (five waves per SIMD)
    t.mr_small = threads <= 256u && points > 8u && mr_small_radices(t.radix, t.passes);
    if(t.mr_small && (t.geom_n == 2048u || t.geom_n == 4096u) && t.passes == 3) {
        // the sizes the plugin picks by itself run their plan as compile-time constants, in an instantiation of their own
        static const int fixed[8][3] = {{5, 10, 8}, {5, 12, 8}, {10, 6, 6}, {11, 5, 8}, {10, 8, 10}, {10, 8, 12}, {10, 10, 10}, {10, 8, 11}};
        const int p0 = t.geom_n == 2048u ? 1 : 5; // the container's four fixed plans (spectrum_tick_kernel's PLAN)
        for(int i = 0; i < 4; ++i)
            if(t.radix[0] == fixed[p0 - 1 + i][0] && t.radix[1] == fixed[p0 - 1 + i][1] && t.radix[2] == fixed[p0 - 1 + i][2])
                t.plan_id = p0 + i;
        if(t.plan_id)
            t.family = Family::FIXED_PLAN;
    }
}

// above 16384 samples and not a power of two: where n/2 = C R with R <= 8192 a length that has a mixed-radix plan, C <= 8
// rows of that transform (big_mr_rows_kernel)
void plan_rows(TransformPlan &t)
{
    const uint32_t np = t.n / 2;
    // ... and where n/2 = C R with C = 8 or 4 and R <= 4096: the rows by Bluestein over the 8192- / 16384-sample geometry INSIDE
    // LDS (big_br_*_kernel) -- every multiple of 16 up here, the slider's 768 positions among them
    // C = 16 where it divides n/2 (every multiple of 32), else 8: the smaller the container the more workgroups a CU holds --
    // 48064 x 256 streams 0.254 ms with 8 rows over 8192 points, 0.194 with 16 over 4096, 0.209 with 32 over 2048
    // (32 rows over 1024 / 2048 points: 0.209 -- profiles/r05m_bluestein_rows_ab.txt; not compiled in any more)
    uint32_t br_c = 0;
    for(uint32_t c = 16; c >= 8u && !br_c; c >>= 1)
        if(np % c == 0 && np / c <= 4096u && np / c >= 512u)
            br_c = c;
    for(uint32_t c = 2; c <= 8 && !t.big_mr(); ++c) {
        if(np % c || np / c > 8192u)
            continue;
        int radix[4] = {0, 0, 0, 0};
        int passes = 0;
        bool whole = false;
        if(c == 2u) { // two rows: on 512 threads where a plan exists -- one kernel (big_mr_whole_kernel)
            passes = plan_mixed_radix(np / c, 512u, radix);
            whole = passes > 0;
        }
        if(passes <= 0)
            passes = plan_mixed_radix(np / c, 1024u, radix);
        // A plan that opens with a prime pass (29 ... 127: wf::mr_pass_prime, p products per point) loses to the Bluestein rows:
        // of the slider's 251 such positions 215 are faster there, by up to 40 % (113x8x9: 0.53 -> 0.31 ms at 256 streams), the
        // other 36 slower by 6 % on average (profiles/r05_sizes_large_before.jsonl)
        if(passes > 0 && !(br_c && radix[0] > 25)) {
            t.family = whole ? Family::MR_TWO_ROWS : Family::MR_ROWS;
            t.passes = passes;
            std::copy(radix, radix + 4, t.radix);
            t.blu = false;  // no chirp tables, no chirped window: the plain packed real transform
            t.big_l = np;   // (complex points per spectrum in the scratch buffer)
            t.big_rows = c;
        }
    }
    if(!t.big_mr() && br_c) {
        t.family = Family::BLUESTEIN_ROWS;
        t.blu = false; // (as above: the plain packed real transform, its rows by chirp-z)
        t.big_l = np;
        t.big_rows = br_c;
        t.br_l = 2048u; // (build_bluestein_rows' container length for rows of more than 512 points)
        while(t.br_l < 2u * (np / br_c) - 1u)
            t.br_l <<= 1;
        t.br_rs = (np / br_c + 1u) & ~1u;
    }
}

} // namespace

TransformPlan plan_transform(const wf_config &cfg, const PlanOverrides &)
{
    TransformPlan t;
    t.n = cfg.fft_size;
    const uint32_t L = (cfg.meter || cfg.waveform) ? 0u : bluestein_length(t.n);
    t.blu = L != 0;
    t.big_l = L > 16384u ? L : (!L && t.n == 65536u) ? 32768u : 0u;
    t.big_rows = t.big_l / 16384u;
    t.geom_n = t.big_l ? 32768u : L ? 2 * L : std::max(t.n, 512u); // big: the row transform's geometry
    if(!t.blu)
        t.family = t.big_l ? Family::WHOLE_65536 : t.n < 512u ? Family::ZERO_PADDED : Family::POW2;
    else if(!t.big_l)
        plan_in_lds(t);
    else {
        t.family = Family::NONE; // (what a size keeps that plan_rows cannot place; every multiple of 16 has rows of one kind or the other)
        plan_rows(t);
    }
    // Split mode: the channels of a stereo pair in different workgroups.  Measured on MI355X: N = 16384 45 -> 52 % of the HBM
    // peak (two workgroups per CU instead of one), N = 8192 57.2 -> 58.5 % (four instead of two), N = 32768 cannot run a
    // pair any other way (mono mixdown and single-channel captures never split).
    t.want_split = t.geom_n >= 8192u;
    t.want_split = t.want_split && cfg.capture_channels == 2 && cfg.stereo;
    // mono mixdown needs both channels' magnitudes; where a workgroup holds one spectrum (132 KB of LDS) the pair runs split
    // as well, channel 1 a launch ahead of channel 0
    t.split_mono = t.geom_n >= 32768u && cfg.capture_channels == 2 && !cfg.stereo;
    t.want_split = t.want_split || t.split_mono;
    if(t.big_l) // the epilogue couples the channels through the rotating verdict words, whatever the channel layout
        t.want_split = true;
    // 2^40 up to 4096 samples, one power of two less per doubling beyond (2^36 at 65536): |X|^2 overflows only above an amplitude
    // of 2^64 / (N * in_scale) = 4096 (+72 dBFS) at every size from 4096 up, and still answers down to |X| ~ 2e-30
    int lg = 0;
    while((1u << lg) < t.n)
        ++lg;
    t.in_scale = std::ldexp(1.0f, std::min(40, 52 - lg));
    return t;
}

// Lanes (see struct wf_hip): two slices once each still fills the chip a couple of times over.  Measured on MI355X
// (cfg3, 8192 spectra per tick, back-to-back ticks): 1 lane 66 us per tick, 2 lanes 58 us.  WF_HIP_LANES overrides.
// Two lanes pay once the batch fills the chip at least twice over (a lane's drain and ramp-up then fall under the other's
// steady state); a batch of one round or less only pays the fork / join events: N = 4096 x 1024 streams -- exactly one
// round of 4 workgroups per CU -- 0.625 on one lane, 0.545 on two; 3 and 4 lanes: -1..-4 % everywhere.
int plan_lanes(const TransformPlan &t, uint32_t n_streams, uint32_t cap_ch, uint32_t num_bars, uint32_t wg_lds, uint32_t wg_threads, int cu_count,
               const PlanOverrides &ov)
{
    const size_t n_spec = (size_t)n_streams * cap_ch;
    const uint32_t M = t.n / 2;
    const bool split = t.want_split;
    const uint32_t cus = (uint32_t)std::max(cu_count, 1);
    const uint32_t wgs = (uint32_t)(n_spec / (split ? 1u : 2u));
    const uint32_t per_cu = std::max(1u, std::min(wg_lds ? (160u * 1024u) / wg_lds : 16u, wg_threads ? 1024u / wg_threads : 16u));
    const uint32_t round = per_cu * cus;
    int lanes = wgs >= 2u * round ? 2 : 1;
    if(wgs >= 3u * round && wgs < 6u * round && !t.blu && M >= 2048 && !(split && num_bars))
        lanes = 3; // round 6, the display-specific kernels (shorter workgroups): three to five rounds of workgroups as three slices --
                   // headline 0.813 -> 0.824, N = 4096 with bars 0.766 -> 0.777, N = 16384 x 1024 streams 0.710 -> 0.719 (with bars +-0: the split
                   // kernels with a display keep two); eight rounds (8192 streams) -0.4 %
                   // without a display, +1 % with bars: two there (profiles/r06w_lanes_slim_kernels.txt)
    if(wgs >= 6u * round && !t.blu && M >= 2048 && !split && num_bars)
        lanes = 3; // longer batches with a bars display: +0.4 ... +1.4 % in four sweeps (8192 streams, bars-only ticks 0.677 -> 0.6815; r06w, r06y)
    if(M <= 512 && wgs >= 6u * round)
        lanes = 3; // the one-wavefront 8-point geometry in long launches: 0.714-0.717 against 0.682-0.683 of the HBM peak at
                   // 16384 streams (steady state, r02j; N = 512 x 16384 streams 0.614 -> 0.636, r06y); from three rounds on instead:
                   // N = 512 x 8192 streams 0.519 -> 0.508 (profiles/r06y_lanes_rule_ab.txt)
    if(per_cu == 1 && wgs >= 2u * round)
        lanes = 3; // one workgroup per CU (32768 samples): fetch, transform and the end of the tick take turns inside a CU, and the
                   // launches of three slices drift apart: 256 streams 0.465 -> 0.513 (two) -> 0.533 (three), 2048 streams 0.472 -> 0.470 -> 0.495
    if(t.big_l) // the transforms through device memory: launch chains of small kernels, nothing to overlap -- except fft_size 65536 in
                // its one kernel, a CU per workgroup again: 256 streams 0.445 -> 0.557 (two) / 0.49 (three), 64 streams (half a round) 0.259 -> 0.253
        // (the rows of the other sizes up here -- mixed radix, Bluestein in LDS -- likewise from two spectra per CU on: their column /
        // rows / epilogue kernels are bound by different things and two slices' chains overlap: 48016 x 256 streams 0.266 -> 0.250 ms,
        // 48000 x 256 0.170 -> 0.160, 17488 x 512 0.164 -> 0.158, 48016 x 1024 1.07 -> 1.02; three lanes +-2 % around two)
        lanes = ((t.big_whole() || t.big_mr() || t.big_br()) && n_spec >= 2u * cus) ? 2 : 1;
    if(ov.lanes)
        lanes = ov.lanes;
    return std::max(1, std::min({lanes, MAX_LANES, (int)n_streams}));
}

} // namespace wf
