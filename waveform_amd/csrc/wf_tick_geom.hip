// wf_tick_geom.hip -- kernel dispatch of ONE FFT geometry: compiled once per geometry (-DWF_TU_GEOM=512 ... 32768, see the
// Makefile), so that the 270 instantiations of spectrum_tick_kernel build in parallel instead of in one translation unit.
// Host side: the launch functions wf_hip_tick calls through wf_hip::launch, and setup_tick_<N>() which wf_hip_create
// (wf_hip_plan.hip) calls to map the handle's finished plan (wf_hip::plan, wf_tick_plan.hpp) to one of them; nothing is planned here.  gfx950 only.
#include <algorithm>
#include <cstdio>

#include "wf_hip_internal.hpp"
#include "wf_kernels.hpp"

#ifndef WF_TU_GEOM
#error "compile with -DWF_TU_GEOM=<fft size of the geometry>"
#endif

namespace {

using wf::host::fail;

// The power-of-two kernels come in display-specific instantiations (spectrum_tick_kernel<.., MIR, DISP>, wf_kernels.hpp): what a
// launch needs is known on the host -- no display at all (DISP 2), bars in the prefix-sum layout and nothing else (DISP 1), anything
// else (DISP 0); with MIR the stores into wf_hip_set_bars_mirrors' buffers.  One launch = one of them, picked here.
inline int display_kind(const wf::TickArgs &a)
{
    if(a.bar.out == nullptr)
        return 2;
    return (a.bar.ps_lanes > 0 && a.bar.curve == 0) ? 1 : 0;
}
using TickKernel = void (*)(wf::TickArgs);

// What a launch of a power-of-two family can ask for -- aligned or not, mirrors or not, display kind 0 / 1 / 2 -- and the
// instantiation that serves it.  The family is everything a launch cannot change; SPECIAL: whether it has display-specific
// instantiations at all (the curve-sharing and decimated kernels keep the general one).  kernel<>() holds the rules that prune the
// 12 requests to the instantiations that exist, once; setup walks the table, the launch indexes it.
template<class G, int SPW, bool SPLIT, int DEC, bool TLDS, bool BOTH, bool SPECIAL> struct Pow2Family {
    template<bool AL, bool MIR, int DISP> static constexpr TickKernel kernel()
    {
        constexpr int disp = SPECIAL ? DISP : 0;
        // the split kernels serve the mirrors in their only instantiation (spectrum_tick_kernel's MIRROR); no display, no mirrors
        constexpr bool mir = MIR && !SPLIT && disp != 2;
        constexpr bool al = AL && !(DEC > 0 && mir); // (the decimated sizes with mirrors: the scalar fetch for both alignments)
        return &wf::spectrum_tick_kernel<G, wf::Variant{.spw = SPW, .aligned = al, .split = SPLIT, .dec = DEC, .tlds = TLDS, .both = BOTH, .mir = mir, .disp = disp}>;
    }
    static constexpr TickKernel table[2][2][3] = {
        {{kernel<false, false, 0>(), kernel<false, false, 1>(), kernel<false, false, 2>()}, {kernel<false, true, 0>(), kernel<false, true, 1>(), kernel<false, true, 2>()}},
        {{kernel<true, false, 0>(), kernel<true, false, 1>(), kernel<true, false, 2>()}, {kernel<true, true, 0>(), kernel<true, true, 1>(), kernel<true, true, 2>()}}};

    static void launch(dim3 grid, dim3 block, size_t lds, hipStream_t st, const wf::TickArgs &a, bool aligned)
    {
        hipLaunchKernelGGL(table[aligned][a.bar.out2_n > 0][display_kind(a)], grid, block, lds, st, a);
    }
    // (entries that alias after pruning get the attribute once more: the same value)
    static int setup_lds(wf_hip *h, int lds)
    {
        for(const auto &by_mir : table)
            for(const auto &by_disp : by_mir)
                for(const TickKernel k : by_disp)
                    WF_HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        return WF_HIP_OK;
    }
};

template<class G> int launch_tick_split(wf_hip *h, const wf::TickArgs &a0, bool aligned, hipStream_t st)
{
    const dim3 block(G::T);
    const size_t lds = wf::tick_lds_bytes<G, 1>();
    // mono mixdown: channel 1 of every stream, then channel 0 (TickArgs::split_ch); stereo pairs: everything at once
    const bool two = h->plan.split_mono;
    for(int pass = 0; pass < (two ? 2 : 1); ++pass) {
        wf::TickArgs a = a0;
        a.split_ch = two ? (uint32_t)(1 - pass) : 0xffffffffu;
        const dim3 grid(two ? a.stream_count : a.stream_count * a.cap_ch);
        Pow2Family<G, 1, true, 0, false, false, true>::launch(grid, block, lds, st, a, aligned);
    }
    return WF_HIP_OK;
}

template<class G> int setup_launch_split(wf_hip *h)
{
    const int lds = (int)wf::tick_lds_bytes<G, 1>();
    WF_TRY_RC((Pow2Family<G, 1, true, 0, false, false, true>::setup_lds(h, lds)));
    h->launch = &launch_tick_split<G>;
    h->wg_lds = (uint32_t)lds;
    h->wg_threads = (uint32_t)G::T;
    h->split = true;
    h->flag_bufs = 3;
    char name[96];
    snprintf(name, sizeof(name), "spectrum_tick_kernel<N=%d,T=%d,R=%dx%dx%d,SPW=1,split>", G::N, G::T, G::R1, G::R2, G::R3);
    h->kernel_name = name;
    return WF_HIP_OK;
}

// FFT sizes 256 / 128 on the 512-point geometry, zero-padded (spectrum_tick_kernel<.., DEC>)
template<class G, int DEC> int launch_tick_dec(wf_hip *, const wf::TickArgs &a, bool aligned, hipStream_t st)
{
    const uint32_t n_spec = a.stream_count * a.cap_ch;
    const dim3 grid((n_spec + 1) / 2), block(G::T * 2);
    const size_t lds = wf::tick_lds_bytes<G, 2>();
    Pow2Family<G, 2, false, DEC, false, false, false>::launch(grid, block, lds, st, a, aligned);
    return WF_HIP_OK;
}

template<class G, int DEC> int setup_launch_dec(wf_hip *h)
{
    const int lds = (int)wf::tick_lds_bytes<G, 2>();
    WF_TRY_RC((Pow2Family<G, 2, false, DEC, false, false, false>::setup_lds(h, lds)));
    h->launch = &launch_tick_dec<G, DEC>;
    h->wg_lds = (uint32_t)lds;
    h->wg_threads = (uint32_t)G::T * 2u;
    char name[96];
    snprintf(name, sizeof(name), "spectrum_tick_kernel<N=%d zero-padded to %d,T=%d,R=%dx%dx%d,SPW=2>", G::N >> DEC, G::N, G::T, G::R1, G::R2, G::R3);
    h->kernel_name = name;
    return WF_HIP_OK;
}

// The instantiations of a Bluestein / mixed-radix family: the general one and, for the small-radix instantiation of the 2048- and
// 4096-sample containers, the four plans it carries as compile-time constants (TransformPlan::plan_id; table row 1 + plan_id - P0,
// row 0: the general one), each with and without the display code (DISP 0 / 2)
template<class G, int SPW, bool SPLIT, bool MR, bool MRS> struct BluFamily {
    static constexpr bool FIXED = MRS && (G::N == 2048 || G::N == 4096);
    static constexpr int P0 = G::N == 2048 ? 1 : 5; // the container's four fixed plans (spectrum_tick_kernel's PLAN)
    template<int ROW, bool NODISP> static constexpr TickKernel kernel()
    {
        constexpr int plan = FIXED && ROW > 0 ? P0 + ROW - 1 : 0;
        return &wf::spectrum_tick_kernel<G, wf::Variant{.spw = SPW, .split = SPLIT, .blu = true, .mr = MR, .mrs = MRS, .disp = NODISP ? 2 : 0, .plan = plan}>;
    }
    static constexpr TickKernel table[5][2] = {{kernel<0, false>(), kernel<0, true>()}, {kernel<1, false>(), kernel<1, true>()}, {kernel<2, false>(), kernel<2, true>()},
                                               {kernel<3, false>(), kernel<3, true>()}, {kernel<4, false>(), kernel<4, true>()}};
    static int row(int plan_id) { return FIXED && plan_id >= P0 && plan_id < P0 + 4 ? 1 + plan_id - P0 : 0; }
};

// Bluestein path (FFT sizes that are not powers of two): always the scalar fetch
template<class G, int SPW, bool SPLIT, bool MR = false, bool MRS = false> int launch_tick_blu(wf_hip *h, const wf::TickArgs &a0, bool, hipStream_t st)
{
    using Family = BluFamily<G, SPW, SPLIT, MR, MRS>;
    const uint32_t n_spec = a0.stream_count * a0.cap_ch;
    const dim3 block(G::T * SPW);
    // (mixed radix: the exchange buffers by the transform's size, MrPlan::lds_cf)
    const size_t lds = wf::tick_lds_bytes<G, SPW>() - (MR ? (size_t)SPW * ((size_t)G::LDS_CF - (size_t)a0.mr.lds_cf) * sizeof(wf::cf) : 0);
    const bool two = SPLIT && h->plan.split_mono; // mono mixdown in two launches (TickArgs::split_ch)
    for(int pass = 0; pass < (two ? 2 : 1); ++pass) {
        wf::TickArgs a = a0;
        a.split_ch = two ? (uint32_t)(1 - pass) : 0xffffffffu;
        const dim3 grid(two ? a.stream_count : (n_spec + SPW - 1) / SPW);
        // (no display: the instantiation without any display code -- spectrum_tick_kernel<.., DISP = 2>; the sizes with a
        // compile-time plan: the instantiation of that plan alone -- <.., PLAN>)
        const bool nodisp = MRS && display_kind(a) == 2; // (the small-radix instantiation only: N = 4160 on the all-radix one measured -1.8 %)
        hipLaunchKernelGGL(Family::table[Family::row(h->plan.plan_id)][nodisp], grid, block, lds, st, a);
    }
    return WF_HIP_OK;
}

template<class G, int SPW, bool SPLIT, bool MR = false, bool MRS = false> int setup_launch_blu(wf_hip *h)
{
    int lds = (int)wf::tick_lds_bytes<G, SPW>();
    // (the attribute belongs to the kernel, not to this handle: always the container's size -- another handle of another fft size
    // on the same instantiation may need all of it)
    for(const auto &by_disp : BluFamily<G, SPW, SPLIT, MR, MRS>::table) // (without fixed plans every row is the general instantiation)
        for(const TickKernel k : by_disp)
            WF_HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    if constexpr(MR) {
        // the spectrum's exchange buffer by the transform's size, not the container's (MrPlan::lds_cf): room for more spectra per CU
        wf::MrPlan &mr = h->tick.mr;
        mr.half = (int)wf::mr_exchange_half(h->N / 2);
        mr.lds_cf = (int)wf::mr_exchange_cf(h->N / 2, (uint32_t)G::LDS_CF);
        mr.s3 = mr.half / 4 + 4;
        // the compile-time plans of the one-wavefront container run IN PLACE (mr_transform_fixed_inplace): without a display -- whose
        // planner has sized its staging by the two-halves buffer already -- the spectrum needs its points and the four-plane result only
        if(G::T == 64 && h->plan.plan_id != 0 && h->num_bars == 0)
            mr.lds_cf = std::min(mr.lds_cf, std::max(mr.half, 4 * mr.s3));
        lds -= SPW * ((int)G::LDS_CF - mr.lds_cf) * (int)sizeof(wf::cf);
    }
    h->launch = &launch_tick_blu<G, SPW, SPLIT, MR, MRS>;
    h->wg_lds = (uint32_t)lds;
    h->wg_threads = (uint32_t)(G::T * SPW);
    h->split = SPLIT;
    char name[160];
    if(MR) {
        char rad[48];
        int o = 0;
        for(int i = 0; i < h->tick.mr.passes; ++i)
            o += snprintf(rad + o, sizeof(rad) - (size_t)o, "%s%d", i ? "x" : "", h->tick.mr.radix[i]);
        snprintf(name, sizeof(name), "spectrum_tick_kernel<N=%u: %u complex points as mixed radix %s,T=%d,SPW=%d%s>", h->N, h->N / 2, rad, G::T, SPW,
                 SPLIT ? ",split" : "");
    } else
        snprintf(name, sizeof(name), "spectrum_tick_kernel<N=%u by Bluestein over %d complex points,T=%d,R=%dx%dx%d,SPW=%d%s>", h->N, G::M, G::T,
                 G::R1, G::R2, G::R3, SPW, SPLIT ? ",split" : "");
    h->kernel_name = name;
    return WF_HIP_OK;
}

// Bluestein proper, or -- the plan has passes -- the same instantiation's fetch and epilogue around a direct mixed-radix transform;
// one-wavefront containers: plans made of small radices take the instantiation that carries only those (five waves per SIMD)
template<class G, int SPW, bool SPLIT> int setup_blu_family(wf_hip *h)
{
    if constexpr(G::N >= 1024) { // (the smallest container a size that is not a power of two ever gets: wf::bluestein_length)
        if(h->plan.mr_in_lds()) {
            if constexpr(G::T <= 256 && G::P > 8) {
                if(h->plan.mr_small)
                    return setup_launch_blu<G, SPW, SPLIT, true, true>(h);
            }
            return setup_launch_blu<G, SPW, SPLIT, true>(h);
        }
    }
    return setup_launch_blu<G, SPW, SPLIT>(h);
}

template<class G, int SPW, bool TLDS, bool BOTH = false> int launch_tick(wf_hip *, const wf::TickArgs &a, bool aligned, hipStream_t st)
{
    const uint32_t n_spec = a.stream_count * a.cap_ch;
    const dim3 grid((n_spec + SPW - 1) / SPW), block(G::T * SPW);
    const size_t lds = wf::tick_lds_bytes<G, SPW>();
    Pow2Family<G, SPW, false, 0, TLDS, BOTH, !BOTH>::launch(grid, block, lds, st, a, aligned);
    return WF_HIP_OK;
}

template<class G, int SPW, bool TLDS, bool BOTH = false> int setup_launch_impl(wf_hip *h)
{
    const int lds = (int)wf::tick_lds_bytes<G, SPW>();
    WF_TRY_RC((Pow2Family<G, SPW, false, 0, TLDS, BOTH, !BOTH>::setup_lds(h, lds)));
    h->launch = &launch_tick<G, SPW, TLDS, BOTH>;
    h->wg_lds = (uint32_t)lds;
    h->wg_threads = (uint32_t)(G::T * SPW);
    char name[112];
    snprintf(name, sizeof(name), "spectrum_tick_kernel<N=%d,T=%d,R=%dx%dx%d,SPW=%d%s%s>", G::N, G::T, G::R1, G::R2, G::R3, SPW,
             TLDS ? ",tables via LDS" : "", BOTH ? ",curve row shared by both spectra" : "");
    h->kernel_name = name;
    return WF_HIP_OK;
}

// Workgroups of two spectra can stage the window / pass-1 twiddle tables in LDS once (spectrum_tick_kernel<.., TLDS>).
// Measured on MI355X (interleaved A/B): N = 1024 63.4 -> 68.7 % of the HBM peak (8-byte table loads, 23 per thread, become
// 8 DMA requests per wavefront), N = 2048 +-1 %, N = 4096 -1.5 % (the extra barrier costs what the halved table traffic
// saves), N = 8192 +1 %: on for the 8-point geometry only.
template<class G, int SPW> int setup_launch(wf_hip *h)
{
    if constexpr(SPW == 2) {
        // (not `if constexpr`: the form a geometry does not take stays instantiated although nothing launches it -- the object's
        // kernels are on record in tests/test_cpu_units.py, and dropping ten per geometry is a change of its own)
        const bool tlds = G::P <= 8;
        // mono mixdown with a curve display: the kernel whose two spectra share the row
        if(h->tick.bar.both_subs && h->N == (uint32_t)G::N) {
            if constexpr(G::P <= 8)
                return setup_launch_impl<G, 2, true, true>(h);
            else
                return setup_launch_impl<G, 2, false, true>(h);
        }
        if(tlds)
            return setup_launch_impl<G, 2, true>(h);
    }
    return setup_launch_impl<G, SPW, false>(h);
}

// the kernel of this handle on geometry G: which of the instantiations above its configuration takes
template<class G> int setup_tick_geometry(wf_hip *h)
{
    const wf_config *cfg = &h->cfg;
    const bool want_split = h->plan.want_split;
    h->waves_per_spectrum = G::T / 64;
    if(h->plan.blu) {
        if constexpr(G::N >= 32768) {
            // (the Bluestein and mixed-radix instantiations of this container keep 1024 threads of 16 points: a mixed-radix
            // plan's last pass has one butterfly per thread at most, and 39 sizes have no plan on 512 threads)
            using GB = wf::GBig;
            h->waves_per_spectrum = GB::T / 64;
            if(want_split)
                return setup_blu_family<GB, 1, true>(h);
            if(cfg->capture_channels == 1)
                return setup_blu_family<GB, 1, false>(h);
            return fail(h, WF_HIP_ERR_RUNTIME, "fft_size %u: no launch plan", cfg->fft_size);
        } else if constexpr(G::T >= 256)
            return want_split ? setup_blu_family<G, 1, true>(h) : (cfg->capture_channels > 1) ? setup_blu_family<G, 2, false>(h) : setup_blu_family<G, 1, false>(h);
        else
            return setup_blu_family<G, 2, false>(h);
    } else if constexpr(G::N == 512) {
        switch(h->N) {
        case 256: return setup_launch_dec<G, 1>(h);
        case 128: return setup_launch_dec<G, 2>(h);
        default: return setup_launch<G, 2>(h);
        }
    } else if constexpr(G::N >= 32768) {
        // one spectrum fills a CU's LDS: a stereo pair runs split, a single captured channel alone; mono mixdown of two
        // channels runs split too, as two launches (TickArgs::split_ch)
        if(want_split)
            return setup_launch_split<G>(h);
        if(cfg->capture_channels == 1)
            return setup_launch<G, 1>(h);
        return fail(h, WF_HIP_ERR_RUNTIME, "fft_size %u: no launch plan", cfg->fft_size);
    } else if constexpr(G::T >= 256)
        return want_split ? setup_launch_split<G>(h) : (cfg->capture_channels > 1) ? setup_launch<G, 2>(h) : setup_launch<G, 1>(h);
    else
        return setup_launch<G, 2>(h);
}

} // namespace

namespace wf::host {

#define WF_CAT2(a, b) a##b
#define WF_CAT(a, b) WF_CAT2(a, b)
int WF_CAT(setup_tick_, WF_TU_GEOM)(wf_hip *h)
{
#if defined(WF_GEOM_ONLY) && (WF_GEOM_ONLY != WF_TU_GEOM) // development builds: one geometry only (tools/variant.sh)
    return fail(h, WF_HIP_ERR_UNSUPPORTED, "development build: only the %d-sample geometry is compiled in", WF_GEOM_ONLY);
#else
    return setup_tick_geometry<WF_CAT(wf::G, WF_TU_GEOM)>(h);
#endif
}

} // namespace wf::host
