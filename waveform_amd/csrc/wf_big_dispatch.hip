// wf_big_dispatch.hip -- kernel dispatch of the FFT sizes whose transform does not fit a CU's LDS (wf_big.hpp: 65536 samples in one
// kernel; the other sizes above 16384 as rows -- mixed radix, or Bluestein inside LDS -- then the epilogue), and of
// big_outputs_kernel for the displays that are finished behind the tick kernel from its stored rows.  gfx950 only.
#include <algorithm>
#include <cstdio>

#include "wf_hip_internal.hpp"
#include "wf_big.hpp"

namespace {

using wf::host::fail;

// fft_size 65536, one kernel: both rows of a spectrum and the end of its tick in one workgroup (wf_big.hpp: big_whole_kernel)
int launch_tick_big_whole(wf_hip *h, const wf::TickArgs &a0, bool aligned, hipStream_t st)
{
    const size_t lds = wf::big_rows_lds_bytes<2>();
    for(int pass = 0; pass < (h->plan.split_mono ? 2 : 1); ++pass) { // mono mixdown: channel 1 of every stream, then channel 0
        wf::TickArgs a = a0;
        a.split_ch = h->plan.split_mono ? (uint32_t)(1 - pass) : 0xffffffffu;
        const dim3 grid(h->plan.split_mono ? a.stream_count : a.stream_count * a.cap_ch);
        if(aligned)
            hipLaunchKernelGGL(wf::big_whole_kernel<true>, grid, dim3(wf::GFold::T), lds, st, a);
        else
            hipLaunchKernelGGL(wf::big_whole_kernel<false>, grid, dim3(wf::GFold::T), lds, st, a);
    }
    if(a0.bar.out != nullptr)
        hipLaunchKernelGGL(wf::big_outputs_kernel, dim3(a0.stream_count * a0.bar.disp_ch), dim3(wf::GBig::T), h->disp.big_out_lds, st, a0);
    WF_HIP_TRY(h, hipGetLastError());
    return WF_HIP_OK;
}

// fft sizes above 16384 whose n/2 is two rows of a mixed-radix transform: both rows and the end of the tick in one workgroup
// (wf_big.hpp: big_mr_whole_kernel)
int launch_tick_big_mrw(wf_hip *h, const wf::TickArgs &a0, hipStream_t st)
{
    const size_t lds = (size_t)(2 * a0.mr.half + 128) * sizeof(wf::cf);
    for(int pass = 0; pass < (h->plan.split_mono ? 2 : 1); ++pass) { // mono mixdown: channel 1 of every stream, then channel 0
        wf::TickArgs a = a0;
        a.split_ch = h->plan.split_mono ? (uint32_t)(1 - pass) : 0xffffffffu;
        const dim3 grid(h->plan.split_mono ? a.stream_count : a.stream_count * a.cap_ch);
        hipLaunchKernelGGL(wf::big_mr_whole_kernel, grid, dim3(wf::GFold::T), lds, st, a);
    }
    if(a0.bar.out != nullptr)
        hipLaunchKernelGGL(wf::big_outputs_kernel, dim3(a0.stream_count * a0.bar.disp_ch), dim3(wf::GBig::T), h->disp.big_out_lds, st, a0);
    WF_HIP_TRY(h, hipGetLastError());
    return WF_HIP_OK;
}

// fft sizes above 16384 with small prime factors: rows of a mixed-radix transform (column step folded into the fetch), then the
// epilogue of the packed real transform (wf_big.hpp)
int launch_tick_big_mr(wf_hip *h, const wf::TickArgs &a0, hipStream_t st)
{
    const uint32_t n_spec = a0.stream_count * a0.cap_ch;
    const uint32_t spec_base = a0.stream_base * a0.cap_ch;
    WF_HIP_TRY(h, hipMemsetAsync(a0.big_nz_out + spec_base, 0, (size_t)n_spec * sizeof(uint32_t), st));
    const dim3 grow(a0.big_c * ((n_spec + 7u) & ~7u)); // (row, spectrum) by XCD: see big_mr_rows_kernel
    hipLaunchKernelGGL(wf::big_mr_rows_kernel, grow, dim3(wf::GBig::T), (size_t)(wf::GBig::LDS_CF + 128) * sizeof(wf::cf), st, a0);
    const uint32_t parts = (h->M + (uint32_t)wf::BIG_TP - 1u) / (uint32_t)wf::BIG_TP;
    for(int pass = 0; pass < (h->plan.split_mono ? 2 : 1); ++pass) { // mono mixdown: channel 1 of every stream, then channel 0
        wf::TickArgs a = a0;
        a.split_ch = h->plan.split_mono ? (uint32_t)(1 - pass) : 0xffffffffu;
        const dim3 grid(parts, h->plan.split_mono ? a.stream_count : n_spec);
        hipLaunchKernelGGL((wf::big_epilogue_kernel<1>), grid, dim3(wf::GBig::T), 0, st, a);
    }
    if(a0.bar.out != nullptr)
        hipLaunchKernelGGL(wf::big_outputs_kernel, dim3(a0.stream_count * a0.bar.disp_ch), dim3(wf::GBig::T), h->disp.big_out_lds, st, a0);
    WF_HIP_TRY(h, hipGetLastError());
    return WF_HIP_OK;
}

// fft sizes above 16384 with a large prime factor: the column step, the rows by Bluestein inside LDS (in place), the epilogue on the
// rows where they lie (wf_big.hpp)
template<class G, int C> int launch_tick_big_br(wf_hip *h, const wf::TickArgs &a0, hipStream_t st)
{
    const uint32_t n_spec = a0.stream_count * a0.cap_ch;
    const uint32_t spec_base = a0.stream_base * a0.cap_ch;
    WF_HIP_TRY(h, hipMemsetAsync(a0.big_nz_out + spec_base, 0, (size_t)n_spec * sizeof(uint32_t), st));
    hipLaunchKernelGGL((wf::big_br_columns_kernel<C>), dim3((a0.big_r + 255u) / 256u, n_spec), dim3(256), 0, st, a0);
    const dim3 grow(a0.big_c * ((n_spec + 7u) & ~7u));
    hipLaunchKernelGGL((wf::big_br_rows_kernel<G>), grow, dim3(G::T), wf::big_br_lds_bytes<G>(), st, a0);
    const uint32_t parts = (h->M + (uint32_t)wf::BIG_TP - 1u) / (uint32_t)wf::BIG_TP;
    for(int pass = 0; pass < (h->plan.split_mono ? 2 : 1); ++pass) {
        wf::TickArgs a = a0;
        a.split_ch = h->plan.split_mono ? (uint32_t)(1 - pass) : 0xffffffffu;
        const dim3 grid(parts, h->plan.split_mono ? a.stream_count : n_spec);
        hipLaunchKernelGGL((wf::big_epilogue_kernel<3>), grid, dim3(wf::GBig::T), 0, st, a);
    }
    if(a0.bar.out != nullptr)
        hipLaunchKernelGGL(wf::big_outputs_kernel, dim3(a0.stream_count * a0.bar.disp_ch), dim3(wf::GBig::T), h->disp.big_out_lds, st, a0);
    WF_HIP_TRY(h, hipGetLastError());
    return WF_HIP_OK;
}

template<int C> int launch_tick_big_br_g(wf_hip *h, const wf::TickArgs &a, hipStream_t st)
{
    switch(h->plan.br_l) { // (16 rows: 2048 points up to n = 32768, 4096 above; 8 rows: 4096 / 8192)
    case 2048u: return launch_tick_big_br<wf::G4096, C>(h, a, st);
    case 4096u: return launch_tick_big_br<wf::G8192, C>(h, a, st);
    default: return launch_tick_big_br<wf::G16384, C>(h, a, st);
    }
}

// one part of a slice, by the plan's family
int launch_tick_big_part(wf_hip *h, const wf::TickArgs &s, bool aligned, hipStream_t st)
{
    switch(h->plan.family) {
    case wf::Family::MR_TWO_ROWS: return launch_tick_big_mrw(h, s, st);
    case wf::Family::MR_ROWS: return launch_tick_big_mr(h, s, st);
    case wf::Family::BLUESTEIN_ROWS: return h->plan.big_rows == 16u ? launch_tick_big_br_g<16>(h, s, st) : launch_tick_big_br_g<8>(h, s, st);
    case wf::Family::WHOLE_65536: return launch_tick_big_whole(h, s, aligned, st);
    default: return fail(h, WF_HIP_ERR_UNSUPPORTED, "fft_size %u: no kernel for this size in this build", h->N); // (unreachable: setup_launch_big refuses)
    }
}

// (a failure that is HIP's leaves its error sticky as well: wf_hip_tick's hipGetLastError() behind the launches reports it)
int launch_tick_big(wf_hip *h, const wf::TickArgs &a, bool aligned, hipStream_t st)
{
    // the kernels of this path index spectra with blockIdx.y (<= 65535): larger slices go out in parts
    const uint32_t part = 65535u / a.cap_ch;
    for(uint32_t off = 0; off < a.stream_count; off += part) {
        wf::TickArgs s = a;
        s.stream_base = a.stream_base + off;
        s.stream_count = std::min(part, a.stream_count - off);
        WF_TRY_RC(launch_tick_big_part(h, s, aligned, st));
    }
    return WF_HIP_OK;
}

} // namespace

namespace wf::host {

int setup_launch_big(wf_hip *h)
{
    const wf::TransformPlan &t = h->plan;
    if(t.big_mr()) {
        WF_HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&wf::big_mr_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)((size_t)(wf::GBig::LDS_CF + 128) * sizeof(wf::cf))));
        WF_HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&wf::big_mr_whole_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)((size_t)(wf::GBig::M + 128) * sizeof(wf::cf))));
    }
    else if(t.big_br()) {
        WF_HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&wf::big_br_rows_kernel<wf::G4096>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)wf::big_br_lds_bytes<wf::G4096>()));
        WF_HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&wf::big_br_rows_kernel<wf::G8192>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)wf::big_br_lds_bytes<wf::G8192>()));
        WF_HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&wf::big_br_rows_kernel<wf::G16384>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)wf::big_br_lds_bytes<wf::G16384>()));
    } else if(!t.big_whole()) // (Family::NONE; no legal size gets here: every multiple of 16 above 16384 has rows of one kind or the other)
        return fail(h, WF_HIP_ERR_UNSUPPORTED, "fft_size %u: neither a power of two nor a length with a row decomposition (a multiple of 16 has one)", h->N);
    // fft_size 65536 (the one power of two up here): both rows and the end of the tick in one kernel, no scratch in device memory
    if(t.big_whole()) {
        WF_HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&wf::big_whole_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)wf::big_rows_lds_bytes<2>()));
        WF_HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&wf::big_whole_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)wf::big_rows_lds_bytes<2>()));
    }
    if(h->disp.big_out_lds)
        WF_HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&wf::big_outputs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)h->disp.big_out_lds));
    h->launch = &launch_tick_big;
    h->split = true;
    h->flag_bufs = 3;
    char name[256];
    if(t.big_mr()) {
        char rad[48];
        const char *form = t.big_mrw() ? "big_mr_whole_kernel<N=%u: both of its %u rows of %u complex points as mixed radix %s and the end of the tick in one workgroup>"
                                      : "big_mr_rows_kernel + big_epilogue_kernel<N=%u: %u rows of %u complex points as mixed radix %s, column step folded into the fetch>";
        int o = 0;
        for(int i = 0; i < t.passes; ++i)
            o += snprintf(rad + o, sizeof(rad) - (size_t)o, "%s%d", i ? "x" : "", t.radix[i]);
        snprintf(name, sizeof(name), form, h->N, t.big_rows, h->M / t.big_rows, rad);
    } else if(t.big_br())
        snprintf(name, sizeof(name), "big_br_{columns,rows}_kernel + big_epilogue_kernel<N=%u: %u rows of %u complex points by Bluestein over %u points inside LDS>",
                 h->N, t.big_rows, h->M / t.big_rows, t.br_l);
    else
        snprintf(name, sizeof(name), "big_whole_kernel<N=%u: both rows of 16384 complex points and the end of the tick in one workgroup>", h->N);
    h->kernel_name = name;
    return WF_HIP_OK;
}

int big_outputs_set_lds(wf_hip *h)
{
    WF_HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void *>(&wf::big_outputs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)h->disp.big_out_lds));
    return WF_HIP_OK;
}

// the display of `rows` displayed rows (a.stream_base ...) from the rows the tick kernel has just stored, one workgroup each
void big_outputs_launch(wf_hip *h, const wf::TickArgs &a, uint32_t rows, hipStream_t st)
{
    hipLaunchKernelGGL(wf::big_outputs_kernel, dim3(rows), dim3(wf::GBig::T), h->disp.big_out_lds, st, a);
}

} // namespace wf::host
