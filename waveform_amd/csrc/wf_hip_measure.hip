// wf_hip_measure.hip -- the measurement outputs of the C ABI in include/wf_hip.h: WF_HIP_OUT_LOUDNESS, _PEAKS, _SIGNAL, _PITCH,
// _BANDS, _STEREO, _CQ, _SCOPE, _GONIO, _SONO, _BITS, _THD, _DELAY, _ONSET, _XFER, _IMPULSE, _CLICK, _IMD, _TEMPO and _HUM.  None of
// them is in the reference and none is part of the tick: each is computed when it is read, by a kernel of its own header, into a
// block the first read allocates.  One table (MEASURES, a row per output in the order of wf_hip_output) says what each output
// is, what its first read sets up and how it is launched; one reader (measure_read) does the rest.  What an output derives from
// the configuration alone is built by plain C++ (wf_measure_tables.cpp, wf_loudness_tables.cpp) and only uploaded here.  The
// loudness producer alone also keeps state between reads: it follows every push (measure_check_push / measure_after_push, called
// by the ingest in wf_hip.hip) and is switched on by wf_hip_enable_loudness.  gfx950 only.
//
// A new measurement output: its kernel in a header of its own, included here and nowhere else, with a wf::RingView in its
// arguments if it reads the rings.  What kernels share lies in headers that hold no kernel (wf_wave_reduce.hpp, wf_ring_stage.hpp,
// wf_fft64_lds.hpp, wf_phat.hpp): no kernel header includes another output's, but for wf_xfer.hpp and wf_impulse.hpp over
// wf_xfer_sums.hpp, wf_thd.hpp and wf_imd.hpp over wf_thd_spectrum.hpp, and wf_onset.hpp and wf_tempo.hpp over wf_onset_column.hpp,
// the heads they share.  If it needs tables, a builder in wf_measure_tables.cpp that sees no handle and no HIP, and a setup
// function here that calls it, keeps the scalars on the handle, states its kernels' dynamic LDS (allow_lds) and uploads; a launch
// function (launch_by_channels where the kernel is instantiated per captured channels), a refusal function and a row at the end
// of MEASURES below, with wf_hip::N_MEASURES one larger; a row of MEASURES and a reader on _MeasureReaders in
// waveform_amd/binding.py.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "wf_hip_internal.hpp"
#include "wf_dev_guard.hpp"
#include "wf_measure_tables.hpp"
#include "wf_loudness.hpp"
#include "wf_peaks.hpp"
#include "wf_signal.hpp"
#include "wf_pitch.hpp"
#include "wf_bands.hpp"
#include "wf_stereo.hpp"
#include "wf_cq.hpp"
#include "wf_scope.hpp"
#include "wf_gonio.hpp"
#include "wf_sono.hpp"
#include "wf_bits.hpp"
#include "wf_thd.hpp"
#include "wf_delay.hpp"
#include "wf_onset.hpp"
#include "wf_xfer.hpp"
#include "wf_impulse.hpp"
#include "wf_click.hpp"
#include "wf_imd.hpp"
#include "wf_tempo.hpp"
#include "wf_hum.hpp"

namespace {

using namespace wf::host;

inline bool loudness_on(const wf_hip *h) { return h->loud.d_state != nullptr; }

int clear_loudness(wf_hip *h, uint32_t first, uint32_t count)
{
    WF_HIP_TRY(h, hipMemsetAsync(h->loud.d_state + first, 0, (size_t)count * sizeof(wf::LoudState), h->stream));
    WF_HIP_TRY(h, hipMemsetAsync(h->loud.d_hist + (size_t)first * 2, 0, (size_t)count * 2 * sizeof(wf::LoudHist), h->stream));
    return WF_HIP_OK;
}

// how the kernels that read the rings see them
wf::RingView ring_view(const wf_hip *h) { return wf::RingView{h->d_ring, h->d_wpos, h->ring_cap, h->ring_stride}; }

// The <1> or <2> instantiation of a kernel by the batch's captured channels, each on its own grid
template<class Args>
void launch_by_channels(const wf_hip *h, void (*one)(Args), void (*two)(Args), dim3 grid_one, dim3 grid_two, uint32_t threads, size_t lds, const Args &a)
{
    if(h->cap_ch == 2)
        hipLaunchKernelGGL(two, grid_two, dim3(threads), lds, h->stream, a);
    else
        hipLaunchKernelGGL(one, grid_one, dim3(threads), lds, h->stream, a);
}
// ... and on the same grid
template<class Args>
void launch_by_channels(const wf_hip *h, void (*one)(Args), void (*two)(Args), dim3 grid, uint32_t threads, size_t lds, const Args &a)
{
    launch_by_channels(h, one, two, grid, grid, threads, lds, a);
}

// what a kernel may ask for as dynamic LDS: a setup function states the most its launches will
template<class Kernel> int allow_lds(wf_hip *h, Kernel *kernel, size_t bytes)
{
    WF_HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return WF_HIP_OK;
}

// One launch function per output: the entries of streams [first, first+count) into d_block, the output's whole block.
// Loudness: the readings are made from the state when asked for, behind the pushes issued so far
int launch_loudness(wf_hip *h, uint32_t first, uint32_t count, void *d_block)
{
    hipLaunchKernelGGL(wf::loudness_read_kernel, dim3(count), dim3(64), 0, h->stream, h->loud.d_state, h->loud.d_hist,
                       static_cast<wf_hip_loudness *>(d_block), first, h->loud.k.sub_frames);
    return WF_HIP_OK;
}

// one wavefront per m_decibels row, behind the ticks issued
int launch_peaks(wf_hip *h, uint32_t first, uint32_t count, void *d_block)
{
    wf::PeaksArgs a{};
    a.rows = h->d_decibels + (size_t)first * h->out_ch * h->M;
    a.out = static_cast<wf_hip_peaks *>(d_block) + (size_t)first * h->out_ch;
    a.n_rows = count * h->out_ch;
    a.M = h->M;
    a.floor_db = (float)h->cfg.floor_db;
    a.hz_per_bin = (double)h->cfg.sample_rate / (double)h->N;
    hipLaunchKernelGGL(wf::peaks_read_kernel, dim3((a.n_rows + wf::WF_PEAKS_WAVES - 1) / wf::WF_PEAKS_WAVES), dim3(64 * wf::WF_PEAKS_WAVES), 0,
                       h->stream, a);
    return WF_HIP_OK;
}

// one workgroup per stream over its newest fft_size frames, behind the pushes issued
int launch_signal(wf_hip *h, uint32_t first, uint32_t count, void *d_block)
{
    wf::SignalArgs a{};
    a.rings = ring_view(h);
    a.out = static_cast<wf_hip_signal *>(d_block) + first;
    a.first = first;
    a.W = h->N; // (<= ring_cap: wf_hip_create sizes the ring from it)
    launch_by_channels(h, wf::signal_read_kernel<1>, wf::signal_read_kernel<2>, dim3(count), wf::WF_SIGNAL_THREADS, 0, a);
    return WF_HIP_OK;
}

// one workgroup per stream over its newest min(fft_size, 4096) frames, behind the pushes issued
int launch_pitch(wf_hip *h, uint32_t first, uint32_t count, void *d_block)
{
    wf::PitchArgs a{};
    a.rings = ring_view(h);
    a.out = static_cast<wf_hip_pitch *>(d_block) + first;
    a.sample_rate = (double)h->cfg.sample_rate;
    a.first = first;
    a.P = std::min<uint32_t>(h->N, WF_HIP_PITCH_MAX_WINDOW); // (a multiple of 16 on spectrum and meter batches; <= ring_cap)
    launch_by_channels(h, wf::pitch_read_kernel<1>, wf::pitch_read_kernel<2>, dim3(count), wf::WF_PITCH_THREADS, 0, a);
    return WF_HIP_OK;
}

// what the band levels derive from the configuration alone (wf::host::bands_tables)
int setup_bands(wf_hip *h)
{
    wf_hip::Bands &b = h->bands;
    const BandsTables t = bands_tables(h->cfg.sample_rate, h->N, h->M, h->tab.window);
    b.covered = t.covered;
    b.enbw = t.enbw;
    // (pageable memory: staged before the call returns, so `t` may go.  A retry after a failed second upload keeps the first)
    if(b.d_edges == nullptr)
        WF_TRY_RC(upload(h, &b.d_edges, t.edges));
    return upload(h, &b.d_weights, t.weights);
}

// one wavefront per m_decibels row, behind the ticks issued
int launch_bands(wf_hip *h, uint32_t first, uint32_t count, void *d_block)
{
    wf::BandsArgs a{};
    a.rows = h->d_decibels + (size_t)first * h->out_ch * h->M;
    a.out = static_cast<wf_hip_bands *>(d_block) + (size_t)first * h->out_ch;
    a.edges = h->bands.d_edges;
    a.n_rows = count * h->out_ch;
    a.M = h->M;
    a.covered = h->bands.covered;
    a.db_min = wf::db_min();
    a.enbw = h->bands.enbw;
    a.weights = h->bands.d_weights;
    hipLaunchKernelGGL(wf::bands_read_kernel, dim3((a.n_rows + wf::WF_BANDS_WAVES - 1) / wf::WF_BANDS_WAVES), dim3(64 * wf::WF_BANDS_WAVES),
                       0, h->stream, a);
    return WF_HIP_OK;
}

// what the stereo image derives from the configuration alone (wf::host::stereo_tables), in one block
int setup_stereo(wf_hip *h)
{
    wf_hip::Stereo &s = h->stereo;
    const StereoTables t = stereo_tables(h->cfg.sample_rate, h->N);
    s.P = t.P;
    s.log2p = t.log2p;
    s.covered = t.covered;
    // (64 KB at P = 4096: the most a workgroup gets without asking; asked for all the same, so that the limit is stated here)
    WF_TRY_RC(allow_lds(h, wf::stereo_read_kernel, WF_HIP_STEREO_MAX_WINDOW * sizeof(double2)));
    return upload(h, &s.d_tab, t.tab); // (pageable memory: staged before the call returns)
}

// one workgroup per stream over its newest P frames of both channels, behind the pushes issued
int launch_stereo(wf_hip *h, uint32_t first, uint32_t count, void *d_block)
{
    const wf_hip::Stereo &s = h->stereo;
    wf::StereoArgs a{};
    a.rings = ring_view(h);
    a.out = static_cast<wf_hip_stereo *>(d_block) + first;
    a.window = s.d_tab;
    a.tw = reinterpret_cast<const double2 *>(s.d_tab + s.P); // (16-byte aligned: P doubles behind a hipMalloc'ed block)
    a.edges = s.d_tab + 2 * (size_t)s.P;
    a.first = first;
    a.P = s.P;
    a.log2p = s.log2p;
    a.covered = s.covered;
    hipLaunchKernelGGL(wf::stereo_read_kernel, dim3(count), dim3(wf::WF_STEREO_THREADS), (size_t)s.P * sizeof(double2), h->stream, a);
    return WF_HIP_OK;
}

// what the constant-Q spectrum derives from the sample rate and the ring alone (wf::host::cq_tables)
int setup_cq(wf_hip *h)
{
    wf_hip::Cq &q = h->cq;
    const CqTables t = cq_tables(h->cfg.sample_rate, h->ring_cap);
    q.max_window = t.max_window;
    q.end_covered = t.end_covered;
    q.first_resolved = t.first_resolved;
    // (128 KB at the cap with two channels: more than a workgroup gets without asking)
    const int lds = (int)(WF_HIP_CQ_MAX_WINDOW * 2 * sizeof(float));
    WF_TRY_RC(allow_lds(h, wf::cq_read_kernel<1>, lds / 2));
    WF_TRY_RC(allow_lds(h, wf::cq_read_kernel<2>, lds));
    // (pageable memory: staged before the call returns, so `t` may go.  A retry after a failed second upload keeps the first)
    if(q.d_sched == nullptr)
        WF_TRY_RC(upload(h, &q.d_sched, t.sched));
    return upload(h, &q.d_tab, t.tab);
}

// one workgroup per stream over the newest Lmax frames of its captured channels, behind the pushes issued
int launch_cq(wf_hip *h, uint32_t first, uint32_t count, void *d_block)
{
    const wf_hip::Cq &q = h->cq;
    wf::CqArgs a{};
    a.rings = ring_view(h);
    a.out = static_cast<wf_hip_cq *>(d_block) + first;
    a.tab = q.d_tab;
    a.sched = q.d_sched;
    a.first = first;
    a.Lmax = q.max_window;
    a.end_covered = q.end_covered;
    a.first_resolved = q.first_resolved;
    const size_t lds = (size_t)h->cap_ch * q.max_window * sizeof(float);
    launch_by_channels(h, wf::cq_read_kernel<1>, wf::cq_read_kernel<2>, dim3(count), wf::WF_CQ_THREADS, lds, a);
    return WF_HIP_OK;
}

// the oscilloscope's window: the newest min(fft_size, WF_HIP_SCOPE_MAX_WINDOW) frames (<= ring_cap)
uint32_t scope_window(const wf_hip *h) { return std::min<uint32_t>(h->N, WF_HIP_SCOPE_MAX_WINDOW); }

// the oscilloscope has no tables: its kernels' dynamic LDS is all its first read asks for
int setup_scope(wf_hip *h)
{
    // (about 71 KB at the cap with two channels, the windows and the kernel's working set behind them: more than a workgroup
    // gets without asking, and two workgroups to a CU)
    WF_TRY_RC(allow_lds(h, wf::scope_read_kernel<1>, wf::scope_lds_bytes(1, WF_HIP_SCOPE_MAX_WINDOW)));
    WF_TRY_RC(allow_lds(h, wf::scope_read_kernel<2>, wf::scope_lds_bytes(2, WF_HIP_SCOPE_MAX_WINDOW)));
    return WF_HIP_OK;
}

// one workgroup per stream over its newest P frames of every captured channel, behind the pushes issued
int launch_scope(wf_hip *h, uint32_t first, uint32_t count, void *d_block)
{
    wf::ScopeArgs a{};
    a.rings = ring_view(h);
    a.out = static_cast<wf_hip_scope *>(d_block) + first;
    a.first = first;
    a.P = scope_window(h);
    a.V = a.P / 2;
    a.K = std::min<uint32_t>(WF_HIP_SCOPE_COLUMNS, a.V);
    const size_t lds = wf::scope_lds_bytes(h->cap_ch, a.P);
    launch_by_channels(h, wf::scope_read_kernel<1>, wf::scope_read_kernel<2>, dim3(count), wf::WF_SCOPE_THREADS, lds, a);
    return WF_HIP_OK;
}

// the vectorscope's window: the newest min(fft_size, WF_HIP_GONIO_MAX_WINDOW) frames (<= ring_cap)
uint32_t gonio_window(const wf_hip *h) { return std::min<uint32_t>(h->N, WF_HIP_GONIO_MAX_WINDOW); }

// the vectorscope has no tables either: its kernel's dynamic LDS is all its first read asks for
int setup_gonio(wf_hip *h)
{
    // (about 74 KB at the cap, both windows and the entry's image behind them: more than a workgroup gets without asking, and two
    // workgroups to a CU)
    WF_TRY_RC(allow_lds(h, wf::gonio_read_kernel, wf::gonio_lds_bytes(WF_HIP_GONIO_MAX_WINDOW)));
    return WF_HIP_OK;
}

// one workgroup per stream over its newest P frames of both captured channels, behind the pushes issued
int launch_gonio(wf_hip *h, uint32_t first, uint32_t count, void *d_block)
{
    wf::GonioArgs a{};
    a.rings = ring_view(h);
    a.out = static_cast<wf_hip_gonio *>(d_block) + first;
    a.first = first;
    a.P = gonio_window(h);
    hipLaunchKernelGGL(wf::gonio_read_kernel, dim3(count), dim3(wf::WF_GONIO_THREADS), wf::gonio_lds_bytes(a.P), h->stream, a);
    return WF_HIP_OK;
}

// what the sonogram derives from the sample rate and the ring alone (wf::host::sono_tables), in one block
int setup_sono(wf_hip *h)
{
    wf_hip::Sono &s = h->sono;
    const SonoTables t = sono_tables(h->cfg.sample_rate, h->ring_cap);
    s.columns = t.columns;
    s.first_covered = t.first_covered;
    s.end_covered = t.end_covered;
    // (64 KB, four columns' transforms: the most a workgroup gets without asking; asked for all the same, so that the limit is
    // stated here.  Two workgroups to a CU)
    WF_TRY_RC(allow_lds(h, wf::sono_read_kernel<1>, wf::WF_SONO_LDS_BYTES));
    WF_TRY_RC(allow_lds(h, wf::sono_read_kernel<2>, wf::WF_SONO_LDS_BYTES));
    return upload(h, &s.d_tab, t.tab); // (pageable memory: staged before the call returns)
}

// one wavefront per column, four columns to a workgroup, over the newest T columns of every captured channel's ring, behind the
// pushes issued
int launch_sono(wf_hip *h, uint32_t first, uint32_t count, void *d_block)
{
    const wf_hip::Sono &s = h->sono;
    constexpr uint32_t P = WF_HIP_SONO_WINDOW;
    wf::SonoArgs a{};
    a.rings = ring_view(h);
    a.window = s.d_tab;
    a.tw = reinterpret_cast<const double2 *>(s.d_tab + P); // (16-byte aligned: P doubles behind a hipMalloc'ed block)
    a.edges = s.d_tab + 2 * (size_t)P;
    a.columns = s.columns; // (>= 4: why_no_sono)
    a.first_covered = s.first_covered;
    a.end_covered = s.end_covered;
    // (streams are indexed by blockIdx.y, at most 65535: larger ranges go out in parts)
    for(uint32_t off = 0; off < count; off += 65535u) {
        const dim3 grid((s.columns + wf::WF_SONO_WAVES - 1) / wf::WF_SONO_WAVES, std::min(65535u, count - off));
        a.out = static_cast<wf_hip_sono *>(d_block) + first + off;
        a.first = first + off;
        launch_by_channels(h, wf::sono_read_kernel<1>, wf::sono_read_kernel<2>, grid, wf::WF_SONO_THREADS, wf::WF_SONO_LDS_BYTES, a);
    }
    return WF_HIP_OK;
}

// the bit meter's window: the newest min(fft_size, WF_HIP_BITS_MAX_WINDOW) frames (<= ring_cap)
uint32_t bits_window(const wf_hip *h) { return std::min<uint32_t>(h->N, WF_HIP_BITS_MAX_WINDOW); }

// the bit meter has no tables: its kernels' dynamic LDS is all its first read asks for
int setup_bits(wf_hip *h)
{
    // (about 69 KB at the cap with two channels, the windows and the kernel's working set behind them: more than a workgroup
    // gets without asking, and two workgroups to a CU)
    WF_TRY_RC(allow_lds(h, wf::bits_read_kernel<1>, wf::bits_lds_bytes(1, WF_HIP_BITS_MAX_WINDOW)));
    WF_TRY_RC(allow_lds(h, wf::bits_read_kernel<2>, wf::bits_lds_bytes(2, WF_HIP_BITS_MAX_WINDOW)));
    return WF_HIP_OK;
}

// one workgroup per stream over its newest P frames of every captured channel, behind the pushes issued
int launch_bits(wf_hip *h, uint32_t first, uint32_t count, void *d_block)
{
    wf::BitsArgs a{};
    a.rings = ring_view(h);
    a.out = static_cast<wf_hip_bits *>(d_block) + first;
    a.first = first;
    a.P = bits_window(h);
    const size_t lds = wf::bits_lds_bytes(h->cap_ch, a.P);
    launch_by_channels(h, wf::bits_read_kernel<1>, wf::bits_read_kernel<2>, dim3(count), wf::WF_BITS_THREADS, lds, a);
    return WF_HIP_OK;
}

// what the distortion and the intermodulation analyser derive from the configuration alone (wf::host::thd_tables), in one block:
// built by whichever of the two outputs is read first
int setup_thd_tables(wf_hip *h)
{
    wf_hip::Thd &d = h->thd;
    if(d.d_tab != nullptr)
        return WF_HIP_OK;
    const ThdTables t = thd_tables(h->cfg.sample_rate, h->N);
    d.P = t.P;
    d.log2p = t.log2p;
    d.S = t.S;
    const int rc = upload(h, &d.d_tab, t.tab); // (pageable memory: staged before the call returns)
    if(rc)
        d.d_tab = nullptr; // (the next first read builds them again)
    return rc;
}

int setup_thd(wf_hip *h)
{
    // (128 KB at P = 8192: twice what a workgroup gets without asking, and one workgroup to a CU)
    const int lds = (int)(WF_HIP_THD_MAX_WINDOW * sizeof(double2));
    WF_TRY_RC(allow_lds(h, wf::thd_read_kernel<1>, lds));
    WF_TRY_RC(allow_lds(h, wf::thd_read_kernel<2>, lds));
    return setup_thd_tables(h);
}

// one workgroup per stream over its newest P frames of every captured channel, behind the pushes issued
int launch_thd(wf_hip *h, uint32_t first, uint32_t count, void *d_block)
{
    const wf_hip::Thd &d = h->thd;
    wf::ThdArgs a{};
    a.rings = ring_view(h);
    a.out = static_cast<wf_hip_thd *>(d_block) + first;
    a.window = d.d_tab;
    a.tw = reinterpret_cast<const double2 *>(d.d_tab + d.P); // (16-byte aligned: P doubles behind a hipMalloc'ed block)
    a.S = d.S;
    a.sample_rate = (double)h->cfg.sample_rate;
    a.first = first;
    a.P = d.P; // (<= fft_size <= ring_cap)
    a.log2p = d.log2p;
    const size_t lds = (size_t)d.P * sizeof(double2);
    launch_by_channels(h, wf::thd_read_kernel<1>, wf::thd_read_kernel<2>, dim3(count), wf::WF_THD_THREADS, lds, a);
    return WF_HIP_OK;
}

// what the delay finder derives from the configuration alone (wf::host::delay_tables), in one block
int setup_delay(wf_hip *h)
{
    wf_hip::Delay &d = h->delay;
    const DelayTables t = delay_tables(h->N);
    d.P = t.P;
    d.log2p = t.log2p;
    // (two regions, 128 KB at P = 4096: twice what a workgroup gets without asking, and one workgroup to a CU)
    const int lds = (int)(2 * WF_HIP_DELAY_MAX_WINDOW * sizeof(double2));
    WF_TRY_RC(allow_lds(h, wf::delay_read_kernel, lds));
    return upload(h, &d.d_tab, t.tab); // (pageable memory: staged before the call returns)
}

// one workgroup per stream over the newest P frames of both captured channels, behind the pushes issued
int launch_delay(wf_hip *h, uint32_t first, uint32_t count, void *d_block)
{
    const wf_hip::Delay &d = h->delay;
    wf::DelayArgs a{};
    a.rings = ring_view(h); // (two captured channels: why_no_delay)
    a.out = static_cast<wf_hip_delay *>(d_block) + first;
    a.window = d.d_tab;
    a.tw = reinterpret_cast<const double2 *>(d.d_tab + d.P); // (16-byte aligned: P doubles behind a hipMalloc'ed block)
    a.sample_rate = (double)h->cfg.sample_rate;
    a.first = first;
    a.P = d.P; // (<= fft_size <= ring_cap)
    a.log2p = d.log2p;
    hipLaunchKernelGGL(wf::delay_read_kernel, dim3(count), dim3(wf::WF_DELAY_THREADS), 2 * (size_t)d.P * sizeof(double2), h->stream, a);
    return WF_HIP_OK;
}

// what the onset detector derives from the sample rate and the ring alone: the sonogram's tables (wf::host::sono_tables), in one block
int setup_onset(wf_hip *h)
{
    wf_hip::Onset &o = h->onset;
    const SonoTables t = sono_tables(h->cfg.sample_rate, h->ring_cap);
    // Ts spectral columns, T = Ts - 1 strengths: Ts H + P <= ring_cap, so the oldest is in the ring wherever in a hop the counter stands
    o.spectral = std::min<uint32_t>(WF_HIP_ONSET_COLUMNS + 1, (h->ring_cap - WF_HIP_ONSET_WINDOW) / WF_HIP_ONSET_HOP); // (>= 28: why_no_onset)
    // (about 69 KB, four columns' transforms, the round's levels and the entry's strengths: more than a workgroup gets without
    // asking, and two workgroups to a CU)
    WF_TRY_RC(allow_lds(h, wf::onset_read_kernel<1>, wf::WF_ONSET_LDS_BYTES));
    WF_TRY_RC(allow_lds(h, wf::onset_read_kernel<2>, wf::WF_ONSET_LDS_BYTES));
    return upload(h, &o.d_tab, t.tab); // (pageable memory: staged before the call returns)
}

// one workgroup per stream, one wavefront per spectral column in rounds of four, over the newest Ts columns of every captured
// channel's ring, behind the pushes issued
int launch_onset(wf_hip *h, uint32_t first, uint32_t count, void *d_block)
{
    const wf_hip::Onset &o = h->onset;
    constexpr uint32_t P = WF_HIP_ONSET_WINDOW;
    wf::OnsetArgs a{};
    a.rings = ring_view(h);
    a.out = static_cast<wf_hip_onset *>(d_block) + first;
    a.window = o.d_tab;
    a.tw = reinterpret_cast<const double2 *>(o.d_tab + P); // (16-byte aligned: P doubles behind a hipMalloc'ed block)
    a.edges = o.d_tab + 2 * (size_t)P;
    a.first = first;
    a.spectral = o.spectral;
    launch_by_channels(h, wf::onset_read_kernel<1>, wf::onset_read_kernel<2>, dim3(count), wf::WF_ONSET_THREADS, wf::WF_ONSET_LDS_BYTES, a);
    return WF_HIP_OK;
}

// what the transfer function and the impulse response derive from the configuration and the ring: P and K, and the delay finder's
// tables at that P.  Each output's first read makes a plan of its own, so neither needs the other read first
int setup_xfer_plan(wf_hip *h, wf_hip::XferPlan &x)
{
    const uint32_t P = xfer_window(h->N, h->ring_cap); // (>= 64: why_no_xfer, why_no_impulse)
    const DelayTables t = delay_tables(P);             // (a power of two <= WF_HIP_DELAY_MAX_WINDOW: its own window)
    x.P = t.P;
    x.log2p = t.log2p;
    x.K = xfer_segments(P, h->ring_cap);
    // (48 KB of dynamic LDS at the cap: what a workgroup gets without asking)
    return upload(h, &x.d_tab, t.tab); // (pageable memory: staged before the call returns)
}
int setup_xfer(wf_hip *h) { return setup_xfer_plan(h, h->xfer); }
int setup_impulse(wf_hip *h) { return setup_xfer_plan(h, h->impulse); }

// one workgroup per stream over the K newest anchored segments of both captured channels, behind the pushes issued
int launch_xfer(wf_hip *h, uint32_t first, uint32_t count, void *d_block)
{
    const wf_hip::XferPlan &x = h->xfer;
    wf::XferArgs a{};
    a.rings = ring_view(h); // (two captured channels: why_no_xfer)
    a.out = static_cast<wf_hip_xfer *>(d_block) + first;
    a.window = x.d_tab;
    a.tw = reinterpret_cast<const double2 *>(x.d_tab + x.P); // (16-byte aligned: P doubles behind a hipMalloc'ed block)
    a.first = first;
    a.P = x.P; // (<= ring_cap / 8)
    a.log2p = x.log2p;
    a.K = x.K;
    hipLaunchKernelGGL(wf::xfer_read_kernel, dim3(count), dim3(wf::WF_XFER_THREADS), (size_t)(x.P + x.P / 2 + 1) * sizeof(double2), h->stream, a);
    return WF_HIP_OK;
}

// one workgroup per stream over the K newest anchored segments of both captured channels, behind the pushes issued
int launch_impulse(wf_hip *h, uint32_t first, uint32_t count, void *d_block)
{
    const wf_hip::XferPlan &x = h->impulse;
    wf::ImpulseArgs a{};
    a.rings = ring_view(h); // (two captured channels: why_no_impulse)
    a.out = static_cast<wf_hip_impulse *>(d_block) + first;
    a.window = x.d_tab;
    a.tw = reinterpret_cast<const double2 *>(x.d_tab + x.P); // (16-byte aligned: P doubles behind a hipMalloc'ed block)
    a.sample_rate = (double)h->cfg.sample_rate;
    a.first = first;
    a.P = x.P; // (<= ring_cap / 8)
    a.log2p = x.log2p;
    a.K = x.K;
    hipLaunchKernelGGL(wf::impulse_read_kernel, dim3(count), dim3(wf::WF_XFER_THREADS), (size_t)(x.P + x.P / 2 + 1) * sizeof(double2), h->stream, a);
    return WF_HIP_OK;
}

// the click detector's window: the newest min(fft_size, WF_HIP_CLICK_MAX_WINDOW) frames (<= ring_cap)
uint32_t click_window(const wf_hip *h) { return std::min<uint32_t>(h->N, WF_HIP_CLICK_MAX_WINDOW); }

// the click detector has no tables: its kernels' dynamic LDS is all its first read asks for
int setup_click(wf_hip *h)
{
    // (about 73 KB at the cap, the window, the residual and the kernel's working set behind them: more than a workgroup gets
    // without asking, and two workgroups to a CU)
    WF_TRY_RC(allow_lds(h, wf::click_read_kernel<1>, wf::click_lds_bytes(WF_HIP_CLICK_MAX_WINDOW)));
    WF_TRY_RC(allow_lds(h, wf::click_read_kernel<2>, wf::click_lds_bytes(WF_HIP_CLICK_MAX_WINDOW)));
    return WF_HIP_OK;
}

// one workgroup per stream and captured channel over its newest P frames, behind the pushes issued
int launch_click(wf_hip *h, uint32_t first, uint32_t count, void *d_block)
{
    wf::ClickArgs a{};
    a.rings = ring_view(h);
    a.out = static_cast<wf_hip_click *>(d_block) + first;
    a.sample_rate = (double)h->cfg.sample_rate;
    a.first = first;
    a.P = click_window(h); // (>= 256: why_no_click)
    const size_t lds = wf::click_lds_bytes(a.P);
    launch_by_channels(h, wf::click_read_kernel<1>, wf::click_read_kernel<2>, dim3(count), dim3(count * 2u), wf::WF_CLICK_THREADS, lds, a);
    return WF_HIP_OK;
}

// the intermodulation analyser's window and tables are the distortion analyser's
int setup_imd(wf_hip *h)
{
    // (128 KB at P = 8192, as setup_thd)
    const int lds = (int)(WF_HIP_THD_MAX_WINDOW * sizeof(double2));
    WF_TRY_RC(allow_lds(h, wf::imd_read_kernel<1>, lds));
    WF_TRY_RC(allow_lds(h, wf::imd_read_kernel<2>, lds));
    return setup_thd_tables(h);
}

// one workgroup per stream over its newest P frames of every captured channel, behind the pushes issued
int launch_imd(wf_hip *h, uint32_t first, uint32_t count, void *d_block)
{
    const wf_hip::Thd &d = h->thd;
    wf::ImdArgs a{};
    a.rings = ring_view(h);
    a.out = static_cast<wf_hip_imd *>(d_block) + first;
    a.window = d.d_tab;
    a.tw = reinterpret_cast<const double2 *>(d.d_tab + d.P); // (16-byte aligned: P doubles behind a hipMalloc'ed block)
    a.S = d.S;
    a.sample_rate = (double)h->cfg.sample_rate;
    a.first = first;
    a.P = d.P; // (<= fft_size <= ring_cap)
    a.log2p = d.log2p;
    const size_t lds = (size_t)d.P * sizeof(double2);
    launch_by_channels(h, wf::imd_read_kernel<1>, wf::imd_read_kernel<2>, dim3(count), wf::WF_THD_THREADS, lds, a);
    return WF_HIP_OK;
}

// what the tempo output derives from the sample rate and the ring alone: the sonogram's tables (wf::host::sono_tables) for its
// columns, the lags and the preference (wf::host::tempo_tables), and the block its columns kernel leaves the strengths in
int setup_tempo(wf_hip *h)
{
    wf_hip::Tempo &m = h->tempo;
    const TempoTables t = tempo_tables(h->cfg.sample_rate, h->ring_cap); // (served: why_no_tempo)
    m.columns = t.plan.columns;
    m.lag_lo = t.plan.lag_lo;
    m.lag_hi = t.plan.lag_hi;
    // (66.5 KB, four columns' transforms and the round's levels: more than a workgroup gets without asking, and two workgroups to a CU)
    WF_TRY_RC(allow_lds(h, wf::tempo_columns_kernel<1>, wf::WF_TEMPO_LDS_BYTES));
    WF_TRY_RC(allow_lds(h, wf::tempo_columns_kernel<2>, wf::WF_TEMPO_LDS_BYTES));
    // (a retry after a failed allocation or upload keeps what succeeded)
    if(m.d_strength == nullptr)
        WF_TRY_RC(dev_alloc(h, &m.d_strength, (size_t)h->n_streams * WF_HIP_TEMPO_COLUMNS));
    if(m.d_tab == nullptr) {
        const int rc = upload(h, &m.d_tab, sono_tables(h->cfg.sample_rate, h->ring_cap).tab); // (pageable memory: staged before the call returns)
        if(rc) {
            m.d_tab = nullptr; // (the next first read builds them again)
            return rc;
        }
    }
    return upload(h, &m.d_prior, t.prior);
}

// the columns in chunks of 64 over the grid, one wavefront per spectral column in rounds of four, then one workgroup per stream
// for the rule: over the newest T + 1 columns of every captured channel's ring, behind the pushes issued
int launch_tempo(wf_hip *h, uint32_t first, uint32_t count, void *d_block)
{
    const wf_hip::Tempo &m = h->tempo;
    constexpr uint32_t P = WF_HIP_TEMPO_WINDOW;
    wf::TempoColumnsArgs c{};
    c.rings = ring_view(h);
    c.strength = m.d_strength;
    c.window = m.d_tab;
    c.tw = reinterpret_cast<const double2 *>(m.d_tab + P); // (16-byte aligned: P doubles behind a hipMalloc'ed block)
    c.edges = m.d_tab + 2 * (size_t)P;
    c.columns = m.columns;
    wf::TempoArgs a{};
    a.rings = c.rings;
    a.strength = m.d_strength;
    a.prior = m.d_prior;
    a.beats = 60.0 * (double)h->cfg.sample_rate / (double)WF_HIP_TEMPO_HOP;
    a.columns = m.columns;
    a.lag_lo = m.lag_lo;
    a.lag_hi = m.lag_hi;
    // (the columns kernel indexes streams by blockIdx.y, at most 65535: larger ranges go out in parts)
    for(uint32_t off = 0; off < count; off += 65535u) {
        const uint32_t part = std::min(65535u, count - off);
        c.first = a.first = first + off;
        a.out = static_cast<wf_hip_tempo *>(d_block) + first + off;
        const dim3 grid((m.columns + wf::WF_TEMPO_CHUNK - 1) / wf::WF_TEMPO_CHUNK, part);
        launch_by_channels(h, wf::tempo_columns_kernel<1>, wf::tempo_columns_kernel<2>, grid, wf::WF_ONSET_THREADS, wf::WF_TEMPO_LDS_BYTES, c);
        hipLaunchKernelGGL(wf::tempo_read_kernel, dim3(part), dim3(wf::WF_TEMPO_THREADS), 0, h->stream, a);
    }
    return WF_HIP_OK;
}

// what the hum detector derives from the sample rate and the ring alone (wf::host::hum_tables): the plan's scalars, the twiddles of
// the M-point transform, the combination twiddles and the search ranges
int setup_hum(wf_hip *h)
{
    wf_hip::Hum &m = h->hum;
    const HumTables t = hum_tables(h->cfg.sample_rate, h->ring_cap); // (served: why_no_hum)
    const HumPlan &p = t.plan;
    m.D = p.D;
    m.N = p.N;
    m.M = p.M;
    m.log2m = p.log2m;
    m.K = p.K;
    m.noise_lo = p.noise_lo;
    m.noise_hi = p.noise_hi;
    m.hz = p.hz;
    // (the staged window, 128 KB at N = 32768, the transform's 16 KB and the bins: the most of every plan, 157.1 KB, with the
    // hand-overs inside the 160 KiB a workgroup may hold -- wf_hum.hpp asserts it -- and one workgroup to a CU)
    WF_TRY_RC(allow_lds(h, wf::hum_read_kernel, wf::hum_lds_bytes(32, 1024, wf::WF_HUM_MAX_BINS - 2)));
    // (a retry after a failed allocation or upload keeps what succeeded; pageable memory: staged before the calls return)
    if(m.d_tw == nullptr)
        WF_TRY_RC(upload(h, &m.d_tw, t.tw));
    if(m.d_comb == nullptr)
        WF_TRY_RC(upload(h, &m.d_comb, t.comb));
    return upload(h, &m.d_ranges, t.ranges);
}

// one workgroup per stream and captured channel over the newest N frames of its ring, behind the pushes issued
int launch_hum(wf_hip *h, uint32_t first, uint32_t count, void *d_block)
{
    const wf_hip::Hum &m = h->hum;
    wf::HumArgs a{};
    a.rings = ring_view(h);
    a.tw = reinterpret_cast<const double2 *>(m.d_tw); // (16-byte aligned: hipMalloc'ed blocks)
    a.comb = reinterpret_cast<const double2 *>(m.d_comb);
    a.ranges = m.d_ranges;
    a.hz = m.hz;
    a.channels = h->cap_ch;
    a.D = m.D;
    a.log2d = (uint32_t)__builtin_ctz(m.D);
    a.N = m.N; // (<= ring_cap)
    a.M = m.M;
    a.log2m = m.log2m;
    a.K = m.K;
    a.noise_lo = m.noise_lo;
    a.noise_hi = m.noise_hi;
    const size_t lds = wf::hum_lds_bytes(m.D, m.M, m.K);
    // (streams by blockIdx.x, channels by blockIdx.y; a grid's x holds any count of streams there is)
    a.first = first;
    a.out = static_cast<wf_hip_hum *>(d_block) + first;
    hipLaunchKernelGGL(wf::hum_read_kernel, dim3(count, h->cap_ch), dim3(wf::WF_HUM_THREADS), lds, h->stream, a);
    return WF_HIP_OK;
}

// why a batch has no such output (nullptr: it has)
const char *why_no_loudness(const wf_hip *h) { return loudness_on(h) ? nullptr : "the loudness producer is not enabled (wf_hip_enable_loudness)"; }
const char *why_no_peaks(const wf_hip *h) { return (h->meter || h->wave) ? "meter / waveform batch: spectral peaks belong to spectrum batches" : nullptr; }
const char *why_no_bands(const wf_hip *h) { return (h->meter || h->wave) ? "meter / waveform batch: band levels belong to spectrum batches" : nullptr; }
const char *why_no_signal(const wf_hip *h)
{
    return h->wave ? "waveform batch: signal statistics belong to spectrum and meter batches (a window of fft_size frames)" : nullptr;
}
const char *why_no_pitch(const wf_hip *h)
{
    if(h->wave)
        return "waveform batch: the pitch belongs to spectrum and meter batches (a window of fft_size frames)";
    return h->N < 64 ? "the pitch needs a window of at least 64 frames" : nullptr;
}

const char *why_no_stereo(const wf_hip *h)
{
    if(h->wave)
        return "waveform batch: the stereo image belongs to spectrum and meter batches (a window of fft_size frames)";
    if(h->cap_ch != 2)
        return "one captured channel: the stereo image needs two (capture_channels == 2)";
    return h->N < 64 ? "the stereo image needs a window of at least 64 frames" : nullptr;
}

const char *why_no_cq(const wf_hip *h)
{
    return h->wave ? "waveform batch: the constant-Q spectrum belongs to spectrum and meter batches" : nullptr;
}

const char *why_no_scope(const wf_hip *h)
{
    if(h->wave)
        return "waveform batch: the oscilloscope belongs to spectrum and meter batches (a window of fft_size frames)";
    return h->N < 64 ? "the oscilloscope needs a window of at least 64 frames" : nullptr;
}

const char *why_no_gonio(const wf_hip *h)
{
    if(h->wave)
        return "waveform batch: the vectorscope belongs to spectrum and meter batches (a window of fft_size frames)";
    return h->cap_ch != 2 ? "one captured channel: the vectorscope needs two (capture_channels == 2)" : nullptr;
}

const char *why_no_sono(const wf_hip *h)
{
    if(h->wave)
        return "waveform batch: the sonogram belongs to spectrum and meter batches";
    return h->ring_cap < 2 * WF_HIP_SONO_WINDOW ? "the sonogram needs a ring of at least 2048 frames (wf_hip_create's ring_frames)" : nullptr;
}

const char *why_no_bits(const wf_hip *h)
{
    return h->wave ? "waveform batch: the bit statistics belong to spectrum and meter batches (a window of fft_size frames)" : nullptr;
}

const char *why_no_thd(const wf_hip *h)
{
    if(h->wave)
        return "waveform batch: the distortion analyser belongs to spectrum and meter batches (a window of fft_size frames)";
    return h->N < 512 ? "the distortion analyser needs a window of at least 512 frames" : nullptr;
}

const char *why_no_delay(const wf_hip *h)
{
    if(h->wave)
        return "waveform batch: the inter-channel delay belongs to spectrum and meter batches (a window of fft_size frames)";
    return h->cap_ch != 2 ? "the inter-channel delay needs two captured channels" : nullptr;
}

const char *why_no_onset(const wf_hip *h)
{
    if(h->wave)
        return "waveform batch: the onset detector belongs to spectrum and meter batches";
    return h->ring_cap < 8192 ? "the onset detector needs a ring of at least 8192 frames (wf_hip_create's ring_frames)" : nullptr;
}

const char *why_no_xfer(const wf_hip *h)
{
    if(h->wave)
        return "waveform batch: the transfer function belongs to spectrum and meter batches (a window of fft_size frames)";
    if(h->cap_ch != 2)
        return "the transfer function needs two captured channels";
    if(h->N < 256)
        return "the transfer function needs a window of at least 256 frames";
    return h->ring_cap < 512 ? "the transfer function needs a ring of at least 512 frames (wf_hip_create's ring_frames)" : nullptr;
}

const char *why_no_impulse(const wf_hip *h)
{
    if(h->wave)
        return "waveform batch: the impulse response belongs to spectrum and meter batches (a window of fft_size frames)";
    if(h->cap_ch != 2)
        return "the impulse response needs two captured channels";
    if(h->N < 256)
        return "the impulse response needs a window of at least 256 frames";
    return h->ring_cap < 512 ? "the impulse response needs a ring of at least 512 frames (wf_hip_create's ring_frames)" : nullptr;
}

const char *why_no_click(const wf_hip *h)
{
    if(h->wave)
        return "waveform batch: the click detector belongs to spectrum and meter batches (a window of fft_size frames)";
    return h->N < 256 ? "the click detector needs a window of at least 256 frames" : nullptr;
}

const char *why_no_imd(const wf_hip *h)
{
    if(h->wave)
        return "waveform batch: the intermodulation analyser belongs to spectrum and meter batches (a window of fft_size frames)";
    return h->N < 512 ? "the intermodulation analyser needs a window of at least 512 frames" : nullptr;
}

const char *why_no_tempo(const wf_hip *h)
{
    if(h->wave)
        return "waveform batch: the tempo belongs to spectrum and meter batches";
    if(h->ring_cap < WF_HIP_TEMPO_MIN_RING)
        return "the tempo needs a ring of at least 131072 frames (wf_hip_create's ring_frames)";
    return tempo_plan(h->cfg.sample_rate, h->ring_cap).served() ? nullptr
                                                                 : "the tempo has fewer than three lags between 240 and 40 BPM at this sample rate";
}

const char *why_no_hum(const wf_hip *h)
{
    if(h->wave)
        return "waveform batch: the hum detector belongs to spectrum and meter batches";
    const HumPlan p = hum_plan(h->cfg.sample_rate, h->ring_cap);
    if(p.served())
        return nullptr;
    return p.too_fast() ? "the hum detector serves no sample rate under 2560 Hz or above 98304 Hz (bins of at most 3 Hz from 32768 frames)"
                        : "the hum detector needs a ring of at least sample_rate / 3 frames (wf_hip_create's ring_frames)";
}

struct Measure {
    wf_hip_output what;
    size_t entry_bytes;
    bool per_row; // one entry per m_decibels row (out_ch per stream), not one per stream
    const char *(*why_not)(const wf_hip *);
    int (*setup)(wf_hip *); // what the output's first read makes before its first launch (nullptr: nothing)
    int (*launch)(wf_hip *, uint32_t first, uint32_t count, void *d_block);
};

// Row i is output WF_HIP_OUT_LOUDNESS + i: its block is wf_hip::d_measure[i], and wf_hip::measure_ready[i] says that its setup has
// been done
constexpr Measure MEASURES[] = {
    {WF_HIP_OUT_LOUDNESS, sizeof(wf_hip_loudness), false, why_no_loudness, nullptr, launch_loudness},
    {WF_HIP_OUT_PEAKS, sizeof(wf_hip_peaks), true, why_no_peaks, nullptr, launch_peaks},
    {WF_HIP_OUT_SIGNAL, sizeof(wf_hip_signal), false, why_no_signal, nullptr, launch_signal},
    {WF_HIP_OUT_PITCH, sizeof(wf_hip_pitch), false, why_no_pitch, nullptr, launch_pitch},
    {WF_HIP_OUT_BANDS, sizeof(wf_hip_bands), true, why_no_bands, setup_bands, launch_bands},
    {WF_HIP_OUT_STEREO, sizeof(wf_hip_stereo), false, why_no_stereo, setup_stereo, launch_stereo},
    {WF_HIP_OUT_CQ, sizeof(wf_hip_cq), false, why_no_cq, setup_cq, launch_cq},
    {WF_HIP_OUT_SCOPE, sizeof(wf_hip_scope), false, why_no_scope, setup_scope, launch_scope},
    {WF_HIP_OUT_GONIO, sizeof(wf_hip_gonio), false, why_no_gonio, setup_gonio, launch_gonio},
    {WF_HIP_OUT_SONO, sizeof(wf_hip_sono), false, why_no_sono, setup_sono, launch_sono},
    {WF_HIP_OUT_BITS, sizeof(wf_hip_bits), false, why_no_bits, setup_bits, launch_bits},
    {WF_HIP_OUT_THD, sizeof(wf_hip_thd), false, why_no_thd, setup_thd, launch_thd},
    {WF_HIP_OUT_DELAY, sizeof(wf_hip_delay), false, why_no_delay, setup_delay, launch_delay},
    {WF_HIP_OUT_ONSET, sizeof(wf_hip_onset), false, why_no_onset, setup_onset, launch_onset},
    {WF_HIP_OUT_XFER, sizeof(wf_hip_xfer), false, why_no_xfer, setup_xfer, launch_xfer},
    {WF_HIP_OUT_IMPULSE, sizeof(wf_hip_impulse), false, why_no_impulse, setup_impulse, launch_impulse},
    {WF_HIP_OUT_CLICK, sizeof(wf_hip_click), false, why_no_click, setup_click, launch_click},
    {WF_HIP_OUT_IMD, sizeof(wf_hip_imd), false, why_no_imd, setup_imd, launch_imd},
    {WF_HIP_OUT_TEMPO, sizeof(wf_hip_tempo), false, why_no_tempo, setup_tempo, launch_tempo},
    {WF_HIP_OUT_HUM, sizeof(wf_hip_hum), false, why_no_hum, setup_hum, launch_hum},
};
static_assert(sizeof(MEASURES) / sizeof(MEASURES[0]) == wf_hip::N_MEASURES, "a row of MEASURES for each of wf_hip's N_MEASURES blocks");

constexpr bool rows_follow_the_enum()
{
    for(int i = 0; i < wf_hip::N_MEASURES; ++i)
        if(MEASURES[i].what != WF_HIP_OUT_LOUDNESS + i)
            return false;
    return true;
}
static_assert(rows_follow_the_enum(), "row i of MEASURES is output WF_HIP_OUT_LOUDNESS + i");

int measure_row(wf_hip_output what) // -1: not a measurement output
{
    const int i = (int)what - (int)WF_HIP_OUT_LOUDNESS;
    return i >= 0 && i < wf_hip::N_MEASURES ? i : -1;
}

size_t bytes_per_stream(const wf_hip *h, const Measure &m) { return m.entry_bytes * (m.per_row ? h->out_ch : 1u); }

} // namespace

// ring trimming would drop frames from the measurement: while the producer is on, nothing longer than the ring is taken
int wf::host::measure_check_push(wf_hip *h, uint32_t frames)
{
    if(loudness_on(h) && frames > h->ring_cap)
        return fail(h, WF_HIP_ERR_INVALID, "push of %u frames exceeds the ring capacity %u while the loudness producer is on", frames, h->ring_cap);
    return WF_HIP_OK;
}

// the loudness producer follows every push: one launch behind the write positions' advance over the frames the push
// appended, ring[wpos - n, wpos) (d_frames: a ragged push's per-stream counts, capped at `frames`)
void wf::host::measure_after_push(wf_hip *h, uint32_t first, uint32_t count, uint32_t frames, const uint32_t *d_frames)
{
    if(!loudness_on(h) || frames == 0)
        return;
    wf::LoudPushArgs a{};
    a.rings = ring_view(h);
    a.frames_per_stream = d_frames;
    a.state = h->loud.d_state;
    a.hist = h->loud.d_hist;
    a.first = first;
    a.frames = frames;
    a.k = h->loud.k;
    // (a wavefront per captured channel)
    launch_by_channels(h, wf::loudness_push_kernel<1>, wf::loudness_push_kernel<2>, dim3(count), 64u * h->cap_ch, 0, a);
}

bool wf::host::measure_source(const wf_hip *h, wf_hip_output what, size_t *per_stream, const char **why)
{
    const int i = measure_row(what);
    if(i < 0)
        return false;
    *why = MEASURES[i].why_not(h);
    *per_stream = *why ? 0 : bytes_per_stream(h, MEASURES[i]);
    return true;
}

int wf::host::measure_read(wf_hip *h, wf_hip_output what, uint32_t first, uint32_t count, void *out)
{
    const int i = measure_row(what);
    const Measure &m = MEASURES[i];
    if(const char *why = m.why_not(h))
        return fail(h, WF_HIP_ERR_INVALID, "%s", why);
    if(out == nullptr)
        return fail(h, WF_HIP_ERR_INVALID, "output pointer is NULL");
    WF_HIP_TRY(h, hipSetDevice(h->device));
    const size_t per = bytes_per_stream(h, m);
    // (the first read may be of a slice: the block is for every stream)
    if(h->d_measure[i] == nullptr)
        WF_TRY_RC(dev_alloc(h, &h->d_measure[i], (size_t)h->n_streams * per));
    // (the flag only behind a setup that succeeded: a first read that failed is set up again by the next)
    if(!h->measure_ready[i]) {
        if(m.setup)
            WF_TRY_RC(m.setup(h));
        h->measure_ready[i] = true;
    }
    WF_TRY_RC(m.launch(h, first, count, h->d_measure[i]));
    WF_HIP_TRY(h, hipGetLastError());
    return read_back(h, h->d_measure[i] + (size_t)first * per, out, (size_t)count * per);
}

int wf_hip_enable_loudness(wf_hip *h, uint32_t first, uint32_t count)
{
    WF_TRY_RC(check_range(h, first, count));
    if(loudness_on(h)) { // on already: restart the range
        WF_HIP_TRY(h, hipSetDevice(h->device));
        WF_TRY_RC(clear_loudness(h, first, count));
        h->main_dirty = true;
        return WF_HIP_OK;
    }
    if(h->cfg.sample_rate % 10 != 0 || h->cfg.sample_rate == 0)
        return fail(h, WF_HIP_ERR_INVALID, "sample_rate %u: the loudness producer's 100 ms step must be whole frames", h->cfg.sample_rate);
    WF_HIP_TRY(h, hipSetDevice(h->device));
    WF_TRY_RC(join_lanes(h));
    wf::LoudState *st = nullptr;
    wf::LoudHist *hist = nullptr;
    int rc = dev_alloc(h, &st, h->n_streams);
    if(rc == WF_HIP_OK) rc = dev_alloc(h, &hist, (size_t)h->n_streams * 2);
    if(rc)
        return rc;
    h->loud.k = wf::host::loudness_coefs(h->cfg.sample_rate);
    h->loud.d_hist = hist;
    h->loud.d_state = st; // from here on every push feeds the producer
    WF_TRY_RC(clear_loudness(h, 0, h->n_streams));
    h->main_dirty = true;
    return WF_HIP_OK;
}
