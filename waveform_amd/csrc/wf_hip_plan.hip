// wf_hip_plan.hip -- the plan step of the C ABI (include/wf_hip.h): wf_hip_create builds a handle from a wf_config -- what
// WAVSource::update() does per source (buffers, FFT plan, window / slope / roll-off / interpolation tables: reference
// src/source.cpp:1169-1290, :837-918), here for a batch, as a sequence of stages (build_handle, at the end of the anonymous
// namespace, is the order on one screen): validate and plan (what needs no device is decided by wf_tick_plan.cpp), open the
// device, allocate state, the display tables, the FFT tables of the plan's family + the kernel instantiation (wf_tick_geom.hip /
// wf_big_dispatch.hip), the lanes, the constant kernel arguments, reset -- and wf_hip_destroy gives it all back (free_bufs,
// src/source.cpp:782-808).  Every stage writes what it decides or uploads straight into the kernels' argument structs on the
// handle (h->tick ...).  Host code only; gfx950 kernels are launched by the other translation units.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "wf_hip_internal.hpp"
#include "wf_geometry.hpp"

namespace wf::host {

thread_local std::string g_create_error;

int fail(wf_hip *h, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if(h)
        h->last_error = buf;
    else
        g_create_error = buf;
    return code;
}

int guard_block(wf_hip *h, void *p, size_t payload_bytes)
{
    hipError_t e = hipMemsetAsync(static_cast<char *>(p) + payload_bytes, GUARD_BYTE, GUARD_BYTES, h->stream);
    if(e != hipSuccess)
        return fail(h, WF_HIP_ERR_RUNTIME, "hipMemsetAsync of a guard failed: %s", hipGetErrorString(e));
    h->guards.emplace_back(p, payload_bytes);
    return WF_HIP_OK;
}

// the guard bytes of every live block, read back and compared (the caller has synchronised the handle's streams)
int check_canaries(wf_hip *h)
{
    if(!h->canary)
        return WF_HIP_OK;
    unsigned char buf[GUARD_BYTES];
    for(size_t i = 0; i < h->guards.size(); ++i) {
        const auto &g = h->guards[i];
        hipError_t e = hipMemcpy(buf, static_cast<char *>(g.first) + g.second, GUARD_BYTES, hipMemcpyDeviceToHost);
        if(e != hipSuccess)
            return fail(h, WF_HIP_ERR_RUNTIME, "reading a guard back failed: %s", hipGetErrorString(e));
        for(size_t b = 0; b < GUARD_BYTES; ++b)
            if(buf[b] != (unsigned char)GUARD_BYTE)
                return fail(h, WF_HIP_ERR_RUNTIME, "WF_HIP_CANARY: device block %zu of %zu (%zu payload bytes) was written %zu bytes past its end",
                            i, h->guards.size(), g.second, b + 1);
    }
    return WF_HIP_OK;
}

} // namespace wf::host

namespace {

using namespace wf::host;

// The development overrides of the plan, from the environment (development builds only; tests/lanes_child.py sets the one there is)
wf::PlanOverrides read_overrides()
{
    wf::PlanOverrides ov;
#ifdef WF_DEV_BUILD
    if(const char *e = std::getenv("WF_HIP_LANES"))
        ov.lanes = std::max(1, std::atoi(e));
#endif
    return ov;
}

// ---- validate and plan: everything that needs no device ------------------------------------------------------------------
int plan_handle(const wf_config *cfg_in, int device, uint32_t max_streams, uint32_t ring_frames, wf_hip **out)
{
    wf::HostTables tab;
    wf_config cfg = *cfg_in;
    uint32_t wave_samples = 0;
    wf::normalize_config(cfg);
    if(cfg.waveform)
        wave_samples = wf::waveform_config(cfg); // update()'s overrides; fft_size becomes the row length (width)
    else if(cfg.meter)
        wf::meter_config(cfg); // update()'s overrides for the mode; fft_size becomes the meter buffer length
    const int rc = wf::build_host_tables(cfg, tab);
    if(rc == WF_HIP_ERR_UNSUPPORTED && cfg.waveform)
        return fail(nullptr, rc, "waveform display: width %u above 8192 points is not implemented", cfg.width);
    if(rc == WF_HIP_ERR_UNSUPPORTED)
        return fail(nullptr, rc, "fft_size %u: implemented is every multiple of 16 from 128 to 65536 (the reference's own range)", cfg.fft_size);
    if(rc)
        return fail(nullptr, rc, "invalid configuration");
    const int ndev = wf_hip_device_count();
    if(ndev <= 0)
        return fail(nullptr, WF_HIP_ERR_NO_DEVICE, "no HIP device available");
    if(device < 0 || device >= ndev)
        return fail(nullptr, WF_HIP_ERR_INVALID, "device %d out of range (0..%d)", device, ndev - 1);

    wf_hip *h = new(std::nothrow) wf_hip();
    if(h == nullptr)
        return fail(nullptr, WF_HIP_ERR_NOMEM, "out of host memory");
    *out = h;
    h->cfg = cfg;
    h->tab = std::move(tab);
    h->interp_shape[0] = h->tab.interp_radius;
    h->interp_shape[1] = h->tab.interp_taps;
    h->device = device;
    if(const char *e = std::getenv("WF_HIP_CANARY")) // guard bytes behind every device block, checked by wf_hip_sync
        h->canary = e[0] == '1';
    h->n_streams = max_streams;
    h->N = cfg.fft_size;
    h->M = cfg.fft_size / 2;
    h->cap_ch = cfg.capture_channels;
    h->out_ch = h->tab.output_channels;
    h->disp_ch = h->tab.display_channels;
    h->num_bars = (uint32_t)h->tab.num_bars;
    h->ring_cap = next_pow2(ring_frames ? std::max(ring_frames, h->N) : std::max(2 * h->N, 4096u));
    h->plan = wf::plan_transform(cfg, wf::PlanOverrides{});
    h->tick.mr.passes = h->plan.passes;
    std::copy(h->plan.radix, h->plan.radix + 4, h->tick.mr.radix);
    h->wave = cfg.waveform != 0;
    h->meter = cfg.meter != 0;
    if(h->wave) {
        // rows of `width` points; the ring holds the history the points are picked from (+ the width zeros of update())
        h->M = h->N;
        h->ring_cap = next_pow2(std::max(ring_frames, 2 * (wave_samples + h->N)));
    }
    // Deep rings (a window of fft_size samples somewhere in a row of >= 256 KB) with a power-of-two row stride put every
    // stream's window at the same offset modulo the stride; 64 KB + 256 B of padding per row spreads them over the memory
    // channels: +2.5-4 % on the 1 MB rows of bench.py (60.0-60.3 -> 61.7-63.2 % of peak, three interleaved runs), nothing
    // to gain on shallow rings.
    h->ring_stride = h->ring_cap + (h->ring_cap >= 65536u ? 16448u : 0u);
    if(h->wave)
        fill_wave_args(h, wave_samples);
    return WF_HIP_OK;
}

// ---- open the device ---------------------------------------------------------------------------------------------------
int open_device(wf_hip *h, int *cu_count)
{
    WF_HIP_TRY(h, hipSetDevice(h->device));
    hipDeviceProp_t prop{};
    WF_HIP_TRY(h, hipGetDeviceProperties(&prop, h->device));
    if(std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(h, WF_HIP_ERR_NO_DEVICE, "device %d is %s; this library contains gfx950 code only", h->device, prop.gcnArchName);
    *cu_count = prop.multiProcessorCount;
    WF_HIP_TRY(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    WF_HIP_TRY(h, hipEventCreate(&h->ev0));
    WF_HIP_TRY(h, hipEventCreate(&h->ev1));
    return WF_HIP_OK;
}

// ---- allocate state ----------------------------------------------------------------------------------------------------
size_t spectra(const wf_hip *h) { return (size_t)h->n_streams * h->cap_ch; }

int finish_create(wf_hip *h)
{
    WF_TRY_RC(wf_hip_reset(h, 0, h->n_streams));
    WF_HIP_TRY(h, hipStreamSynchronize(h->stream));
    return WF_HIP_OK;
}

int create_waveform(wf_hip *h)
{
    WF_TRY_RC(dev_alloc(h, &h->d_cend, (size_t)h->n_streams));
    WF_TRY_RC(dev_alloc(h, &h->d_wts, (size_t)h->n_streams));
    WF_TRY_RC(dev_alloc(h, &h->d_decibels, (size_t)h->n_streams * h->out_ch * h->M));
    WF_TRY_RC(dev_alloc(h, &h->d_flags, (size_t)h->n_streams));
    h->kernel_name = "waveform_tick_kernel";
    return finish_create(h);
}

// level meter: rings, consumption points, two floats of state per channel, one bar per channel
int create_meter(wf_hip *h)
{
    WF_TRY_RC(dev_alloc(h, &h->d_mend, (size_t)h->n_streams));
    WF_TRY_RC(dev_alloc(h, &h->d_meter_buf, spectra(h)));
    WF_TRY_RC(dev_alloc(h, &h->d_meter_val, spectra(h)));
    WF_TRY_RC(dev_alloc(h, &h->d_flags, (size_t)h->n_streams));
    WF_TRY_RC(dev_alloc(h, &h->d_bars, spectra(h)));
    h->kernel_name = "meter_tick_kernel";
    fill_meter_args(h);
    return finish_create(h);
}

int alloc_spectrum_state(wf_hip *h)
{
    const wf_config *cfg = &h->cfg;
    WF_TRY_RC(dev_alloc(h, &h->d_tsmooth, spectra(h) * h->M));
    WF_TRY_RC(dev_alloc(h, &h->d_decibels, (size_t)h->n_streams * h->out_ch * h->M));
    h->flag_bufs = h->plan.want_split ? 3 : 1;
    WF_TRY_RC(dev_alloc(h, &h->d_flags, (size_t)h->flag_bufs * h->n_streams));
    if(h->plan.want_split)
        WF_TRY_RC(dev_alloc(h, &h->d_verdict, 3 * spectra(h)));
    if(h->num_bars)
        WF_TRY_RC(dev_alloc(h, &h->d_bars, (size_t)h->n_streams * h->disp_ch * h->num_bars));
    if(h->num_bars && cfg->mirror_freq_axis) // the value render_bars / render_curve see above the middle before the mirror (BarArgs::pre_out)
        WF_TRY_RC(dev_alloc(h, &h->d_bars_pre, (size_t)h->n_streams * h->disp_ch));
#ifdef WF_PHASE_TIMING
    WF_TRY_RC(dev_alloc(h, &h->tick.phase_clock, spectra(h) * 16));
#endif
    if(!cfg->vertices)
        return WF_HIP_OK;
    if(cfg->vertices > 3u || (cfg->vertices == 3u && (!cfg->bars || cfg->step_width < 1 || cfg->step_gap < 0)) || (cfg->vertices == 2u && cfg->bars) ||
       (!cfg->bars && !cfg->curve))
        return fail(h, WF_HIP_ERR_INVALID, "cfg.vertices: 1 needs bars or curve, 2 the curve, 3 bars with step_width >= 1 and step_gap >= 0");
    // a display narrower than one bar (m_num_bars == 0), or steps taller than the channel: the reference allocates no vertex
    // buffer ("Tried to allocate vbuf of size: 0", src/source.cpp:1044) and draws nothing -- wf_hip_num_vertices() == 0
    wf::VertexTables vtab;
    if(h->num_bars != 0)
        wf::build_vertex_tables(*cfg, (int)h->num_bars, vtab);
    if(h->num_bars != 0 && vtab.per_row > 0) {
        const size_t rows = (size_t)h->n_streams * h->disp_ch;
        float *d_cap_xy = nullptr;
        WF_TRY_RC(dev_alloc(h, &h->d_vert_counts, rows));
        WF_HIP_TRY(h, hipMemsetAsync(h->d_vert_counts, 0, rows * sizeof(uint32_t), h->stream));
        WF_TRY_RC(dev_alloc(h, &h->d_verts, rows * vtab.per_row));
        WF_HIP_TRY(h, hipMemsetAsync(h->d_verts, 0, rows * vtab.per_row * sizeof(wf::f4), h->stream));
        WF_TRY_RC(upload(h, &d_cap_xy, vtab.cap_xy));
        WF_HIP_TRY(h, hipStreamSynchronize(h->stream));
        fill_vertex_args(h, vtab, d_cap_xy);
    }
    return WF_HIP_OK;
}

// the kernel always multiplies by the window and slope tables; a disabled feature is a table of ones (x * 1.0f == x)
int upload_window_tables(wf_hip *h)
{
    const std::vector<float> ones_m(h->M, 1.0f);
    const float in_scale = h->plan.in_scale;
    std::vector<float> win_dev(h->N, in_scale);
    for(size_t i = 0; i < h->tab.window.size() && i < win_dev.size(); ++i)
        win_dev[i] = h->tab.window[i] * in_scale; // (exact)
    WF_TRY_RC(upload(h, &h->tick.window, win_dev));
    WF_TRY_RC(upload(h, &h->tick.slope, h->tab.slope.empty() ? ones_m : h->tab.slope));
    WF_HIP_TRY(h, hipStreamSynchronize(h->stream));
    return upload(h, &h->tick.rolloff, h->tab.rolloff);
}

// ---- the display tables ------------------------------------------------------------------------------------------------
// what a display plan has to fit its tables and staging into: the kernel that finishes the outputs, its threads, points per
// thread and registers, and the floats of the spectrum's exchange buffer
struct DisplayRoom {
    bool own_kernel; // the outputs come from the stored rows, by big_outputs_kernel
    size_t lds_floats;
    int threads, points, kmax;
};

// the display's scalars (BarArgs), from the configuration
void fill_bar_scalars(wf_hip *h)
{
    wf::BarArgs &b = h->tick.bar;
    b.gauss_radius = h->tab.gauss_radius;
    b.entries = (int)h->tab.bar_coef.size();
    b.num_bars = (int)h->num_bars;
    b.mirror = h->cfg.mirror_freq_axis ? 1 : 0;
    b.border_top = h->tab.border_top;
    b.border_bottom = h->tab.border_bottom;
    b.ceiling = (float)h->cfg.ceiling_db;
    b.dbrange = (float)(h->cfg.ceiling_db - h->cfg.floor_db);
    b.inv_dbrange = 1.0f / b.dbrange;
    b.lerp_mixed = ((b.border_top <= 0 && b.border_bottom >= 0) || (b.border_top >= 0 && b.border_bottom <= 0)) ? 1 : 0;
    b.disp_ch = h->disp_ch;
}

// one curve point per thread and step; the filter stages the row's points in the spectrum's LDS
int plan_curve(wf_hip *h, DisplayRoom &room)
{
    const wf_config *cfg = &h->cfg;
    wf::BarArgs &b = h->tick.bar;
    wf::CurveLaneTables cl;
    // mono mixdown with both channels of a stream in one workgroup: the one displayed row is finished by the threads
    // of both spectra (spectrum_tick_kernel, BarArgs::both_subs) -- the kernels that exist with BOTH: wf_tick_geom.hip, setup_launch
    const bool both = !cfg->stereo && cfg->capture_channels == 2 && !room.own_kernel && !h->plan.want_split && !h->plan.blu && h->N >= 1024u;
    b.both_subs = both ? 1 : 0;
    if(both)
        room.threads *= 2;
    if(!wf::curve_lanes(h->tab, *cfg, room.threads, room.kmax, cl))
        return fail(h, WF_HIP_ERR_INVALID, "curve display: no point table for width %u at fft_size %u", cfg->width, h->N);
    b.out_steps = cl.steps;
    b.curve = cl.x.empty() ? 1 : 2; // (Catmull-Rom: positions only, weights on the device)
    // wider than a thread's registers hold (always on the large-transform path, whose outputs have a kernel of their own): points are finished as they are produced
    b.stream_steps = (cl.steps > room.kmax || room.own_kernel) ? 1 : 0;
    WF_TRY_RC(upload(h, &b.cur_coef, cl.coef));
    WF_TRY_RC(upload(h, &b.cur_base, cl.base));
    WF_TRY_RC(upload(h, &b.cur_x, cl.x));
    WF_HIP_TRY(h, hipStreamSynchronize(h->stream)); // the staging vectors die here
    return WF_HIP_OK;
}

// bars finished inside the tick kernel: the first layout of prefix sums, wave-private pieces, segments that this display admits
// (none: the flat tables, chunk by chunk)
int plan_bar_layout(wf_hip *h, const DisplayRoom &room)
{
    wf::BarArgs &b = h->tick.bar;
    const int threads = room.threads, points = room.points;
    wf::BarLaneTables lanes;
    // wave-private pieces first (no barrier, DPP scan, last-arriver sum: wf_host_tables.hpp BarPieceTables); not with the
    // filter (its inputs are staged by bar index behind a barrier anyway) nor on the zero-padded sizes
    wf::BarPieceTables pieces;
    bool want_pieces = h->tab.gauss_radius == 0 && h->N >= 512u;
    if(h->plan.blu) // Bluestein proper keeps bar_segments' layouts (its instantiations are compiled without this one); the sizes
                    // that run as a mixed-radix transform take it
        want_pieces = want_pieces && h->plan.mr_in_lds();
#ifdef WF_DEV_BUILD
    if(const char *e = std::getenv("WF_HIP_BAR_PIECES"))
        want_pieces = want_pieces && e[0] != '0';
#endif
    // prefix-sum layout first (BarPsTables: float64 prefix sums of the row in registers, one lane per sub-band -- no
    // per-thread coefficient table at all); power-of-two sizes from 512 samples, no Gaussian filter
    wf::BarPsTables ps;
    bool want_ps = h->tab.gauss_radius == 0 && h->N >= 512u && !h->plan.blu;
#ifdef WF_DEV_BUILD
    if(const char *e = std::getenv("WF_HIP_BAR_PS"))
        want_ps = want_ps && e[0] != '0';
#endif
    if(want_ps && wf::bar_ps(h->tab, threads, ps) && wf::ps_lds_floats(h->M) <= room.lds_floats) {
        b.ps_lanes = ps.num_lanes;
        b.out_steps = 1;
        WF_TRY_RC(upload(h, &b.ps_tab, ps.tab));
        WF_HIP_TRY(h, hipStreamSynchronize(h->stream)); // the staging vector dies here
        want_pieces = false;
    }
    if(want_pieces && wf::bar_pieces(h->tab, threads, points, points / 4 + 2, pieces) && (size_t)h->M + (size_t)pieces.num_slots <= room.lds_floats) {
        b.piece_mode = 1; // (seg_group holds BarPieceTables::info, bar_seg its bar_piece)
        b.num_segs = pieces.num_segs;
        b.lane_blocks = pieces.blocks;
        b.out_steps = 1;
        WF_TRY_RC(upload(h, &b.lane_coef, pieces.coef));
        WF_TRY_RC(upload(h, &b.lane_base, pieces.base));
        WF_TRY_RC(upload(h, &b.seg_group, pieces.info));
        WF_TRY_RC(upload(h, &b.bar_seg, pieces.bar_piece));
        WF_HIP_TRY(h, hipStreamSynchronize(h->stream)); // the staging vectors die here
    }
    // (wave-local layout: no workgroup barrier inside the reduction; not with the filter, whose inputs are staged by
    // bar index behind a barrier anyway)
    const bool local = h->tab.gauss_radius == 0;
    if(!b.piece_mode && b.ps_lanes == 0 && wf::bar_segments(h->tab, threads, points / 4 + 2, lanes, local)) {
        b.wave_local = lanes.wave_local ? 1 : 0;
        b.num_segs = lanes.num_segs;
        b.lane_blocks = lanes.blocks;
        b.out_steps = 1;
        WF_TRY_RC(upload(h, &b.lane_coef, lanes.coef));
        WF_TRY_RC(upload(h, &b.lane_base, lanes.base));
        WF_TRY_RC(upload(h, &b.bar_seg, lanes.bar_seg));
        WF_TRY_RC(upload(h, &b.seg_group, lanes.seg_group));
        WF_TRY_RC(upload(h, &b.lead_bar, lanes.lead_bar));
        WF_TRY_RC(upload(h, &b.lead_end, lanes.lead_end));
        WF_HIP_TRY(h, hipStreamSynchronize(h->stream)); // the staging vectors die here
    }
    return WF_HIP_OK;
}

// big_outputs_kernel: the whole row in LDS, two guard zeros, then the filter's staging
int plan_own_kernel_display(wf_hip *h)
{
    wf::BarArgs &b = h->tick.bar;
    const size_t staged = h->tab.gauss_radius > 0 ? (size_t)h->num_bars + 2 * (size_t)(h->tab.gauss_radius - 1) + h->tab.gauss.size() : 0;
    // (bars read their bins from the row in device memory: only the staging lives in LDS; a curve parks the row first)
    const size_t parked = b.curve ? (size_t)h->M + 2 : 0;
    b.stage_off = (int)parked;
    // bars: the entries in tasks of at most 2048 (a multiple of 64), one wavefront each; their sums meet in LDS
    b.big_num_tasks = 0;
    if(!b.curve && !h->tab.bar_off.empty()) {
        std::vector<int> task, bar_task(h->tab.bar_off.size(), 0);
        const int cap = 2048;
        for(size_t bq = 0; bq + 1 < h->tab.bar_off.size(); ++bq) {
            bar_task[bq] = (int)(task.size() / 4);
            const int e0 = h->tab.bar_off[bq], e1 = h->tab.bar_off[bq + 1];
            const int parts = std::max(1, (e1 - e0 + cap - 1) / cap);
            const int per = (((e1 - e0 + parts - 1) / parts) + 63) & ~63;
            for(int q = 0; q < parts; ++q) {
                const int lo = std::min(e0 + q * per, e1), hi = std::min(lo + per, e1);
                if(q == 0 || lo < hi) {
                    // a task whose entries walk consecutive bins (every bar of an interpolated display does: a band and its
                    // taps) says where it starts: the kernel then forms the bins' addresses instead of loading them first
                    bool run = lo < hi;
                    for(int e = lo + 1; e < hi && run; ++e)
                        run = h->tab.bar_bin[(size_t)e] == h->tab.bar_bin[(size_t)lo] + (e - lo);
                    task.push_back((int)bq);
                    task.push_back(lo);
                    task.push_back(hi);
                    task.push_back(run ? h->tab.bar_bin[(size_t)lo] : -1);
                }
            }
        }
        bar_task.back() = (int)(task.size() / 4);
        b.big_num_tasks = (int)(task.size() / 4);
        WF_TRY_RC(upload(h, &b.big_task, task));
        WF_TRY_RC(upload(h, &b.big_bar_task, bar_task));
        WF_HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    h->disp.big_out_lds = std::max<size_t>(((parked + staged + (size_t)b.big_num_tasks) * sizeof(float) + 15) & ~(size_t)15, 16);
    if(h->disp.big_out_lds > 160u * 1024u)
        return fail(h, WF_HIP_ERR_UNSUPPORTED, "fft_size %u with filter_mode gauss over %u outputs: row + staging exceed a CU's LDS", h->N, h->num_bars);
    return WF_HIP_OK;
}

int longest_bar(const wf_hip *h)
{
    int longest = 0;
    for(uint32_t q = 0; q < h->num_bars; ++q)
        longest = std::max(longest, h->tab.bar_off[(size_t)q + 1] - h->tab.bar_off[(size_t)q]);
    return longest;
}

// the Gaussian filter inside the tick kernel, staged in the spectrum's LDS: the row with radius-1 zeros on either side, then the
// weights.  *chunk_cap: the product scratch of the chunked form, which shrinks by the staging
int plan_filter_staging(wf_hip *h, const DisplayRoom &room, size_t *chunk_cap)
{
    wf::BarArgs &b = h->tick.bar;
    const size_t lds_floats = room.lds_floats;
    const size_t staged = (size_t)h->num_bars + 2 * (size_t)(h->tab.gauss_radius - 1) + h->tab.gauss.size();
    if(b.stream_steps) {
        // wide curve: the points are staged behind the dB row (and the two guard zeros of the Catmull-Rom taps)
        if(h->M + 2 + staged > lds_floats)
            return fail(h, WF_HIP_ERR_UNSUPPORTED,
                        "filter_mode gauss: %u curve points + the filter's staging do not fit behind the row in this configuration's on-chip buffer (%zu floats)",
                        h->num_bars, lds_floats);
        b.stage_off = (int)h->M + 2;
    } else if(b.out_steps == 0) {
        // bars in chunked form (more bars than threads): the staging area sits at the end of the buffer, the product
        // scratch shrinks by it and must still hold the longest bar
        if(staged + (size_t)longest_bar(h) + h->M > lds_floats)
            return fail(h, WF_HIP_ERR_UNSUPPORTED, "filter_mode gauss: %u bars + the filter's staging do not fit this configuration's on-chip buffer (%zu floats)",
                        h->num_bars, lds_floats);
        *chunk_cap -= staged;
        b.stage_off = (int)(lds_floats - staged);
    } else if(staged > lds_floats)
        return fail(h, WF_HIP_ERR_UNSUPPORTED, "filter_mode gauss: %u outputs per row do not fit this configuration's on-chip staging (%zu floats)", h->num_bars,
                    lds_floats);
    return WF_HIP_OK;
}

// One display plan.  ext == false: the outputs are finished inside the tick kernel, from the dB row parked in the
// spectrum's exchange buffer (or, beyond a CU's LDS, by big_outputs_kernel).  Where the row's points + the Gaussian
// filter's staging do not fit that buffer -- wide filtered curves and many narrow filtered bars at small fft sizes: the
// reference allows width <= 3840 and radius <= 32 at every size (src/source.cpp:287, :409) -- the plan is made again with
// ext == true: the tick kernel stores its rows and big_outputs_kernel (one workgroup per displayed row, up to 160 KB of
// LDS) derives the outputs from them through L2, as it does for the transforms beyond a CU's LDS.
int plan_outputs(wf_hip *h, bool ext)
{
    const wf_config *cfg = &h->cfg;
    wf::BarArgs &b = h->tick.bar;
    fill_bar_scalars(h);
    WF_TRY_RC(upload(h, &b.coef, h->tab.bar_coef));
    WF_TRY_RC(upload(h, &b.bin, h->tab.bar_bin));
    WF_TRY_RC(upload(h, &b.off, h->tab.bar_off));
    WF_TRY_RC(upload(h, &b.count, h->tab.band_widths));
    DisplayRoom room{h->plan.big_l != 0 || ext, 0, 64, 16, 0};
    wf::dispatch_geometry(ext ? 32768u : h->plan.geom_n, [&](auto g) {
        using G = decltype(g);
        room.lds_floats = (size_t)G::LDS_CF * 2; // LDS scratch for the products: what is left of a spectrum's exchange buffer behind the M dB values
        room.threads = G::T;
        room.points = G::P;
    });
    // the kernels that run on wf::GBig's 1024 threads of 16 points whatever the power-of-two kernel of that size does:
    // big_outputs_kernel, and the Bluestein / mixed-radix instantiations of the largest container (setup_launch_blu)
    if(room.own_kernel || (h->plan.blu && h->plan.geom_n == 32768u)) {
        room.lds_floats = (size_t)wf::GBig::LDS_CF * 2;
        room.threads = wf::GBig::T;
        room.points = wf::GBig::P;
    }
    if(!room.own_kernel && h->plan.mr_in_lds()) // the exchange buffer is sized by the transform there (MrPlan::lds_cf, setup_launch_blu)
        room.lds_floats = 2u * (size_t)wf::mr_exchange_cf(h->N / 2, (uint32_t)(room.lds_floats / 2));
    int lpb = 1;
    while(lpb < 64 && (uint32_t)(room.threads / (lpb * 2)) >= h->num_bars)
        lpb *= 2;
    b.lanes_per_bar = lpb;
    room.kmax = room.threads <= 64 ? 16 : 8; // wf::OutVals<G>::KMAX
    if(!cfg->bars && cfg->curve)
        WF_TRY_RC(plan_curve(h, room));
    else if(!room.own_kernel) // (big_outputs_kernel reduces its bars from the flat tables, one wavefront per bar)
        WF_TRY_RC(plan_bar_layout(h, room));
    size_t chunk_cap = room.lds_floats > h->M ? room.lds_floats - h->M : 0; // LDS scratch for the products: what is left behind the dB row
    if(room.own_kernel)
        WF_TRY_RC(plan_own_kernel_display(h));
    else if(h->tab.gauss_radius > 0)
        WF_TRY_RC(plan_filter_staging(h, room, &chunk_cap));
    if(h->tab.gauss_radius > 0) {
        WF_TRY_RC(upload(h, &b.gauss, h->tab.gauss));
        WF_TRY_RC(upload(h, &b.gauss_wsum, h->tab.gauss_wsum));
        WF_HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if(b.num_segs == 0 && b.ps_lanes == 0 && !b.curve && !room.own_kernel && (size_t)longest_bar(h) > chunk_cap) // chunked form: a chunk holds at least one whole bar
        return fail(h, WF_HIP_ERR_UNSUPPORTED, "bars: the widest band (%d bins and taps) does not fit the on-chip scratch (%zu floats)", longest_bar(h), chunk_cap);
    const std::vector<int> chunks = wf::bar_chunks(h->tab, chunk_cap);
    WF_TRY_RC(upload(h, &b.chunk, chunks));
    WF_HIP_TRY(h, hipStreamSynchronize(h->stream));
    b.num_chunks = (int)chunks.size() - 1;
    return WF_HIP_OK;
}

int plan_display(wf_hip *h)
{
    if(!h->num_bars)
        return WF_HIP_OK;
    const size_t mark = h->allocs.size();
    int orc = plan_outputs(h, false);
    if(orc == WF_HIP_ERR_UNSUPPORTED && h->plan.big_l == 0) {
        // give back what the first plan uploaded, forget what it decided, plan again for big_outputs_kernel
        WF_HIP_TRY(h, hipStreamSynchronize(h->stream));
        while(h->allocs.size() > mark) {
            void *gone = h->allocs.back();
            h->guards.erase(std::remove_if(h->guards.begin(), h->guards.end(), [gone](const auto &g) { return g.first == gone; }), h->guards.end());
            (void)hipFree(gone);
            h->allocs.pop_back();
        }
        h->tick.bar = wf::BarArgs{};
        h->disp = wf_hip::DisplayPlan{};
        h->disp.ext_outputs = true;
        orc = plan_outputs(h, true);
    }
    WF_TRY_RC(orc);
    if(h->disp.ext_outputs && h->disp.big_out_lds)
        WF_TRY_RC(big_outputs_set_lds(h));
    return WF_HIP_OK;
}

// ---- the FFT tables, one function per family ------------------------------------------------------------------------------
// the twiddle tables of the geometry that runs the batch + the kernel instantiation
int setup_geometry(wf_hip *h)
{
    int setup_rc = WF_HIP_ERR_UNSUPPORTED;
    std::vector<wf::cfloat> tw1, tw2, tws;
    wf::dispatch_geometry(h->plan.geom_n, [&](auto g) {
        using G = decltype(g);
        wf::build_twiddles(G::M, G::R1, G::R2, G::R3, tw1, tw2, tws);
        h->waves_per_spectrum = G::T / 64;
        // transforms beyond a CU's LDS (wf_big_dispatch.hip), else the fused kernel of this geometry (wf_tick_geom.hip: one object per geometry)
        if(h->plan.big_l) {
            if constexpr(G::N == 32768)
                setup_rc = setup_launch_big(h);
        } else if constexpr(G::N == 512)
            setup_rc = setup_tick_512(h);
        else if constexpr(G::N == 1024)
            setup_rc = setup_tick_1024(h);
        else if constexpr(G::N == 2048)
            setup_rc = setup_tick_2048(h);
        else if constexpr(G::N == 4096)
            setup_rc = setup_tick_4096(h);
        else if constexpr(G::N == 8192)
            setup_rc = setup_tick_8192(h);
        else if constexpr(G::N == 16384)
            setup_rc = setup_tick_16384(h);
        else
            setup_rc = setup_tick_32768(h);
    });
    WF_TRY_RC(setup_rc);
    if(h->tick.mr.passes > 0 && h->tick.mr.radix[0] > 25) {
        // a mixed-radix plan that opens with a prime pass (wf::mr_pass_prime): its W_p^m goes where the power-of-two kernels keep
        // their pass-2 twiddles -- the tick kernel stages that table in LDS anyway and the mixed-radix passes do not use it
        wf::build_prime_twiddles(h->tick.mr.radix[0], tw2.size(), tw2);
        WF_TRY_RC(upload(h, &h->tick.mr.wp, tw2)); // (the large-FFT rows kernel reads it from device memory)
    }
    WF_TRY_RC(upload(h, &h->tick.tw1, tw1));
    WF_TRY_RC(upload(h, &h->tick.tw2, tw2));
    WF_TRY_RC(upload(h, &h->tick.tws, tws));
    WF_HIP_TRY(h, hipStreamSynchronize(h->stream)); // the staging vectors die here
    return WF_HIP_OK;
}

// mixed radix inside LDS: the window table the power-of-two kernels use (it is uploaded for every handle), W_(N/2)^m for the
// passes and W_N^k for the real split; none of Bluestein's chirp tables
int upload_mixed_radix_tables(wf_hip *h)
{
    std::vector<wf::cfloat> tw, w;
    wf::build_mixed_radix_tables(h->N, h->tick.mr.passes, h->tick.mr.radix, tw, h->tick.mr.tw_off, w);
    WF_TRY_RC(upload(h, &h->tick.mr.tw, tw));
    WF_TRY_RC(upload(h, &h->tick.blu_w, w));
    WF_HIP_TRY(h, hipStreamSynchronize(h->stream));
    return WF_HIP_OK;
}

int upload_bluestein_tables(wf_hip *h)
{
    wf::BluesteinTables bt;
    wf::build_bluestein(h->cfg, h->tab, bt);
    for(auto &v : bt.a) { // the window sits in this table on the Bluestein paths (in_scale)
        v.re *= h->plan.in_scale;
        v.im *= h->plan.in_scale;
    }
    WF_TRY_RC(upload(h, &h->tick.blu_a, bt.a));
    WF_TRY_RC(upload(h, &h->tick.blu_b, bt.b));
    WF_TRY_RC(upload(h, &h->tick.blu_q, bt.q));
    WF_TRY_RC(upload(h, &h->tick.blu_qr, bt.qr));
    WF_TRY_RC(upload(h, &h->tick.blu_w, bt.w));
    WF_HIP_TRY(h, hipStreamSynchronize(h->stream));
    return WF_HIP_OK;
}

// mixed-radix rows: the rows' passes (a transform of R = n / 2 / C points) and the column step's W_C^(c k1)
int upload_mr_rows_tables(wf_hip *h)
{
    wf::TickArgs &a = h->tick;
    const uint32_t rows = h->plan.big_rows;
    std::vector<wf::cfloat> tw, unused;
    wf::build_mixed_radix_tables(2u * (h->M / rows), a.mr.passes, a.mr.radix, tw, a.mr.tw_off, unused);
    std::vector<wf::cf> wc(64, wf::cf{1.0f, 0.0f});
    const double two_pi = 6.283185307179586476925286766559;
    for(uint32_t k1 = 0; k1 < rows; ++k1)
        for(uint32_t c = 0; c < rows; ++c) {
            const double ang = -two_pi * (double)((c * k1) % rows) / (double)rows;
            wc[k1 * 8u + c] = wf::cf{(float)std::cos(ang), (float)std::sin(ang)};
        }
    WF_TRY_RC(upload(h, &a.mr.tw, tw));
    WF_TRY_RC(upload(h, &a.big_wc, wc));
    WF_HIP_TRY(h, hipStreamSynchronize(h->stream));
    a.mr.half = (int)wf::GBig::M / 2; // (the rows kernel's two halves of the 132 KB buffer; its Z goes to device memory)
    a.mr.s3 = h->plan.big_mrw() ? a.mr.half / 4 + 4 : 0; // (big_mr_whole_kernel leaves a row's Z in the buffer: mr_z_addr's four planes)
    a.mr.lds_cf = 0;
    a.big_c = rows;
    a.big_r = h->M / rows;
    return WF_HIP_OK;
}

// Bluestein rows inside LDS: the container geometry's twiddles in place of the batch geometry's, FFT(chirp), the closing chirp (the
// column step is a radix-C butterfly in registers); *rowtw, the table of column twiddle x opening chirp, goes where the other
// paths keep their column twiddles (upload_big_tables)
int upload_bluestein_rows_tables(wf_hip *h, std::vector<wf::cfloat> *rowtw)
{
    wf::TickArgs &a = h->tick;
    std::vector<wf::cfloat> bhat, q, tw1, tw2, unused;
    if(wf::build_bluestein_rows(h->plan.big_l, h->plan.big_rows, *rowtw, bhat, q) != h->plan.br_l)
        return fail(h, WF_HIP_ERR_RUNTIME, "Bluestein rows: container length");
    wf::dispatch_geometry(2u * h->plan.br_l, [&](auto g) {
        using G = decltype(g);
        wf::build_twiddles(G::M, G::R1, G::R2, G::R3, tw1, tw2, unused);
    });
    WF_TRY_RC(upload(h, &a.tw1, tw1));
    WF_TRY_RC(upload(h, &a.tw2, tw2));
    WF_TRY_RC(upload(h, &a.blu_b, bhat));
    WF_TRY_RC(upload(h, &a.blu_q, q));
    WF_HIP_TRY(h, hipStreamSynchronize(h->stream));
    a.big_c = h->plan.big_rows;
    a.big_r = h->M / h->plan.big_rows;
    return WF_HIP_OK;
}

// every transform beyond a CU's LDS: the column twiddles, the real-split twiddles, the scratch in device memory
int upload_big_tables(wf_hip *h, const std::vector<wf::cfloat> &br_rowtw)
{
    wf::TickArgs &a = h->tick;
    const wf::TransformPlan &t = h->plan;
    std::vector<wf::cfloat> twb, twsb;
    wf::build_big_twiddles(t.big_l, t.big_rows, h->N, twb, twsb);
    WF_TRY_RC(upload(h, &a.big_tw, t.big_br() ? br_rowtw : twb));
    WF_TRY_RC(upload(h, &a.big_tws, twsb));
    WF_HIP_TRY(h, hipStreamSynchronize(h->stream));
    wf::cf *z = nullptr;
    if(t.big_whole() || t.big_mrw()) { // (fft_size 65536 and the two-row mixed-radix sizes: no scratch at all, the magnitudes stay in registers)
    } else if(t.big_br()) { // (columns -> rows in place -> epilogue)
        WF_TRY_RC(dev_alloc(h, &z, spectra(h) * t.big_rows * t.br_rs));
    } else { // (mixed-radix rows: they read the ring themselves: one scratch buffer, for Z)
        WF_TRY_RC(dev_alloc(h, &z, spectra(h) * t.big_l));
    }
    a.big_z = z;
    WF_TRY_RC(dev_alloc(h, &a.big_nz_out, spectra(h)));
    a.big_nz = a.big_nz_out;
    a.big_m = h->N / 2;
    a.big_l = t.big_br() ? t.big_rows * t.br_rs : t.big_l;
    a.big_rs = t.br_rs;
    return WF_HIP_OK;
}

int upload_fft_tables(wf_hip *h)
{
    const wf::TransformPlan &t = h->plan;
    WF_TRY_RC(setup_geometry(h));
    if(t.mr_in_lds())
        WF_TRY_RC(upload_mixed_radix_tables(h));
    else if(t.blu)
        WF_TRY_RC(upload_bluestein_tables(h));
    std::vector<wf::cfloat> br_rowtw;
    if(t.big_mr())
        WF_TRY_RC(upload_mr_rows_tables(h));
    if(t.big_br())
        WF_TRY_RC(upload_bluestein_rows_tables(h, &br_rowtw));
    if(t.big_l)
        WF_TRY_RC(upload_big_tables(h, br_rowtw));
    return WF_HIP_OK;
}

// ---- the lanes ---------------------------------------------------------------------------------------------------------
int open_lanes(wf_hip *h, int cu_count)
{
    int lanes = wf::plan_lanes(h->plan, h->n_streams, h->cap_ch, h->num_bars, h->wg_lds, h->wg_threads, cu_count, read_overrides());
#ifdef WF_PHASE_TIMING
    lanes = 1;
#endif
    for(int l = 1; l < lanes; ++l) {
        WF_HIP_TRY(h, hipStreamCreateWithFlags(&h->lane_stream[l], hipStreamNonBlocking));
        WF_HIP_TRY(h, hipEventCreateWithFlags(&h->ev_lane[l], hipEventDisableTiming));
    }
    if(lanes > 1)
        WF_HIP_TRY(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    h->n_lanes = lanes;
    return WF_HIP_OK;
}

// ---- the constant arguments that no earlier stage decided ------------------------------------------------------------------
void fill_tick_constants(wf_hip *h)
{
    wf::TickArgs &a = h->tick;
    const wf::TransformPlan &t = h->plan;
    a.ring_cap = h->ring_cap;
    a.ring_stride = h->ring_stride;
    a.ring_mask = h->ring_cap - 1;
    a.split_ch = 0xffffffffu;
    a.half_coef = 0.5f * (2.0f / h->tab.window_sum); // mag_coefficient (reference src/source_generic.cpp:110), halved: the
                                                     // kernel produces 2X[k] from the real split
    a.half_coef *= 1.0f / t.in_scale; // the window tables on the device carry in_scale
    a.slope_step = h->tab.slope.empty() ? 0.0f : (float)(3.0 * (double)h->cfg.slope / (double)(h->M - 1));
    a.row_bins = h->M;
    if(t.blu || t.big_l)
        a.blu_n = h->N; // (beyond a CU's LDS: the window length the underflow test compares with)
    a.db_min = wf::db_min();
    a.silent_floor = (float)(h->cfg.floor_db - 10);
    a.n_streams = h->n_streams;
    a.stream_count = h->n_streams;
    a.cap_ch = h->cap_ch;
    a.out_ch = h->out_ch;
    uint32_t mode = 0;
    if(h->cfg.tsmoothing != WF_TSMOOTH_NONE) mode |= wf::WF_MODE_TSMOOTH;
    if(h->cfg.fast_peaks) mode |= wf::WF_MODE_FAST_PEAKS;
    if(h->cfg.stereo) mode |= wf::WF_MODE_STEREO;
    if(!h->tab.slope.empty()) mode |= wf::WF_MODE_SLOPE;
    if(a.rolloff) mode |= wf::WF_MODE_ROLLOFF;
    if(!h->tab.window.empty()) mode |= wf::WF_MODE_WINDOW;
    if(!h->cfg.stereo && h->cap_ch > 1) mode |= wf::WF_MODE_MONO_MIX;
    if(h->cfg.normalize_volume) mode |= wf::WF_MODE_NORMALIZE;
    a.mode = mode;
}

// the stages of wf_hip_create behind the plan, in order
int build_handle(wf_hip *h)
{
    int cu_count = 0;
    WF_TRY_RC(open_device(h, &cu_count));
    WF_TRY_RC(dev_alloc(h, &h->d_ring, spectra(h) * h->ring_stride));
    WF_TRY_RC(dev_alloc(h, &h->d_wpos, (size_t)h->n_streams));
    if(h->wave)
        return create_waveform(h);
    if(h->meter)
        return create_meter(h);
    WF_TRY_RC(alloc_spectrum_state(h));
    WF_TRY_RC(upload_window_tables(h));
    WF_TRY_RC(plan_display(h));
    WF_TRY_RC(upload_fft_tables(h));
    WF_TRY_RC(open_lanes(h, cu_count));
    fill_tick_constants(h);
    return finish_create(h);
}

} // namespace

extern "C" {

int wf_hip_create(const wf_config *cfg, int device, uint32_t max_streams, uint32_t ring_frames, wf_hip **out)
{
    if(out == nullptr)
        return WF_HIP_ERR_INVALID;
    *out = nullptr;
    if(cfg == nullptr || max_streams == 0)
        return fail(nullptr, WF_HIP_ERR_INVALID, "cfg is NULL or max_streams is 0");
    wf_hip *h = nullptr;
    WF_TRY_RC(plan_handle(cfg, device, max_streams, ring_frames, &h));
    const int rc = build_handle(h);
    if(rc != WF_HIP_OK) {
        g_create_error = h->last_error;
        wf_hip_destroy(h);
        return rc;
    }
    *out = h;
    return WF_HIP_OK;
}

void wf_hip_destroy(wf_hip *h)
{
    if(h == nullptr)
        return;
    (void)hipSetDevice(h->device);
    for(int l = 1; l < wf_hip::MAX_LANES; ++l)
        if(h->lane_stream[l])
            (void)hipStreamSynchronize(h->lane_stream[l]);
    if(h->stream)
        (void)hipStreamSynchronize(h->stream);
    for(int l = 1; l < wf_hip::MAX_LANES; ++l) {
        if(h->ev_lane[l]) (void)hipEventDestroy(h->ev_lane[l]);
        if(h->lane_stream[l]) (void)hipStreamDestroy(h->lane_stream[l]);
    }
    if(h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    for(void *p : h->allocs)
        (void)hipFree(p);
    if(h->copy_stream)
        (void)hipStreamSynchronize(h->copy_stream);
    for(int i = 0; i < 2; ++i) {
        if(h->ev_copied[i]) (void)hipEventDestroy(h->ev_copied[i]);
        for(wf_hip::IngestSlot *s : {&h->ingest_slot[i], &h->sq_slot[i]}) { // (their device blocks went with h->allocs)
            if(s->ev_consumed) (void)hipEventDestroy(s->ev_consumed);
            if(s->h_frames) (void)hipHostFree(s->h_frames);
        }
    }
    if(h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
    if(h->read_stream)
        (void)hipStreamSynchronize(h->read_stream);
    for(wf_hip::ReadSlot &s : h->read_slot) { // (their device blocks went with h->allocs)
        if(s.ev_snap) (void)hipEventDestroy(s.ev_snap);
        if(s.ev_read) (void)hipEventDestroy(s.ev_read);
    }
    if(h->read_stream) (void)hipStreamDestroy(h->read_stream);
    for(auto e : h->ev_bars_lane)
        if(e) (void)hipEventDestroy(e);
    for(int i = 0; i < 2; ++i) {
        if(h->ev_words[i]) (void)hipEventDestroy(h->ev_words[i]);
        if(h->h_words[i]) (void)hipHostFree(h->h_words[i]);
    }
    if(h->ev0) (void)hipEventDestroy(h->ev0);
    if(h->ev1) (void)hipEventDestroy(h->ev1);
    if(h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

} // extern "C"
