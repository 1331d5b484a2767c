// wf_hip.hip -- the entry points of the C ABI in include/wf_hip.h other than create / destroy (wf_hip_plan.hip) and the
// measurement outputs (wf_hip_measure.hip): audio ingest, the tick, per-stream settings, readbacks, timing -- host side + the
// launches of the small kernels (rings, level meter, waveform display, RMS, vertex fill).  The fused spectrum kernel is launched through wf_hip::launch
// with the arguments of tick_args(): the handle's constant wf_hip::tick + the per-tick part
// (wf_tick_geom.hip, wf_big_dispatch.hip).  The two pipelines that run beside the compute stream -- the ingest from page-locked
// memory and wf_hip_read_async -- each keep their per-slot state in one record (wf_hip::IngestSlot, wf_hip::ReadSlot) and have a
// section here that states the slots' ordering rule once, with the helpers every path goes through ("pipelined ingest",
// "pipelined readback").  gfx950 only.  There is no CPU fallback: every entry point either drives the device or fails.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "wf_hip_internal.hpp"
#include "wf_geometry.hpp"
#include "wf_ring.hpp"
#include "wf_pcm.hpp"
#include "wf_wire.hpp"
#include "wf_meter.hpp"
#include "wf_rms.hpp"
#include "wf_wave.hpp"
#include "wf_vertex.hpp"

// the small kernels' argument structs of a handle (wf_hip::small); this unit alone includes the headers that define them
struct wf::host::SmallArgs {
    wf::MeterArgs meter{};   // level-meter batches
    wf::WaveArgs wave{};     // waveform batches
    wf::VertexArgs vertex{}; // cfg.vertices; per_row == 0: no vertex fill
    wf::RmsArgs rms{};       // wf_hip_enable_input_rms
};

namespace wf::host {

static SmallArgs &small_args(wf_hip *h)
{
    if(!h->small)
        h->small = std::make_shared<SmallArgs>();
    return *h->small;
}

void fill_meter_args(wf_hip *h)
{
    wf::MeterArgs &m = small_args(h).meter;
    m.ring_cap = h->ring_cap;
    m.ring_stride = h->ring_stride;
    m.ring_mask = h->ring_cap - 1;
    m.size = h->N;
    m.db_min = wf::db_min();
    m.silent_floor = (float)(h->cfg.floor_db - 10);
    m.border_top = h->tab.border_top;
    m.border_bottom = h->tab.border_bottom;
    m.ceiling = (float)h->cfg.ceiling_db;
    m.dbrange = (float)(h->cfg.ceiling_db - h->cfg.floor_db);
    m.n_streams = h->n_streams;
    m.cap_ch = h->cap_ch;
    m.rms = h->cfg.meter_rms ? 1u : 0u;
    m.tsmooth = (h->cfg.tsmoothing != WF_TSMOOTH_NONE) ? 1u : 0u;
    m.fast_peaks = h->cfg.fast_peaks ? 1u : 0u;
}

void fill_wave_args(wf_hip *h, uint32_t wave_samples)
{
    wf::WaveArgs &w = small_args(h).wave;
    w.ring_mask = h->ring_cap - 1;
    w.ring_stride = h->ring_stride;
    w.step_ns = ((unsigned long long)h->cfg.meter_ms * 1000000ull) / h->N; // src/source_generic.cpp:299
    w.waveform_samples = wave_samples; // m_waveform_samples
    w.width = h->N;
    w.sample_rate = h->cfg.sample_rate;
    w.n_streams = h->n_streams;
    w.cap_ch = h->cap_ch;
    w.out_ch = h->out_ch;
    w.stereo = h->cfg.stereo ? 1u : 0u;
    w.normalize = h->cfg.normalize_volume ? 1u : 0u;
    w.db_min = wf::db_min();
}

void fill_vertex_args(wf_hip *h, const wf::VertexTables &vt, const float *d_cap_xy)
{
    wf::VertexArgs &v = small_args(h).vertex;
    v.cap_xy = d_cap_xy;
    v.disp_ch = h->disp_ch;
    v.num_bars = (int)h->num_bars;
    v.per_row = vt.per_row;
    v.per_bar = vt.per_bar;
    v.mode = vt.mode;
    v.bar_stride = vt.bar_stride;
    v.bar_width = h->cfg.bar_width;
    v.cpos = vt.cpos;
    v.bottom = vt.bottom;
    v.channel_offset = vt.channel_offset;
    v.cap_radius = vt.cap_radius;
    v.rounded = h->cfg.rounded_caps ? 1 : 0;
    v.cap_tris = vt.cap_tris;
    v.bottom_caps = vt.bottom_caps;
    v.radial = vt.radial;
    v.bot_offset = vt.bot_offset;
    v.step_width = h->cfg.step_width;
    v.step_stride = vt.step_stride;
    v.max_steps = vt.max_steps;
}

} // namespace wf::host

namespace {

using namespace wf::host;

// volume_compensation, reference src/source_generic.cpp:163 (:381 for the waveform) with dbfs() of src/source.hpp:293-299
float volume_compensation(const wf_hip *h, float rms)
{
    const float rms_db = (rms > 0.0f) ? 20.0f * std::log10(rms) : wf::db_min();
    return std::min(h->cfg.volume_target - rms_db, h->cfg.max_gain);
}

// The arguments of one tick: the handle's constant part (h->tick, written by wf_hip_create where each value is decided) + what
// can change between ticks -- the tick's own parameters, the state other entry points own, the flag rotation, the mirrors.
// stream_base / stream_count are the whole batch here; wf_hip_tick narrows them per lane.
wf::TickArgs tick_args(const wf_hip *h, const wf_hip_tick_params *p)
{
    wf::TickArgs a = h->tick;
    a.ring = h->d_ring;
    a.wpos = h->d_wpos;
    a.tsmooth = h->d_tsmooth;
    a.decibels = h->d_decibels;
    a.delay = p->delay_frames;
    a.delay_stream = h->d_delay;
    a.stream_flags = cur_flags(h);
    if(h->split) {
        const uint32_t nxt = (h->flag_cur + 1) % 3, clr = (h->flag_cur + 2) % 3;
        const size_t n_spec = (size_t)h->n_streams * h->cap_ch;
        a.flags_out = h->d_flags + (size_t)nxt * h->n_streams;
        a.verdict_in = h->d_verdict + (size_t)h->flag_cur * n_spec;
        a.verdict_out = h->d_verdict + (size_t)nxt * n_spec;
        a.verdict_clear = h->d_verdict + (size_t)clr * n_spec;
    }
    // mono mixdown keeps storing its row: the silence quirk adds the stale row to the partner's magnitudes (wf_kernels.hpp)
    const bool mono_mix_rows = !h->cfg.stereo && h->cap_ch > 1;
    a.skip_decibels = ((p->flags & WF_HIP_TICK_NO_DECIBELS) && !mono_mix_rows) ? 1u : 0u;
    a.bars_only = h->d_bars_only;
    a.stale_row = h->d_stale_row;
    if(h->d_bars) {
        a.bar.out = h->d_bars;
        a.bar.pre_out = h->d_bars_pre;
        a.bar.out2_n = (int)h->mirror_n;
        for(uint32_t j = 0; j < h->mirror_n; ++j)
            a.bar.out2_delta[j] = (long long)(h->bars_mirror[h->mirror_next][j] - h->d_bars);
    }
    a.g = wf::gravity_for(h->cfg, p->seconds);
    a.g2 = 1.0f - a.g;
    if(h->cfg.normalize_volume) {
        a.vol_comp = volume_compensation(h, p->input_rms);
        a.vol_comp_stream = h->d_vol_comp; // per-stream values once wf_hip_set_input_rms has been used
    }
    return a;
}

wf::MeterArgs meter_args(const wf_hip *h, const wf_hip_tick_params *p)
{
    wf::MeterArgs m = h->small->meter;
    m.ring = h->d_ring;
    m.wpos = h->d_wpos;
    m.mend = h->d_mend;
    m.meter_buf = h->d_meter_buf;
    m.meter_val = h->d_meter_val;
    m.stream_flags = h->d_flags;
    m.bars = h->d_bars;
    m.delay = p->delay_frames;
    m.delay_stream = h->d_delay;
    m.g = wf::gravity_for(h->cfg, p->seconds);
    m.g2 = 1.0f - m.g;
    return m;
}

wf::WaveArgs wave_args(const wf_hip *h, const wf_hip_tick_params *p)
{
    wf::WaveArgs w = h->small->wave;
    w.ring = h->d_ring;
    w.wpos = h->d_wpos;
    w.cend = h->d_cend;
    w.wts = h->d_wts;
    w.rows = h->d_decibels;
    w.stream_flags = h->d_flags;
    w.delay = p->delay_frames;
    w.delay_stream = h->d_delay;
    w.audio_ts = p->audio_ts_ns;
    w.audio_ts_stream = h->d_audio_ts;
    if(w.normalize) {
        w.vol_comp = volume_compensation(h, p->input_rms);
        w.vol_comp_stream = h->d_vol_comp;
    }
    return w;
}

// the vertex fill of streams [lo, hi), behind their bars
wf::VertexArgs vertex_args(const wf_hip *h, uint32_t lo, uint32_t hi)
{
    wf::VertexArgs v = h->small->vertex;
    v.bars = h->d_bars;
    v.verts = h->d_verts;
    v.counts = h->d_vert_counts;
    v.stream_base = lo;
    v.stream_count = hi - lo;
    return v;
}

// update_input_rms of every stream (what WAVSource::tick does first, src/source.cpp:1330-1331); leaves the per-stream volume
// compensation where the tick kernels read it.  No-op unless wf_hip_enable_input_rms has been called.
void launch_input_rms(wf_hip *h, const wf_hip_tick_params *p)
{
    if(h->d_rms_ring == nullptr)
        return;
    wf::RmsArgs r = h->small->rms; // (the producer's constants: enable_rms_producer)
    r.rms_ring = h->d_rms_ring;
    r.bsum = h->d_rms_bsum;
    r.wpos = h->d_wpos;
    r.flags = cur_flags(h);
    r.rend = h->d_rend;
    r.delay = p->delay_frames;
    r.delay_stream = h->d_delay;
    r.input_rms = h->d_input_rms;
    r.vol_comp = h->d_vol_comp;
    hipLaunchKernelGGL(wf::input_rms_kernel, dim3(h->n_streams), dim3(64), 0, h->stream, r);
}

} // namespace

int wf::host::join_lanes(wf_hip *h)
{
    if(h->lanes_pending) {
        WF_HIP_TRY(h, hipSetDevice(h->device));
        for(int l = 1; l < h->n_lanes; ++l)
            WF_HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_lane[l], 0));
        h->lanes_pending = false;
    }
    h->main_dirty = true;
    return WF_HIP_OK;
}

int wf::host::check_range(wf_hip *h, uint32_t first, uint32_t count)
{
    if(h == nullptr)
        return WF_HIP_ERR_INVALID;
    if(count == 0 || first >= h->n_streams || count > h->n_streams - first)
        return fail(h, WF_HIP_ERR_INVALID, "stream range [%u, %u+%u) outside 0..%u", first, first, count, h->n_streams);
    return join_lanes(h);
}

int wf::host::read_back(wf_hip *h, const void *d, void *out, size_t bytes)
{
    if(out == nullptr)
        return fail(h, WF_HIP_ERR_INVALID, "output pointer is NULL");
    WF_HIP_TRY(h, hipSetDevice(h->device));
    WF_HIP_TRY(h, hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, h->stream));
    WF_HIP_TRY(h, hipStreamSynchronize(h->stream));
    return WF_HIP_OK;
}

int wf::host::upload_words(wf_hip *h, void *d_dst, const void *src, size_t bytes)
{
    const uint32_t k = h->words_next++ & 1u;
    if(h->ev_words[k] == nullptr)
        WF_HIP_TRY(h, hipEventCreateWithFlags(&h->ev_words[k], hipEventDisableTiming));
    else
        WF_HIP_TRY(h, hipEventSynchronize(h->ev_words[k])); // the copy that used this block two calls ago (long done)
    if(h->h_words_bytes[k] < bytes) {
        if(h->h_words[k])
            (void)hipHostFree(h->h_words[k]);
        h->h_words[k] = nullptr;
        h->h_words_bytes[k] = 0;
        const size_t want = std::max<size_t>(bytes, 4096);
        WF_HIP_TRY(h, hipHostMalloc(&h->h_words[k], want, hipHostMallocDefault));
        h->h_words_bytes[k] = want;
    }
    std::memcpy(h->h_words[k], src, bytes);
    WF_HIP_TRY(h, hipMemcpyAsync(d_dst, h->h_words[k], bytes, hipMemcpyHostToDevice, h->stream));
    WF_HIP_TRY(h, hipEventRecord(h->ev_words[k], h->stream));
    return WF_HIP_OK;
}

namespace {

// frees a block handed out by dev_alloc (the caller has made sure nothing enqueued still uses it)
void dev_release(wf_hip *h, void *p)
{
    if(p == nullptr)
        return;
    for(size_t i = 0; i < h->allocs.size(); ++i)
        if(h->allocs[i] == p) {
            h->allocs[i] = h->allocs.back();
            h->allocs.pop_back();
            break;
        }
    // (its guard entry goes with it: the next block may get the same address with another size)
    h->guards.erase(std::remove_if(h->guards.begin(), h->guards.end(), [p](const auto &g) { return g.first == p; }), h->guards.end());
    (void)hipFree(p);
}

// staging blocks grow geometrically and the outgrown block is released once the stream has drained it
size_t grown(size_t have, size_t need) { return std::max(need, have + have / 2); }

// replaces *d by a block of at least `count` elements (the caller has made sure that nothing enqueued still uses the old one)
template<class T> int grow_stage(wf_hip *h, T **d, size_t *have, size_t count)
{
    dev_release(h, *d);
    *d = nullptr;
    const size_t want = grown(*have, count);
    *have = 0;
    T *p = nullptr;
    WF_TRY_RC(dev_alloc(h, &p, want));
    *d = p;
    *have = want;
    return WF_HIP_OK;
}

// the blocking pushes' block: every use of it is on `stream`, so draining the stream frees it
int ensure_stage(wf_hip *h, size_t floats)
{
    if(h->stage_floats >= floats)
        return WF_HIP_OK;
    WF_HIP_TRY(h, hipStreamSynchronize(h->stream)); // the old block may still feed a ring append
    return grow_stage(h, &h->d_stage, &h->stage_floats, floats);
}

// the squared-peak ring follows the pushed audio (wf_hip_enable_input_rms) -- as opposed to being fed by the host
inline bool rms_follows_audio(const wf_hip *h) { return h->d_rms_ring != nullptr && !h->rms_feed; }

constexpr uint32_t PUSH_SLICE = 16384; // streams per launch of the ingest kernels (rows = streams * cap_ch <= 65535)

// the RMS ring follows every push (before wpos advances): squared peaks, then the sums of the blocks the push completed
void rms_after_push(wf_hip *h, uint32_t first, uint32_t count, uint32_t frames)
{
    hipLaunchKernelGGL(wf::rms_block_kernel, dim3(frames / wf::RMS_BLOCK + 1, count), dim3(64), 0, h->stream, h->d_rms_ring,
                       h->d_rms_bsum, h->d_wpos, h->rms_cap, first, frames);
}

// What a uniform push of `frames` must satisfy, and a ragged one of `count` streams (frames[i] capped at max_frames): checked by
// the float, PCM and synth entry points alike
int check_uniform_push(wf_hip *h, uint32_t frames)
{
    if(rms_follows_audio(h) && frames > h->rms_cap)
        return fail(h, WF_HIP_ERR_INVALID, "push of %u frames exceeds the RMS ring capacity %u", frames, h->rms_cap);
    return measure_check_push(h, frames);
}

int check_ragged_push(wf_hip *h, uint32_t count, const uint32_t *frames, uint32_t max_frames)
{
    if(rms_follows_audio(h))
        return fail(h, WF_HIP_ERR_INVALID, "ragged pushes are not available while the device RMS producer follows the audio (wf_hip_enable_input_rms)");
    if(count > 65535u)
        return fail(h, WF_HIP_ERR_INVALID, "at most 65535 streams per ragged push");
    for(uint32_t i = 0; i < count; ++i)
        WF_TRY_RC(measure_check_push(h, std::min(frames[i], max_frames)));
    return WF_HIP_OK;
}

// The end of every append, behind the kernels that wrote the rings: the write positions advance (a ragged push's kernel has
// advanced them itself: d_frames != nullptr), then the loudness producer follows
int finish_push(wf_hip *h, uint32_t first, uint32_t count, uint32_t frames, const uint32_t *d_frames)
{
    if(d_frames == nullptr)
        hipLaunchKernelGGL(wf::wpos_advance_kernel, dim3((count + 255) / 256), dim3(256), 0, h->stream, h->d_wpos, cur_flags(h),
                           first, count, frames);
    measure_after_push(h, first, count, frames, d_frames);
    WF_HIP_TRY(h, hipGetLastError());
    if(d_frames == nullptr && frames % 4u)
        h->all_aligned = false; // (a ragged push: its caller, from the counts -- fill_counts)
    return WF_HIP_OK;
}

// d_src feeds the audio rings (nullptr: zeros); d_rms_src feeds the squared-peak ring when the producer is enabled
// (capture_audio takes the RMS from the packet even when it is muted, src/source.cpp:1842-1871 vs :1879-1880)
int push_common(wf_hip *h, uint32_t first, uint32_t count, const float *d_src, const float *d_rms_src, uint32_t frames)
{
    if(frames == 0)
        return WF_HIP_OK;
    // a packet longer than the ring keeps its newest ring_cap frames, as CircularBuffer + capture_audio's trimming would
    WF_TRY_RC(check_uniform_push(h, frames));
    // the kernels index (stream, channel) rows by blockIdx.y (at most 65535): larger batches go in slices
    for(uint32_t off = 0; off < count; off += PUSH_SLICE) {
        const uint32_t cnt = std::min(PUSH_SLICE, count - off);
        const size_t skip = (size_t)off * h->cap_ch * frames;
        const dim3 grid((frames + 255) / 256 > 64 ? 64 : (frames + 255) / 256, cnt * h->cap_ch), block(256);
        hipLaunchKernelGGL(wf::ring_push_kernel, grid, block, 0, h->stream, h->d_ring, h->d_wpos, h->ring_cap, h->ring_stride, h->cap_ch,
                           first + off, d_src ? d_src + skip : nullptr, frames);
        if(rms_follows_audio(h)) {
            hipLaunchKernelGGL(wf::rms_push_kernel, dim3(grid.x, cnt), block, 0, h->stream, h->d_rms_ring, h->d_wpos, h->rms_cap,
                               h->cap_ch, first + off, d_rms_src ? d_rms_src + skip : nullptr, frames);
            rms_after_push(h, first + off, cnt, frames);
        }
    }
    return finish_push(h, first, count, frames, nullptr);
}

// ---- pipelined ingest ---------------------------------------------------------------------------------------------------
// A push from page-locked memory goes through one of two slots (wf_hip::IngestSlot): the copy stream fills the slot's staging
// block, ev_copied[slot] hands it to `stream`, whose kernels read it, and the slot's ev_consumed says that they have.  The audio
// pushes (float, PCM; uniform or ragged) use h->ingest_slot[], the squared-peak feed h->sq_slot[]; every one of them reads:
// validate, slot_ready, copy, hand_over, launch, slot_consumed.
int ensure_copy_stream(wf_hip *h)
{
    if(h->copy_stream != nullptr)
        return WF_HIP_OK;
    WF_HIP_TRY(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    for(int i = 0; i < 2; ++i) {
        WF_HIP_TRY(h, hipEventCreateWithFlags(&h->ev_copied[i], hipEventDisableTiming));
        WF_HIP_TRY(h, hipEventCreateWithFlags(&h->ingest_slot[i].ev_consumed, hipEventDisableTiming));
        WF_HIP_TRY(h, hipEventCreateWithFlags(&h->sq_slot[i].ev_consumed, hipEventDisableTiming));
    }
    return WF_HIP_OK;
}

// Makes the slot ready for a copy of `floats` into its staging block and, for a ragged push, for `counts` > 0 frame counts.
// The ordering rule of the slots: what the slot's last push enqueued may still read its staging.  Where this push is about to
// touch the slot from the HOST -- a ragged push rewrites the page-locked counts that the last H2D copy reads, a block that is
// too small is released -- the host waits for ev_consumed.  Otherwise only device memory is reused, by the copy this push puts
// on the copy stream: the copy stream waits, the host does not.
int slot_ready(wf_hip *h, wf_hip::IngestSlot &s, size_t floats, uint32_t counts)
{
    const bool from_host = counts != 0 || s.stage_floats < floats;
    if(s.used && from_host)
        WF_HIP_TRY(h, hipEventSynchronize(s.ev_consumed));
    else if(s.used)
        WF_HIP_TRY(h, hipStreamWaitEvent(h->copy_stream, s.ev_consumed, 0));
    if(s.stage_floats < floats)
        WF_TRY_RC(grow_stage(h, &s.d_stage, &s.stage_floats, floats));
    if(s.frames_cap < counts) {
        dev_release(h, s.d_frames);
        s.d_frames = nullptr;
        if(s.h_frames)
            (void)hipHostFree(s.h_frames);
        s.h_frames = nullptr;
        s.frames_cap = 0;
        const size_t want = std::max<size_t>(counts, 64);
        WF_TRY_RC(dev_alloc(h, &s.d_frames, want));
        WF_HIP_TRY(h, hipHostMalloc(reinterpret_cast<void **>(&s.h_frames), want * sizeof(uint32_t), hipHostMallocDefault));
        s.frames_cap = want;
    }
    return WF_HIP_OK;
}

// the caller's frame counts, none above `clamp`, into the slot's page-locked block (behind slot_ready); what the callers
// derive from them
struct SlotCounts {
    bool aligned = true;  // every count is a multiple of 4 (wf_hip::all_aligned)
    uint32_t longest = 0;
};
constexpr uint32_t NO_CLAMP = 0xffffffffu;
SlotCounts fill_counts(wf_hip::IngestSlot &s, const uint32_t *frames, uint32_t count, uint32_t clamp)
{
    SlotCounts c;
    for(uint32_t i = 0; i < count; ++i) {
        s.h_frames[i] = std::min(frames[i], clamp);
        c.aligned = c.aligned && (s.h_frames[i] % 4u) == 0;
        c.longest = std::max(c.longest, s.h_frames[i]);
    }
    return c;
}

// behind the copy of the samples: the `counts` frame counts of a ragged push follow them, `copied` (ev_copied[slot]) marks the
// end of the slot's copies and the compute stream waits for it; whatever is enqueued behind (the tick) is ordered by the stream
int hand_over(wf_hip *h, wf_hip::IngestSlot &s, hipEvent_t copied, uint32_t counts)
{
    if(counts)
        WF_HIP_TRY(h, hipMemcpyAsync(s.d_frames, s.h_frames, (size_t)counts * sizeof(uint32_t), hipMemcpyHostToDevice, h->copy_stream));
    WF_HIP_TRY(h, hipEventRecord(copied, h->copy_stream));
    WF_HIP_TRY(h, hipStreamWaitEvent(h->stream, copied, 0));
    return WF_HIP_OK;
}

// behind the kernels that read the slot's staging
int slot_consumed(wf_hip *h, wf_hip::IngestSlot &s)
{
    WF_HIP_TRY(h, hipEventRecord(s.ev_consumed, h->stream));
    s.used = true;
    return WF_HIP_OK;
}

// ---- pipelined readback -------------------------------------------------------------------------------------------------
// wf_hip_read_async goes through one of two slots (wf_hip::ReadSlot): `stream` produces what the slot's copies read -- the ticks'
// outputs where they lie, the slot's snapshot, its silent bytes --, ev_snap hands it to the readback stream, whose D2H copies no
// later tick has to wait for, and ev_read, recorded once behind all of them, says that they have landed.  The ordering rule of
// the slots: the HOST waits for ev_read before anything of the slot is touched again -- its blocks released or overwritten, its
// events recorded (read_slot_ready; the caller's buffers: wf_hip_readback_done).  What the copies read where it lies (rows, bars,
// vertices, m_input_rms) has no snapshot: whatever overwrites it next waits for ev_read on the DEVICE (wait_rows_in_flight).
// Every path reads: validate, read_slot_ready, its launches on `stream`, to_read_stream, its copies (copy_out), copies_issued.
int ensure_read_stream(wf_hip *h)
{
    if(h->read_stream != nullptr)
        return WF_HIP_OK;
    WF_HIP_TRY(h, hipStreamCreateWithFlags(&h->read_stream, hipStreamNonBlocking));
    for(wf_hip::ReadSlot &s : h->read_slot) {
        WF_HIP_TRY(h, hipEventCreateWithFlags(&s.ev_snap, hipEventDisableTiming));
        WF_HIP_TRY(h, hipEventCreateWithFlags(&s.ev_read, hipEventDisableTiming));
    }
    return WF_HIP_OK;
}

// Frees the slot -- the host waits for its previous copies, BEFORE any block of it is released or overwritten -- and makes room
// for a snapshot of `floats` and for `silent` bytes of m_last_silent (0: the path uses no such block)
int read_slot_ready(wf_hip *h, wf_hip::ReadSlot &s, size_t floats, size_t silent)
{
    constexpr size_t FLOOR = 256; // elements: a handful of streams does not regrow its blocks one by one
    WF_TRY_RC(ensure_read_stream(h));
    if(s.used)
        WF_HIP_TRY(h, hipEventSynchronize(s.ev_read));
    if(s.snap_floats < floats)
        WF_TRY_RC(grow_stage(h, &s.d_snap, &s.snap_floats, std::max(floats, FLOOR)));
    if(s.silent_bytes < silent)
        WF_TRY_RC(grow_stage(h, &s.d_silent, &s.silent_bytes, std::max(silent, FLOOR)));
    return WF_HIP_OK;
}

// behind what `stream` holds for the slot (the ticks enqueued so far, the snapshot, the silent bytes): the readback stream waits
// for it
int to_read_stream(wf_hip *h, wf_hip::ReadSlot &s)
{
    WF_HIP_TRY(h, hipEventRecord(s.ev_snap, h->stream));
    WF_HIP_TRY(h, hipStreamWaitEvent(h->read_stream, s.ev_snap, 0));
    return WF_HIP_OK;
}

// one of the slot's copies
int copy_out(wf_hip *h, void *pinned, const void *d_src, size_t bytes)
{
    WF_HIP_TRY(h, hipMemcpyAsync(pinned, d_src, bytes, hipMemcpyDeviceToHost, h->read_stream));
    return WF_HIP_OK;
}

// Behind the slot's copies, whose result is `copies_rc`: ALSO when one of them failed, ev_read is recorded behind whatever went
// out, so that the next use of the slot, wf_hip_readback_done and -- `in_place`: the copies read the rows where they lie -- the
// next tick wait for the right thing
int copies_issued(wf_hip *h, wf_hip::ReadSlot &s, bool in_place, int copies_rc)
{
    const hipError_t e = hipEventRecord(s.ev_read, h->read_stream);
    if(e == hipSuccess) {
        s.used = true;
        s.rows_in_flight = s.rows_in_flight || in_place;
    }
    WF_TRY_RC(copies_rc);
    WF_HIP_TRY(h, e);
    return WF_HIP_OK;
}

// whatever is about to overwrite rows (a tick of a spectrum or waveform batch, wf_hip_reset) first makes `stream` wait -- on the
// device -- for the copies that read them where they lie
int wait_rows_in_flight(wf_hip *h)
{
    for(wf_hip::ReadSlot &s : h->read_slot)
        if(s.rows_in_flight) {
            WF_HIP_TRY(h, hipStreamWaitEvent(h->stream, s.ev_read, 0));
            s.rows_in_flight = false;
            h->main_dirty = true;
        }
    return WF_HIP_OK;
}

// ---- wf_hip_push_pcm ----------------------------------------------------------------------------------------------------
// (what a format value means -- validity, bytes, layout, sample kind, alignment: wf_pcm_formats.hpp)
using PcmLaunch = void (*)(dim3, hipStream_t, const wf::PcmPushArgs &);
template<uint32_t Fmt, bool Interleaved, bool Ragged>
void launch_pcm(dim3 grid, hipStream_t stream, const wf::PcmPushArgs &a)
{
    hipLaunchKernelGGL((wf::ring_push_pcm_kernel<Fmt, Interleaved, Ragged>), grid, dim3(wf::PCM_THREADS), 0, stream, a);
}
template<uint32_t Fmt, bool Interleaved, bool Ragged>
void launch_wire(dim3 grid, hipStream_t stream, const wf::PcmPushArgs &a)
{
    hipLaunchKernelGGL((wf::ring_push_wire_kernel<Fmt, Interleaved, Ragged>), grid, dim3(wf::PCM_THREADS), 0, stream, a);
}
template<bool Interleaved, bool Ragged>
PcmLaunch pcm_launcher_of(uint32_t kind)
{
    switch(kind) {
    case WF_HIP_PCM_U8: return launch_pcm<WF_HIP_PCM_U8, Interleaved, Ragged>;
    case WF_HIP_PCM_S16: return launch_pcm<WF_HIP_PCM_S16, Interleaved, Ragged>;
    case WF_HIP_PCM_S32: return launch_pcm<WF_HIP_PCM_S32, Interleaved, Ragged>;
    case WF_HIP_PCM_F32: return launch_pcm<WF_HIP_PCM_F32, Interleaved, Ragged>;
    case WF_HIP_WIRE_S24: return launch_wire<WF_HIP_WIRE_S24, Interleaved, Ragged>;
    case WF_HIP_WIRE_S24_BE: return launch_wire<WF_HIP_WIRE_S24_BE, Interleaved, Ragged>;
    case WF_HIP_WIRE_S16_BE: return launch_wire<WF_HIP_WIRE_S16_BE, Interleaved, Ragged>;
    case WF_HIP_WIRE_ULAW: return launch_wire<WF_HIP_WIRE_ULAW, Interleaved, Ragged>;
    case WF_HIP_WIRE_ALAW: return launch_wire<WF_HIP_WIRE_ALAW, Interleaved, Ragged>;
    default: return nullptr; // (no format: pcm_check has refused it)
    }
}
PcmLaunch pcm_launcher(uint32_t format, bool ragged)
{
    const uint32_t kind = wf::pcm_sample_kind(format);
    return wf::pcm_is_interleaved(format) ? (ragged ? pcm_launcher_of<true, true>(kind) : pcm_launcher_of<true, false>(kind))
                                          : (ragged ? pcm_launcher_of<false, true>(kind) : pcm_launcher_of<false, false>(kind));
}

// the descriptor's rules (include/wf_hip.h); nothing is enqueued before they hold
int pcm_check(wf_hip *h, uint32_t count, const wf_hip_pcm *pcm)
{
    if(pcm == nullptr || pcm->data == nullptr)
        return fail(h, WF_HIP_ERR_INVALID, "pcm or pcm->data is NULL");
    if(!wf::pcm_format_valid(pcm->format))
        return fail(h, WF_HIP_ERR_INVALID, "format %u is not a wf_hip_pcm_format or a wf_hip_wire_format", pcm->format);
    if(pcm->channels < 1 || pcm->channels > 8)
        return fail(h, WF_HIP_ERR_INVALID, "%u channels: a packet has 1..8", pcm->channels);
    if(pcm->channels < h->cap_ch || pcm->channel_base > pcm->channels - h->cap_ch || (h->cap_ch > 1 && pcm->channel_base != 0))
        return fail(h, WF_HIP_ERR_INVALID, "cannot capture %u channel(s) from channel %u of a %u-channel packet", h->cap_ch, pcm->channel_base,
                    pcm->channels);
    if(pcm->memory > WF_HIP_PCM_DEVICE || (pcm->memory == WF_HIP_PCM_PINNED && pcm->slot > 1))
        return fail(h, WF_HIP_ERR_INVALID, "memory %u / slot %u: expected host, pinned with slot 0 / 1, or device", pcm->memory, pcm->slot);
    if(pcm->memory == WF_HIP_PCM_DEVICE && (uintptr_t)pcm->data % wf::pcm_device_alignment(pcm->format))
        return fail(h, WF_HIP_ERR_INVALID, "device data is not aligned to its sample's natural alignment");
    if(pcm->frames_per_stream) {
        if(pcm->memory != WF_HIP_PCM_PINNED || pcm->frames == 0)
            return fail(h, WF_HIP_ERR_INVALID, "a ragged push needs WF_HIP_PCM_PINNED memory and frames (max_frames) > 0");
        return check_ragged_push(h, count, pcm->frames_per_stream, pcm->frames);
    }
    return check_uniform_push(h, pcm->frames);
}

// the H2D copy of a host packet into `dst`: interleaved (or every plane captured) in one piece; planar with more channels than
// captured: only the captured planes, one 2-D copy over the streams.  Returns the staged layout's channel count and base.
hipError_t pcm_copy(wf_hip *h, void *dst, const wf_hip_pcm *pcm, uint32_t count, hipStream_t stream, uint32_t *channels, uint32_t *base)
{
    const size_t plane = (size_t)pcm->frames * wf::pcm_sample_bytes(pcm->format);
    const size_t block = plane * pcm->channels;
    if(wf::pcm_is_interleaved(pcm->format) || pcm->channels == h->cap_ch) {
        *channels = pcm->channels;
        *base = pcm->channel_base;
        return hipMemcpyAsync(dst, pcm->data, block * count, hipMemcpyHostToDevice, stream);
    }
    *channels = h->cap_ch;
    *base = 0;
    return hipMemcpy2DAsync(dst, plane * h->cap_ch, static_cast<const unsigned char *>(pcm->data) + plane * pcm->channel_base, block,
                            plane * h->cap_ch, count, hipMemcpyHostToDevice, stream);
}

// the append: ring_push_pcm_kernel or ring_push_wire_kernel over the (staged) packet, then what push_common runs behind ring_push_kernel
int pcm_append(wf_hip *h, uint32_t first, uint32_t count, const wf_hip_pcm *pcm, const void *d_src, uint32_t channels, uint32_t base,
               const uint32_t *d_frames)
{
    const bool ragged = d_frames != nullptr;
    const uint32_t bps = wf::pcm_sample_bytes(pcm->format), frames = pcm->frames;
    wf::PcmPushArgs a{};
    a.ring = h->d_ring;
    a.wpos = h->d_wpos;
    a.flags = cur_flags(h);
    a.ring_cap = h->ring_cap;
    a.ring_stride = h->ring_stride;
    a.cap_ch = h->cap_ch;
    a.block_bytes = (size_t)channels * frames * bps;
    a.channels = channels;
    a.base = base;
    a.frames = frames;
    a.frames_per_stream = d_frames;
    a.rms_ring = rms_follows_audio(h) ? h->d_rms_ring : nullptr;
    a.rms_cap = h->rms_cap;
    const PcmLaunch launch = pcm_launcher(pcm->format, ragged);
    if(launch == nullptr)
        return fail(h, WF_HIP_ERR_INVALID, "format %u has no append kernel", pcm->format);
    if(ragged) {
        a.first = first;
        a.src = static_cast<const unsigned char *>(d_src);
        launch(dim3(1, count), h->stream, a);
        return finish_push(h, first, count, frames, d_frames);
    }
    const uint32_t tile = wf::wire_tile_frames(wf::pcm_is_interleaved(pcm->format), channels, bps); // (both kernels' tile)
    const uint32_t tiles = (uint32_t)std::min<size_t>(((size_t)frames + tile - 1) / tile, 64);
    for(uint32_t off = 0; off < count; off += PUSH_SLICE) {
        const uint32_t cnt = std::min(PUSH_SLICE, count - off);
        a.first = first + off;
        a.src = static_cast<const unsigned char *>(d_src) + (size_t)off * a.block_bytes;
        launch(dim3(tiles, cnt), h->stream, a);
        if(a.rms_ring)
            rms_after_push(h, first + off, cnt, frames);
    }
    return finish_push(h, first, count, frames, nullptr);
}

} // namespace

extern "C" {

int wf_hip_abi_version(void) { return WF_HIP_ABI_VERSION; }

int wf_hip_device_count(void)
{
    int n = 0;
    if(hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

const char *wf_hip_last_error(const wf_hip *h) { return h ? h->last_error.c_str() : g_create_error.c_str(); }

// update(): m_rms_sync_buf empty, m_input_rms_buf = 0, m_input_rms = 0 (src/source.cpp:1144-1152); no-op unless the device
// producer is enabled
static int reset_rms_producer(wf_hip *h, uint32_t first, uint32_t count)
{
    if(h->d_rms_ring == nullptr)
        return WF_HIP_OK;
    const size_t nblk = h->rms_cap / wf::RMS_BLOCK;
    WF_HIP_TRY(h, hipMemsetAsync(h->d_rms_ring + (size_t)first * h->rms_cap, 0, (size_t)count * h->rms_cap * sizeof(float), h->stream));
    WF_HIP_TRY(h, hipMemsetAsync(h->d_rms_bsum + (size_t)first * nblk, 0, (size_t)count * nblk * sizeof(float), h->stream));
    WF_HIP_TRY(h, hipMemsetAsync(h->d_rend + first, 0, (size_t)count * sizeof(uint32_t), h->stream));
    WF_HIP_TRY(h, hipMemsetAsync(h->d_input_rms + first, 0, (size_t)count * sizeof(float), h->stream));
    return WF_HIP_OK;
}

int wf_hip_reset(wf_hip *h, uint32_t first, uint32_t count)
{
    int rc = check_range(h, first, count);
    if(rc)
        return rc;
    WF_HIP_TRY(h, hipSetDevice(h->device));
    WF_TRY_RC(wait_rows_in_flight(h)); // the fills below overwrite rows a readback may still be copying
    const size_t spec0 = (size_t)first * h->cap_ch, nspec = (size_t)count * h->cap_ch;
    if(h->wave) {
        // update() in waveform mode (src/source.cpp:1142, :1172-1182, :1243-1248): rows = DB_MIN, rings = width zeros, m_waveform_ts = 0
        WF_HIP_TRY(h, hipMemsetAsync(h->d_ring + spec0 * h->ring_stride, 0, nspec * h->ring_stride * sizeof(float), h->stream));
        WF_HIP_TRY(h, hipMemsetAsync(h->d_flags + first, 0, (size_t)count * sizeof(uint32_t), h->stream));
        WF_HIP_TRY(h, hipMemsetAsync(h->d_cend + first, 0, (size_t)count * sizeof(uint32_t), h->stream));
        WF_HIP_TRY(h, hipMemsetAsync(h->d_wts + first, 0, (size_t)count * sizeof(unsigned long long), h->stream));
        const size_t ndb = (size_t)count * h->out_ch * h->M;
        hipLaunchKernelGGL(wf::fill_f32_kernel, dim3((unsigned)std::min<size_t>((ndb + 255) / 256, 4096)), dim3(256), 0, h->stream,
                           h->d_decibels + (size_t)first * h->out_ch * h->M, ndb, wf::db_min());
        hipLaunchKernelGGL(wf::fill_u32_kernel, dim3((count + 255) / 256), dim3(256), 0, h->stream, h->d_wpos + first, (size_t)count,
                           h->N);
        WF_HIP_TRY(h, hipGetLastError());
        if(first == 0 && count == h->n_streams)
            h->all_aligned = true;
        return reset_rms_producer(h, first, count); // waveform batches normalise too (src/source_generic.cpp:376-388)
    }
    if(h->meter) {
        // update() in meter mode (src/source.cpp:1123-1127, :1181, :1243): empty rings (no zero pre-fill), meter buffer 0,
        // m_meter_buf = m_meter_val = DB_MIN, m_last_silent = false
        WF_HIP_TRY(h, hipMemsetAsync(h->d_ring + spec0 * h->ring_stride, 0, nspec * h->ring_stride * sizeof(float), h->stream));
        WF_HIP_TRY(h, hipMemsetAsync(h->d_flags + first, 0, (size_t)count * sizeof(uint32_t), h->stream));
        WF_HIP_TRY(h, hipMemsetAsync(h->d_wpos + first, 0, (size_t)count * sizeof(uint32_t), h->stream));
        WF_HIP_TRY(h, hipMemsetAsync(h->d_mend + first, 0, (size_t)count * sizeof(uint32_t), h->stream));
        const dim3 g((unsigned)((nspec + 255) / 256)), b(256);
        hipLaunchKernelGGL(wf::fill_f32_kernel, g, b, 0, h->stream, h->d_meter_buf + spec0, nspec, wf::db_min());
        hipLaunchKernelGGL(wf::fill_f32_kernel, g, b, 0, h->stream, h->d_meter_val + spec0, nspec, wf::db_min());
        hipLaunchKernelGGL(wf::fill_f32_kernel, g, b, 0, h->stream, h->d_bars + spec0, nspec, h->tab.border_bottom);
        WF_HIP_TRY(h, hipGetLastError());
        if(first == 0 && count == h->n_streams)
            h->all_aligned = true;
        return WF_HIP_OK;
    }
    // m_tsmooth_buf = 0, rings = zeros with N samples "written", m_decibels = DB_MIN, m_last_silent = false
    WF_HIP_TRY(h, hipMemsetAsync(h->d_tsmooth + spec0 * h->M, 0, nspec * h->M * sizeof(float), h->stream));
    WF_HIP_TRY(h, hipMemsetAsync(h->d_ring + spec0 * h->ring_stride, 0, nspec * h->ring_stride * sizeof(float), h->stream));
    for(uint32_t b = 0; b < h->flag_bufs; ++b)
        WF_HIP_TRY(h, hipMemsetAsync(h->d_flags + (size_t)b * h->n_streams + first, 0, (size_t)count * sizeof(uint32_t), h->stream));
    if(h->d_row_verdict)
        WF_HIP_TRY(h, hipMemsetAsync(h->d_row_verdict + spec0 * h->waves_per_spectrum, 0, nspec * h->waves_per_spectrum * sizeof(uint32_t), h->stream));
    if(h->d_verdict) // rows of DB_MIN: nothing above floor - 10
        for(uint32_t b = 0; b < 3; ++b)
            WF_HIP_TRY(h, hipMemsetAsync(h->d_verdict + (size_t)b * h->n_streams * h->cap_ch + spec0, 0, nspec * sizeof(uint32_t), h->stream));
    const size_t ndb = (size_t)count * h->out_ch * h->M;
    hipLaunchKernelGGL(wf::fill_f32_kernel, dim3((unsigned)std::min<size_t>((ndb + 255) / 256, 4096)), dim3(256), 0, h->stream,
                       h->d_decibels + (size_t)first * h->out_ch * h->M, ndb, wf::db_min());
    hipLaunchKernelGGL(wf::fill_u32_kernel, dim3((count + 255) / 256), dim3(256), 0, h->stream, h->d_wpos + first, (size_t)count,
                       h->N);
    if(h->d_bars) {
        // what render_bars shows for rows of DB_MIN: every bar at border_bottom (zero height)
        const size_t nb = (size_t)count * h->disp_ch * h->num_bars;
        hipLaunchKernelGGL(wf::fill_f32_kernel, dim3((unsigned)std::min<size_t>((nb + 255) / 256, 4096)), dim3(256), 0, h->stream,
                           h->d_bars + (size_t)first * h->disp_ch * h->num_bars, nb, h->tab.border_bottom);
        if(h->d_bars_pre)
            hipLaunchKernelGGL(wf::fill_f32_kernel, dim3(((size_t)count * h->disp_ch + 255) / 256), dim3(256), 0, h->stream,
                               h->d_bars_pre + (size_t)first * h->disp_ch, (size_t)count * h->disp_ch, h->tab.border_bottom);
    }
    if(h->d_verts) {
        // no geometry until the first tick, as after create
        const size_t pv = (size_t)h->disp_ch * h->small->vertex.per_row;
        WF_HIP_TRY(h, hipMemsetAsync(h->d_verts + (size_t)first * pv, 0, (size_t)count * pv * sizeof(wf::f4), h->stream));
        WF_HIP_TRY(h, hipMemsetAsync(h->d_vert_counts + (size_t)first * h->disp_ch, 0, (size_t)count * h->disp_ch * sizeof(uint32_t), h->stream));
    }
    WF_HIP_TRY(h, hipGetLastError());
    // the mirror set being written holds the bars of the ticks before this reset: the next hand-over copies the handle's own bars
    // (the reset state of these streams) in, as it does before any tick
    if(h->mirror_n)
        h->mirror_fresh = false;
    int rrc = reset_rms_producer(h, first, count);
    if(rrc)
        return rrc;
    if(first == 0 && count == h->n_streams)
        h->all_aligned = true; // every write position is back at fft_size
    return WF_HIP_OK;
}

uint32_t wf_hip_fft_size(const wf_hip *h) { return h ? h->N : 0; }
uint32_t wf_hip_num_streams(const wf_hip *h) { return h ? h->n_streams : 0; }
uint32_t wf_hip_capture_channels(const wf_hip *h) { return h ? h->cap_ch : 0; }
uint32_t wf_hip_output_channels(const wf_hip *h) { return h ? h->out_ch : 0; }
uint32_t wf_hip_display_channels(const wf_hip *h) { return h ? h->disp_ch : 0; }
uint32_t wf_hip_num_bars(const wf_hip *h) { return h ? h->num_bars : 0; }
uint32_t wf_hip_ring_frames(const wf_hip *h) { return h ? h->ring_cap : 0; }

static int push_host(wf_hip *h, uint32_t first, uint32_t count, const float *samples, uint32_t frames, bool muted)
{
    int rc = check_range(h, first, count);
    if(rc)
        return rc;
    if(samples == nullptr)
        return fail(h, WF_HIP_ERR_INVALID, "samples is NULL");
    WF_HIP_TRY(h, hipSetDevice(h->device));
    const size_t n = (size_t)count * h->cap_ch * frames;
    // the staging block may still feed a previous push: the copy below is ordered after it on the same stream
    rc = ensure_stage(h, n);
    if(rc)
        return rc;
    WF_HIP_TRY(h, hipMemcpyAsync(h->d_stage, samples, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    rc = push_common(h, first, count, muted ? nullptr : h->d_stage, h->d_stage, frames);
    if(rc)
        return rc;
    // `samples` is borrowed only for the duration of the call (pageable memory: the copy has been staged by the
    // runtime when hipMemcpyAsync returns; pinned memory: wait for it)
    WF_HIP_TRY(h, hipStreamSynchronize(h->stream));
    return WF_HIP_OK;
}

int wf_hip_push_audio(wf_hip *h, uint32_t first, uint32_t count, const float *samples, uint32_t frames)
{
    return push_host(h, first, count, samples, frames, false);
}

int wf_hip_push_audio_muted(wf_hip *h, uint32_t first, uint32_t count, const float *samples, uint32_t frames)
{
    if(samples != nullptr && h != nullptr && rms_follows_audio(h))
        return push_host(h, first, count, samples, frames, true); // the RMS producer takes the packet's samples
    // a packet without data, or nobody to read it: CircularBuffer::push_back_zero
    int rc = check_range(h, first, count);
    if(rc)
        return rc;
    WF_HIP_TRY(h, hipSetDevice(h->device));
    return push_common(h, first, count, nullptr, nullptr, frames);
}

int wf_hip_push_audio_async(wf_hip *h, uint32_t first, uint32_t count, const float *pinned_samples, uint32_t frames, uint32_t slot)
{
    int rc = check_range(h, first, count);
    if(rc)
        return rc;
    if(pinned_samples == nullptr || slot > 1)
        return fail(h, WF_HIP_ERR_INVALID, "samples is NULL or slot is not 0 / 1");
    WF_HIP_TRY(h, hipSetDevice(h->device));
    wf_hip::IngestSlot &s = h->ingest_slot[slot];
    const size_t n = (size_t)count * h->cap_ch * frames;
    WF_TRY_RC(ensure_copy_stream(h));
    WF_TRY_RC(slot_ready(h, s, n, 0));
    WF_HIP_TRY(h, hipMemcpyAsync(s.d_stage, pinned_samples, n * sizeof(float), hipMemcpyHostToDevice, h->copy_stream));
    WF_TRY_RC(hand_over(h, s, h->ev_copied[slot], 0));
    WF_TRY_RC(push_common(h, first, count, s.d_stage, s.d_stage, frames));
    return slot_consumed(h, s);
}

int wf_hip_push_audio_ragged_async(wf_hip *h, uint32_t first, uint32_t count, const float *pinned_samples, const uint32_t *frames,
                                   uint32_t max_frames, uint32_t slot)
{
    WF_TRY_RC(check_range(h, first, count));
    if(pinned_samples == nullptr || frames == nullptr || slot > 1 || max_frames == 0)
        return fail(h, WF_HIP_ERR_INVALID, "samples or frames is NULL, max_frames is 0 or slot is not 0 / 1");
    WF_TRY_RC(check_ragged_push(h, count, frames, max_frames));
    WF_HIP_TRY(h, hipSetDevice(h->device));
    wf_hip::IngestSlot &s = h->ingest_slot[slot];
    const size_t n = (size_t)count * h->cap_ch * max_frames;
    WF_TRY_RC(ensure_copy_stream(h));
    WF_TRY_RC(slot_ready(h, s, n, count));
    const SlotCounts c = fill_counts(s, frames, count, NO_CLAMP);
    WF_HIP_TRY(h, hipMemcpyAsync(s.d_stage, pinned_samples, n * sizeof(float), hipMemcpyHostToDevice, h->copy_stream));
    WF_TRY_RC(hand_over(h, s, h->ev_copied[slot], count));
    hipLaunchKernelGGL(wf::ring_push_ragged_kernel, dim3(1, count), dim3(256), 0, h->stream, h->d_ring, h->d_wpos,
                       cur_flags(h), h->ring_cap, h->ring_stride, h->cap_ch, first, s.d_stage, s.d_frames, max_frames);
    WF_TRY_RC(finish_push(h, first, count, max_frames, s.d_frames));
    WF_TRY_RC(slot_consumed(h, s));
    if(!c.aligned)
        h->all_aligned = false;
    return WF_HIP_OK;
}

int wf_hip_ingest_done(wf_hip *h, uint32_t slot)
{
    if(h == nullptr || slot > 1)
        return WF_HIP_ERR_INVALID;
    if(!h->ingest_slot[slot].used && !h->sq_slot[slot].used)
        return WF_HIP_OK;
    WF_HIP_TRY(h, hipSetDevice(h->device));
    WF_HIP_TRY(h, hipEventSynchronize(h->ev_copied[slot])); // the slot's last H2D copy (samples or squared peaks)
    return WF_HIP_OK;
}

void *wf_hip_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if(hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}

void wf_hip_host_free(void *p)
{
    if(p)
        (void)hipHostFree(p);
}

int wf_hip_push_audio_device(wf_hip *h, uint32_t first, uint32_t count, const float *d_samples, uint32_t frames)
{
    int rc = check_range(h, first, count);
    if(rc)
        return rc;
    if(d_samples == nullptr)
        return fail(h, WF_HIP_ERR_INVALID, "d_samples is NULL");
    WF_HIP_TRY(h, hipSetDevice(h->device));
    return push_common(h, first, count, d_samples, d_samples, frames);
}

int wf_hip_push_synth(wf_hip *h, uint32_t first, uint32_t count, uint64_t seed, uint32_t stream_id0, uint64_t index0,
                      uint32_t frames)
{
    int rc = check_range(h, first, count);
    if(rc)
        return rc;
    if(frames == 0)
        return WF_HIP_OK;
    WF_TRY_RC(check_uniform_push(h, frames));
    WF_HIP_TRY(h, hipSetDevice(h->device));
    const uint32_t gx = std::min<uint32_t>((frames + 255) / 256, 256);
    for(uint32_t off = 0; off < count; off += PUSH_SLICE) {
        const uint32_t cnt = std::min(PUSH_SLICE, count - off);
        hipLaunchKernelGGL(wf::ring_synth_kernel, dim3(gx, cnt * h->cap_ch), dim3(256), 0, h->stream, h->d_ring, h->d_wpos,
                           h->ring_cap, h->ring_stride, h->cap_ch, first + off, seed, stream_id0 + off, index0, frames);
        if(rms_follows_audio(h)) {
            hipLaunchKernelGGL(wf::rms_synth_kernel, dim3(gx, cnt), dim3(256), 0, h->stream, h->d_rms_ring, h->d_wpos, h->rms_cap,
                               h->cap_ch, first + off, seed, stream_id0 + off, index0, frames);
            rms_after_push(h, first + off, cnt, frames);
        }
    }
    return finish_push(h, first, count, frames, nullptr);
}

int wf_hip_push_pcm(wf_hip *h, uint32_t first, uint32_t count, const wf_hip_pcm *pcm)
{
    if(h == nullptr)
        return WF_HIP_ERR_INVALID;
    WF_TRY_RC(pcm_check(h, count, pcm));
    WF_TRY_RC(check_range(h, first, count));
    const bool ragged = pcm->frames_per_stream != nullptr;
    if(pcm->frames == 0)
        return WF_HIP_OK;
    WF_HIP_TRY(h, hipSetDevice(h->device));
    const uint32_t bps = wf::pcm_sample_bytes(pcm->format);
    if(pcm->memory == WF_HIP_PCM_DEVICE)
        return pcm_append(h, first, count, pcm, pcm->data, pcm->channels, pcm->channel_base, nullptr);
    // the bytes that cross the bus: whole frames of an interleaved packet, the captured planes of a planar one
    const uint32_t staged_ch = wf::pcm_is_interleaved(pcm->format) ? pcm->channels : h->cap_ch;
    const size_t floats = ((size_t)count * staged_ch * pcm->frames * bps + 3) / 4; // (the staging blocks are the float paths')
    uint32_t channels = 0, base = 0;
    if(pcm->memory == WF_HIP_PCM_HOST) {
        WF_TRY_RC(ensure_stage(h, floats)); // (ordered after the previous push's append on the same stream)
        WF_HIP_TRY(h, pcm_copy(h, h->d_stage, pcm, count, h->stream, &channels, &base));
        WF_TRY_RC(pcm_append(h, first, count, pcm, h->d_stage, channels, base, nullptr));
        WF_HIP_TRY(h, hipStreamSynchronize(h->stream)); // `data` is borrowed for the call only
        return WF_HIP_OK;
    }
    // WF_HIP_PCM_PINNED: wf_hip_push_audio_async's pipeline
    wf_hip::IngestSlot &s = h->ingest_slot[pcm->slot];
    const uint32_t counts = ragged ? count : 0;
    WF_TRY_RC(ensure_copy_stream(h));
    WF_TRY_RC(slot_ready(h, s, floats, counts));
    const SlotCounts c = fill_counts(s, pcm->frames_per_stream, counts, NO_CLAMP);
    WF_HIP_TRY(h, pcm_copy(h, s.d_stage, pcm, count, h->copy_stream, &channels, &base));
    WF_TRY_RC(hand_over(h, s, h->ev_copied[pcm->slot], counts));
    WF_TRY_RC(pcm_append(h, first, count, pcm, s.d_stage, channels, base, ragged ? s.d_frames : nullptr));
    WF_TRY_RC(slot_consumed(h, s));
    if(!c.aligned)
        h->all_aligned = false;
    return WF_HIP_OK;
}

// roctx ranges around the tick ("Tracing": the reference has none either; the timeline of a profiled process
// then shows the host's part of every tick next to the kernels).  Opt-in -- WF_HIP_ROCTX=1 in the environment -- and resolved at
// run time from the profiler's own marker library (librocprofiler-sdk-roctx.so, else libroctx64.so): the product links neither.
extern "C++" {
namespace {
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    Roctx()
    {
        const char *e = std::getenv("WF_HIP_ROCTX");
        if(e == nullptr || e[0] == '0')
            return;
        for(const char *name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
            if(void *lib = dlopen(name, RTLD_NOW | RTLD_LOCAL)) {
                push = reinterpret_cast<int (*)(const char *)>(dlsym(lib, "roctxRangePushA"));
                pop = reinterpret_cast<int (*)()>(dlsym(lib, "roctxRangePop"));
                if(push && pop)
                    return;
                push = nullptr;
                pop = nullptr;
            }
        }
    }
};
const Roctx &roctx()
{
    static const Roctx r; // (thread-safe initialisation)
    return r;
}
} // namespace
} // extern "C++"

static int wf_hip_tick_impl(wf_hip *h, const wf_hip_tick_params *p);
int wf_hip_tick(wf_hip *h, const wf_hip_tick_params *p)
{
    const Roctx &rx = roctx();
    if(rx.push == nullptr)
        return wf_hip_tick_impl(h, p);
    rx.push("wf_hip_tick");
    const int rc = wf_hip_tick_impl(h, p);
    rx.pop();
    return rc;
}

static int wf_hip_tick_impl(wf_hip *h, const wf_hip_tick_params *p)
{
    if(h == nullptr || p == nullptr)
        return WF_HIP_ERR_INVALID;
    if((uint64_t)p->delay_frames + h->max_stream_delay + (h->wave ? h->small->wave.waveform_samples : h->N) > h->ring_cap)
        return fail(h, WF_HIP_ERR_INVALID, "delay_frames %u (+ per-stream %u) + fft_size %u exceeds the ring capacity %u", p->delay_frames,
                    h->max_stream_delay, h->N, h->ring_cap);
    if((p->flags & WF_HIP_TICK_NO_DECIBELS) && h->num_bars == 0)
        return fail(h, WF_HIP_ERR_INVALID, "WF_HIP_TICK_NO_DECIBELS on a configuration without bars or curve: the tick would produce nothing");
    WF_HIP_TRY(h, hipSetDevice(h->device));
    if(h->wave) {
        WF_TRY_RC(wait_rows_in_flight(h)); // the waveform rows are read back the same way
        launch_input_rms(h, p);
        const wf::WaveArgs w = wave_args(h, p);
        hipLaunchKernelGGL(wf::waveform_tick_kernel, dim3((h->n_streams + wf::WAVE_STREAMS - 1) / wf::WAVE_STREAMS), dim3(wf::WAVE_THREADS), 0, h->stream, w);
        WF_HIP_TRY(h, hipGetLastError());
        return WF_HIP_OK;
    }
    if(h->meter) {
        const wf::MeterArgs m = meter_args(h, p);
        hipLaunchKernelGGL(wf::meter_tick_kernel, dim3(h->n_streams), dim3(wf::METER_THREADS), 0, h->stream, m);
        WF_HIP_TRY(h, hipGetLastError());
        return WF_HIP_OK;
    }
    const bool mono_mix_rows = !h->cfg.stereo && h->cap_ch > 1;
    wf_hip_tick_params p_rows;
    if((p->flags & WF_HIP_TICK_NO_DECIBELS) && (h->plan.big_l || h->disp.ext_outputs)) {
        // the outputs of this batch are derived from the stored rows (big_outputs_kernel): the rows are stored regardless --
        // the flag only ever promised that they MAY be stale
        p_rows = *p;
        p_rows.flags &= ~WF_HIP_TICK_NO_DECIBELS;
        p = &p_rows;
    }
    if((p->flags & WF_HIP_TICK_NO_DECIBELS) && !mono_mix_rows && h->d_stale_row == nullptr) {
        if(h->cfg.floor_db - 10 >= 0)
            return fail(h, WF_HIP_ERR_INVALID, "WF_HIP_TICK_NO_DECIBELS needs floor_db < 10 (a skipped channel's row must be negative)");
        int rc = dev_alloc(h, &h->d_stale_row, (size_t)h->M);
        if(rc)
            return rc;
        hipLaunchKernelGGL(wf::fill_f32_kernel, dim3((h->M + 255) / 256), dim3(256), 0, h->stream, h->d_stale_row, (size_t)h->M, wf::db_min());
        if(!h->split) {
            rc = dev_alloc(h, &h->d_row_verdict, (size_t)h->n_streams * h->cap_ch * h->waves_per_spectrum);
            if(rc)
                return rc;
        }
        rc = dev_alloc(h, &h->d_bars_only, 1);
        if(rc)
            return rc;
        const wf::BarsOnlyState st{h->d_row_verdict, h->d_stale_row, 0u}; // this tick's rows are still current
        WF_HIP_TRY(h, hipMemcpyAsync(h->d_bars_only, &st, sizeof(st), hipMemcpyHostToDevice, h->stream));
        WF_HIP_TRY(h, hipStreamSynchronize(h->stream)); // `st` dies here
        h->main_dirty = true;
    }
    WF_TRY_RC(wait_rows_in_flight(h)); // this tick's row stores wait for a readback still in flight
    if(h->d_rms_ring)
        WF_TRY_RC(join_lanes(h)); // (never pending: the RMS producer keeps the batch on one lane)
    launch_input_rms(h, p);
    wf::TickArgs a = tick_args(h, p);
    const bool aligned = h->all_aligned && h->stream_delays_aligned && (p->delay_frames % 4u) == 0;
    const int lanes = h->d_rms_ring ? 1 : h->n_lanes; // update_input_rms runs on `stream` ahead of every tick: one lane
    if(lanes > 1 && h->main_dirty) {
        WF_HIP_TRY(h, hipEventRecord(h->ev_fork, h->stream));
        for(int l = 1; l < lanes; ++l)
            WF_HIP_TRY(h, hipStreamWaitEvent(h->lane_stream[l], h->ev_fork, 0));
    }
    h->main_dirty = false;
    for(int l = 0; l < lanes; ++l) {
        const uint32_t lo = (uint32_t)((uint64_t)h->n_streams * l / lanes), hi = (uint32_t)((uint64_t)h->n_streams * (l + 1) / lanes);
        a.stream_base = lo;
        a.stream_count = hi - lo;
        hipStream_t st = l == 0 ? h->stream : h->lane_stream[l];
        if(h->disp.ext_outputs) {
            // the tick kernel stores rows only; the display comes from them, one workgroup per displayed row
            wf::TickArgs rows_only = a;
            rows_only.bar.out = nullptr;
            WF_TRY_RC(h->launch(h, rows_only, aligned, st));
            if(hi > lo)
                big_outputs_launch(h, a, (hi - lo) * h->disp_ch, st);
        } else
            WF_TRY_RC(h->launch(h, a, aligned, st));
        if(h->d_verts && hi > lo)
            hipLaunchKernelGGL(wf::vertex_fill_kernel, dim3((hi - lo) * h->disp_ch), dim3(256), 0, st, vertex_args(h, lo, hi));
        if(l > 0)
            WF_HIP_TRY(h, hipEventRecord(h->ev_lane[l], h->lane_stream[l]));
    }
    if(lanes > 1)
        h->lanes_pending = true;
    WF_HIP_TRY(h, hipGetLastError());
    if(h->d_row_verdict && !h->verdict_tracking) {
        // this tick left a verdict for every row; later ticks read those (the flag flips behind this tick's kernels, on every lane)
        h->verdict_tracking = true;
        WF_TRY_RC(join_lanes(h));
        const wf::BarsOnlyState st{h->d_row_verdict, h->d_stale_row, 1u};
        WF_HIP_TRY(h, hipMemcpyAsync(h->d_bars_only, &st, sizeof(st), hipMemcpyHostToDevice, h->stream));
        WF_HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if(h->split)
        h->flag_cur = (h->flag_cur + 1) % 3; // what the kernel wrote is what the next tick (and the readers) see
    if(h->mirror_n)
        h->mirror_fresh = true;
    return WF_HIP_OK;
}

int wf_hip_set_hidden(wf_hip *h, uint32_t first, uint32_t count, const uint8_t *mask)
{
    WF_TRY_RC(check_range(h, first, count));
    if(mask == nullptr)
        return fail(h, WF_HIP_ERR_INVALID, "mask is NULL");
    if(h->meter || h->wave)
        for(uint32_t i = 0; i < count; ++i)
            if(mask[i] == WF_HIP_STARVED)
                return fail(h, WF_HIP_ERR_INVALID, "WF_HIP_STARVED applies to spectrum batches only");
    WF_HIP_TRY(h, hipSetDevice(h->device));
    if(h->mask_bytes < count) {
        WF_TRY_RC(dev_alloc(h, &h->d_mask, (size_t)count));
        h->mask_bytes = count;
    }
    WF_HIP_TRY(h, hipMemcpyAsync(h->d_mask, mask, count, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(wf::set_hidden_kernel, dim3((count + 255) / 256), dim3(256), 0, h->stream, cur_flags(h), first, count,
                       h->d_mask);
    WF_HIP_TRY(h, hipGetLastError());
    WF_HIP_TRY(h, hipStreamSynchronize(h->stream)); // `mask` is borrowed for the call only
    return WF_HIP_OK;
}

int wf_hip_set_stream_delay(wf_hip *h, uint32_t first, uint32_t count, const uint32_t *delay_frames)
{
    int rc = check_range(h, first, count);
    if(rc)
        return rc;
    if(delay_frames == nullptr)
        return fail(h, WF_HIP_ERR_INVALID, "delay_frames is NULL");
    uint32_t mx = 0;
    bool al = true;
    for(uint32_t i = 0; i < count; ++i) {
        mx = std::max(mx, delay_frames[i]);
        al = al && (delay_frames[i] % 4u) == 0;
    }
    const uint32_t window = h->wave ? h->small->wave.waveform_samples : h->N; // the same capacity term as wf_hip_tick
    if((uint64_t)mx + window > h->ring_cap)
        return fail(h, WF_HIP_ERR_INVALID, "stream delay %u + window %u exceeds the ring capacity %u", mx, window, h->ring_cap);
    WF_HIP_TRY(h, hipSetDevice(h->device));
    if(h->d_delay == nullptr) {
        rc = dev_alloc(h, &h->d_delay, (size_t)h->n_streams);
        if(rc)
            return rc;
        WF_HIP_TRY(h, hipMemsetAsync(h->d_delay, 0, (size_t)h->n_streams * sizeof(uint32_t), h->stream));
    }
    WF_TRY_RC(upload_words(h, h->d_delay + first, delay_frames, (size_t)count * sizeof(uint32_t))); // (staged: `delay_frames` is borrowed for the call only, and the call does not wait)
    h->max_stream_delay = std::max(h->max_stream_delay, mx);
    h->stream_delays_aligned = h->stream_delays_aligned && al; // conservative: never switches back to the vector fetch
    return WF_HIP_OK;
}

int wf_hip_set_stream_audio_ts(wf_hip *h, uint32_t first, uint32_t count, const uint64_t *audio_ts_ns)
{
    int rc = check_range(h, first, count);
    if(rc)
        return rc;
    if(!h->wave)
        return fail(h, WF_HIP_ERR_INVALID, "per-stream audio timestamps belong to waveform batches");
    if(audio_ts_ns == nullptr)
        return fail(h, WF_HIP_ERR_INVALID, "audio_ts_ns is NULL");
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit timestamps");
    WF_HIP_TRY(h, hipSetDevice(h->device));
    if(h->d_audio_ts == nullptr) {
        rc = dev_alloc(h, &h->d_audio_ts, (size_t)h->n_streams);
        if(rc)
            return rc;
        WF_HIP_TRY(h, hipMemsetAsync(h->d_audio_ts, 0, (size_t)h->n_streams * sizeof(unsigned long long), h->stream));
    }
    WF_TRY_RC(upload_words(h, h->d_audio_ts + first, audio_ts_ns, (size_t)count * sizeof(uint64_t))); // (staged, no wait: see upload_words)
    return WF_HIP_OK;
}

int wf_hip_set_input_rms(wf_hip *h, uint32_t first, uint32_t count, const float *rms)
{
    int rc = check_range(h, first, count);
    if(rc)
        return rc;
    if(rms == nullptr)
        return fail(h, WF_HIP_ERR_INVALID, "rms is NULL");
    if(h->d_rms_ring)
        return fail(h, WF_HIP_ERR_INVALID, "m_input_rms is produced on the device (wf_hip_enable_input_rms); it cannot be set");
    WF_HIP_TRY(h, hipSetDevice(h->device));
    if(h->d_vol_comp == nullptr) {
        rc = dev_alloc(h, &h->d_vol_comp, (size_t)h->n_streams);
        if(rc)
            return rc;
        const std::vector<float> init(h->n_streams, volume_compensation(h, 0.0f));
        WF_HIP_TRY(h, hipMemcpyAsync(h->d_vol_comp, init.data(), init.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
        WF_HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    std::vector<float> v(count);
    for(uint32_t i = 0; i < count; ++i)
        v[i] = volume_compensation(h, rms[i]); // of every stream
    WF_HIP_TRY(h, hipMemcpyAsync(h->d_vol_comp + first, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    WF_HIP_TRY(h, hipStreamSynchronize(h->stream)); // the staging vector dies here
    return WF_HIP_OK;
}

static int enable_rms_producer(wf_hip *h, bool feed)
{
    if(h == nullptr)
        return WF_HIP_ERR_INVALID;
    if(!h->cfg.normalize_volume || h->meter)
        return fail(h, WF_HIP_ERR_INVALID, "the device RMS producer needs a spectrum or waveform batch with cfg.normalize_volume");
    if(h->d_rms_ring)
        return h->rms_feed == feed ? WF_HIP_OK : fail(h, WF_HIP_ERR_INVALID, "the device RMS producer is already enabled in the other mode");
    WF_HIP_TRY(h, hipSetDevice(h->device));
    WF_TRY_RC(join_lanes(h));
    h->rms_size = h->cfg.sample_rate & ~15u; // m_input_rms_size, src/source.cpp:1147
    if(h->rms_size == 0)
        return fail(h, WF_HIP_ERR_INVALID, "sample_rate %u is too small for the RMS window", h->cfg.sample_rate);
    // the window + every A/V-sync delay the audio rings admit + the two ragged blocks at its ends (feed mode: the window,
    // the ragged blocks and one feed of up to a window's length)
    h->rms_cap = feed ? next_pow2(2 * h->rms_size + 2 * wf::RMS_BLOCK)
                      : next_pow2(h->rms_size + (h->wave ? h->ring_cap : h->ring_cap - h->N) + 2 * wf::RMS_BLOCK);
    const size_t nblk = h->rms_cap / wf::RMS_BLOCK;
    float *ring = nullptr, *bsum = nullptr;
    int rc = dev_alloc(h, &ring, (size_t)h->n_streams * h->rms_cap);
    if(rc == WF_HIP_OK) rc = dev_alloc(h, &bsum, (size_t)h->n_streams * nblk);
    if(rc == WF_HIP_OK) rc = dev_alloc(h, &h->d_rend, (size_t)h->n_streams);
    if(rc == WF_HIP_OK) rc = dev_alloc(h, &h->d_input_rms, (size_t)h->n_streams);
    if(rc == WF_HIP_OK && h->d_vol_comp == nullptr) rc = dev_alloc(h, &h->d_vol_comp, (size_t)h->n_streams);
    if(rc)
        return rc;
    // audio captured before this call counts as silence (m_input_rms_buf starts as zeros); the first tick's kernel
    // fills d_vol_comp before the spectrum kernel reads it
    WF_HIP_TRY(h, hipMemsetAsync(ring, 0, (size_t)h->n_streams * h->rms_cap * sizeof(float), h->stream));
    WF_HIP_TRY(h, hipMemsetAsync(bsum, 0, (size_t)h->n_streams * nblk * sizeof(float), h->stream));
    WF_HIP_TRY(h, hipMemsetAsync(h->d_rend, 0, (size_t)h->n_streams * sizeof(uint32_t), h->stream));
    WF_HIP_TRY(h, hipMemsetAsync(h->d_input_rms, 0, (size_t)h->n_streams * sizeof(float), h->stream));
    h->d_rms_bsum = bsum;
    h->rms_feed = feed;
    wf::RmsArgs &r = small_args(h).rms;
    r.rms_cap = h->rms_cap;
    r.size = h->rms_size;
    r.volume_target = h->cfg.volume_target;
    r.max_gain = h->cfg.max_gain;
    r.db_min = wf::db_min();
    r.n_streams = h->n_streams;
    r.feed = feed ? 1u : 0u;
    h->d_rms_ring = ring; // from here on every push feeds it (or, feed mode, wf_hip_push_rms_ragged_async does)
    h->main_dirty = true;
    return WF_HIP_OK;
}

int wf_hip_enable_input_rms(wf_hip *h, int feed) { return enable_rms_producer(h, feed != 0); }

int wf_hip_push_rms_ragged_async(wf_hip *h, uint32_t first, uint32_t count, const float *pinned_sq, const uint32_t *frames, uint32_t max_frames,
                                 uint32_t slot)
{
    int rc = check_range(h, first, count);
    if(rc)
        return rc;
    if(pinned_sq == nullptr || frames == nullptr || slot > 1 || max_frames == 0)
        return fail(h, WF_HIP_ERR_INVALID, "values or frames is NULL, max_frames is 0 or slot is not 0 / 1");
    if(!h->rms_feed)
        return fail(h, WF_HIP_ERR_INVALID, "wf_hip_push_rms_ragged_async needs wf_hip_enable_input_rms(h, 1)");
    if(max_frames > h->rms_size)
        return fail(h, WF_HIP_ERR_INVALID, "a feed of %u values per stream exceeds the RMS window (%u)", max_frames, h->rms_size);
    WF_HIP_TRY(h, hipSetDevice(h->device));
    wf_hip::IngestSlot &s = h->sq_slot[slot];
    const size_t n = (size_t)count * max_frames;
    WF_TRY_RC(ensure_copy_stream(h));
    WF_TRY_RC(slot_ready(h, s, n, count)); // (in use two feeds ago)
    const SlotCounts c = fill_counts(s, frames, count, max_frames);
    if(c.longest == 0)
        return WF_HIP_OK; // nothing to consume this frame (sync_rms_buffer returns false for every stream)
    // rows are max_frames apart; only the part any stream uses crosses the bus when the rows are short
    if(c.longest == max_frames || count == 1)
        WF_HIP_TRY(h, hipMemcpyAsync(s.d_stage, pinned_sq, (count == 1 ? (size_t)c.longest : n) * sizeof(float), hipMemcpyHostToDevice, h->copy_stream));
    else
        WF_HIP_TRY(h, hipMemcpy2DAsync(s.d_stage, (size_t)max_frames * sizeof(float), pinned_sq, (size_t)max_frames * sizeof(float),
                                       (size_t)c.longest * sizeof(float), count, hipMemcpyHostToDevice, h->copy_stream));
    WF_TRY_RC(join_lanes(h));
    WF_TRY_RC(hand_over(h, s, h->ev_copied[slot], count));
    hipLaunchKernelGGL(wf::rms_feed_ragged_kernel, dim3(count), dim3(256), 0, h->stream, h->d_rms_ring, h->d_rms_bsum, h->d_rend, h->rms_cap, first,
                       s.d_stage, s.d_frames, max_frames);
    WF_HIP_TRY(h, hipGetLastError());
    WF_TRY_RC(slot_consumed(h, s));
    h->main_dirty = true;
    return WF_HIP_OK;
}

int wf_hip_sync(wf_hip *h)
{
    if(h == nullptr)
        return WF_HIP_ERR_INVALID;
    WF_HIP_TRY(h, hipSetDevice(h->device));
    WF_TRY_RC(join_lanes(h));
    WF_HIP_TRY(h, hipStreamSynchronize(h->stream));
    if(h->canary) { // (everything that can write has drained: the side streams too)
        if(h->copy_stream) WF_HIP_TRY(h, hipStreamSynchronize(h->copy_stream));
        if(h->read_stream) WF_HIP_TRY(h, hipStreamSynchronize(h->read_stream));
        return check_canaries(h);
    }
    return WF_HIP_OK;
}

uint32_t wf_hip_num_vertices(const wf_hip *h) { return (h && h->d_verts) ? (uint32_t)h->small->vertex.per_row : 0u; }

const float *wf_hip_vertices_device(wf_hip *h)
{
    if(h == nullptr || h->d_verts == nullptr)
        return nullptr;
    (void)join_lanes(h);
    return reinterpret_cast<const float *>(h->d_verts);
}

// where an output other than a measurement lives on the device and how large it is per stream; nullptr + a text when the
// batch has none
static const void *output_source(const wf_hip *h, wf_hip_output what, size_t *per_stream, const char **why)
{
    *per_stream = 0;
    *why = "";
    switch(what) {
    case WF_HIP_OUT_DECIBELS:
        if(h->meter) { *why = "meter batch: there is no m_decibels; read the levels (WF_HIP_OUT_METER)"; return nullptr; }
        *per_stream = (size_t)h->out_ch * h->M * sizeof(float);
        return h->d_decibels;
    case WF_HIP_OUT_BARS:
        if(h->d_bars == nullptr) { *why = "configuration has no bars (cfg.bars == 0 and cfg.curve == 0)"; return nullptr; }
        *per_stream = (size_t)h->disp_ch * h->num_bars * sizeof(float);
        return h->d_bars;
    case WF_HIP_OUT_PREMIRROR:
        if(h->d_bars_pre == nullptr) { *why = "the configuration has no mirrored display (cfg.mirror_freq_axis == 0, or no bars / curve)"; return nullptr; }
        *per_stream = (size_t)h->disp_ch * sizeof(float);
        return h->d_bars_pre;
    case WF_HIP_OUT_VERTICES:
        if(h->d_verts == nullptr) { *why = "configuration has no vertex fill (cfg.vertices == 0)"; return nullptr; }
        *per_stream = (size_t)h->disp_ch * h->small->vertex.per_row * sizeof(wf::f4);
        return h->d_verts;
    case WF_HIP_OUT_VERTEX_COUNTS:
        if(h->d_vert_counts == nullptr) { *why = "configuration has no vertex fill (cfg.vertices == 0)"; return nullptr; }
        *per_stream = (size_t)h->disp_ch * sizeof(uint32_t);
        return h->d_vert_counts;
    case WF_HIP_OUT_LAST_SILENT:
        *per_stream = sizeof(uint8_t); // (read as flag words, narrowed on the host)
        return h->d_flags;
    case WF_HIP_OUT_TSMOOTH:
        if(h->meter || h->wave) { *why = "meter / waveform batch: there is no m_tsmooth_buf"; return nullptr; }
        *per_stream = (size_t)h->cap_ch * h->M * sizeof(float);
        return h->d_tsmooth;
    case WF_HIP_OUT_METER:
        if(!h->meter) { *why = "not a meter batch (cfg.meter == 0)"; return nullptr; }
        *per_stream = (size_t)h->cap_ch * sizeof(float);
        return h->d_meter_val;
    case WF_HIP_OUT_INPUT_RMS:
        if(h->d_input_rms == nullptr) { *why = "the device RMS producer is not enabled (wf_hip_enable_input_rms)"; return nullptr; }
        *per_stream = sizeof(float);
        return h->d_input_rms;
    case WF_HIP_OUT_WAVEFORM_TS:
        if(!h->wave || h->d_wts == nullptr) { *why = "m_waveform_ts belongs to waveform batches"; return nullptr; }
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t));
        *per_stream = sizeof(uint64_t);
        return h->d_wts;
    case WF_HIP_OUT_LOUDNESS:
    case WF_HIP_OUT_PEAKS:
    case WF_HIP_OUT_SIGNAL:
    case WF_HIP_OUT_PITCH:
    case WF_HIP_OUT_BANDS:
    case WF_HIP_OUT_STEREO:
    case WF_HIP_OUT_CQ:
    case WF_HIP_OUT_SCOPE:
    case WF_HIP_OUT_GONIO:
    case WF_HIP_OUT_SONO:
    case WF_HIP_OUT_BITS:
    case WF_HIP_OUT_THD:
    case WF_HIP_OUT_DELAY:
    case WF_HIP_OUT_ONSET:
    case WF_HIP_OUT_XFER:
    case WF_HIP_OUT_IMPULSE:
    case WF_HIP_OUT_CLICK:
    case WF_HIP_OUT_IMD:
    case WF_HIP_OUT_TEMPO:
    case WF_HIP_OUT_HUM:
        break; // (never asked here: measure_source answers for them)
    }
    *why = "unknown output";
    return nullptr;
}

size_t wf_hip_output_bytes(const wf_hip *h, wf_hip_output what)
{
    if(h == nullptr)
        return 0;
    size_t per = 0;
    const char *why = nullptr;
    if(measure_source(h, what, &per, &why))
        return per;
    return output_source(h, what, &per, &why) ? per : 0;
}

int wf_hip_read(wf_hip *h, wf_hip_output what, uint32_t first, uint32_t count, void *out)
{
    WF_TRY_RC(check_range(h, first, count));
    size_t per = 0;
    const char *why = nullptr;
    if(measure_source(h, what, &per, &why))
        return measure_read(h, what, first, count, out);
    const void *src = output_source(h, what, &per, &why);
    if(src == nullptr)
        return fail(h, WF_HIP_ERR_INVALID, "%s", why);
    if(out == nullptr)
        return fail(h, WF_HIP_ERR_INVALID, "output pointer is NULL");
    if(what == WF_HIP_OUT_LAST_SILENT) { // the flag words of the buffer the newest tick wrote, narrowed to one byte per stream
        std::vector<uint32_t> tmp(count);
        WF_TRY_RC(read_back(h, cur_flags(h) + first, tmp.data(), count * sizeof(uint32_t)));
        for(uint32_t i = 0; i < count; ++i)
            static_cast<uint8_t *>(out)[i] = (tmp[i] & wf::WF_STREAM_LAST_SILENT) ? 1 : 0;
        return WF_HIP_OK;
    }
    return read_back(h, static_cast<const char *>(src) + (size_t)first * per, out, (size_t)count * per);
}

// ---- wf_hip_read_async (the slots' helpers: "pipelined readback" above) ---------------------------------------------------
// every output the caller named is one the batch has, or the call is refused with the text wf_hip_read gives for that output:
// before anything is enqueued or any state of the slot changes
static int check_outputs(wf_hip *h, const wf_hip_readback *dst)
{
    const std::pair<const void *, wf_hip_output> named[] = {
        {dst->rows, WF_HIP_OUT_DECIBELS},     {dst->meter, WF_HIP_OUT_METER},       {dst->bars, WF_HIP_OUT_BARS},
        {dst->premirror, WF_HIP_OUT_PREMIRROR}, {dst->vertices, WF_HIP_OUT_VERTICES}, {dst->vertex_counts, WF_HIP_OUT_VERTEX_COUNTS},
        {dst->input_rms, WF_HIP_OUT_INPUT_RMS}};
    for(const auto &o : named) {
        size_t per = 0;
        const char *why = nullptr;
        if(o.first && output_source(h, o.second, &per, &why) == nullptr)
            return fail(h, WF_HIP_ERR_INVALID, "%s", why);
    }
    return WF_HIP_OK;
}

// m_last_silent of streams [first, first+count) as bytes (for the D2H copy of wf_hip_read_async's rows and meter levels)
__global__ void silent_bytes_kernel(const uint32_t *flags, uint32_t first, uint32_t count, uint8_t *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i < count)
        out[i] = (flags[first + i] & wf::WF_STREAM_LAST_SILENT) ? 1 : 0;
}

static int silent_bytes(wf_hip *h, uint32_t first, uint32_t count, wf_hip::ReadSlot &s)
{
    hipLaunchKernelGGL(silent_bytes_kernel, dim3((count + 255) / 256), dim3(256), 0, h->stream, cur_flags(h), first, count, s.d_silent);
    WF_HIP_TRY(h, hipGetLastError());
    return WF_HIP_OK;
}

// the bars alone: from a snapshot behind the ticks enqueued so far (device to device, a few MB at most), so that later ticks
// neither wait for the D2H copy nor disturb it
static int read_bars_snapshot_async(wf_hip *h, uint32_t first, uint32_t count, float *pinned_out, wf_hip::ReadSlot &s)
{
    const size_t per = (size_t)h->disp_ch * h->num_bars, n = count * per;
    WF_TRY_RC(read_slot_ready(h, s, n, 0));
    WF_HIP_TRY(h, hipMemcpyAsync(s.d_snap, h->d_bars + first * per, n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    WF_TRY_RC(to_read_stream(h, s));
    return copies_issued(h, s, false, copy_out(h, pinned_out, s.d_snap, n * sizeof(float)));
}

// meter batches: the levels from a snapshot of the few floats (the next tick overwrites m_meter_val) + m_last_silent
static int read_meter_async(wf_hip *h, uint32_t first, uint32_t count, float *pinned_levels, uint8_t *pinned_last_silent, wf_hip::ReadSlot &s)
{
    const size_t n = (size_t)count * h->cap_ch;
    WF_TRY_RC(read_slot_ready(h, s, n, count));
    WF_HIP_TRY(h, hipMemcpyAsync(s.d_snap, h->d_meter_val + (size_t)first * h->cap_ch, n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    WF_TRY_RC(silent_bytes(h, first, count, s));
    WF_TRY_RC(to_read_stream(h, s));
    int rc = copy_out(h, pinned_levels, s.d_snap, n * sizeof(float));
    if(rc == WF_HIP_OK)
        rc = copy_out(h, pinned_last_silent, s.d_silent, count);
    return copies_issued(h, s, false, rc);
}

// The copies of a rows readback: the rows straight out of m_decibels, m_last_silent, then the riders -- m_input_rms, the bars, the
// vertices and their counts, the points in front of the mirror -- from where the tick, its vertex fill and the RMS producer left
// them (the readback stream waits for all of them on every lane; check_outputs has made sure the batch has them)
static int rows_copies(wf_hip *h, uint32_t first, uint32_t count, const wf_hip_readback *dst, const wf_hip::ReadSlot &s)
{
    const size_t per = (size_t)h->out_ch * h->M, bars = (size_t)h->disp_ch * h->num_bars;
    WF_TRY_RC(copy_out(h, dst->rows, h->d_decibels + first * per, count * per * sizeof(float)));
    WF_TRY_RC(copy_out(h, dst->last_silent, s.d_silent, count));
    if(dst->input_rms)
        WF_TRY_RC(copy_out(h, dst->input_rms, h->d_input_rms + first, (size_t)count * sizeof(float)));
    if(dst->bars)
        WF_TRY_RC(copy_out(h, dst->bars, h->d_bars + first * bars, count * bars * sizeof(float)));
    if(dst->vertices) {
        const size_t pv = (size_t)h->disp_ch * h->small->vertex.per_row;
        WF_TRY_RC(copy_out(h, dst->vertices, h->d_verts + first * pv, count * pv * sizeof(wf::f4)));
    }
    if(dst->vertex_counts)
        WF_TRY_RC(copy_out(h, dst->vertex_counts, h->d_vert_counts + (size_t)first * h->disp_ch, (size_t)count * h->disp_ch * sizeof(uint32_t)));
    if(dst->premirror)
        WF_TRY_RC(copy_out(h, dst->premirror, h->d_bars_pre + (size_t)first * h->disp_ch, (size_t)count * h->disp_ch * sizeof(float)));
    return WF_HIP_OK;
}

static int read_rows_async(wf_hip *h, uint32_t first, uint32_t count, const wf_hip_readback *dst, wf_hip::ReadSlot &s)
{
    WF_TRY_RC(read_slot_ready(h, s, 0, count));
    WF_TRY_RC(silent_bytes(h, first, count, s));
    WF_TRY_RC(to_read_stream(h, s));
    return copies_issued(h, s, true, rows_copies(h, first, count, dst, s));
}

int wf_hip_read_async(wf_hip *h, uint32_t first, uint32_t count, const wf_hip_readback *dst, uint32_t slot)
{
    WF_TRY_RC(check_range(h, first, count));
    if(dst == nullptr || slot > 1)
        return fail(h, WF_HIP_ERR_INVALID, "destination set is NULL or slot is not 0 / 1");
    const bool riders = dst->premirror || dst->vertices || dst->vertex_counts || dst->input_rms;
    if(dst->meter) {
        if(dst->last_silent == nullptr || dst->rows || dst->bars || riders)
            return fail(h, WF_HIP_ERR_INVALID, "wf_hip_read_async: meter goes with last_silent and nothing else");
    } else if(dst->rows == nullptr) {
        if(dst->bars == nullptr || dst->last_silent || riders)
            return fail(h, WF_HIP_ERR_INVALID, "wf_hip_read_async: without rows only the bars can be read (rows + last_silent lead every other combination)");
    } else if(dst->last_silent == nullptr)
        return fail(h, WF_HIP_ERR_INVALID, "wf_hip_read_async: rows go with last_silent");
    WF_TRY_RC(check_outputs(h, dst));
    WF_HIP_TRY(h, hipSetDevice(h->device));
    wf_hip::ReadSlot &s = h->read_slot[slot];
    if(dst->meter)
        return read_meter_async(h, first, count, dst->meter, dst->last_silent, s);
    if(dst->rows == nullptr)
        return read_bars_snapshot_async(h, first, count, dst->bars, s);
    return read_rows_async(h, first, count, dst, s);
}

int wf_hip_readback_done(wf_hip *h, uint32_t slot)
{
    if(h == nullptr || slot > 1)
        return WF_HIP_ERR_INVALID;
    if(!h->read_slot[slot].used)
        return WF_HIP_OK;
    WF_HIP_TRY(h, hipSetDevice(h->device));
    WF_HIP_TRY(h, hipEventSynchronize(h->read_slot[slot].ev_read));
    return WF_HIP_OK;
}

int wf_hip_copy_bars_device_async(wf_hip *h, uint32_t first, uint32_t count, void *d_out, void *consumer_stream)
{
    if(h == nullptr)
        return WF_HIP_ERR_INVALID;
    if(count == 0 || first >= h->n_streams || count > h->n_streams - first)
        return fail(h, WF_HIP_ERR_INVALID, "stream range [%u, %u+%u) outside 0..%u", first, first, count, h->n_streams);
    if(h->d_bars == nullptr)
        return fail(h, WF_HIP_ERR_INVALID, "configuration has no bars (cfg.bars == 0 and cfg.curve == 0)");
    if(d_out == nullptr || consumer_stream == nullptr)
        return fail(h, WF_HIP_ERR_INVALID, "output pointer or consumer stream is NULL");
    const size_t per = (size_t)h->disp_ch * h->num_bars;
    WF_HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t cs = static_cast<hipStream_t>(consumer_stream);
    // The lanes are NOT joined: a join would put the next tick's lanes behind the handle's stream again and take away the
    // overlap of one tick's tail with the next one's head (measured: 110 -> 143 us per tick at 8192 streams).  Every lane
    // copies the bars of its own slice on its own stream, behind the tick it has just run and in front of its next one.
    const int lanes = h->lanes_pending ? h->n_lanes : 1;
    for(int l = 0; l < lanes; ++l) {
        const uint32_t lo = lanes == 1 ? 0u : (uint32_t)((uint64_t)h->n_streams * l / lanes);
        const uint32_t hi = lanes == 1 ? h->n_streams : (uint32_t)((uint64_t)h->n_streams * (l + 1) / lanes);
        const uint32_t a = std::max(lo, first), b = std::min(hi, first + count);
        if(a >= b)
            continue;
        hipStream_t st = l == 0 ? h->stream : h->lane_stream[l];
        if(h->ev_bars_lane[l] == nullptr)
            WF_HIP_TRY(h, hipEventCreateWithFlags(&h->ev_bars_lane[l], hipEventDisableTiming));
        WF_HIP_TRY(h, hipMemcpyAsync(static_cast<float *>(d_out) + (size_t)(a - first) * per, h->d_bars + (size_t)a * per,
                                     (size_t)(b - a) * per * sizeof(float), hipMemcpyDeviceToDevice, st));
        WF_HIP_TRY(h, hipEventRecord(h->ev_bars_lane[l], st));
        WF_HIP_TRY(h, hipStreamWaitEvent(cs, h->ev_bars_lane[l], 0));
    }
    return WF_HIP_OK;
}

int wf_hip_set_bars_mirrors(wf_hip *h, uint32_t n, void *const *d_out0, void *const *d_out1)
{
    if(h == nullptr)
        return WF_HIP_ERR_INVALID;
    if(n > 8 || (n > 0 && (d_out0 == nullptr || d_out1 == nullptr)))
        return fail(h, WF_HIP_ERR_INVALID, "wf_hip_set_bars_mirrors: at most 8 buffers per set, both sets given");
    if(n > 0) {
        if(h->d_bars == nullptr || h->meter || h->wave)
            return fail(h, WF_HIP_ERR_INVALID, "configuration has no bars (cfg.bars == 0 and cfg.curve == 0, or a level-meter / waveform batch)");
        if(h->disp.ext_outputs || h->plan.big_l != 0 || h->plan.blu)
            return fail(h, WF_HIP_ERR_UNSUPPORTED, "fft_size %u: only the power-of-two sizes up to 32768 whose display the tick kernel finishes itself write further bars buffers; copy the bars with wf_hip_copy_bars_device_async", h->N);
        for(uint32_t j = 0; j < n; ++j)
            if(d_out0[j] == nullptr || d_out1[j] == nullptr || d_out0[j] == d_out1[j] || d_out0[j] == (void *)h->d_bars || d_out1[j] == (void *)h->d_bars)
                return fail(h, WF_HIP_ERR_INVALID, "wf_hip_set_bars_mirrors: buffer %u of a set is NULL, the same in both sets or the handle's own", j);
    }
    // ticks still in flight write the old buffers: they must have run before the sets are replaced (and the caller frees them)
    if(h->mirror_n) {
        WF_HIP_TRY(h, hipSetDevice(h->device));
        WF_HIP_TRY(h, hipStreamSynchronize(h->stream));
        for(int l = 1; l < h->n_lanes; ++l)
            if(h->lane_stream[l])
                WF_HIP_TRY(h, hipStreamSynchronize(h->lane_stream[l]));
    }
    for(uint32_t j = 0; j < 8; ++j) {
        h->bars_mirror[0][j] = j < n ? static_cast<float *>(d_out0[j]) : nullptr;
        h->bars_mirror[1][j] = j < n ? static_cast<float *>(d_out1[j]) : nullptr;
    }
    h->mirror_n = n;
    h->mirror_next = 0;
    h->mirror_fresh = false;
    return WF_HIP_OK;
}

int wf_hip_bars_mirror_ready(wf_hip *h, void *consumer_stream, void **d_out)
{
    if(h == nullptr || d_out == nullptr)
        return WF_HIP_ERR_INVALID;
    if(h->mirror_n == 0)
        return fail(h, WF_HIP_ERR_INVALID, "no mirror buffers set (wf_hip_set_bars_mirrors)");
    if(consumer_stream == nullptr)
        return fail(h, WF_HIP_ERR_INVALID, "consumer stream is NULL");
    float *const *set = h->bars_mirror[h->mirror_next];
    WF_HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t cs = static_cast<hipStream_t>(consumer_stream);
    const size_t per = (size_t)h->disp_ch * h->num_bars;
    // as wf_hip_copy_bars_device_async: the lanes are not joined -- the consumer waits for each of them
    const int lanes = h->lanes_pending ? h->n_lanes : 1;
    for(int l = 0; l < lanes; ++l) {
        hipStream_t st = l == 0 ? h->stream : h->lane_stream[l];
        if(h->ev_bars_lane[l] == nullptr)
            WF_HIP_TRY(h, hipEventCreateWithFlags(&h->ev_bars_lane[l], hipEventDisableTiming));
        if(!h->mirror_fresh) {
            // no tick has written this set: the handle's own bars stand in (each lane copies the slice its ticks write)
            const uint32_t lo = lanes == 1 ? 0u : (uint32_t)((uint64_t)h->n_streams * l / lanes);
            const uint32_t hi = lanes == 1 ? h->n_streams : (uint32_t)((uint64_t)h->n_streams * (l + 1) / lanes);
            for(uint32_t j = 0; j < h->mirror_n && hi > lo; ++j)
                WF_HIP_TRY(h, hipMemcpyAsync(set[j] + (size_t)lo * per, h->d_bars + (size_t)lo * per, (size_t)(hi - lo) * per * sizeof(float), hipMemcpyDefault, st));
        }
        WF_HIP_TRY(h, hipEventRecord(h->ev_bars_lane[l], st));
        WF_HIP_TRY(h, hipStreamWaitEvent(cs, h->ev_bars_lane[l], 0));
    }
    *d_out = set[0];
    h->mirror_next ^= 1u;
    h->mirror_fresh = false;
    return WF_HIP_OK;
}

int wf_hip_wait_event(wf_hip *h, void *event)
{
    if(h == nullptr || event == nullptr)
        return WF_HIP_ERR_INVALID;
    WF_HIP_TRY(h, hipSetDevice(h->device));
    hipEvent_t ev = static_cast<hipEvent_t>(event);
    WF_HIP_TRY(h, hipStreamWaitEvent(h->stream, ev, 0));
    for(int l = 1; l < h->n_lanes; ++l)
        if(h->lane_stream[l])
            WF_HIP_TRY(h, hipStreamWaitEvent(h->lane_stream[l], ev, 0));
    return WF_HIP_OK;
}

int wf_hip_write_tsmooth(wf_hip *h, uint32_t first, uint32_t count, const float *in)
{
    int rc = check_range(h, first, count);
    if(rc)
        return rc;
    if(in == nullptr)
        return fail(h, WF_HIP_ERR_INVALID, "input pointer is NULL");
    if(h->meter || h->wave)
        return fail(h, WF_HIP_ERR_INVALID, "meter / waveform batch: there is no m_tsmooth_buf");
    const size_t per = (size_t)h->cap_ch * h->M;
    WF_HIP_TRY(h, hipSetDevice(h->device));
    WF_HIP_TRY(h, hipMemcpyAsync(h->d_tsmooth + first * per, in, count * per * sizeof(float), hipMemcpyHostToDevice, h->stream));
    WF_HIP_TRY(h, hipStreamSynchronize(h->stream));
    return WF_HIP_OK;
}

float *wf_hip_decibels_device(wf_hip *h) { return h ? h->d_decibels : nullptr; }
float *wf_hip_bars_device(wf_hip *h) { return h ? h->d_bars : nullptr; }
void *wf_hip_stream(wf_hip *h)
{
    if(h == nullptr)
        return nullptr;
    (void)join_lanes(h); // whatever the caller orders behind this stream is ordered behind every tick enqueued so far
    return (void *)h->stream;
}

size_t wf_hip_table(const wf_hip *h, wf_hip_table_id which, const void **out)
{
    if(out)
        *out = nullptr;
    if(h == nullptr)
        return 0;
    auto give = [&](const auto &v) -> size_t {
        if(out)
            *out = v.empty() ? nullptr : static_cast<const void *>(v.data());
        return v.size();
    };
    switch(which) {
    case WF_HIP_TABLE_WINDOW: return give(h->tab.window);
    case WF_HIP_TABLE_WINDOW_SUM:
        if(out)
            *out = &h->tab.window_sum;
        return 1;
    case WF_HIP_TABLE_SLOPE: return give(h->tab.slope);
    case WF_HIP_TABLE_ROLLOFF: return give(h->tab.rolloff);
    case WF_HIP_TABLE_INTERP_INDICES: return give(h->tab.interp_indices);
    case WF_HIP_TABLE_BAND_WIDTHS: return give(h->tab.band_widths);
    case WF_HIP_TABLE_INTERP_WEIGHTS: return give(h->tab.interp_weights);
    case WF_HIP_TABLE_INTERP_SHAPE:
        if(out)
            *out = h->interp_shape;
        return 2;
    }
    return 0;
}
float wf_hip_gravity(const wf_hip *h, float seconds) { return wf::gravity_for(h->cfg, seconds); }
float wf_hip_db_min(void) { return wf::db_min(); }

int wf_hip_time_begin(wf_hip *h)
{
    if(h == nullptr)
        return WF_HIP_ERR_INVALID;
    WF_HIP_TRY(h, hipSetDevice(h->device));
    WF_TRY_RC(join_lanes(h));
    WF_HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    return WF_HIP_OK;
}

int wf_hip_time_end(wf_hip *h, float *elapsed_ms)
{
    if(h == nullptr || elapsed_ms == nullptr)
        return WF_HIP_ERR_INVALID;
    WF_HIP_TRY(h, hipSetDevice(h->device));
    WF_TRY_RC(join_lanes(h));
    WF_HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    WF_HIP_TRY(h, hipEventSynchronize(h->ev1));
    WF_HIP_TRY(h, hipEventElapsedTime(elapsed_ms, h->ev0, h->ev1));
    return WF_HIP_OK;
}

int wf_hip_time_ticks(wf_hip *h, const wf_hip_tick_params *p, uint32_t ticks, uint32_t hop, float *avg_kernel_ms)
{
    if(h == nullptr || p == nullptr || ticks == 0 || avg_kernel_ms == nullptr)
        return WF_HIP_ERR_INVALID;
    // the walk starts over at the oldest window when it has reached the newest sample
    const uint32_t period = hop ? p->delay_frames / hop + 1 : ticks;
    WF_HIP_TRY(h, hipSetDevice(h->device));
    WF_TRY_RC(join_lanes(h));
    // events recorded on the handle's own stream, around the fused kernels only (the lanes fork behind ev0 and are joined
    // in front of ev1)
    WF_HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    wf_hip_tick_params q = *p;
    for(uint32_t i = 0; i < ticks; ++i) {
        q.delay_frames = p->delay_frames - (i % period) * hop;
        int rc = wf_hip_tick(h, &q);
        if(rc)
            return rc;
    }
    WF_TRY_RC(join_lanes(h));
    WF_HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    WF_HIP_TRY(h, hipEventSynchronize(h->ev1));
    float ms = 0.0f;
    WF_HIP_TRY(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    *avg_kernel_ms = ms / (float)ticks;
    return WF_HIP_OK;
}

// Test aid: the streams' sample counters (write position, RMS / meter / waveform consumption points) move on by `frames`, as
// if that much more audio had been captured before what the rings hold now -- `frames` must be a multiple of every ring
// capacity, so that positions keep addressing the same ring cells.  Lets a test reach the 2^32-sample wrap-around (a day
// of audio at 48 kHz) without pushing a day of audio.
#ifdef WF_DEV_BUILD
extern "C" int wf_hip_debug_age(wf_hip *h, uint32_t first, uint32_t count, uint32_t frames)
{
    int rc = check_range(h, first, count);
    if(rc)
        return rc;
    if(frames % h->ring_cap || (h->d_rms_ring && frames % h->rms_cap))
        return fail(h, WF_HIP_ERR_INVALID, "frames must be a multiple of the ring capacity %u%s", h->ring_cap, h->d_rms_ring ? " and of the RMS ring's" : "");
    WF_HIP_TRY(h, hipSetDevice(h->device));
    WF_TRY_RC(join_lanes(h));
    hipLaunchKernelGGL(wf::age_kernel, dim3((count + 255) / 256), dim3(256), 0, h->stream, h->d_wpos, h->d_rend, h->d_mend, h->d_cend, first, count,
                       frames);
    WF_HIP_TRY(h, hipGetLastError());
    h->main_dirty = true;
    return WF_HIP_OK;
}
#endif

#ifdef WF_PHASE_TIMING
// development aid: copies the per-workgroup s_memtime stamps of the last tick (16 per workgroup)
extern "C" int wf_hip_debug_phase_clock(wf_hip *h, unsigned long long *out, size_t n)
{
    if(hipMemcpy(out, h->tick.phase_clock, n * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess)
        return WF_HIP_ERR_RUNTIME;
    return WF_HIP_OK;
}
#endif

const char *wf_hip_kernel_name(const wf_hip *h) { return h ? h->kernel_name.c_str() : ""; }

uint32_t wf_hip_launches_per_tick(const wf_hip *h)
{
    if(h == nullptr)
        return 0;
    if(h->wave || h->meter)
        return 1;
    return (uint32_t)(h->d_rms_ring ? 1 : h->n_lanes) * (h->plan.split_mono ? 2u : 1u);
}

uint64_t wf_hip_algorithmic_bytes_per_tick(const wf_hip *h, uint32_t flags)
{
    if(h == nullptr)
        return 0;
    if(h->wave) // read + write every row (the shift), plus the samples picked from the rings (not counted: <= width per row)
        return (uint64_t)h->n_streams * h->out_ch * h->N * 8ull;
    if(h->meter) // read the meter buffer of every captured channel; state, level and bar are a few floats per channel
        return (uint64_t)h->n_streams * h->cap_ch * (4ull * h->N + 20ull);
    // read the N-sample window of every captured channel, read + write the smoothing
    // state (M floats each way) when temporal smoothing is on, write M dB values per displayed/output channel
    // (stereo: both channels; mono mixdown: one), plus the bar heights when the configuration has bars.
    const uint64_t n_spec = (uint64_t)h->n_streams * h->cap_ch;
    uint64_t bytes = n_spec * 4ull * h->N;
    if(h->cfg.tsmoothing != WF_TSMOOTH_NONE)
        bytes += n_spec * 8ull * h->M;
    const bool mono_mix = !h->cfg.stereo && h->cap_ch > 1;
    const uint64_t out_rows = (uint64_t)h->n_streams * (mono_mix ? 1u : h->out_ch);
    if(!(flags & WF_HIP_TICK_NO_DECIBELS) || mono_mix || h->plan.big_l || h->disp.ext_outputs) // the mono-mixdown row is stored in either mode;
                                                                                       // so are rows the outputs are derived from
        bytes += out_rows * 4ull * h->M;
    bytes += (uint64_t)h->n_streams * h->disp_ch * h->num_bars * 4ull;
    return bytes;
}

} // extern "C"
