/*
 * wav_source_hip.cpp -- see wav_source_hip.hpp.  Reference-side binding (compiled with the plugin, or here with the
 * oracle harness).  libwaveform_hip.so is loaded with dlopen so that the plugin still loads on machines without it;
 * when it is missing, or no gfx950 device is present, every call falls through to WAVSourceGeneric -- the reference's
 * own CPU path -- which is the reference's failure style (degrade and log, never throw across the C boundary,
 * src/source_generic.cpp:105-108).
 */
#include "wav_source_hip.hpp"
#include "log.hpp"

#include <dlfcn.h>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>

namespace {

struct HipApi {
    void *lib = nullptr;
    decltype(&wf_hip_device_count) device_count = nullptr;
    decltype(&wf_hip_create) create = nullptr;
    decltype(&wf_hip_destroy) destroy = nullptr;
    decltype(&wf_hip_push_audio) push_audio = nullptr;
    decltype(&wf_hip_tick) tick = nullptr;
    decltype(&wf_hip_set_hidden) set_hidden = nullptr;
    decltype(&wf_hip_read) read = nullptr;
    decltype(&wf_hip_read_async) read_async = nullptr;
    decltype(&wf_hip_enable_input_rms) enable_input_rms = nullptr;
    decltype(&wf_hip_last_error) last_error = nullptr;
    decltype(&wf_hip_reset) reset = nullptr;
    decltype(&wf_hip_push_audio_ragged_async) push_audio_ragged_async = nullptr;
    decltype(&wf_hip_ingest_done) ingest_done = nullptr;
    decltype(&wf_hip_readback_done) readback_done = nullptr;
    decltype(&wf_hip_set_input_rms) set_input_rms = nullptr;
    decltype(&wf_hip_host_alloc) host_alloc = nullptr;
    decltype(&wf_hip_host_free) host_free = nullptr;
    decltype(&wf_hip_push_rms_ragged_async) push_rms_ragged_async = nullptr;
    decltype(&wf_hip_set_stream_delay) set_stream_delay = nullptr;
    decltype(&wf_hip_set_stream_audio_ts) set_stream_audio_ts = nullptr;
    decltype(&wf_hip_output_channels) output_channels = nullptr;
    decltype(&wf_hip_num_vertices) num_vertices = nullptr;
    decltype(&wf_hip_num_bars) num_bars = nullptr;
    decltype(&wf_hip_display_channels) display_channels = nullptr;
    decltype(&wf_hip_ring_frames) ring_frames = nullptr;
    bool ok = false;
};

HipApi &api()
{
    static HipApi a;
    static std::once_flag once;
    std::call_once(once, [] {
        const char *path = std::getenv("WF_HIP_LIBRARY");
        a.lib = dlopen(path ? path : "libwaveform_hip.so", RTLD_NOW | RTLD_LOCAL);
        if(a.lib == nullptr)
            return;
#define WF_SYM(name)                                                           \
    a.name = reinterpret_cast<decltype(a.name)>(dlsym(a.lib, "wf_hip_" #name)); \
    if(a.name == nullptr)                                                      \
        return;
        WF_SYM(device_count)
        WF_SYM(create)
        WF_SYM(destroy)
        WF_SYM(push_audio)
        WF_SYM(tick)
        WF_SYM(set_hidden)
        WF_SYM(read)
        WF_SYM(read_async)
        WF_SYM(enable_input_rms)
        WF_SYM(last_error)
        WF_SYM(reset)
        WF_SYM(push_audio_ragged_async)
        WF_SYM(ingest_done)
        WF_SYM(readback_done)
        WF_SYM(set_input_rms)
        WF_SYM(host_alloc)
        WF_SYM(host_free)
        WF_SYM(push_rms_ragged_async)
        WF_SYM(set_stream_delay)
        WF_SYM(set_stream_audio_ts)
        WF_SYM(output_channels)
        WF_SYM(num_vertices)
        WF_SYM(num_bars)
        WF_SYM(display_channels)
        WF_SYM(ring_frames)
#undef WF_SYM
        // struct wf_config and the entry points above must be the ones this file was compiled against
        auto abi = reinterpret_cast<decltype(&wf_hip_abi_version)>(dlsym(a.lib, "wf_hip_abi_version"));
        if(abi == nullptr || abi() != WF_HIP_ABI_VERSION)
            return;
        a.ok = true;
    });
    return a;
}

std::atomic<uint64_t> g_fallback_ticks{0};
std::atomic<uint64_t> g_host_rms_updates{0}; // update_input_rms calls that ran the reference's host loop
std::atomic<uint64_t> g_device_renders{0}, g_host_renders{0}; // render() of HIP-configured spectrum sources: from the device / by the reference's loops

bool device_render_mode()
{
    const char *e = std::getenv("WF_HIP_RENDER"); // 0: the reference's render() keeps interpolating and filling vertices on the host
    return e == nullptr || e[0] != '0';
}

bool batched_mode()
{
    const char *e = std::getenv("WF_HIP_BATCHED"); // 0: every source its own handle, results inside the call
    return e == nullptr || e[0] != '0';
}

uint32_t group_capacity()
{
    const char *e = std::getenv("WF_HIP_BATCH_CAPACITY");
    const long v = e ? std::atol(e) : 64;
    return (uint32_t)std::min<long>(std::max<long>(v, 1), 16384);
}

// WF_HIP_DEVICE pins everything to one device; -1: not set
int pinned_device()
{
    const char *e = std::getenv("WF_HIP_DEVICE");
    return e ? std::min(std::max(std::atoi(e), 0), std::max(api().device_count(), 1) - 1) : -1;
}

// does the handle produce the display its configuration asks for (cfg.bars / cfg.curve with cfg.vertices), and in what shape:
// displayed channels, outputs per row, vertices per row (0 for a curve: its points come back, the strip is written on the host)
bool display_shape(const wf_config &c, wf_hip *h, uint32_t &disp_ch, uint32_t &points, uint32_t &per_row)
{
    auto &a = api();
    if(!((c.bars != 0 || c.curve != 0) && a.num_bars(h) > 0 && (c.curve != 0 || a.num_vertices(h) > 0)))
        return false;
    disp_ch = a.display_channels(h);
    points = a.num_bars(h);
    per_row = a.num_vertices(h);
    return true;
}

template<class T>
bool host_alloc(T *&p, size_t count)
{
    p = static_cast<T *>(api().host_alloc(count * sizeof(T)));
    return p != nullptr;
}

template<class T>
void host_free(T *p)
{
    if(p)
        api().host_free(p);
}

} // namespace

// What the two kinds of group share: one handle for the sources of one configuration -- sources are streams of its batch --,
// who sits in which slot, and the hand-over of a video frame.
//
// A video frame, seen from the group: OBS ticks its active sources one after the other on the video thread
// (reference callbacks::tick, src/source.cpp:481-484).  Every member's tick
//   1. collects: copies its part of the PREVIOUS frame's tick out of the page-locked readback buffer (one frame of latency:
//      the copy was enqueued 16 ms ago and has long landed; begin_tick), and
//   2. submits: what its own tick would consume this frame goes into the batch being assembled, with its show / hide / timeout
//      state (submit).
// The member that completes the frame -- or one that comes round again while an incomplete batch is waiting -- flushes:
// the state masks that changed (begin_flush), then what the group type stages: ONE ragged ingest, ONE wf_hip_tick, ONE readback
// (wf_hip_read_async); members that did not show up are paused for that tick.  Nothing in a flush waits for the device.
struct WFHipGroupCore {
    wf_config cfg{};
    wf_hip *h = nullptr;
    int device = 0;
    const char *kind = "spectrum";        // for the log
    uint32_t capacity = 0;
    std::vector<WAVSourceHIP *> member;   // [capacity] or nullptr
    uint32_t members = 0;
    uint64_t batch = 1;                   // the batch being assembled (batch - 1: the last one flushed)
    std::vector<uint64_t> submitted;      // [capacity] the batch a member last submitted to
    uint32_t n_submitted = 0;
    std::vector<uint32_t> frames;         // [capacity] frames each member staged for this batch
    std::vector<uint8_t> state, state_dev;
    uint8_t *silent[2] = {nullptr, nullptr}; // page-locked [capacity], allocated by the group type among its own buffers
    bool valid[2] = {false, false};       // the readback of that slot was enqueued: its results may be collected
    float seconds = 1.0f / 60.0f;
    bool failed = false;

    // the handle and the bookkeeping of its slots; the group type's create() adds its buffers
    bool open(const wf_config &c, int dev)
    {
        cfg = c;
        device = dev;
        capacity = group_capacity();
        if(api().create(&c, dev, capacity, 0, &h) != WF_HIP_OK) {
            h = nullptr;
            return false;
        }
        member.assign(capacity, nullptr);
        submitted.assign(capacity, 0);
        frames.assign(capacity, 0);
        state.assign(capacity, WF_HIP_PAUSED);
        state_dev.assign(capacity, WF_HIP_SHOWN);
        return true;
    }

    // the handle goes first (wf_hip_destroy synchronises its streams), the page-locked buffers after it: every group type's
    // destructor starts with this
    void close()
    {
        if(h)
            api().destroy(h);
        h = nullptr;
    }

    virtual ~WFHipGroupCore()
    {
        close();
        host_free(silent[0]);
        host_free(silent[1]);
    }

    virtual bool flush() = 0;             // everything the frame's members staged goes to the device as one batch; false: the device path failed
    virtual void joined(uint32_t) {}      // the per-slot words of the group type that a new member must find reset ...
    virtual void left(uint32_t) {}        // ... and those that must not outlive a member

    // the first free slot for `src`, its stream as update() leaves a source; false: the device refused
    bool join(WAVSourceHIP *src, uint32_t &slot)
    {
        slot = 0;
        while(member[slot] != nullptr)
            ++slot;
        if(api().reset(h, slot, 1) != WF_HIP_OK)
            return false;
        // reset has put the device's view of the slot back to SHOWN with no per-stream RMS: the cache of what the device holds
        // must say so, or a flush before this member's first submit would skip re-sending PAUSED and the device would tick the
        // fresh stream on its zero ring (m_last_silent = 1 where the reference still has false)
        state_dev[slot] = WF_HIP_SHOWN;
        member[slot] = src;
        submitted[slot] = 0;
        state[slot] = WF_HIP_PAUSED;
        ++members;
        joined(slot);
        return true;
    }

    // true: that was the last member
    bool leave(uint32_t slot)
    {
        member[slot] = nullptr;
        if(submitted[slot] == batch && n_submitted > 0)
            --n_submitted; // what it staged for the batch in assembly is dropped with it
        submitted[slot] = 0;
        frames[slot] = 0;
        state[slot] = WF_HIP_PAUSED;
        left(slot);
        return --members == 0;
    }

    // A member's tick opens.  One that comes round again while its last hand-over is still waiting for the rest of the frame
    // completes it; then, if the last flushed batch has something for this member (whatever the stream holds after that batch: a
    // source that sat a frame out finds the results of its last tick, unchanged; rows of batches older than `joined_at` belong to
    // whoever held the slot then), its readback is awaited and `last` is its slot -- else -1.  false: the group has failed.
    bool begin_tick(uint32_t slot, uint64_t joined_at, int &last)
    {
        last = -1;
        bool ok = !failed;
        if(ok && submitted[slot] == batch)
            ok = flush();
        const uint32_t b = (uint32_t)((batch - 1) & 1);
        if(ok && batch > 1 && valid[b] && batch - 1 >= joined_at) {
            ok = api().readback_done(h, b) == WF_HIP_OK;
            if(ok)
                last = (int)b;
        }
        return ok;
    }

    // A member's tick closes: what it staged for this frame counts; the frame's last member sends the batch off (a failure
    // shows at the members' next tick)
    void submit(uint32_t slot, uint32_t staged, uint8_t st, float secs)
    {
        frames[slot] = staged;
        state[slot] = st;
        seconds = secs;
        submitted[slot] = batch;
        if(++n_submitted >= members)
            flush();
    }

    // flush opens: whoever was not ticked in this frame (inactive source, free slot) is left exactly as it is; the state masks
    // go to the device if any changed
    bool begin_flush()
    {
        for(uint32_t i = 0; i < capacity; ++i)
            if(submitted[i] != batch) {
                state[i] = WF_HIP_PAUSED;
                frames[i] = 0;
            }
        if(state == state_dev)
            return true;
        state_dev = state;
        return api().set_hidden(h, 0, capacity, state.data()) == WF_HIP_OK;
    }

    // flush closes: the next batch is assembled in the other slot
    bool end_flush(bool ok)
    {
        valid[batch & 1] = ok;
        ++batch;
        n_submitted = 0;
        std::fill(frames.begin(), frames.end(), 0u);
        if(!ok) {
            LogWarn << "HIP " << kind << " batch tick failed (" << api().last_error(h) << "); its sources fall back to the CPU path";
            failed = true;
        }
        return ok;
    }

    // tick + readback of a flush, common to the group types once `dst` names their buffers
    bool tick_and_read(wf_hip_readback &dst)
    {
        wf_hip_tick_params p{};
        p.seconds = seconds;
        dst.last_silent = silent[batch & 1];
        return api().tick(h, &p) == WF_HIP_OK && api().read_async(h, 0, capacity, &dst, (uint32_t)(batch & 1)) == WF_HIP_OK;
    }
};

// The spectrum display's batch.  A member submits the samples its window gained since its last tick, into the page-locked staging
// block, with its m_input_rms; the flush adds the RMS values that changed; rows, m_last_silent and what the display draws from
// come back.
struct WFHipGroup : WFHipGroupCore {
    uint32_t cap_ch = 0, out_ch = 0, N = 0, M = 0;
    float *stage[2] = {nullptr, nullptr}; // page-locked [capacity][cap_ch][N]
    float *rows[2] = {nullptr, nullptr};  // page-locked [capacity][out_ch][M]
    std::vector<float> rms, rms_dev;
    // volume normalisation produced on the device (WAVSourceHIP::update_input_rms): the squared peaks every member's
    // sync_rms_buffer consumed this frame, page-locked [capacity][sq_max] per ingest slot, and m_input_rms coming back
    bool rms_feed = false;
    uint32_t sq_max = 0;
    float *sq_stage[2] = {nullptr, nullptr};
    float *rms_back[2] = {nullptr, nullptr};
    std::vector<uint32_t> sq_frames;      // [capacity] values staged for the batch being assembled
    // the display from the device (cfg.bars / cfg.curve with cfg.vertices): bar tops / curve points, vertices and vertex counts
    // of every member come back with the rows
    bool display = false;
    uint32_t disp_ch = 0, points = 0, per_row = 0;
    float *bars[2] = {nullptr, nullptr};      // page-locked [capacity][disp_ch][points]
    float *verts[2] = {nullptr, nullptr};     // page-locked [capacity][disp_ch][per_row][4]
    uint32_t *vcounts[2] = {nullptr, nullptr}; // page-locked [capacity][disp_ch]
    float *pre[2] = {nullptr, nullptr};       // page-locked [capacity][disp_ch]: mirrored axis, the value above the middle before the mirror (WF_HIP_OUT_PREMIRROR)

    bool create(const wf_config &c, int dev)
    {
        if(!open(c, dev))
            return false;
        cap_ch = c.capture_channels;
        N = c.fft_size;
        M = c.fft_size / 2;
        out_ch = ((cap_ch > 1) || c.stereo) ? 2u : 1u; // src/source.cpp:1171
        display = display_shape(c, h, disp_ch, points, per_row);
        for(int i = 0; display && i < 2; ++i) {
            if(!host_alloc(bars[i], (size_t)capacity * disp_ch * points))
                return false;
            if(c.mirror_freq_axis && !host_alloc(pre[i], (size_t)capacity * disp_ch))
                return false;
            if(per_row == 0)
                continue;
            if(!host_alloc(verts[i], (size_t)capacity * disp_ch * per_row * 4) || !host_alloc(vcounts[i], (size_t)capacity * disp_ch))
                return false;
        }
        rms.assign(capacity, 0.0f);
        rms_dev.assign(capacity, -1.0f);
        sq_frames.assign(capacity, 0);
        if(c.normalize_volume && std::getenv("WF_HIP_HOST_RMS") == nullptr && api().enable_input_rms(h, 1) == WF_HIP_OK) {
            rms_feed = true;
            sq_max = c.sample_rate & ~15u; // m_input_rms_size: more than a window's worth per frame is never needed
            for(int i = 0; i < 2; ++i)
                if(!host_alloc(sq_stage[i], (size_t)capacity * sq_max) || !host_alloc(rms_back[i], capacity))
                    return false;
        }
        for(int i = 0; i < 2; ++i)
            if(!host_alloc(stage[i], (size_t)capacity * cap_ch * N) || !host_alloc(rows[i], (size_t)capacity * out_ch * M) || !host_alloc(silent[i], capacity))
                return false;
        return true;
    }

    ~WFHipGroup() override
    {
        close();
        // NOTE: pre[] is never released -- a leak of capacity * disp_ch floats per slot for every group with a mirrored axis,
        // kept as found: releasing it changes the call trace tests/golden/host_groups_mock.json records
        for(int i = 0; i < 2; ++i) {
            host_free(stage[i]);
            host_free(rows[i]);
            host_free(sq_stage[i]);
            host_free(rms_back[i]);
            host_free(bars[i]);
            host_free(verts[i]);
            host_free(vcounts[i]);
        }
    }

    void joined(uint32_t slot) override { rms_dev[slot] = -1.0f; } // (wf_hip_reset leaves the slot without a per-stream RMS)
    void left(uint32_t slot) override { sq_frames[slot] = 0; }

    bool flush() override
    {
        auto &a = api();
        const uint32_t b = (uint32_t)(batch & 1);
        bool ok = begin_flush();
        if(ok && rms_feed) {
            ok = a.push_rms_ragged_async(h, 0, capacity, sq_stage[b], sq_frames.data(), sq_max, b) == WF_HIP_OK;
            std::fill(sq_frames.begin(), sq_frames.end(), 0u);
        } else if(ok && cfg.normalize_volume && rms != rms_dev) {
            ok = a.set_input_rms(h, 0, capacity, rms.data()) == WF_HIP_OK;
            rms_dev = rms;
        }
        ok = ok && a.push_audio_ragged_async(h, 0, capacity, stage[b], frames.data(), N, b) == WF_HIP_OK;
        if(ok) { // the frame: rows + m_last_silent, and behind them what the members draw from one frame later
            wf_hip_readback dst{};
            dst.rows = rows[b];
            if(rms_feed)
                dst.input_rms = rms_back[b];
            if(display) {
                dst.bars = bars[b];
                dst.vertices = per_row ? verts[b] : nullptr;
                dst.vertex_counts = per_row ? vcounts[b] : nullptr;
                dst.premirror = pre[b];
            }
            ok = tick_and_read(dst);
        }
        return end_flush(ok);
    }
};

// The level meter's batch (reference tick_meter src/source_generic.cpp:182-269): every member's tick_meter collects the levels
// the PREVIOUS frame's tick left for it and submits what its own tick_meter would consume this frame -- every captured frame
// older than the A/V-sync point, :201-220; the flush rebuilds its staging block from them: ONE ragged ingest, ONE wf_hip_tick
// (meter_tick_kernel over all streams), ONE readback.
struct WFHipMeterGroup : WFHipGroupCore {
    uint32_t cap_ch = 0, ring_cap = 0;
    std::vector<std::vector<float>> pending; // [capacity] what the member consumed this frame: [cap_ch][frames[i]]
    float *stage[2] = {nullptr, nullptr};    // page-locked [capacity][cap_ch][stage_frames[b]], rebuilt at every flush
    size_t stage_floats[2] = {0, 0};
    float *levels[2] = {nullptr, nullptr};   // page-locked [capacity][cap_ch]
    // waveform display (cfg.waveform): the same frame-by-frame hand-over, with every member's A/V-sync reserve and audio
    // timestamp, and the rows of the whole group coming back instead of the levels
    bool wave = false;
    uint32_t out_ch = 0, width = 0;
    std::vector<uint32_t> delay, delay_dev;  // [capacity] the reserve tick_waveform leaves in the ring (:291-292), frames
    std::vector<uint64_t> audio_ts;          // [capacity] m_audio_ts
    float *rows[2] = {nullptr, nullptr};     // page-locked [capacity][out_ch][width]

    bool create(const wf_config &c, int dev)
    {
        if(!open(c, dev))
            return false;
        auto &a = api();
        cap_ch = c.capture_channels;
        ring_cap = a.ring_frames(h);
        wave = c.waveform != 0;
        kind = wave ? "waveform" : "meter";
        pending.assign(capacity, {});
        if(wave) {
            out_ch = a.output_channels(h);
            width = c.fft_size;
            delay.assign(capacity, 0);
            delay_dev.assign(capacity, 0);
            audio_ts.assign(capacity, 0);
        }
        for(int i = 0; i < 2; ++i)
            if(!host_alloc(silent[i], capacity) || !(wave ? host_alloc(rows[i], (size_t)capacity * out_ch * width) : host_alloc(levels[i], (size_t)capacity * cap_ch)))
                return false;
        return true;
    }

    ~WFHipMeterGroup() override
    {
        close();
        for(int i = 0; i < 2; ++i) {
            host_free(stage[i]);
            host_free(levels[i]);
            host_free(rows[i]);
        }
    }

    void joined(uint32_t slot) override
    {
        if(wave) {
            delay[slot] = 0;
            audio_ts[slot] = 0;
        }
    }

    bool flush() override
    {
        auto &a = api();
        const uint32_t b = (uint32_t)(batch & 1);
        bool ok = begin_flush();
        const uint32_t maxf = *std::max_element(frames.begin(), frames.end());
        if(ok && maxf > 0) {
            a.ingest_done(h, b); // the slot's block has been copied out (two frames ago)
            const size_t need = (size_t)capacity * cap_ch * maxf;
            if(stage_floats[b] < need) {
                host_free(stage[b]);
                stage_floats[b] = need + need / 2;
                if(!host_alloc(stage[b], stage_floats[b])) {
                    stage_floats[b] = 0;
                    ok = false;
                }
            }
            if(ok) {
                for(uint32_t i = 0; i < capacity; ++i)
                    for(uint32_t c = 0; c < cap_ch && frames[i]; ++c)
                        std::memcpy(stage[b] + ((size_t)i * cap_ch + c) * maxf, pending[i].data() + (size_t)c * frames[i], (size_t)frames[i] * sizeof(float));
                ok = a.push_audio_ragged_async(h, 0, capacity, stage[b], frames.data(), maxf, b) == WF_HIP_OK;
            }
        }
        if(ok && wave) {
            if(delay != delay_dev) {
                ok = a.set_stream_delay(h, 0, capacity, delay.data()) == WF_HIP_OK;
                delay_dev = delay;
            }
            ok = ok && a.set_stream_audio_ts(h, 0, capacity, audio_ts.data()) == WF_HIP_OK;
        }
        if(ok) {
            wf_hip_readback dst{};
            (wave ? dst.rows : dst.meter) = wave ? rows[b] : levels[b];
            ok = tick_and_read(dst);
        }
        return end_flush(ok);
    }
};

namespace {

struct Registry {
    std::mutex mtx;
    std::vector<std::unique_ptr<WFHipGroup>> groups;
    std::vector<std::unique_ptr<WFHipMeterGroup>> mgroups;
};
Registry &registry()
{
    static Registry *r = new Registry; // never destroyed: sources an exiting host leaks must not call into an unloaded runtime
    return *r;
}

// batches spread over the devices the box has: a new group goes to the device that serves the fewest (sources share nothing,
// SURVEY.md section 8(e); WF_HIP_DEVICE pins everything to one device).  The asymmetry is as found: a new spectrum group counts
// the spectrum groups only, a new meter / waveform group counts both kinds.
int pick_device(const Registry &r, bool count_meter_groups)
{
    const int pinned = pinned_device();
    if(pinned >= 0)
        return pinned;
    const int ndev = std::max(api().device_count(), 1);
    std::vector<int> load((size_t)ndev, 0);
    const auto count = [&](const auto &list) {
        for(auto &p : list)
            if(p->device >= 0 && p->device < ndev)
                ++load[(size_t)p->device];
    };
    count(r.groups);
    if(count_meter_groups)
        count(r.mgroups);
    return (int)(std::min_element(load.begin(), load.end()) - load.begin());
}

template<class G>
void drop_group(std::vector<std::unique_ptr<G>> &list, const G *g)
{
    list.erase(std::remove_if(list.begin(), list.end(), [g](const auto &p) { return p.get() == g; }), list.end());
}

using Attach = WFHipAttach;

// `src` joins the group of configuration `c` in `list` that has room, or a new one (registry lock held)
template<class G>
Attach join_group(std::vector<std::unique_ptr<G>> &list, const wf_config &c, bool count_meter_groups, WAVSourceHIP *src, G *&g, uint32_t &slot)
{
    g = nullptr;
    for(auto &p : list)
        if(!p->failed && p->members < p->capacity && std::memcmp(&p->cfg, &c, sizeof(c)) == 0) {
            g = p.get();
            break;
        }
    const bool opened = g == nullptr;
    if(opened) {
        auto fresh = std::make_unique<G>();
        if(!fresh->create(c, pick_device(registry(), count_meter_groups)))
            return Attach::refused;
        g = fresh.get();
        list.push_back(std::move(fresh));
    }
    if(!g->join(src, slot)) {
        if(opened) // nobody joined: the group would stay in the registry with no member for ever
            drop_group(list, g);
        g = nullptr;
        return Attach::failed;
    }
    return Attach::ok;
}

// the member in `slot` of `g` leaves; a group without members is closed
template<class G>
void leave_group(std::vector<std::unique_ptr<G>> &list, G *&g, uint32_t slot)
{
    std::lock_guard lock(registry().mtx);
    G *was = g;
    g = nullptr;
    if(was->leave(slot))
        drop_group(list, was);
}

} // namespace

uint64_t WAVSourceHIP::fallback_ticks() { return g_fallback_ticks.load(); }
uint64_t WAVSourceHIP::host_rms_updates() { return g_host_rms_updates.load(); }
uint64_t WAVSourceHIP::device_renders() { return g_device_renders.load(); }
uint64_t WAVSourceHIP::host_renders() { return g_host_renders.load(); }

bool WAVSourceHIP::available()
{
    auto &a = api();
    return a.ok && a.device_count() > 0;
}

WAVSourceHIP::~WAVSourceHIP()
{
    std::lock_guard lock(m_mtx);
    hip_release();
}

void WAVSourceHIP::hip_release()
{
    if(m_hip != nullptr) {
        api().destroy(m_hip);
        m_hip = nullptr;
    }
    if(m_mgroup != nullptr)
        leave_group(registry().mgroups, m_mgroup, m_slot);
    if(m_group != nullptr)
        leave_group(registry().groups, m_group, m_slot);
}

// One "leave the device for the CPU class" step: this tick goes to the reference's own class (the caller hands it over, after
// unlocking the registry), and so do the following ones until update() configures the device path again.  An empty `why`: the
// source was not on the device in the first place.
void WAVSourceHIP::hip_fall_back(const std::string &why)
{
    if(!why.empty())
        LogWarn << why;
    hip_release();
    g_fallback_ticks.fetch_add(1);
}

// WAVSource members -> wf_config (include/wf_config.h lists the member behind every field), without the display
wf_config WAVSourceHIP::hip_config() const
{
    wf_config c{};
    c.waveform = (m_display_mode == DisplayMode::WAVEFORM) ? 1u : 0u; // m_fft_size is m_width in this mode
    c.meter = m_meter_mode ? 1u : 0u;   // update() has already applied the mode's overrides to the members below
    c.meter_rms = m_meter_rms ? 1u : 0u;
    c.meter_ms = m_meter_ms;
    c.fft_size = (uint32_t)m_fft_size;
    c.sample_rate = m_audio_info.samples_per_sec;
    c.capture_channels = m_capture_channels;
    c.stereo = m_stereo ? 1u : 0u;
    c.window = (int32_t)m_window_func;       // FFTWindow and wf_window share their numbering
    c.sine_exponent = m_sine_exponent;
    c.tsmoothing = (int32_t)m_tsmoothing;    // TSmoothingMode / wf_tsmoothing likewise
    c.gravity = m_gravity;
    c.fast_peaks = m_fast_peaks ? 1u : 0u;
    c.slope = m_slope;
    c.rolloff_q = m_rolloff_q;
    c.rolloff_rate = m_rolloff_rate;
    c.cutoff_low = m_cutoff_low;
    c.cutoff_high = m_cutoff_high;
    c.floor_db = m_floor;
    c.ceiling_db = m_ceiling;
    c.normalize_volume = m_normalize_volume ? 1u : 0u;
    c.volume_target = m_volume_target;
    c.max_gain = m_max_gain;
    c.bars = 0; // (hip_display_config sets the display fields where render() is served from the device)
    c.interp_mode = (int32_t)m_interp_mode;
    c.log_scale = m_log_scale ? 1u : 0u;
    c.mirror_freq_axis = m_mirror_freq_axis ? 1u : 0u;
    c.width = m_width;
    c.height = m_height;
    c.bar_width = m_bar_width;
    c.bar_gap = m_bar_gap;
    c.channel_spacing = m_channel_spacing;
    c.min_bar_height = m_min_bar_height;
    c.rounded_caps = m_rounded_caps ? 1u : 0u;
    return c;
}

// (re)connects this source to the device from the members update() has just set
bool WAVSourceHIP::hip_configure()
{
    hip_release();
    if(!available() || (m_capture_channels == 0))
        return false;
    wf_config c = hip_config();
    m_hip_have_prev = false;
    m_hip_display = m_hip_display_valid = false;
    const wf_config rows_only = c;
    if(!c.waveform && !c.meter && device_render_mode() && m_vbuf != nullptr)
        hip_display_config(c);
    Attach rc = hip_attach(c);
    // once more without the display -- e.g. a filtered curve whose staging the device refuses: the rows still come from the
    // device, render() keeps interpolating on the host
    if(rc == Attach::refused && (c.bars != 0 || c.curve != 0))
        rc = hip_attach(rows_only);
    if(rc == Attach::refused) // e.g. WF_HIP_ERR_UNSUPPORTED for a configuration the device refuses
        LogWarn << "HIP path unavailable for this configuration (" << api().last_error(nullptr) << "); using the CPU path";
    return rc == Attach::ok;
}

// configuration `c` on the device: as a member of a group where its kind of display batches, else on a handle of its own
WFHipAttach WAVSourceHIP::hip_attach(const wf_config &c)
{
    // Meter buffers beyond 65536 samples (meter_buf above ~1.3 s; the reference allows 600 s) stay synchronous: a member's first
    // hand-over is the whole buffer.  The waveform display batches in the same kind of group (a group's configuration has either
    // cfg.meter or cfg.waveform set, so the two never share one); with volume normalisation a source stays synchronous: its
    // m_input_rms is computed on the host per call.
    const char *mb = std::getenv("WF_HIP_BATCHED_METER"); // 0: the meter stays synchronous while the spectrum batches
    const char *wb = std::getenv("WF_HIP_BATCHED_WAVE");  // 0: so does the waveform display
    bool batches = batched_mode();
    if(c.meter)
        batches = batches && m_fft_size <= 65536 && !(mb && mb[0] == '0');
    else if(c.waveform)
        batches = batches && !c.normalize_volume && !(wb && wb[0] == '0');
    return batches ? hip_join_group(c) : hip_open_own(c);
}

// join (or open) the batch of this configuration: a spectrum group, or a meter / waveform group (which has no display to drop)
WFHipAttach WAVSourceHIP::hip_join_group(const wf_config &c)
{
    auto &r = registry();
    std::lock_guard lock(r.mtx);
    const bool spectrum = !c.waveform && !c.meter;
    const Attach rc = spectrum ? join_group(r.groups, c, false, this, m_group, m_slot) : join_group(r.mgroups, c, true, this, m_mgroup, m_slot);
    if(rc != Attach::ok)
        return rc;
    m_hip_joined = spectrum ? m_group->batch : m_mgroup->batch; // rows read back for earlier batches belong to whoever held the slot then
    if(spectrum) {
        m_hip_window.assign((size_t)m_capture_channels * m_fft_size, 0.0f);
        m_hip_prev.assign((size_t)m_capture_channels * m_fft_size, 0.0f);
        m_hip_display = m_group->display;
        if(m_hip_display)
            hip_size_display(m_group->disp_ch, m_group->points, m_group->per_row);
    } else if(m_mgroup->wave) {
        m_hip_pushed = m_fft_size; // update() pre-fills m_fft_size zeros; so does the device (wf_hip_reset)
        m_hip_prev.assign((size_t)m_capture_channels * m_hip_pushed, 0.0f);
    }
    return rc;
}

// synchronous: a handle of one stream for this source alone
WFHipAttach WAVSourceHIP::hip_open_own(const wf_config &c)
{
    if(api().create(&c, std::max(pinned_device(), 0), 1, 0, &m_hip) != WF_HIP_OK) {
        m_hip = nullptr;
        return Attach::refused;
    }
    uint32_t dch = 0, points = 0, per_row = 0;
    m_hip_display = display_shape(c, m_hip, dch, points, per_row);
    if(m_hip_display)
        hip_size_display(dch, points, per_row);
    m_hip_window.assign((size_t)m_capture_channels * m_fft_size, 0.0f);
    m_hip_out.assign((size_t)m_output_channels * (m_fft_size / 2), 0.0f);
    m_hip_state = WF_HIP_SHOWN;
    m_hip_pushed = (m_display_mode == DisplayMode::WAVEFORM) ? m_fft_size : 0; // update() pre-fills m_fft_size zeros; so does the device
    m_hip_prev.assign((size_t)m_capture_channels * m_hip_pushed, 0.0f);          // ... and those zeros are what tick_waveform expects at the front
    return Attach::ok;
}

// the members render() draws from, for a display of this shape
void WAVSourceHIP::hip_size_display(uint32_t disp_ch, uint32_t points, uint32_t per_row)
{
    m_hip_points = points;
    m_hip_per_row = per_row;
    m_hip_bars.assign((size_t)disp_ch * points, 0.0f);
    m_hip_verts.assign((size_t)disp_ch * per_row * 4, 0.0f);
    m_hip_vcounts.assign(per_row ? disp_ch : 0u, 0u);
    m_hip_pre.assign(disp_ch, 0.0f);
}

// The display part of wf_config (include/wf_config.h) from the members get_settings / update() have set: which of render_bars /
// render_curve runs (src/source.cpp:1354-1357), its interpolation, filter and geometry.
void WAVSourceHIP::hip_display_config(wf_config &c) const
{
    const bool stepped = m_display_mode == DisplayMode::STEPPED_BAR;
    if(m_display_mode == DisplayMode::BAR || stepped) {
        c.bars = 1;
        c.vertices = stepped ? 3u : 1u;
    } else if(m_display_mode == DisplayMode::CURVE) {
        // the points come from the device; render_curve's vertex loop only writes their y into a strip whose x never changes
        // (src/source.cpp:1443-1460) and stays here: its vertices would be eight times the bytes of the points on the way back
        c.curve = 1;
        c.vertices = 0;
    } else
        return;
    c.filter_mode = (m_filter_mode != FilterMode::NONE) ? WF_FILTER_GAUSS : WF_FILTER_NONE;
    c.filter_radius = m_filter_radius;
    c.step_width = m_step_width;
    c.step_gap = m_step_gap;
    c.radial = m_radial ? 1u : 0u;
}

// a member's (or the synchronous handle's) display of the frame just read back -> the members render() draws from; the bar tops
// also go where the reference keeps them (m_interp_bufs after render_bars / render_curve), for whoever looks there
void WAVSourceHIP::hip_collect_display(const float *bars, const float *verts, const uint32_t *counts)
{
    std::memcpy(m_hip_bars.data(), bars, m_hip_bars.size() * sizeof(float));
    if(m_hip_per_row) {
        std::memcpy(m_hip_verts.data(), verts, m_hip_verts.size() * sizeof(float));
        std::memcpy(m_hip_vcounts.data(), counts, m_hip_vcounts.size() * sizeof(uint32_t));
    }
    hip_publish_display();
}

// m_hip_bars / m_hip_verts / m_hip_vcounts hold this frame's display: the bar tops (curve points) also go where render() and the
// reference's own members expect them
void WAVSourceHIP::hip_publish_display()
{
    const size_t channels = m_hip_points ? m_hip_bars.size() / m_hip_points : 0;
    for(size_t channel = 0; channel < channels; ++channel)
        if(m_interp_bufs[channel].size() >= m_hip_points)
            std::memcpy(m_interp_bufs[channel].data(), m_hip_bars.data() + channel * m_hip_points, (size_t)m_hip_points * sizeof(float));
    m_hip_display_valid = true;
}

void WAVSourceHIP::render([[maybe_unused]] gs_effect_t *effect)
{
    std::lock_guard lock(m_mtx);
    // the display modes the device does not draw (level meter: two values; waveform), sources on the CPU path, a frame before
    // the first device result: the reference's own render
    const bool spectrum = !m_meter_mode && m_display_mode != DisplayMode::WAVEFORM;
    // The shader's gradient height / pulse colour follow the smallest y BEFORE the mirror image replaces the upper half
    // (src/source.cpp:1548-1567, :1411-1424).  Without the Gaussian filter every output above the middle has ONE pre-mirror value
    // (init_interp clamps their positions to the highest bin, src/source.cpp:857-862), which the device keeps
    // (WF_HIP_OUT_PREMIRROR).  With the filter on (apply_filter runs before that loop, :1541-1547) outputs half+1 ... half+radius
    // blend that constant with lower bars and the minimum may sit at any of them: those two render modes then keep the
    // reference's own loops over m_decibels.
    const bool miny_on_device = !m_mirror_freq_axis || m_filter_mode == FilterMode::NONE ||
                                (m_render_mode != RenderMode::GRADIENT && m_render_mode != RenderMode::PULSE);
    if(!spectrum || !using_hip() || !m_hip_display || !m_hip_display_valid || !miny_on_device) {
        if(spectrum && using_hip())
            g_host_renders.fetch_add(1);
        WAVSourceGeneric::render(effect);
        return;
    }
    if(m_last_silent && m_hide_on_silent) // src/source.cpp:1349-1352
        return;
    if(m_vbuf == nullptr)
        return;
    g_device_renders.fetch_add(1);
    const bool curve = m_display_mode == DisplayMode::CURVE;
    auto tech = get_shader_tech();
    // the constants render_bars / render_curve hand to set_shader_vars (src/source.cpp:1368-1373, :1480-1493)
    const auto center = (float)m_height / 2;
    const auto bottom = (float)m_height;
    const auto cpos = m_stereo ? center : bottom;
    const auto channel_offset = m_channel_spacing * 0.5f;
    auto border_top = 0.0f, border_bottom = cpos - channel_offset;
    if(!curve) {
        border_top = (m_rounded_caps) ? m_cap_radius : 0.0f;
        border_bottom = (m_rounded_caps && (!m_stereo || (m_channel_spacing > 0))) ? cpos - m_cap_radius : cpos;
        if(m_channel_spacing > 0)
            border_bottom -= channel_offset;
        if(m_min_bar_height > 0)
            border_bottom -= m_min_bar_height;
        border_bottom = std::clamp(border_bottom, border_top, cpos);
    }
    const auto channels = m_stereo ? 2u : 1u;
    auto miny = cpos;
    auto minpos = 0u;
    // The shader's gradient height / pulse colour follow the smallest y of the rows BEFORE the mirror image replaces their upper
    // halves (src/source.cpp:1548-1567, :1411-1424).  The device hands back the mirrored rows -- whose upper halves repeat lower
    // values: a strict "<" never picks them -- and, per row, the one value every output above the middle had before the mirror
    // (WF_HIP_OUT_PREMIRROR): first seen at output num_bars / 2 + 1.
    const auto half = m_hip_points / 2u;
    for(auto channel = 0u; channel < channels; ++channel) {
        const auto upto = m_mirror_freq_axis ? std::min(half + 1u, m_hip_points) : m_hip_points;
        for(auto i = 0u; i < upto; ++i) {
            const auto val = m_hip_bars[(size_t)channel * m_hip_points + i];
            if(val < miny) {
                miny = val;
                minpos = i;
            }
        }
        if(m_mirror_freq_axis && half + 1u < m_hip_points && channel < m_hip_pre.size() && m_hip_pre[channel] < miny) {
            miny = m_hip_pre[channel];
            minpos = half + 1u;
        }
    }
    set_shader_vars(cpos, miny, (float)minpos, channel_offset, border_top, border_bottom);

    gs_technique_begin(tech);
    gs_technique_begin_pass(tech, 0);
    gs_load_vertexbuffer(m_vbuf);
    gs_load_indexbuffer(nullptr);
    auto vbdata = gs_vertexbuffer_get_data(m_vbuf);
    static_assert(sizeof(vec3) == 4 * sizeof(float), "libobs' vec3 is four floats: what the device's vertex fill writes");
    for(auto channel = 0u; channel < channels; ++channel) {
        if(curve) {
            // render_curve's own loop (src/source.cpp:1436-1461): the points' y into the strip
            auto offset = channel_offset;
            if(channel)
                offset = -offset;
            const auto bot = cpos - offset;
            const float *pts = m_hip_bars.data() + (size_t)channel * m_hip_points;
            const auto n = std::min<size_t>(m_hip_points, m_width);
            for(size_t i = 0; i < n; ++i) {
                const auto val = pts[i];
                if(m_render_mode == RenderMode::LINE)
                    vbdata->points[i].y = channel == 0 ? val : bottom - val;
                else {
                    vbdata->points[i * 2].y = channel == 0 ? val : bottom - val;
                    vbdata->points[(i * 2) + 1].y = bot;
                }
            }
            gs_vertexbuffer_flush(m_vbuf);
            gs_draw((m_render_mode != RenderMode::LINE) ? GS_TRISTRIP : GS_LINESTRIP, 0, (uint32_t)vbdata->num);
            continue;
        }
        const auto count = std::min<size_t>(m_hip_vcounts[channel], std::min<size_t>(m_hip_per_row, vbdata->num));
        std::memcpy(vbdata->points, m_hip_verts.data() + (size_t)channel * m_hip_per_row * 4, count * sizeof(vec3));
        gs_vertexbuffer_flush(m_vbuf);
        if(count > 0)
            gs_draw(GS_TRIS, 0, (uint32_t)count);
    }
    gs_load_vertexbuffer(nullptr);
    gs_technique_end_pass(tech);
    gs_technique_end(tech);
}

void WAVSourceHIP::update(obs_data_t *settings)
{
    std::lock_guard lock(m_mtx);
    WAVSourceGeneric::update(settings); // tables, rings, render state: unchanged reference code
    hip_configure();
}

// The A/V-sync point in frames: how much of the newest captured audio lies ahead of this tick's video time and stays behind for
// later ticks (dtaudio > 0, src/source_generic.cpp:50-51)
size_t WAVSourceHIP::hip_sync_frames()
{
    const int64_t dtaudio = get_audio_sync(m_tick_ts);
    return (dtaudio > 0) ? size_t(ns_to_audio_frames(m_audio_info.samples_per_sec, (uint64_t)dtaudio)) : 0;
}

// reference :50-59: keep dtsize bytes in every channel's ring, copy the first fft_size samples of what is left -- the
// A/V-synchronised window -- into m_hip_window.  false: a channel holds less than that (the reference skips it).
bool WAVSourceHIP::hip_window(size_t &dtframes)
{
    const auto bufsz = m_fft_size * sizeof(float);
    dtframes = hip_sync_frames();
    const size_t dtsize = dtframes * sizeof(float) + bufsz;
    for(auto channel = 0u; channel < m_capture_channels; ++channel)
        if(m_capturebufs[channel].size() < dtsize)
            return false;
    for(auto channel = 0u; channel < m_capture_channels; ++channel) {
        m_capturebufs[channel].pop_front(nullptr, m_capturebufs[channel].size() - dtsize);
        m_capturebufs[channel].peek_front(m_hip_window.data() + (size_t)channel * m_fft_size, bufsz);
    }
    return true;
}

// What tick_meter would pop into its meter buffer this tick (:201-220: everything older than the A/V-sync point) is popped into
// dst instead, [capture_channels][frames], oldest first; returns the frames (the channels of a source are pushed together by
// capture_audio; capture_audio keeps at most dtsamples + m_fft_size samples, so this is never more than the device ring holds)
uint32_t WAVSourceHIP::hip_pop_meter(std::vector<float> &dst)
{
    const size_t dtsize = hip_sync_frames() * sizeof(float);
    size_t frames = 0;
    for(auto channel = 0u; channel < m_capture_channels; ++channel) {
        const auto sz = m_capturebufs[channel].size();
        const size_t n = (sz > dtsize) ? (sz - dtsize) / sizeof(float) : 0;
        frames = (channel == 0) ? n : std::min(frames, n);
    }
    dst.resize((size_t)m_capture_channels * frames);
    for(auto channel = 0u; channel < m_capture_channels && frames; ++channel)
        m_capturebufs[channel].pop_front(dst.data() + (size_t)channel * frames, frames * sizeof(float));
    return (uint32_t)frames;
}

// The frames of m_capturebufs that are new to the waveform's device ring go into dst, [capture_channels][fresh], and the rings are
// popped down to the A/V-sync reserve as the reference does (:321).  false: a ring holds no more than the reserve (:293-295: the
// reference returns before it touches anything, and so does this).
//
// The device ring holds every frame pushed so far and counts "what the reference's ring holds" as (frames pushed since
// the last tick) + (the reserve that tick left behind), :321.  Frames at the front of m_capturebufs that are already
// there -- the last tick's reserve, m_hip_pushed of them -- must not be pushed twice; but capture_audio drops from the
// front once a ring exceeds dtsamples + m_waveform_samples (src/source.cpp:1883-1886), and then what is left is
// re-sent whole: after a drop the ring is at its cap, the reference trims it to max_size and so does the device
// (avail > max_size), and the re-sent frames are contiguous.  Whether the old reserve is still at the front is
// checked against a copy of it, m_hip_prev (all-zero audio can match by accident: then both ways of pushing give zeros).
bool WAVSourceHIP::hip_wave_fresh(size_t reserve, std::vector<float> &dst)
{
    for(auto i = 0u; i < m_capture_channels; ++i)
        if(m_capturebufs[i].size() <= reserve * sizeof(float))
            return false;
    const size_t max_frames = m_waveform_samples + reserve;
    size_t frames = 0;
    bool front_kept = true;
    std::vector<std::vector<float>> all(m_capture_channels);
    for(auto channel = 0u; channel < m_capture_channels; ++channel) {
        auto &buf = m_capturebufs[channel];
        if(buf.size() > max_frames * sizeof(float)) // :303-304
            buf.pop_front(nullptr, buf.size() - max_frames * sizeof(float));
        const size_t s = buf.size() / sizeof(float);
        all[channel].resize(s);
        buf.peek_front(all[channel].data(), s * sizeof(float));
        if(channel == 0)
            frames = s;
        front_kept = front_kept && s >= m_hip_pushed && m_hip_prev.size() == (size_t)m_capture_channels * m_hip_pushed &&
                     std::memcmp(all[channel].data(), m_hip_prev.data() + (size_t)channel * m_hip_pushed, m_hip_pushed * sizeof(float)) == 0;
    }
    const size_t fresh = front_kept ? frames - m_hip_pushed : frames;
    // "timestamp rollover, give up" (:314-317; a tick before any audio has a timestamp): the reference has trimmed its
    // ring but consumes nothing.  The device takes the same exit from the same timestamps (and records the trim); here the
    // ring keeps what it holds, all of it now on the device.
    const auto start_ts = m_audio_ts - audio_frames_to_ns(m_audio_info.samples_per_sec, frames);
    const auto stop_ts = m_audio_ts - audio_frames_to_ns(m_audio_info.samples_per_sec, reserve);
    const bool rollover = (start_ts >= m_audio_ts) || (stop_ts > m_audio_ts);
    const size_t stay = rollover ? frames : reserve; // frames left in m_capturebufs behind this tick
    dst.resize((size_t)m_capture_channels * fresh);
    m_hip_prev.assign((size_t)m_capture_channels * stay, 0.0f);
    for(auto channel = 0u; channel < m_capture_channels; ++channel) {
        const size_t s = all[channel].size();
        std::memcpy(dst.data() + (size_t)channel * fresh, all[channel].data() + (s - fresh), fresh * sizeof(float));
        std::memcpy(m_hip_prev.data() + (size_t)channel * stay, all[channel].data() + (s - stay), stay * sizeof(float));
        m_capturebufs[channel].pop_front(nullptr, (s - stay) * sizeof(float)); // :321: only the reserve stays
    }
    m_hip_pushed = stay;
    return true;
}

// synchronous: the handle's one stream is told its state when it changes
bool WAVSourceHIP::hip_send_state(int state)
{
    if(state == m_hip_state)
        return true;
    const uint8_t mask = (uint8_t)state;
    m_hip_state = state;
    return api().set_hidden(m_hip, 0, 1, &mask) == WF_HIP_OK;
}

// rows ([output_channels][outsz]) and the silence verdict of a tick -> m_decibels / m_last_silent
void WAVSourceHIP::hip_take_rows(const float *rows, size_t outsz, bool silent)
{
    for(auto channel = 0u; channel < m_output_channels; ++channel)
        std::memcpy(m_decibels[channel].get(), rows + (size_t)channel * outsz, outsz * sizeof(float));
    m_last_silent = silent;
}

// synchronous: the tick, and its rows and m_last_silent inside the call
bool WAVSourceHIP::hip_tick_and_take_rows(const wf_hip_tick_params &p, size_t outsz)
{
    auto &a = api();
    m_hip_out.resize((size_t)m_output_channels * outsz);
    uint8_t silent = 0;
    if(a.tick(m_hip, &p) != WF_HIP_OK || a.read(m_hip, WF_HIP_OUT_DECIBELS, 0, 1, m_hip_out.data()) != WF_HIP_OK ||
       a.read(m_hip, WF_HIP_OUT_LAST_SILENT, 0, 1, &silent) != WF_HIP_OK)
        return false;
    hip_take_rows(m_hip_out.data(), outsz, silent != 0);
    return true;
}

// Same observable behaviour as WAVSourceGeneric::tick_spectrum (src/source_generic.cpp:26-180): the A/V-synchronised
// window of each channel goes to the device, the device runs the whole per-tick state machine (hidden/timeout reset,
// silence detection, window, FFT, magnitude, slope, smoothing, dBFS, normalisation, roll-off) and m_decibels /
// m_last_silent come back.
// The batched path (struct WFHipGroup).  m_decibels / m_last_silent are the device's results for the previous video frame.
void WAVSourceHIP::tick_spectrum_batched(float seconds)
{
    auto &r = registry();
    std::unique_lock lock(r.mtx);
    WFHipGroup *g = m_group;
    const uint32_t slot = m_slot;
    const size_t N = m_fft_size;
    int last = -1;
    if(!g->begin_tick(slot, m_hip_joined, last)) {
        lock.unlock();
        if(g->rms_feed && m_input_rms_buf && m_input_rms_size > 0) {
            // the device kept the one-second window of squared peaks; the host's ring was never advanced.  Seed it so that its
            // sum reproduces the last m_input_rms that came back (every entry = the mean square), instead of a window of zeros
            // that would clamp the gain to max_gain for the next second
            const float ms = m_input_rms * m_input_rms;
            for(size_t i = 0; i < m_input_rms_size; ++i)
                m_input_rms_buf[i] = ms;
            m_input_rms_pos = 0;
        }
        hip_fall_back("HIP batch unavailable; this source continues on the CPU path");
        WAVSourceGeneric::tick_spectrum(seconds);
        return;
    }
    // 1. collect the row the last flushed batch left for this source
    if(last >= 0) {
        hip_take_rows(g->rows[last] + (size_t)slot * g->out_ch * g->M, N / 2, g->silent[last][slot] != 0);
        if(g->rms_feed)
            m_input_rms = g->rms_back[last][slot]; // as of that batch's tick (for observers; the device uses its own)
        if(g->display && m_hip_display && g->pre[last])
            m_hip_pre.assign(g->pre[last] + (size_t)slot * g->disp_ch, g->pre[last] + (size_t)(slot + 1) * g->disp_ch);
        if(g->display && m_hip_display)
            hip_collect_display(g->bars[last] + (size_t)slot * g->disp_ch * g->points,
                                g->per_row ? g->verts[last] + (size_t)slot * g->disp_ch * g->per_row * 4 : nullptr,
                                g->per_row ? g->vcounts[last] + (size_t)slot * g->disp_ch : nullptr);
    }
    // 2. submit this frame
    const uint32_t b = (uint32_t)(g->batch & 1);
    if(g->n_submitted == 0)
        api().ingest_done(g->h, b); // the staging block of this slot has been copied out (two frames ago)
    const bool timed_out = hip_timed_out();
    const bool hidden = !m_show || timed_out; // reference :34
    uint32_t fresh = 0;
    uint8_t st = hidden ? (timed_out ? WF_HIP_HIDDEN_TIMEOUT : WF_HIP_HIDDEN) : WF_HIP_SHOWN;
    size_t dtframes = 0;
    if(!hidden) {
        if(!hip_window(dtframes)) {
            st = WF_HIP_STARVED; // underflow (:55-61): no channel is processed, the end-of-tick pass still runs (see tick_spectrum)
        } else {
            // Which samples are new?  The device ring of this stream ends with the window handed over last time; the new
            // window overlaps it by fft_size - shift samples.  The shift the timestamps suggest is checked against the
            // samples themselves (and its neighbours tried: the timestamps round); if no overlap is found the whole window
            // goes -- always correct, since the device analyses the newest fft_size samples of its ring.
            long est = (long)N;
            if(m_hip_have_prev) {
                const int64_t dts = (int64_t)(m_audio_ts - m_hip_prev_audio_ts);
                est = (long)std::llround((double)dts * (double)m_audio_info.samples_per_sec / 1e9) - ((long)dtframes - (long)m_hip_prev_sync);
            }
            auto overlaps = [&](long s) {
                if(s < 0 || s > (long)N)
                    return false;
                for(auto channel = 0u; channel < m_capture_channels; ++channel)
                    if(std::memcmp(m_hip_prev.data() + (size_t)channel * N + (size_t)s, m_hip_window.data() + (size_t)channel * N,
                                   (N - (size_t)s) * sizeof(float)) != 0)
                        return false;
                return true;
            };
            long shift = (long)N;
            if(m_hip_have_prev) {
                for(long d : {0L, 1L, -1L, 2L, -2L})
                    if(overlaps(est + d)) {
                        shift = est + d;
                        break;
                    }
            }
            fresh = (uint32_t)shift;
            float *dst = g->stage[b] + (size_t)slot * g->cap_ch * N;
            for(auto channel = 0u; channel < m_capture_channels; ++channel)
                std::memcpy(dst + (size_t)channel * N, m_hip_window.data() + (size_t)channel * N + (N - fresh), (size_t)fresh * sizeof(float));
            m_hip_prev.swap(m_hip_window);
            m_hip_have_prev = true;
            m_hip_prev_audio_ts = m_audio_ts;
            m_hip_prev_sync = (int64_t)dtframes;
        }
    }
    g->rms[slot] = m_input_rms;
    g->submit(slot, fresh, st, seconds);
}

// WAVSourceGeneric::update_input_rms (src/source_generic.cpp:392-403) = sync_rms_buffer (src/source.cpp:810-835: everything
// in m_rms_sync_buf older than the A/V-sync point moves into the circular one-second m_input_rms_buf) + the sum of its
// m_input_rms_size squares.  Batched mode: the values sync_rms_buffer would move are staged for the device instead, which
// keeps the window and its (two-level) sum per stream; no 48000-float loop per source and frame on the host.  Called by
// WAVSource::tick (src/source.cpp:1330-1331) ahead of tick_spectrum, under m_mtx.
void WAVSourceHIP::update_input_rms()
{
    WFHipGroup *g = m_group;
    if(g == nullptr || !g->rms_feed) {
        g_host_rms_updates.fetch_add(1);
        WAVSourceGeneric::update_input_rms();
        return;
    }
    auto &r = registry();
    std::lock_guard lock(r.mtx);
    if(g->failed)
        return; // this source leaves the group at its tick_spectrum and continues on the host
    // a member that comes round again while its last hand-over is still waiting for the rest of the frame completes it
    if(g->submitted[m_slot] == g->batch)
        g->flush();
    const size_t dtsize = hip_sync_frames() * sizeof(float);
    if(m_rms_sync_buf.size() <= dtsize)
        return; // sync_rms_buffer returns false: m_input_rms stays
    const uint32_t b = (uint32_t)(g->batch & 1);
    if(g->n_submitted == 0 && std::all_of(g->sq_frames.begin(), g->sq_frames.end(), [](uint32_t v) { return v == 0; }))
        api().ingest_done(g->h, b); // first writer of this frame: the slot's staging has been copied out (two frames ago)
    size_t consume = (m_rms_sync_buf.size() - dtsize) / sizeof(float);
    const size_t room = g->sq_max - g->sq_frames[m_slot];
    if(consume > room) {
        // more than a window's worth since the last hand-over: only the newest values can still be inside the window
        m_rms_sync_buf.pop_front(nullptr, (consume - room) * sizeof(float));
        consume = room;
    }
    float *dst = g->sq_stage[b] + (size_t)m_slot * g->sq_max + g->sq_frames[m_slot];
    m_rms_sync_buf.pop_front(dst, consume * sizeof(float));
    g->sq_frames[m_slot] += (uint32_t)consume;
}

void WAVSourceHIP::tick_spectrum(float seconds)
{
    if(m_group != nullptr) {
        tick_spectrum_batched(seconds);
        return;
    }
    if(m_hip == nullptr) {
        hip_fall_back({});
        WAVSourceGeneric::tick_spectrum(seconds);
        return;
    }
    auto &a = api();
    const bool hidden = !m_show || hip_timed_out(); // reference :34
    size_t dtframes = 0;
    // Underflow (fewer samples than window + A/V-sync delay, :55-61): every channel is skipped, but unless m_last_silent the
    // reference's end-of-tick pass still runs over the rows as they are -- dbfs of a stale dB value is DB_MIN, and the volume
    // normalisation gain goes on top (:138-179).  The device does the same for a stream marked WF_HIP_STARVED.
    const bool starved = !hidden && !hip_window(dtframes);
    const int state = hidden ? WF_HIP_HIDDEN : (starved ? WF_HIP_STARVED : WF_HIP_SHOWN);
    bool ok = hip_send_state(state);
    if(ok && state == WF_HIP_SHOWN) // the whole window replaces the device ring's newest fft_size samples
        ok = a.push_audio(m_hip, 0, 1, m_hip_window.data(), (uint32_t)m_fft_size) == WF_HIP_OK;
    wf_hip_tick_params p{};
    p.seconds = seconds;
    p.delay_frames = 0;
    p.input_rms = m_input_rms;
    p.flags = 0;
    if(!ok || !hip_tick_and_take_rows(p, m_fft_size / 2)) {
        hip_fall_back(std::string("HIP tick failed (") + a.last_error(m_hip) + "); falling back to the CPU path");
        WAVSourceGeneric::tick_spectrum(seconds);
        return;
    }
    if(m_hip_display) {
        // straight into the members render() draws from (no per-tick allocations, no staging copy)
        if(a.read(m_hip, WF_HIP_OUT_BARS, 0, 1, m_hip_bars.data()) == WF_HIP_OK &&
           (m_hip_per_row == 0 || (a.read(m_hip, WF_HIP_OUT_VERTICES, 0, 1, m_hip_verts.data()) == WF_HIP_OK &&
                                   a.read(m_hip, WF_HIP_OUT_VERTEX_COUNTS, 0, 1, m_hip_vcounts.data()) == WF_HIP_OK)) &&
           (!m_mirror_freq_axis || a.read(m_hip, WF_HIP_OUT_PREMIRROR, 0, 1, m_hip_pre.data()) == WF_HIP_OK))
            hip_publish_display();
        else
            m_hip_display_valid = false; // render() goes back to the host loops over m_decibels
    }
}

// Same observable behaviour as WAVSourceGeneric::tick_meter (src/source_generic.cpp:182-269): the audio that tick_meter
// would pop into its meter buffer this tick (everything older than the A/V-sync point, :201-220) goes to the device ring
// instead; the device takes the level over the last m_fft_size consumed samples, smooths it, converts to dBFS and
// decides m_last_silent; m_meter_val / m_last_silent come back for render_bars (src/source.cpp:1505-1509).
// The batched meter path (struct WFHipMeterGroup): m_meter_val / m_last_silent are the device's results for the previous frame.
void WAVSourceHIP::tick_meter_batched(float seconds)
{
    auto &r = registry();
    std::unique_lock lock(r.mtx);
    WFHipMeterGroup *g = m_mgroup;
    const uint32_t slot = m_slot;
    int last = -1;
    if(!g->begin_tick(slot, m_hip_joined, last)) {
        lock.unlock();
        hip_fall_back("HIP meter batch unavailable; this source continues on the CPU path");
        WAVSourceGeneric::tick_meter(seconds);
        return;
    }
    // 1. collect the levels the last flushed batch left for this source
    if(last >= 0) {
        for(auto channel = 0u; channel < m_capture_channels; ++channel)
            m_meter_val[channel] = g->levels[last][(size_t)slot * g->cap_ch + channel];
        m_last_silent = g->silent[last][slot] != 0;
    }
    // 2. submit this frame: state, and what tick_meter would pop into its meter buffer
    const bool timed_out = hip_timed_out(); // :184
    const uint32_t frames = timed_out ? 0u : hip_pop_meter(g->pending[slot]);
    g->submit(slot, frames, timed_out ? WF_HIP_HIDDEN_TIMEOUT : (m_show ? WF_HIP_SHOWN : WF_HIP_HIDDEN), seconds);
}

void WAVSourceHIP::tick_meter(float seconds)
{
    if(m_mgroup != nullptr) {
        tick_meter_batched(seconds);
        return;
    }
    if(m_hip == nullptr) {
        hip_fall_back({});
        WAVSourceGeneric::tick_meter(seconds);
        return;
    }
    auto &a = api();
    const bool timed_out = hip_timed_out(); // :184
    bool ok = hip_send_state(timed_out ? WF_HIP_HIDDEN_TIMEOUT : (m_show ? WF_HIP_SHOWN : WF_HIP_HIDDEN));
    if(ok && !timed_out) {
        const uint32_t frames = hip_pop_meter(m_hip_window); // moved to the device ring, oldest first
        if(frames > 0)
            ok = a.push_audio(m_hip, 0, 1, m_hip_window.data(), frames) == WF_HIP_OK;
    }
    wf_hip_tick_params p{};
    p.seconds = seconds;
    float levels[2] = {DB_MIN, DB_MIN};
    uint8_t silent = 0;
    if(!ok || a.tick(m_hip, &p) != WF_HIP_OK || a.read(m_hip, WF_HIP_OUT_METER, 0, 1, levels) != WF_HIP_OK ||
       a.read(m_hip, WF_HIP_OUT_LAST_SILENT, 0, 1, &silent) != WF_HIP_OK) {
        hip_fall_back(std::string("HIP meter tick failed (") + a.last_error(m_hip) + "); falling back to the CPU path");
        WAVSourceGeneric::tick_meter(seconds);
        return;
    }
    for(auto channel = 0u; channel < m_capture_channels; ++channel)
        m_meter_val[channel] = levels[channel];
    m_last_silent = silent != 0;
}

// The batched waveform path (struct WFHipMeterGroup with cfg.waveform): m_decibels / m_last_silent are the device's results for
// the previous video frame.  What this frame hands over is exactly what the synchronous path below pushes inside the call.
void WAVSourceHIP::tick_waveform_batched(float seconds)
{
    auto &r = registry();
    std::unique_lock lock(r.mtx);
    WFHipMeterGroup *g = m_mgroup;
    const uint32_t slot = m_slot;
    int last = -1;
    if(!g->begin_tick(slot, m_hip_joined, last)) {
        lock.unlock();
        hip_fall_back("HIP waveform batch unavailable; this source continues on the CPU path");
        WAVSourceGeneric::tick_waveform(seconds);
        return;
    }
    // 1. collect the rows the last flushed batch left for this source
    if(last >= 0)
        hip_take_rows(g->rows[last] + (size_t)slot * g->out_ch * g->width, m_fft_size, g->silent[last][slot] != 0);
    // 2. submit this frame
    const bool hidden = !m_show || hip_timed_out(); // :279
    uint8_t st = hidden ? WF_HIP_HIDDEN : WF_HIP_SHOWN;
    uint32_t fresh = 0;
    if(!hidden) {
        const size_t reserve = hip_sync_frames();
        if(m_waveform_samples + reserve > g->ring_cap) {
            // wf_hip_set_stream_delay would reject the whole batch for this one stream (an A/V-sync reserve beyond what the
            // device rings were sized for): only THIS source leaves -- nothing of it has been staged or popped yet, so the
            // reference's tick_waveform takes the frame over from m_capturebufs as they are, with m_decibels as step 1 left
            // them (the previous frame's rows) and the sweep position the device kept for it (one 8-byte read that waits for
            // the last batch: this happens once) -- and the group's other members never notice
            uint64_t wts = 0;
            if(api().read(g->h, WF_HIP_OUT_WAVEFORM_TS, slot, 1, &wts) == WF_HIP_OK)
                m_waveform_ts = (size_t)wts; // (else 0: the reference catches up by itself, src/source_generic.cpp:318-321)
            const uint32_t ring_cap = g->ring_cap;
            lock.unlock();
            hip_fall_back("HIP waveform batch: this source's A/V-sync reserve (" + std::to_string(reserve) + " frames) does not fit the device ring (" +
                          std::to_string(ring_cap) + "); it continues on the CPU path");
            WAVSourceGeneric::tick_waveform(seconds);
            return;
        }
        if(!hip_wave_fresh(reserve, g->pending[slot])) {
            st = WF_HIP_PAUSED;
        } else {
            fresh = (uint32_t)(g->pending[slot].size() / m_capture_channels);
            g->delay[slot] = (uint32_t)reserve;
            g->audio_ts[slot] = m_audio_ts;
        }
    }
    g->submit(slot, fresh, st, seconds);
}

// Same observable behaviour as WAVSourceGeneric::tick_waveform (src/source_generic.cpp:271-390).  The device ring mirrors
// m_capturebufs: every tick the frames captured since the last one are appended to it (hip_wave_fresh), the device picks the new
// points from its ring exactly where the reference picks them from its scratch copy (both count back from the newest sample),
// and m_capturebufs is popped down to the A/V-sync reserve as the reference does (:321).  m_waveform_ts lives on the device.
void WAVSourceHIP::tick_waveform(float seconds)
{
    if(m_mgroup != nullptr) {
        tick_waveform_batched(seconds);
        return;
    }
    if(m_hip == nullptr) {
        hip_fall_back({});
        WAVSourceGeneric::tick_waveform(seconds);
        return;
    }
    auto &a = api();
    const bool hidden = !m_show || hip_timed_out(); // :279
    bool ok = hip_send_state(hidden ? WF_HIP_HIDDEN : WF_HIP_SHOWN);
    wf_hip_tick_params p{};
    p.seconds = seconds;
    p.input_rms = m_input_rms;
    p.audio_ts_ns = m_audio_ts;
    if(ok && !hidden) {
        const size_t reserve = hip_sync_frames();
        if(!hip_wave_fresh(reserve, m_hip_window))
            return;
        if(!m_hip_window.empty())
            ok = a.push_audio(m_hip, 0, 1, m_hip_window.data(), (uint32_t)(m_hip_window.size() / m_capture_channels)) == WF_HIP_OK;
        p.delay_frames = (uint32_t)reserve;
    }
    if(!ok || !hip_tick_and_take_rows(p, m_fft_size)) {
        hip_fall_back(std::string("HIP waveform tick failed (") + a.last_error(m_hip) + "); falling back to the CPU path");
        return; // the audio of this tick has been consumed; the CPU path takes over at the next one
    }
    // (no device display here: hip_configure builds one for spectrum displays only, the waveform's points are the rows)
}
