// tests/mock/mock_wf_hip.cpp -- TEST HARNESS: a host-only stand-in for libwaveform_hip.so with the entry points the reference-side
// binding (host/wav_source_hip.cpp) resolves, so that the binding -- its process-wide group registry, the registry mutex against
// every source's m_mtx, members joining and leaving batches, the double-buffered staging -- runs on a GPU-less box under
// ThreadSanitizer (tests/test_sanitizers.py; the HIP runtime itself does not start under that tool).  A stream's rows are a
// deterministic function of the audio it has received since its last reset, so the stress test's "a source that survived the
// chaos equals a fresh one" check means something here too.  Nothing here is product code.
//
// A plain build of this file (build/libwfhip_mock_plain.so) also records HOW the binding called it: a running hash over every entry
// point it came in through -- the scalar arguments and the contents of the arrays (staged audio up to each stream's frame count,
// state masks, delays, timestamps, RMS values, squared peaks, tick parameters), handles by their order of creation, never an
// address -- read with wf_hip_mock_trace() (tests/test_host_groups_mock_cpu.py).  Two environment knobs, both off by default:
//   WF_MOCK_RMS_FEED=1    wf_hip_enable_input_rms succeeds (the device RMS feed of WAVSourceHIP::update_input_rms)
//   WF_MOCK_FAIL_TICK=N   the N-th wf_hip_tick of the process fails (a group fails, its members fall back)
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "wf_hip.h"

struct wf_hip {
    wf_config cfg{};
    uint32_t n = 0, N = 0, M = 0, cap = 1, out = 1, disp = 1, bars = 0;
    uint64_t id = 0;                // the handle's place in the order of creation: what the call trace knows it by
    bool rms_feed = false;
    std::vector<uint64_t> sum;      // per stream: a checksum of everything pushed since the reset
    std::vector<uint64_t> rsum;     // per stream: likewise for the squared peaks of the RMS feed
    std::vector<uint8_t> state, silent;
    std::vector<float> rows;        // [n][out][M]
    std::string err;
};
static thread_local std::string g_err;

static uint64_t mix(uint64_t h, const float *p, size_t n)
{
    for(size_t i = 0; i < n; ++i) {
        uint32_t u;
        std::memcpy(&u, p + i, 4);
        h = (h ^ u) * 1099511628211ull;
    }
    return h;
}

// the call trace: one running hash for the process, taken under its mutex for the length of an entry
static std::mutex g_trace_mtx;
static uint64_t g_trace = 1469598103934665603ull, g_handles = 0, g_ticks = 0;
struct Trace {
    std::lock_guard<std::mutex> lock{g_trace_mtx};
    explicit Trace(const char *entry, const wf_hip *h = nullptr)
    {
        bytes(entry, std::strlen(entry));
        u(h ? h->id : 0);
    }
    void bytes(const void *p, size_t n)
    {
        const unsigned char *c = static_cast<const unsigned char *>(p);
        for(size_t i = 0; i < n; ++i)
            g_trace = (g_trace ^ c[i]) * 1099511628211ull;
    }
    void u(uint64_t v) { bytes(&v, sizeof(v)); }
    void f(float v) { bytes(&v, sizeof(v)); }
    template<class T> void arr(const T *p, size_t n) { bytes(p, n * sizeof(T)); }
};

extern "C" {
uint64_t wf_hip_mock_trace(void)
{
    std::lock_guard<std::mutex> lock(g_trace_mtx);
    return g_trace;
}
int wf_hip_abi_version(void) { return WF_HIP_ABI_VERSION; }
int wf_hip_device_count(void)
{
    Trace t("device_count");
    return 1;
}
const char *wf_hip_last_error(const wf_hip *h)
{
    Trace t("last_error", h);
    return h ? h->err.c_str() : g_err.c_str();
}
int wf_hip_create(const wf_config *cfg, int device, uint32_t max_streams, uint32_t ring_frames, wf_hip **out)
{
    auto *h = new wf_hip;
    {
        Trace t("create");
        h->id = ++g_handles;
        t.u(h->id);
        t.bytes(cfg, sizeof(*cfg));
        t.u((uint64_t)(int64_t)device);
        t.u(max_streams);
        t.u(ring_frames);
    }
    h->cfg = *cfg;
    h->n = max_streams;
    h->N = cfg->fft_size;
    h->M = cfg->waveform ? cfg->fft_size : cfg->fft_size / 2;
    h->cap = cfg->capture_channels;
    h->out = (cfg->capture_channels > 1 || cfg->stereo) ? 2u : 1u;
    h->disp = cfg->stereo ? 2u : 1u;
    h->bars = cfg->bars ? 26u : (cfg->curve ? cfg->width : 0u);
    h->sum.assign(h->n, 1469598103934665603ull);
    h->rsum.assign(h->n, 1469598103934665603ull);
    h->state.assign(h->n, 0);
    h->silent.assign(h->n, 0);
    h->rows.assign((size_t)h->n * h->out * h->M, -758.0f);
    *out = h;
    return WF_HIP_OK;
}
void wf_hip_destroy(wf_hip *h)
{
    {
        Trace t("destroy", h);
    }
    delete h;
}
int wf_hip_reset(wf_hip *h, uint32_t first, uint32_t count)
{
    {
        Trace t("reset", h);
        t.u(first);
        t.u(count);
    }
    for(uint32_t s = first; s < first + count; ++s) {
        h->sum[s] = 1469598103934665603ull;
        h->rsum[s] = 1469598103934665603ull;
        h->state[s] = 0;
        h->silent[s] = 0;
        for(size_t k = 0; k < (size_t)h->out * h->M; ++k)
            h->rows[(size_t)s * h->out * h->M + k] = -758.0f;
    }
    return WF_HIP_OK;
}
static uint32_t vertices_of(const wf_hip *h) { return (h->cfg.vertices && h->cfg.bars) ? h->bars * 6u : 0u; }
uint32_t wf_hip_output_channels(const wf_hip *h)
{
    Trace t("output_channels", h);
    return h->out;
}
uint32_t wf_hip_display_channels(const wf_hip *h)
{
    Trace t("display_channels", h);
    return h->disp;
}
uint32_t wf_hip_num_bars(const wf_hip *h)
{
    Trace t("num_bars", h);
    return h->bars;
}
uint32_t wf_hip_num_vertices(const wf_hip *h)
{
    Trace t("num_vertices", h);
    return vertices_of(h);
}
void *wf_hip_host_alloc(size_t bytes)
{
    {
        Trace t("host_alloc");
        t.u(bytes);
    }
    return std::calloc(bytes ? bytes : 1, 1);
}
void wf_hip_host_free(void *p)
{
    {
        Trace t("host_free");
    }
    std::free(p);
}
int wf_hip_push_audio(wf_hip *h, uint32_t first, uint32_t count, const float *samples, uint32_t frames)
{
    {
        Trace t("push_audio", h);
        t.u(first);
        t.u(count);
        t.u(frames);
        t.arr(samples, (size_t)count * h->cap * frames);
    }
    for(uint32_t s = 0; s < count; ++s)
        h->sum[first + s] = mix(h->sum[first + s], samples + (size_t)s * h->cap * frames, (size_t)h->cap * frames);
    return WF_HIP_OK;
}
int wf_hip_push_audio_ragged_async(wf_hip *h, uint32_t first, uint32_t count, const float *p, const uint32_t *frames, uint32_t max_frames, uint32_t slot)
{
    {
        Trace t("push_audio_ragged_async", h);
        t.u(first);
        t.u(count);
        t.u(max_frames);
        t.u(slot);
        t.arr(frames, count);
        for(uint32_t s = 0; s < count; ++s)
            for(uint32_t c = 0; c < h->cap; ++c)
                t.arr(p + ((size_t)s * h->cap + c) * max_frames, frames[s]);
    }
    for(uint32_t s = 0; s < count; ++s)
        for(uint32_t c = 0; c < h->cap; ++c)
            h->sum[first + s] = mix(h->sum[first + s], p + ((size_t)s * h->cap + c) * max_frames, frames[s]);
    return WF_HIP_OK;
}
int wf_hip_ingest_done(wf_hip *h, uint32_t slot)
{
    Trace t("ingest_done", h);
    t.u(slot);
    return WF_HIP_OK;
}
int wf_hip_readback_done(wf_hip *h, uint32_t slot)
{
    Trace t("readback_done", h);
    t.u(slot);
    return WF_HIP_OK;
}
int wf_hip_set_hidden(wf_hip *h, uint32_t first, uint32_t count, const uint8_t *mask)
{
    Trace t("set_hidden", h);
    t.u(first);
    t.u(count);
    t.arr(mask, count);
    for(uint32_t i = 0; i < count; ++i)
        h->state[first + i] = mask[i];
    return WF_HIP_OK;
}
int wf_hip_set_input_rms(wf_hip *h, uint32_t first, uint32_t count, const float *rms)
{
    Trace t("set_input_rms", h);
    t.u(first);
    t.u(count);
    t.arr(rms, count);
    return WF_HIP_OK;
}
int wf_hip_enable_input_rms(wf_hip *h, int feed)
{
    Trace t("enable_input_rms", h);
    t.u((uint64_t)(int64_t)feed);
    const char *e = std::getenv("WF_MOCK_RMS_FEED");
    if(e != nullptr && e[0] == '1') {
        h->rms_feed = true;
        return WF_HIP_OK;
    }
    h->err = "mock: no device RMS producer";
    return WF_HIP_ERR_UNSUPPORTED;
}
int wf_hip_push_rms_ragged_async(wf_hip *h, uint32_t first, uint32_t count, const float *p, const uint32_t *frames, uint32_t max_frames, uint32_t slot)
{
    Trace t("push_rms_ragged_async", h);
    t.u(first);
    t.u(count);
    t.u(max_frames);
    t.u(slot);
    t.arr(frames, count);
    for(uint32_t s = 0; s < count; ++s) {
        t.arr(p + (size_t)s * max_frames, frames[s]);
        h->rsum[first + s] = mix(h->rsum[first + s], p + (size_t)s * max_frames, frames[s]);
    }
    return WF_HIP_OK;
}
int wf_hip_set_stream_delay(wf_hip *h, uint32_t first, uint32_t count, const uint32_t *delay)
{
    Trace t("set_stream_delay", h);
    t.u(first);
    t.u(count);
    t.arr(delay, count);
    return WF_HIP_OK;
}
int wf_hip_set_stream_audio_ts(wf_hip *h, uint32_t first, uint32_t count, const uint64_t *ts)
{
    Trace t("set_stream_audio_ts", h);
    t.u(first);
    t.u(count);
    t.arr(ts, count);
    return WF_HIP_OK;
}
int wf_hip_tick(wf_hip *h, const wf_hip_tick_params *p)
{
    {
        Trace t("tick", h);
        t.f(p->seconds);
        t.u(p->delay_frames);
        t.f(p->input_rms);
        t.u(p->flags);
        t.u(p->audio_ts_ns);
        const char *e = std::getenv("WF_MOCK_FAIL_TICK");
        if(++g_ticks == (e ? std::strtoull(e, nullptr, 10) : 0)) {
            h->err = "mock: this tick was told to fail";
            return WF_HIP_ERR_RUNTIME;
        }
    }
    for(uint32_t s = 0; s < h->n; ++s) {
        if(h->state[s] == WF_HIP_PAUSED)
            continue;
        const bool hidden = h->state[s] == WF_HIP_HIDDEN || h->state[s] == WF_HIP_HIDDEN_TIMEOUT;
        h->silent[s] = hidden ? 1 : 0;
        float *r = h->rows.data() + (size_t)s * h->out * h->M;
        for(size_t k = 0; k < (size_t)h->out * h->M; ++k)
            r[k] = hidden ? -758.0f : -20.0f - (float)((h->sum[s] + k) % 97u);
    }
    return WF_HIP_OK;
}
uint32_t wf_hip_ring_frames(const wf_hip *h)
{
    Trace t("ring_frames", h);
    return 1u << 20;
}
int wf_hip_set_bars_mirrors(wf_hip *, uint32_t, void *const *, void *const *) { return WF_HIP_ERR_UNSUPPORTED; }
int wf_hip_bars_mirror_ready(wf_hip *, void *, void **) { return WF_HIP_ERR_INVALID; }
// the one reader: every output a deterministic function of what the stream has received
static int read_out(wf_hip *h, wf_hip_output what, uint32_t first, uint32_t count, void *out_)
{
    switch(what) {
    case WF_HIP_OUT_DECIBELS:
        std::memcpy(out_, h->rows.data() + (size_t)first * h->out * h->M, (size_t)count * h->out * h->M * sizeof(float));
        return WF_HIP_OK;
    case WF_HIP_OUT_LAST_SILENT:
        std::memcpy(out_, h->silent.data() + first, count);
        return WF_HIP_OK;
    case WF_HIP_OUT_PREMIRROR:
        std::memset(out_, 0, (size_t)count * h->disp * sizeof(float));
        return WF_HIP_OK;
    case WF_HIP_OUT_INPUT_RMS: { // 0 as ever without the feed; with it a function of the squared peaks the stream was fed
        float *out = static_cast<float *>(out_);
        for(uint32_t i = 0; i < count; ++i)
            out[i] = h->rms_feed ? 0.001f * (float)(h->rsum[first + i] % 1000u) : 0.0f;
        return WF_HIP_OK;
    }
    case WF_HIP_OUT_WAVEFORM_TS:
        std::memset(out_, 0, (size_t)count * sizeof(uint64_t));
        return WF_HIP_OK;
    case WF_HIP_OUT_METER: {
        float *out = static_cast<float *>(out_);
        for(uint32_t i = 0; i < count * h->cap; ++i)
            out[i] = -20.0f - (float)(h->sum[first + i / h->cap] % 31u);
        return WF_HIP_OK;
    }
    case WF_HIP_OUT_BARS: {
        float *out = static_cast<float *>(out_);
        for(size_t i = 0; i < (size_t)count * h->disp * h->bars; ++i)
            out[i] = 10.0f + (float)((h->sum[first + i / ((size_t)h->disp * h->bars)] + i) % 200u);
        return WF_HIP_OK;
    }
    case WF_HIP_OUT_VERTICES:
        std::memset(out_, 0, (size_t)count * h->disp * vertices_of(h) * 4 * sizeof(float));
        return WF_HIP_OK;
    case WF_HIP_OUT_VERTEX_COUNTS: {
        uint32_t *out = static_cast<uint32_t *>(out_);
        for(uint32_t i = 0; i < count * h->disp; ++i)
            out[i] = vertices_of(h);
        return WF_HIP_OK;
    }
    default: return WF_HIP_ERR_INVALID;
    }
}
int wf_hip_read(wf_hip *h, wf_hip_output what, uint32_t first, uint32_t count, void *out_)
{
    {
        Trace t("read", h);
        t.u((uint64_t)what);
        t.u(first);
        t.u(count);
    }
    return read_out(h, what, first, count, out_);
}
// the pipelined reader: the mock copies at once
int wf_hip_read_async(wf_hip *h, uint32_t first, uint32_t count, const wf_hip_readback *d, uint32_t slot)
{
    {
        Trace t("read_async", h);
        t.u(first);
        t.u(count);
        t.u(slot);
        // which outputs were asked for (the destinations themselves are addresses)
        t.u((d->rows ? 1u : 0u) | (d->last_silent ? 2u : 0u) | (d->bars ? 4u : 0u) | (d->premirror ? 8u : 0u) | (d->vertices ? 16u : 0u) |
            (d->vertex_counts ? 32u : 0u) | (d->input_rms ? 64u : 0u) | (d->meter ? 128u : 0u));
    }
    if(d->rows) read_out(h, WF_HIP_OUT_DECIBELS, first, count, d->rows);
    if(d->last_silent) read_out(h, WF_HIP_OUT_LAST_SILENT, first, count, d->last_silent);
    if(d->bars) read_out(h, WF_HIP_OUT_BARS, first, count, d->bars);
    if(d->premirror) read_out(h, WF_HIP_OUT_PREMIRROR, first, count, d->premirror);
    if(d->vertices) read_out(h, WF_HIP_OUT_VERTICES, first, count, d->vertices);
    if(d->vertex_counts) read_out(h, WF_HIP_OUT_VERTEX_COUNTS, first, count, d->vertex_counts);
    if(d->input_rms) read_out(h, WF_HIP_OUT_INPUT_RMS, first, count, d->input_rms);
    if(d->meter) read_out(h, WF_HIP_OUT_METER, first, count, d->meter);
    return WF_HIP_OK;
}
}
