// wf_hip_internal.hpp -- what the translation units of libwaveform_hip.so share: the handle -- which holds the kernels' argument
// structs themselves (wf_hip::tick and the four small ones: a value fixed at create lives there and nowhere else) --, the error helpers and the
// functions by which the plan (wf_hip_plan.hip), the entry points (wf_hip.hip; the measurement outputs: wf_hip_measure.hip) and the kernel dispatch (wf_tick_geom.hip, one
// object per FFT geometry; wf_big_dispatch.hip for the transforms beyond a CU's LDS) call each other.  Not installed: the
// library's interface is include/wf_hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "wf_hip.h"

namespace wf { struct LoudState; struct LoudHist; } // (wf_loudness.hpp: device code, seen by wf_hip_measure.hip alone)
// MeterArgs, WaveArgs, VertexArgs and RmsArgs of this handle: their headers define kernels, so wf_hip.hip alone sees the type
namespace wf::host { struct SmallArgs; }
#include "wf_dev_guard.hpp"
#include "wf_host_tables.hpp"
#include "wf_loudness_tables.hpp"
#include "wf_tick_args.hpp" // TickArgs, BarsOnlyState (plain structs, no device code)
#include "wf_tick_plan.hpp"

struct wf_hip {
    wf_config cfg{};
    wf::HostTables tab;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_bars_lane[4] = {nullptr, nullptr, nullptr, nullptr}; // wf_hip_copy_bars_device_async: a lane's part of the copy has been made
    // Lanes: a large batch is ticked as n_lanes slices of streams, slice 0 on `stream`, the others on their own HIP streams.
    // Consecutive ticks of a slice are ordered by its stream; slices share nothing, so while no other call intervenes the
    // tail of one slice's launch overlaps the head of another's (a lone launch leaves the chip draining for a workgroup's
    // lifetime at both ends).  Every other entry point first makes `stream` wait for the lanes (join_lanes) and the next
    // tick makes the lanes wait for `stream`: outside wf_hip_tick the handle behaves as if it had the one stream.
    static constexpr int MAX_LANES = wf::MAX_LANES;
    int n_lanes = 1;
    uint32_t wg_lds = 0, wg_threads = 0; // dynamic LDS and threads of one workgroup of the tick kernel (how many fit a CU)
    hipStream_t lane_stream[MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_lane[MAX_LANES] = {nullptr, nullptr, nullptr, nullptr}, ev_fork = nullptr;
    bool lanes_pending = false; // a lane holds work `stream` has not waited for
    bool main_dirty = true;     // `stream` holds work the lanes have not waited for
    // pipelined ingest (wf_hip_push_audio_async and the other pushes from page-locked memory; wf_hip.hip, "pipelined ingest"):
    // a copy stream and two slots, used alternately by the caller
    struct IngestSlot {
        float *d_stage = nullptr;         // device staging block: filled on the copy stream, read by the kernels on `stream`
        size_t stage_floats = 0;
        uint32_t *d_frames = nullptr;     // ragged pushes: per-stream frame counts ...
        uint32_t *h_frames = nullptr;     // ... and the page-locked copy their H2D reads from
        size_t frames_cap = 0;
        hipEvent_t ev_consumed = nullptr; // the kernels that read the slot's staging have finished
        bool used = false;                // ev_consumed has been recorded
    };
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_copied[2] = {nullptr, nullptr}; // the slot's last H2D copy, of samples or of squared peaks, has finished (host
                                                  // buffer free, staging full): wf_hip_ingest_done waits for it
    IngestSlot ingest_slot[2];                    // audio, float or PCM
    IngestSlot sq_slot[2];                        // the squared peaks of wf_hip_push_rms_ragged_async ([count][max_frames])
    // pipelined readback (wf_hip_read_async; wf_hip.hip, "pipelined readback"): a stream for the D2H copies and two slots, used
    // alternately by the caller
    struct ReadSlot {
        float *d_snap = nullptr;          // snapshot of the bars alone or of the meter levels: filled on `stream`, copied out on read_stream
        size_t snap_floats = 0;
        uint8_t *d_silent = nullptr;      // m_last_silent as bytes (rows and meter readbacks): filled and copied out the same way
        size_t silent_bytes = 0;
        hipEvent_t ev_snap = nullptr;     // `stream` has produced what the slot's copies read
        hipEvent_t ev_read = nullptr;     // the slot's last D2H copy has landed: wf_hip_readback_done waits for it
        bool used = false;                // ev_read has been recorded
        bool rows_in_flight = false;      // the copies read the rows (bars, vertices ...) in place: the next tick waits for ev_read
    };
    hipStream_t read_stream = nullptr;
    ReadSlot read_slot[2];
    uint32_t n_streams = 0;
    uint32_t ring_cap = 0;
    uint32_t ring_stride = 0;        // floats between consecutive rings: ring_cap + padding (see wf_hip_create)
    uint32_t N = 0, M = 0;
    uint32_t cap_ch = 1, out_ch = 1, disp_ch = 1;
    uint32_t num_bars = 0;
    bool all_aligned = true; // every push so far was a multiple of 4 frames
    // The kernels' arguments.  What is fixed at create and used only as a kernel argument -- tables, layout flags, sizes,
    // coefficients -- is written into these structs where it is decided or uploaded, and read from them; the handle keeps no
    // copy.  What can change after create, or is read by other entry points (the d_* fields below, the flag rotation, the
    // mirrors), stays a handle field and is patched into a copy per tick (wf_hip.hip: tick_args and its kin).
    wf::TransformPlan plan;          // which transform family runs the batch, decided once (wf_tick_plan.hpp)
    wf::TickArgs tick{};             // spectrum batches
    std::shared_ptr<wf::host::SmallArgs> small; // the same for the level meter, the waveform display, the vertex fill and the RMS producer
    // the display decisions that are no kernel arguments; the second display plan (ext_outputs) starts from a default one
    struct DisplayPlan {
        bool ext_outputs = false;    // the outputs are derived from the stored rows by big_outputs_kernel behind the tick kernel
                                     // (displays whose staging does not fit the tick kernel's exchange buffer)
        size_t big_out_lds = 0;      // dynamic LDS of big_outputs_kernel
    } disp;
    // device memory
    float *d_ring = nullptr;
    uint32_t *d_wpos = nullptr;
    float *d_tsmooth = nullptr;
    float *d_decibels = nullptr;
    uint32_t *d_flags = nullptr;     // [flag_bufs][n_streams]; the buffer flag_cur holds the current m_last_silent / hidden bits
    uint32_t *d_verdict = nullptr;   // split mode: [3][n_streams * cap_ch] "row has a value > floor - 10" (TickArgs::verdict_*)
    uint32_t flag_bufs = 1, flag_cur = 0;
    // bars-only ticks on a batch that does not run split: per-wavefront row verdicts (TickArgs::row_verdict), allocated by the
    // first tick that carries WF_HIP_TICK_NO_DECIBELS; from the tick after it the silence test reads them instead of the rows
    uint32_t *d_row_verdict = nullptr;
    float *d_stale_row = nullptr;    // [M] of DB_MIN (BarsOnlyState::stale_row), allocated with the first bars-only tick
    wf::BarsOnlyState *d_bars_only = nullptr; // the kernel's view of the three fields above
    uint32_t waves_per_spectrum = 1;
    bool verdict_tracking = false;
    bool split = false;              // the channels of a stream run in different workgroups (spectrum_tick_kernel<.., SPLIT>)
    int interp_shape[2] = {0, 0};    // {tab.interp_radius, tab.interp_taps} (WF_HIP_TABLE_INTERP_SHAPE)
    float *d_bars = nullptr;
    float *d_bars_pre = nullptr;    // BarArgs::pre_out: [n_streams][disp_ch], mirrored displays only
    // wf_hip_set_bars_mirrors: the caller-owned buffers the ticks also write their bars into -- the mirror_n buffers of the write
    // set; wf_hip_bars_mirror_ready hands the write set over and makes the other one the write set
    float *bars_mirror[2][8] = {};
    uint32_t mirror_n = 0;
    uint32_t mirror_next = 0;       // the set the ticks write
    bool mirror_fresh = false;      // a tick has written set mirror_next since it became the write set
    wf::f4 *d_verts = nullptr;
    uint32_t *d_vert_counts = nullptr; // [n_streams][disp_ch] vertices of each row's draw call
    uint32_t *d_delay = nullptr;     // [n_streams] A/V-sync delay per stream (wf_hip_set_stream_delay), or nullptr
    uint32_t max_stream_delay = 0;   // largest value ever set (ring-capacity check of the tick)
    unsigned long long *d_audio_ts = nullptr; // [n_streams] m_audio_ts per stream of a waveform batch (wf_hip_set_stream_audio_ts), or nullptr
    bool stream_delays_aligned = true; // all of them multiples of 4 frames (vector fetch without straddling)
    float *d_vol_comp = nullptr;     // [n_streams] volume compensation per stream (wf_hip_set_input_rms), or nullptr
    // volume-normalisation producer on the device (wf_hip_enable_input_rms): update_input_rms per stream and tick
    float *d_rms_ring = nullptr;     // [n_streams][rms_cap] squared peaks (capture_audio's m_rms_sync_buf)
    float *d_rms_bsum = nullptr;     // [n_streams][rms_cap / RMS_BLOCK]
    uint32_t *d_rend = nullptr;      // [n_streams] consumption point of sync_rms_buffer
    bool rms_feed = false;           // the squared peaks come from the host (wf_hip_push_rms_ragged_async), not from the pushed audio
    float *d_input_rms = nullptr;    // [n_streams] m_input_rms
    // the measurement outputs (wf_hip_measure.hip): the block of each row of its table, [n_streams] entries or
    // [n_streams][out_ch], allocated by the output's first read, which also runs the row's setup (measure_ready: it has succeeded)
    // (N_MEASURES: the rows of that table, WF_HIP_OUT_LOUDNESS to the last wf_hip_output; a static_assert there holds the two together)
    static constexpr int N_MEASURES = 20;
    char *d_measure[N_MEASURES] = {};
    bool measure_ready[N_MEASURES] = {};
    // the loudness producer (wf_hip_enable_loudness; wf_loudness.hpp), d_state == nullptr while it is off
    struct Loudness {
        wf::LoudState *d_state = nullptr;         // [n_streams]
        wf::LoudHist *d_hist = nullptr;           // [n_streams][2]: integrated, range
        wf::LoudCoefs k{};
    } loud;
    // what WF_HIP_OUT_BANDS derives from the configuration (setup_bands, at its first read: wf::host::bands_tables; wf_bands.hpp)
    struct Bands {
        double *d_edges = nullptr;                // [WF_HIP_NUM_BANDS + 1] the band edges in bins
        double *d_weights = nullptr;              // [M][2] the squared A and C weights of every bin
        uint32_t covered = 0;                     // wf_hip_bands::covered of this batch
        double enbw = 1.0;                        // the window's equivalent noise bandwidth in bins
    } bands;
    // what WF_HIP_OUT_STEREO derives from the configuration (setup_stereo, at its first read: wf::host::stereo_tables; wf_stereo.hpp)
    struct Stereo {
        double *d_tab = nullptr;                  // [P] window, [P / 2][2] twiddles, [WF_HIP_NUM_BANDS + 1] band edges in bins of P
        uint32_t P = 0, log2p = 0;                // the window: a power of two
        uint32_t covered = 0;                     // wf_hip_stereo::covered of this batch
    } stereo;
    // what WF_HIP_OUT_CQ derives from the configuration and the ring (setup_cq, at its first read: wf::host::cq_tables; wf_cq.hpp)
    struct Cq {
        double *d_tab = nullptr;                  // [end_covered][WF_CQ_BIN_DOUBLES] steps, 4 / L_b, L_b and the lanes' start values
        uint32_t *d_sched = nullptr;              // [WF_CQ_SCHED_WORDS] which wave takes which bins, in which order
        uint32_t max_window = 0;                  // Lmax
        uint32_t end_covered = 0, first_resolved = 0;
    } cq;
    // what WF_HIP_OUT_SONO derives from the sample rate and the ring (setup_sono, at its first read: wf::host::sono_tables; wf_sono.hpp)
    struct Sono {
        double *d_tab = nullptr;                  // [P] window, [P / 2][2] twiddles, [WF_HIP_SONO_BANDS + 1] band edges in bins of P
        uint32_t columns = 0;                     // T
        uint32_t first_covered = 0, end_covered = 0;
    } sono;
    // what WF_HIP_OUT_THD and WF_HIP_OUT_IMD derive from the configuration (setup_thd or setup_imd, whichever output is read
    // first: wf::host::thd_tables; wf_thd.hpp, wf_imd.hpp)
    struct Thd {
        double *d_tab = nullptr;                  // [P] taper, [P / 2][2] twiddles
        uint32_t P = 0, log2p = 0;                // the window: a power of two
        double S = 0.0;                           // P sum w^2 / 4: the lobe power of a sine of amplitude 1
    } thd;
    // what WF_HIP_OUT_DELAY derives from the configuration (setup_delay, at its first read: wf::host::delay_tables; wf_delay.hpp)
    struct Delay {
        double *d_tab = nullptr;                  // [P] taper, [P / 2][2] twiddles
        uint32_t P = 0, log2p = 0;                // the window: a power of two
    } delay;
    // what WF_HIP_OUT_ONSET derives from the sample rate and the ring (setup_onset, at its first read: wf::host::sono_tables; wf_onset.hpp)
    struct Onset {
        double *d_tab = nullptr;                  // [P] window, [P / 2][2] twiddles, [WF_HIP_ONSET_BANDS + 1] band edges in bins of P
        uint32_t spectral = 0;                    // Ts = T + 1 spectral columns
    } onset;
    // what WF_HIP_OUT_TEMPO derives from the sample rate and the ring (setup_tempo, at its first read: wf::host::sono_tables and
    // wf::host::tempo_tables; wf_tempo.hpp)
    struct Tempo {
        double *d_tab = nullptr;                  // [P] window, [P / 2][2] twiddles, [WF_HIP_ONSET_BANDS + 1] band edges in bins of P
        double *d_prior = nullptr;                // [WF_HIP_TEMPO_MAX_LAG + 1] w[L]
        float *d_strength = nullptr;              // [n_streams][WF_HIP_TEMPO_COLUMNS] the columns kernel's strengths, by age
        uint32_t columns = 0;                     // T
        uint32_t lag_lo = 0, lag_hi = 0;
    } tempo;
    // what WF_HIP_OUT_HUM derives from the sample rate and the ring (setup_hum, at its first read: wf::host::hum_tables; wf_hum.hpp)
    struct Hum {
        double *d_tw = nullptr;                   // [M / 2][2] twiddles of the M-point transform
        double *d_comb = nullptr;                 // [D][K + 2][2] the combination twiddles W_N^(r k), k = -1 .. K
        uint32_t *d_ranges = nullptr;             // [2][16] the bins searched for every (family, harmonic): first, then last
        uint32_t D = 0, N = 0, M = 0, log2m = 0, K = 0;
        uint32_t noise_lo = 0, noise_hi = 0;
        double hz = 0.0;
    } hum;
    // what WF_HIP_OUT_XFER and WF_HIP_OUT_IMPULSE derive from the configuration and the ring (setup_xfer_plan, at each output's first
    // read: wf::host::delay_tables at their own P; wf_xfer.hpp, wf_impulse.hpp).  A plan and a block each, so that neither output
    // needs the other read first
    struct XferPlan {
        double *d_tab = nullptr;                  // [P] taper, [P / 2][2] twiddles
        uint32_t P = 0, log2p = 0;                // the segment: a power of two
        uint32_t K = 0;                           // segments
    } xfer, impulse;
    uint32_t rms_cap = 0, rms_size = 0;
    // waveform batches (cfg.waveform): N = M = width (points per row), there is no FFT state
    bool wave = false;
    uint32_t *d_cend = nullptr;      // [n_streams] samples consumed so far
    unsigned long long *d_wts = nullptr; // [n_streams] m_waveform_ts
    // level-meter batches (cfg.meter): N is the meter buffer length, there is no FFT state
    bool meter = false;
    uint32_t *d_mend = nullptr;      // [n_streams] consumption point of tick_meter
    float *d_meter_buf = nullptr;    // [n_streams * cap_ch] m_meter_buf
    float *d_meter_val = nullptr;    // [n_streams * cap_ch] m_meter_val
    // The device copies of the window (and, for Bluestein, chirped-window) tables carry a power-of-two factor and the magnitude
    // coefficient its inverse: scaling by 2^k is exact, the transform is linear, and |X|^2 = re^2 + im^2 -- the one place where
    // the path squares -- then stays representable down to |X| ~ 1e-31 instead of ~1e-19 (hypotf in the reference answers for
    // the whole float range: the first ticks behind a reset through a narrow window, a few samples under sin^16 tails, give
    // |X| ~ 1e-26).  Headroom: N * amplitude * in_scale squared must stay below FLT_MAX; the factor is 2^40 up to 4096 samples and
    // halves with every doubling beyond (wf::plan_transform), which keeps the overflow point at an amplitude of 4096 (+72 dBFS) from
    // 4096 samples up (the reference's hypotf overflows far later still: a stated deviation).  (plan.in_scale)
    uint8_t *d_mask = nullptr;
    size_t mask_bytes = 0;
    float *d_stage = nullptr;
    size_t stage_floats = 0;
    // per-stream words the host sets every video frame (wf_hip_set_stream_delay / _audio_ts): staged in page-locked memory of
    // the handle's own, two blocks used alternately, so that the calls copy and return instead of draining the stream
    void *h_words[2] = {nullptr, nullptr};
    size_t h_words_bytes[2] = {0, 0};
    hipEvent_t ev_words[2] = {nullptr, nullptr};
    uint32_t words_next = 0;
    std::vector<void *> allocs;
    bool canary = false;                                  // WF_HIP_CANARY=1 at create: guard bytes behind every block, checked by wf_hip_sync
    std::vector<std::pair<void *, size_t>> guards;        // (block, payload bytes) of every guarded block still alive
    std::string last_error;
    std::string kernel_name;
    // launch description, fixed at create
    int (*launch)(wf_hip *, const wf::TickArgs &, bool aligned, hipStream_t) = nullptr;
};

namespace wf::host {

// text of the last failed wf_hip_create of this thread (wf_hip_last_error(NULL))
extern thread_local std::string g_create_error;
// records the message on the handle (or, h == nullptr, as the create error) and returns `code`
int fail(wf_hip *h, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));

#define WF_TRY_RC(expr)                 \
    do {                                \
        const int rc_ = (expr);         \
        if(rc_ != WF_HIP_OK)            \
            return rc_;                 \
    } while(0)

#define WF_HIP_TRY(h, expr)                                                                                       \
    do {                                                                                                          \
        hipError_t e_ = (expr);                                                                                   \
        if(e_ != hipSuccess)                                                                                      \
            return fail((h), WF_HIP_ERR_RUNTIME, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                        __LINE__);                                                                                \
    } while(0)

// Every device block carries 256 bytes of slack behind its payload (some kernels read -- never write -- a few words past a row).
// With WF_HIP_CANARY=1 in the environment of wf_hip_create the slack is a guard: filled with GUARD_BYTE when the block is made,
// checked by wf_hip_sync (check_canaries): a kernel that wrote past its buffer turns the next sync into WF_HIP_ERR_RUNTIME
// naming the block (there is no compute-sanitizer on this stack).
constexpr size_t GUARD_BYTES = 256;
constexpr int GUARD_BYTE = 0xA5;
int guard_block(wf_hip *h, void *p, size_t payload_bytes); // wf_hip_plan.hip
int check_canaries(wf_hip *h);                             // wf_hip_plan.hip

template<class T> int dev_alloc(wf_hip *h, T **out, size_t count)
{
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, count * sizeof(T) + GUARD_BYTES);
    if(e != hipSuccess)
        return fail(h, WF_HIP_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
    h->allocs.push_back(p);
    *out = static_cast<T *>(p);
    if(h->canary)
        return guard_block(h, p, count * sizeof(T));
    return WF_HIP_OK;
}

template<class T> int upload(wf_hip *h, T **out, const std::vector<T> &v)
{
    *out = nullptr;
    if(v.empty())
        return WF_HIP_OK;
    int rc = dev_alloc(h, out, v.size());
    if(rc)
        return rc;
    WF_HIP_TRY(h, hipMemcpyAsync(*out, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, h->stream));
    return WF_HIP_OK;
}
// the same into a table pointer of an argument struct (`const float *coef` ...)
template<class T> int upload(wf_hip *h, const T **out, const std::vector<T> &v)
{
    T *p = nullptr;
    const int rc = upload(h, &p, v);
    *out = p;
    return rc;
}
// ... and a complex table as the host builders leave it (wf::cfloat and wf::cf: the same two floats)
inline int upload(wf_hip *h, const wf::cf **out, const std::vector<wf::cfloat> &v)
{
    static_assert(sizeof(wf::cfloat) == sizeof(wf::cf), "twiddle layout");
    wf::cf *p = nullptr;
    *out = nullptr;
    if(v.empty())
        return WF_HIP_OK;
    const int rc = dev_alloc(h, &p, v.size());
    if(rc)
        return rc;
    WF_HIP_TRY(h, hipMemcpyAsync(p, v.data(), v.size() * sizeof(wf::cf), hipMemcpyHostToDevice, h->stream));
    *out = p;
    return WF_HIP_OK;
}

// the flag buffer the newest tick wrote: the current m_last_silent / hidden bits of every stream
inline uint32_t *cur_flags(const wf_hip *h) { return h->d_flags + (size_t)h->flag_cur * h->n_streams; }

inline uint32_t next_pow2(uint32_t v)
{
    uint32_t p = 1;
    while(p < v)
        p <<= 1;
    return p;
}

// `bytes` of per-stream words from a borrowed host array to `d_dst`, without waiting for the stream: through one of the handle's
// two page-locked staging blocks (wf_hip.hip)
int upload_words(wf_hip *h, void *d_dst, const void *src, size_t bytes);

// wf_hip.hip, for the entry points that live elsewhere.  join_lanes: what every entry point other than wf_hip_tick starts with --
// `stream` waits for what the lanes hold, and the next tick's lanes will wait for what the call enqueues on `stream`
int join_lanes(wf_hip *h);
int check_range(wf_hip *h, uint32_t first, uint32_t count);        // refuses a stream range outside the batch, then joins the lanes
int read_back(wf_hip *h, const void *d, void *out, size_t bytes); // device to host on `stream`; returns when the bytes have arrived
// the constant part of the small argument structs (h->small), for wf_hip_create
void fill_meter_args(wf_hip *h);
void fill_wave_args(wf_hip *h, uint32_t wave_samples);
void fill_vertex_args(wf_hip *h, const wf::VertexTables &vt, const float *d_cap_xy);

// wf_hip_measure.hip: the measurement outputs.  The ingest's two hooks -- what a push of `frames` must satisfy while a producer
// follows the pushes, and that producer's launch behind the advance of the write positions (d_frames: a ragged push's counts)
int measure_check_push(wf_hip *h, uint32_t frames);
void measure_after_push(wf_hip *h, uint32_t first, uint32_t count, uint32_t frames, const uint32_t *d_frames);
// false: `what` is no measurement output.  Else *why is the refusal's text (*per_stream 0), or nullptr with the bytes per stream
bool measure_source(const wf_hip *h, wf_hip_output what, size_t *per_stream, const char **why);
// wf_hip_read of a measurement output: computes streams [first, first+count) on `stream` and copies them to `out`
int measure_read(wf_hip *h, wf_hip_output what, uint32_t first, uint32_t count, void *out);

// ---- kernel dispatch -----------------------------------------------------------------------------------------------------
// One object file per geometry (wf_tick_geom.hip compiled with -DWF_TU_GEOM=<N>): picks the spectrum_tick_kernel instantiation
// of this handle's configuration (plain / staged tables / shared curve row / split / zero-padded / Bluestein / mixed radix),
// sets its dynamic-LDS attribute and leaves h->launch, h->wg_lds, h->wg_threads, h->split, h->flag_bufs, h->kernel_name
// (mixed radix: also the exchange buffer's size, h->tick.mr.half / s3 / lds_cf).  h->plan says which family; nothing is planned here.
int setup_tick_512(wf_hip *h);
int setup_tick_1024(wf_hip *h);
int setup_tick_2048(wf_hip *h);
int setup_tick_4096(wf_hip *h);
int setup_tick_8192(wf_hip *h);
int setup_tick_16384(wf_hip *h);
int setup_tick_32768(wf_hip *h);
// wf_big_dispatch.hip: fft sizes whose transform does not fit a CU's LDS, and big_outputs_kernel for the displays that are
// finished behind the tick kernel (h->disp.ext_outputs)
int setup_launch_big(wf_hip *h);
int big_outputs_set_lds(wf_hip *h);
void big_outputs_launch(wf_hip *h, const wf::TickArgs &a, uint32_t rows, hipStream_t st);

} // namespace wf::host
