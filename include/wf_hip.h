/*
 * wf_hip.h -- C ABI of libwaveform_hip.so, the MI355X (gfx950) implementation of
 * phandasm/waveform's per-tick DSP: the spectrum path and, behind the same interface, the
 * level meter, the waveform display and the volume-normalisation RMS.
 *
 * Boundary.  The reference selects its DSP kernels through four virtuals on
 * WAVSource (src/source.hpp:273-277: update_input_rms, tick_spectrum, tick_meter,
 * tick_waveform); callbacks::create (src/source.cpp:87-102) instantiates WAVSourceAVX2 /
 * WAVSourceAVX / WAVSourceGeneric.  This library is what a fourth subclass, WAVSourceHIP,
 * calls from its tick_spectrum() / tick_meter() / tick_waveform() overrides
 * (host/wav_source_hip.hpp; the binding a maintainer adds is in INTEGRATION.md).
 * One wf_hip handle serves a *batch* of independent sources ("streams") that share
 * one configuration, because a GPU only pays off batched.
 *
 * Mapping of entry points to the reference code they replace:
 *   wf_hip_create        WAVSource::update(): buffers, FFTW plan, window/slope/rolloff/
 *                        interp tables (src/source.cpp:1169-1290, :837-918)
 *   wf_hip_destroy       WAVSource::free_bufs() (src/source.cpp:782-808)
 *   wf_hip_reset         state init in update(): m_tsmooth_buf = 0, m_decibels = DB_MIN,
 *                        rings pre-filled with N zero samples (:1170-1182, :1243-1248)
 *   wf_hip_push_audio*   WAVSource::capture_audio(): CircularBuffer::push_back per channel
 *                        (src/source.cpp:1873-1886, src/circular_buffer.hpp:42-63)
 *   wf_hip_tick          WAVSource*::tick_spectrum(seconds) for every stream of the batch
 *                        (src/source_generic.cpp:26-180 -- the parity target; AVX variants
 *                        src/source_avx.cpp:29-200, src/source_avx2.cpp:24-209), plus, when
 *                        the configuration displays bars, the bar reduction of render_bars
 *                        (src/source.cpp:1500-1557; src/filter.hpp:160-211)
 *   wf_hip_read[_async]  reading m_decibels / m_interp_bufs / m_tsmooth_buf / m_meter_val ... (wf_hip_output)
 *   wf_hip_enable_input_rms
 *                        capture_audio's RMS part + sync_rms_buffer + update_input_rms
 *                        (src/source.cpp:1842-1871, :810-835; src/source_generic.cpp:392-403)
 *   wf_hip_enable_loudness
 *                        not in the reference: BS.1770-4 / EBU R128 loudness and true peak of every stream, measured as
 *                        the pushes arrive (WF_HIP_OUT_LOUDNESS)
 *   WF_HIP_OUT_PEAKS     not in the reference: the strongest spectral peaks of every m_decibels row, found on the device
 *                        when read
 *   WF_HIP_OUT_SIGNAL    not in the reference: level, DC, clipping and stereo phase correlation of every stream's newest
 *                        window of audio, measured on the device when read
 *   WF_HIP_OUT_PITCH     not in the reference: the fundamental frequency of every stream's newest window of audio (YIN),
 *                        estimated on the device when read
 *   WF_HIP_OUT_BANDS     not in the reference: third-octave band levels (IEC 61260-1) and the Z / A / C weighted level
 *                        (IEC 61672-1) of every m_decibels row, summed on the device when read
 *   WF_HIP_OUT_STEREO    not in the reference: correlation, coherence, phase and balance between the two captured channels in
 *                        each third-octave band, from a float64 transform of every stream's newest window on the device when read
 *   WF_HIP_OUT_CQ        not in the reference: a constant-Q spectrum, one level per semitone from C0 to B9, of every stream's
 *                        newest audio in the rings, correlated in float64 on the device when read
 *   WF_HIP_OUT_SCOPE     not in the reference (its "waveform" mode is a level history, not the wave): a triggered oscilloscope
 *                        trace of every stream's newest window of audio, triggered and reduced to columns on the device when read
 *   WF_HIP_OUT_GONIO     not in the reference: a stereo vectorscope (goniometer), the mid/side Lissajous picture of every stream's
 *                        newest window of audio as a 64 x 64 image of frame counts, ranged and counted on the device when read
 *   WF_HIP_OUT_SONO      not in the reference: a spectrogram (sonogram) of every stream's newest audio in the rings, up to 64
 *                        columns 256 frames apart by 64 bands of an eighth of an octave, the columns anchored to the stream's
 *                        sample counter, transformed in float64 on the device when read
 *   WF_HIP_OUT_BITS      not in the reference: a bit meter, per captured channel the sample-value histogram, the activity of each
 *                        bit, the word length, the over-range count and the longest run of identical samples of every stream's
 *                        newest window of audio, counted on the device when read
 *   WF_HIP_OUT_THD       not in the reference: a distortion analyser, per captured channel the fundamental of a test tone, its
 *                        harmonics, THD, THD+N, SNR, SFDR and the noise floor, from a float64 transform of every stream's newest
 *                        window through a -180 dB taper on the device when read
 *   WF_HIP_OUT_DELAY     not in the reference: a delay finder, by how many frames one captured channel lags the other and whether
 *                        one of them is inverted, from the floored-PHAT cross-correlation of every stream's newest window, in
 *                        float64 on the device when read
 *   WF_HIP_OUT_ONSET     not in the reference: an onset detector, the onset strength of every stream's newest audio in the rings
 *                        in columns of 256 frames, in total and in three frequency groups, with the onsets picked from it by a
 *                        fixed rule, anchored to the sample counter, in float64 on the device when read
 *   WF_HIP_OUT_XFER      not in the reference: a dual-channel analyser's transfer function, the gain, phase and coherence against
 *                        frequency of one captured channel against the other with the programme as the stimulus, averaged over the
 *                        13 to 32 half-overlapped segments in every stream's rings, anchored to the sample counter, in float64 on
 *                        the device when read
 *   WF_HIP_OUT_IMPULSE   not in the reference: the same analyser's response against time, the impulse response of one captured
 *                        channel against the other from the regularised average of the same segments, its energy-time curve and
 *                        the up to eight strongest arrivals with their delay, level and polarity, in float64 on the device when
 *                        read
 *   WF_HIP_OUT_CLICK     not in the reference: a click detector, per captured channel the clicks, pops and splices of every
 *                        stream's newest window of audio -- the frames that a linear predictor fitted to the window cannot account
 *                        for -- as a count, a rate and the up to eight strongest events, in float64 on the device when read
 *   WF_HIP_OUT_IMD       not in the reference: a two-tone intermodulation analyser, per captured channel the two tones of a
 *                        twin-tone stimulus, their sum and difference products of orders 2 .. 5, total IMD, the difference-frequency
 *                        (IEC 60268-3) and modulation (DIN / SMPTE) distortion and the noise floor, from the distortion analyser's
 *                        float64 spectrum of every stream's newest window on the device when read
 *   WF_HIP_OUT_TEMPO     not in the reference: tempo and beat phase, the onset strength of up to 2048 columns of every stream's
 *                        rings, its autocorrelation, the tempo with a second candidate, and the frames of the last and the next
 *                        beat on the sample counter, in float64 on the device when read
 *   WF_HIP_OUT_HUM       not in the reference: a mains hum detector, per captured channel whether a 50 or a 60 Hz line with its
 *                        harmonics up to the 8th stands above the programme, the mains frequency, the level of the hum against the
 *                        total and of every line, from the low bins of an exact float64 transform of the newest up to 32768 frames
 *                        of every stream's rings on the device when read
 * FFT sizes: every multiple of 16 from 128 to 65536, the reference's own range with "enable large FFT" (src/source.cpp:349,
 * :359-363, :562-565).  Powers of two up to 32768 and the other sizes up to 16384 -- as a mixed-radix transform where the
 * size has small prime factors and at most one prime factor of up to 127 (the automatic sizes, 114 of the slider's 120
 * positions that are not powers of two), by Bluestein's algorithm otherwise -- run inside one fused kernel; 65536 runs in one
 * kernel of its own; the other sizes above 16384 as rows of n/2 = C R points with one complex scratch buffer in device memory
 * (wf_big.hpp: rows of a mixed-radix transform -- two rows: in one kernel without scratch --, or rows by Bluestein inside LDS; 12-28 % of
 * the HBM roofline).
 * Anything else -> WF_HIP_ERR_UNSUPPORTED.
 *
 * Waveform display.  A handle created from a configuration with cfg.waveform != 0 is a *waveform batch*: wf_hip_tick runs
 * WAVSource*::tick_waveform (src/source_generic.cpp:271-390) for every stream -- a history of cfg.width dBFS points per
 * channel, extended by one point per meter_ms / width of newly consumed audio -- and WF_HIP_OUT_DECIBELS holds the rows
 * ([count][output_channels][width]; wf_hip_fft_size() == width as m_fft_size does in this mode).  The tick needs
 * wf_hip_tick_params::audio_ts_ns.  Widths up to 8192 points.
 *
 * Level meter.  A handle created from a configuration with cfg.meter != 0 is a *meter batch*: wf_hip_tick runs
 * WAVSource*::tick_meter (src/source_generic.cpp:182-269; AVX src/source_avx.cpp:202-322) for every stream -- the
 * meter buffer is the last wf_hip_fft_size() samples consumed from the device ring, RMS or peak over it, temporal
 * smoothing, dBFS, m_last_silent -- and WF_HIP_OUT_METER / WF_HIP_OUT_BARS hold m_meter_val and the bars
 * render_bars draws from it (src/source.cpp:1505-1509, :1548-1557).  Spectrum-only entry points
 * (WF_HIP_OUT_DECIBELS, WF_HIP_OUT_TSMOOTH / wf_hip_write_tsmooth, wf_hip_table) fail with WF_HIP_ERR_INVALID on a meter batch.
 *
 * Conventions: plain C types only; every function returns WF_HIP_OK (0) or a negative
 * wf_hip_status, never throws, never aborts; wf_hip_last_error() gives the text.  A handle
 * is used by one thread at a time (the reference holds m_mtx around tick/update,
 * src/source.cpp:1326,1079); different handles may be used concurrently.  Host buffers
 * passed in are borrowed for the duration of the call.  All work of a handle is issued on
 * its own HIP stream; functions that return data to the host synchronise that stream.
 *
 * There is NO CPU fallback in this library: without a usable gfx950 device
 * wf_hip_create fails with WF_HIP_ERR_NO_DEVICE and the caller keeps using its
 * CPU class (WAVSourceGeneric) -- the reference's own failure mode for a missing
 * FFTW plan is to skip the channel (src/source_generic.cpp:105-108).
 */
#ifndef WF_HIP_H
#define WF_HIP_H
#include <stddef.h>
#include <stdint.h>
#include "wf_config.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_HIP_ABI_VERSION 13

typedef enum wf_hip_status {
    WF_HIP_OK = 0,
    WF_HIP_ERR_INVALID = -1,     /* bad argument / configuration */
    WF_HIP_ERR_UNSUPPORTED = -2, /* legal for the reference, not implemented here (e.g. a waveform display wider than 8192 points) */
    WF_HIP_ERR_NO_DEVICE = -3,   /* no usable HIP device */
    WF_HIP_ERR_RUNTIME = -4,     /* a HIP call failed; see wf_hip_last_error */
    WF_HIP_ERR_NOMEM = -5
} wf_hip_status;

typedef struct wf_hip wf_hip; /* opaque */

/* ---- library ---------------------------------------------------------------------- */
int wf_hip_abi_version(void);
/* number of usable HIP devices (0 when there is none; never fails) */
int wf_hip_device_count(void);
/* text of the last error on this handle (or of the last failed create when h == NULL) */
const char *wf_hip_last_error(const wf_hip *h);

/* ---- lifetime ----------------------------------------------------------------------- */
/* max_streams: batch size (independent WAVSource instances sharing cfg).
 * ring_frames: capacity of each per-channel device ring in samples; 0 = default
 *              (smallest power of two >= max(2 * fft_size, 4096)). Rounded up to a power of two.  A packet longer than
 *              the ring keeps its newest ring_frames samples. */
int wf_hip_create(const wf_config *cfg, int device, uint32_t max_streams, uint32_t ring_frames, wf_hip **out);
void wf_hip_destroy(wf_hip *h);
/* re-initialise streams [first, first+count) as update() does; afterwards they read, and tick, as the same streams of a
 * freshly created handle given the settings listed as left in force below (the loudness state among them).  Re-initialised:
 *   spectrum batches  m_tsmooth_buf = 0, rings = N zeros with the write position at N, m_decibels = DB_MIN, m_last_silent and
 *                     the hidden state (wf_hip_set_hidden) cleared, bars and premirror at the bottom border, vertices and
 *                     vertex counts 0 (no geometry until the next tick)
 *   meter batches     empty rings, m_meter_buf = m_meter_val = DB_MIN, m_last_silent and the hidden state cleared
 *   waveform batches  rings = width zeros, rows DB_MIN, m_waveform_ts = 0, the hidden state cleared
 *   all               the device RMS producer's state (wf_hip_enable_input_rms): m_input_rms = 0, nothing measured yet;
 *                     the next wf_hip_bars_mirror_ready hands over the handle's own bars (the reset state of these streams)
 *                     instead of a set the ticks before the reset wrote
 * Left in force, as settings rather than state: the per-stream delay (wf_hip_set_stream_delay), the values given by
 * wf_hip_set_input_rms, the audio timestamps (wf_hip_set_stream_audio_ts), the loudness state (wf_hip_enable_loudness
 * restarts it), the mirror buffers (wf_hip_set_bars_mirrors) and which of their two sets the ticks write.  A readback issued
 * before the call (wf_hip_read_async) still returns the state before it. */
int wf_hip_reset(wf_hip *h, uint32_t first, uint32_t count);

/* ---- geometry of the batch ---------------------------------------------------------- */
uint32_t wf_hip_fft_size(const wf_hip *h);
uint32_t wf_hip_num_streams(const wf_hip *h);
uint32_t wf_hip_capture_channels(const wf_hip *h);
uint32_t wf_hip_output_channels(const wf_hip *h);  /* m_output_channels */
uint32_t wf_hip_display_channels(const wf_hip *h); /* m_stereo ? 2 : 1 */
uint32_t wf_hip_num_bars(const wf_hip *h);         /* outputs per displayed row: m_num_bars with cfg.bars, m_width with cfg.curve
                                                      (render_curve, src/source.cpp:1360-1425), 0 with neither */
uint32_t wf_hip_ring_frames(const wf_hip *h);

/* ---- audio ingest ------------------------------------------------------------------- */
/* Append `frames` samples per channel to streams [first, first+count).
 * Layout of `samples` (host memory): [count][capture_channels][frames], planar float32 --
 * what capture_audio receives per source in audio_data::data[] (src/source.cpp:1873-1882). */
int wf_hip_push_audio(wf_hip *h, uint32_t first, uint32_t count, const float *samples, uint32_t frames);
/* Pipelined ingest: page-locked host buffers (wf_hip_host_alloc) are copied by DMA without the runtime's bounce buffer, on a
 * second HIP stream of the handle, so that the copy of the next packet runs under the tick of the previous one; the ring
 * append is ordered behind the copy, the next tick behind the append.  The call does not wait: `samples` must stay
 * untouched until wf_hip_ingest_done(slot) -- two buffers used alternately (slot 0 / 1) keep a 60 fps loop from ever waiting.
 * Layout as wf_hip_push_audio.  Measured (4096 stereo streams, one 800-frame hop each per step). */
int wf_hip_push_audio_async(wf_hip *h, uint32_t first, uint32_t count, const float *pinned_samples, uint32_t frames, uint32_t slot);
/* blocks until the copy issued with `slot` (0 or 1) has left the host buffer */
int wf_hip_ingest_done(wf_hip *h, uint32_t slot);
/* Hops of different lengths (a plugin's sources tick with whatever their capture buffers gained): stream first+i appends
 * frames[i] <= max_frames frames from pinned_samples[i][channel][0 .. max_frames); frames[i] == 0 leaves it alone.
 * `frames` is copied before the call returns; `pinned_samples` follows the rules of wf_hip_push_audio_async (slot 0 / 1,
 * wf_hip_ingest_done).  Not available while the device RMS producer is enabled. */
int wf_hip_push_audio_ragged_async(wf_hip *h, uint32_t first, uint32_t count, const float *pinned_samples, const uint32_t *frames,
                                   uint32_t max_frames, uint32_t slot);

/* page-locked host memory for wf_hip_push_audio_async (hipHostMalloc); NULL on failure */
void *wf_hip_host_alloc(size_t bytes);
void wf_hip_host_free(void *p);
/* Same, from a device pointer on the handle's device (no PCIe crossing). */
int wf_hip_push_audio_device(wf_hip *h, uint32_t first, uint32_t count, const float *d_samples, uint32_t frames);
/* Same, but the samples are generated on the device by the counter hash of wf_synth.h:
 * stream s, channel c receives wf_synth_noise(seed, stream_id0 + s, c, index0 + i), i < frames. */
int wf_hip_push_synth(wf_hip *h, uint32_t first, uint32_t count, uint64_t seed, uint32_t stream_id0,
                      uint64_t index0, uint32_t frames);
/* muted / silent packet: the rings receive `frames` zeros, CircularBuffer::push_back_zero (src/source.cpp:1879-1880).  `samples`
 * (layout of wf_hip_push_audio) may be NULL: a packet without data.  A muted packet that still carries samples (muted &&
 * !m_ignore_mute) passes them: capture_audio takes the volume-normalisation RMS from the packet itself
 * (src/source.cpp:1842-1871), so the device RMS producer (wf_hip_enable_input_rms) receives them; without the producer they are
 * not read. */
int wf_hip_push_audio_muted(wf_hip *h, uint32_t first, uint32_t count, const float *samples, uint32_t frames);

/* ---- audio ingest in any libobs sample format ------------------------------------------
 * capture_audio takes channels m_channel_base .. m_channel_base + m_capture_channels out of a packet of up to
 * MAX_AUDIO_CHANNELS (8) channels (src/source.cpp:1827-1828, :1872-1886; a mono capture picks its channel with the P_CHANNEL
 * setting, :333, :1089-1103).  wf_hip_push_pcm does the same with the packet in its own sample format: the bus carries the
 * packet's bytes (s16: half of float32, u8: a quarter) and the device converts, picks the captured channels and appends them
 * to the rings -- and, where the RMS producer follows the audio, their squared per-frame peak (:1842-1871) -- in one pass.
 * Values are libobs' enum audio_format. */
typedef enum wf_hip_pcm_format {
    WF_HIP_PCM_U8 = 1, WF_HIP_PCM_S16, WF_HIP_PCM_S32, WF_HIP_PCM_F32,                        /* interleaved: [frames][channels] */
    WF_HIP_PCM_U8_PLANAR, WF_HIP_PCM_S16_PLANAR, WF_HIP_PCM_S32_PLANAR, WF_HIP_PCM_F32_PLANAR /* planar: [channels][frames] */
} wf_hip_pcm_format;
/* What decoders, network streams and capture devices send and libobs has no name for.  The values go in the same
 * wf_hip_pcm.format field; 9..15, 21..23 and everything from 29 on are no format. */
typedef enum wf_hip_wire_format {
    WF_HIP_WIRE_S24 = 16,   /* 3 bytes, little-endian, two's complement, packed (no padding byte) */
    WF_HIP_WIRE_S24_BE,     /* 17: the same, big-endian (RTP L24) */
    WF_HIP_WIRE_S16_BE,     /* 18: big-endian int16 (RTP L16) */
    WF_HIP_WIRE_ULAW,       /* 19: ITU-T G.711 mu-law, 1 byte */
    WF_HIP_WIRE_ALAW,       /* 20: ITU-T G.711 A-law, 1 byte */
    /* planar: the interleaved value + 8 */
    WF_HIP_WIRE_S24_PLANAR = 24, WF_HIP_WIRE_S24_BE_PLANAR, WF_HIP_WIRE_S16_BE_PLANAR, WF_HIP_WIRE_ULAW_PLANAR, WF_HIP_WIRE_ALAW_PLANAR
} wf_hip_wire_format;
/* The conversion to the float32 the rings hold is exact (bit for bit what these expressions give in float):
 *   u8:  (x - 128) * 2^-7      s16: x * 2^-15      s32: (float)x * 2^-31, (float)x rounded to nearest even
 *   f32: the bits pass unchanged
 * -- the full-scale mapping audio converters use.  The wire formats:
 *   s24, s24_be: the three bytes (least / most significant first) sign-extended to int x, then (float)x * 2^-23: -2^23 reads
 *                -1.0f, 2^23 - 1 reads 0x1.fffffcp-1f; every 24-bit integer is a float32, so nothing is lost
 *   s16_be:      the two bytes swapped, then x * 2^-15
 *   mu-law:      u = ~b & 0xFF, e = (u >> 4) & 7, m = u & 15, mag = (((m << 3) + 0x84) << e) - 0x84, v = u & 0x80 ? -mag : mag;
 *                (float)v * 2^-15.  0x00 reads -32124 * 2^-15, 0x80 +32124 * 2^-15, both zero codes (0xFF, 0x7F) +0.0f
 *   A-law:       a = b ^ 0x55, e = (a >> 4) & 7, m = a & 15, mag = e ? ((m << 4) + 0x108) << (e - 1) : (m << 4) + 8,
 *                v = a & 0x80 ? mag : -mag; (float)v * 2^-15.  0xD5 reads +8 * 2^-15, 0xAA +32256 * 2^-15
 * -- G.711's 14- and 13-bit linear values at the top of a 16-bit word, as telephony decoders give them. */
typedef enum wf_hip_pcm_memory {
    WF_HIP_PCM_HOST = 0,   /* any host memory; the call returns once the packet has been copied (wf_hip_push_audio) */
    WF_HIP_PCM_PINNED = 1, /* wf_hip_host_alloc memory; does not wait, `slot` as wf_hip_push_audio_async / wf_hip_ingest_done */
    WF_HIP_PCM_DEVICE = 2  /* device memory of the handle's device, read in place (wf_hip_push_audio_device) */
} wf_hip_pcm_memory;
typedef struct wf_hip_pcm {
    const void *data;                  /* the blocks of streams first .. first+count-1, one after the other: stream i's block
                                          starts at i * channels * frames * bytes_per_sample (packed 24-bit: any byte) */
    uint32_t format;                   /* wf_hip_pcm_format or wf_hip_wire_format */
    uint32_t channels;                 /* channels in the packet, 1..8 */
    uint32_t channel_base;             /* first captured channel (m_channel_base): channel_base + capture_channels <= channels;
                                          a two-channel capture needs 0 (the asserts of src/source.cpp:1827-1828) */
    uint32_t frames;                   /* frames per stream; with frames_per_stream: the block size (max_frames) */
    const uint32_t *frames_per_stream; /* NULL, or [count] frame counts <= frames: a ragged push by the rules of
                                          wf_hip_push_audio_ragged_async (WF_HIP_PCM_PINNED only; not while the RMS producer
                                          follows the audio; at most 65535 streams) */
    uint32_t memory;                   /* wf_hip_pcm_memory */
    uint32_t slot;                     /* WF_HIP_PCM_PINNED: 0 / 1, released by wf_hip_ingest_done(slot) */
} wf_hip_pcm;
/* Appends the captured channels of `pcm` to streams [first, first+count), as wf_hip_push_audio* does with planar float32: a
 * packet longer than the ring keeps its newest ring_frames frames, every handle kind (spectrum, level meter, waveform) takes
 * it.  Host packets cross the bus in their own width; a planar one with more channels than captured sends only the
 * captured planes.  WF_HIP_ERR_INVALID before anything is enqueued for a bad format, channel count, channel pick, memory
 * kind, slot, a NULL pointer, or device data not aligned to its sample's natural alignment (its size; 1 for packed 24-bit,
 * 2 for s16_be). */
int wf_hip_push_pcm(wf_hip *h, uint32_t first, uint32_t count, const wf_hip_pcm *pcm);

/* ---- the tick ------------------------------------------------------------------------- */
typedef struct wf_hip_tick_params {
    float seconds;          /* tick_spectrum(seconds): only TVEXPONENTIAL smoothing uses it */
    uint32_t delay_frames;  /* audio already captured beyond the tick time: the window is the fft_size
                               samples ending delay_frames before the newest one
                               (dtaudio > 0 in src/source_generic.cpp:50-51) */
    float input_rms;        /* m_input_rms, only read when cfg.normalize_volume; the same value for every stream unless
                               wf_hip_set_input_rms has given the streams their own */
    uint32_t flags;         /* WF_HIP_TICK_* */
    uint64_t audio_ts_ns;   /* m_audio_ts: end-of-audio timestamp of the newest pushed sample (src/source.cpp:1829-1832), in ns;
                               only waveform batches read it (tick_waveform places its points in time with it) */
} wf_hip_tick_params;
/* bars/curve-only batch mode: skip the m_decibels store (cfg.bars or cfg.curve must be set).  The silence state machine
 * (src/source_generic.cpp:74-95) keeps working: the kernel leaves a one-word verdict per row ("a value > floor - 10") for the
 * next tick's test instead.  After the first such tick, WF_HIP_OUT_DECIBELS holds rows only as fresh as the last tick
 * without the flag that rewrote them.  Mono mixdown of two captured channels stores its (single) row regardless, and so do
 * the batches whose outputs are derived from the stored rows by a kernel of their own (fft sizes beyond a CU's LDS; displays
 * whose Gaussian-filter staging does not fit the tick kernel's on-chip buffer): there the flag is accepted and changes nothing. */
#define WF_HIP_TICK_NO_DECIBELS 1u

/* Asynchronous: enqueues the fused kernel for all streams on the handle's stream. */
int wf_hip_tick(wf_hip *h, const wf_hip_tick_params *p);
/* show()/hide()/capture-timeout per stream: hidden streams take the reset branch of
 * tick_spectrum (src/source_generic.cpp:34-48).  mask[i] != 0 -> hidden.  tick_meter tells the two causes apart
 * (capture timeout: the meter buffer is cleared and nothing is consumed, src/source_generic.cpp:184-199; !m_show: the
 * audio is consumed, then the state is reset, :222-230), so a host passes WF_HIP_HIDDEN_TIMEOUT for the former. */
#define WF_HIP_SHOWN 0
#define WF_HIP_HIDDEN 1          /* !m_show */
#define WF_HIP_HIDDEN_TIMEOUT 2  /* m_tick_ts - m_capture_ts > CAPTURE_TIMEOUT */
#define WF_HIP_PAUSED 3          /* the source was not ticked in this video frame (OBS ticks only active sources; a waveform source whose buffers
                                    hold no more than the A/V-sync reserve returns before it touches anything, src/source_generic.cpp:293-295) --
                                    the next wf_hip_tick leaves the stream exactly as it is, the device RMS producer's m_input_rms and
                                    its sync_rms_buffer position included (update_input_rms belongs to the tick); cleared by any other
                                    value */
#define WF_HIP_STARVED 4         /* spectrum batches whose host keeps the sources' own buffers (the plugin binding): the source holds fewer
                                    samples than window + A/V-sync delay (src/source_generic.cpp:55-61: every channel is skipped) -- the
                                    next wf_hip_tick processes no channel of the stream but still runs the reference's end-of-tick pass
                                    over the rows as they are (:138-179: dbfs of a stale dB value is DB_MIN; volume normalisation and
                                    roll-off on top), as the kernel does for a stream whose device ring is that short; stays until
                                    another value is set */
int wf_hip_set_hidden(wf_hip *h, uint32_t first, uint32_t count, const uint8_t *mask);
/* A/V-sync delay per stream, in frames (dtaudio > 0 of each source, src/source_generic.cpp:50-51), for batches whose
 * sources run on their own audio timestamps: stream first+i analyses the window ending delay[i] + the tick's common
 * delay_frames before its newest sample; stays in force until the next call for that stream.  Each delay[i] + fft_size
 * must fit the ring (and so must their sum with any wf_hip_tick_params::delay_frames used later). */
int wf_hip_set_stream_delay(wf_hip *h, uint32_t first, uint32_t count, const uint32_t *delay_frames);
/* Waveform batches whose sources run on their own audio timestamps (the plugin's batched mode): m_audio_ts of stream
 * first+i (src/source.hpp; what tick_waveform measures every point's time against, src/source_generic.cpp:306-331), in
 * nanoseconds.  Stays in force until the next call for that stream; once any stream has been given one,
 * wf_hip_tick_params::audio_ts_ns is ignored (streams never set read 0: "no audio has a timestamp yet").
 * WF_HIP_ERR_INVALID for batches that are not waveform displays. */
int wf_hip_set_stream_audio_ts(wf_hip *h, uint32_t first, uint32_t count, const uint64_t *audio_ts_ns);
/* m_input_rms per stream (what update_input_rms leaves, src/source_generic.cpp:392-403), for batches whose streams are
 * normalised independently (cfg.normalize_volume): rms[i] belongs to stream first+i and stays in force until the next
 * call for that stream.  Once any stream has been given a value, wf_hip_tick_params::input_rms is ignored (streams never
 * set read 0, i.e. the full max_gain, as a source that has not seen audio yet does).  The volume compensation
 * min(volume_target - dbfs(rms), max_gain) (src/source_generic.cpp:163) is evaluated here, on the host, in float. */
int wf_hip_set_input_rms(wf_hip *h, uint32_t first, uint32_t count, const float *rms);
/* Volume normalisation produced on the device: update_input_rms for every stream (src/source_generic.cpp:392-403 with
 * sync_rms_buffer, src/source.cpp:810-835, fed by the RMS part of capture_audio, :1842-1871).  feed == 0: after this call every
 * wf_hip_push_* also appends the squared per-frame peak of the captured channels to a per-stream RMS ring, and every
 * wf_hip_tick first recomputes m_input_rms over the m_input_rms_size (= sample_rate & -16) frames that end at the
 * A/V-sync point, as WAVSource::tick does (src/source.cpp:1330-1331); wf_hip_tick_params::input_rms is then ignored and
 * wf_hip_set_input_rms fails.  Needs cfg.normalize_volume (spectrum or waveform batches).  Audio pushed before the call
 * counts as silence.
 * feed != 0: the same producer for hosts that already hold capture_audio's per-frame squared peaks -- the plugin binding: the
 * reference's own capture_audio fills m_rms_sync_buf (src/source.cpp:1842-1871, from the packet even when it is muted),
 * and WAVSourceHIP::update_input_rms (the override of src/source.hpp:273, src/source_generic.cpp:392-403) hands what
 * sync_rms_buffer would move into m_input_rms_buf this tick (src/source.cpp:810-835) to
 * wf_hip_push_rms_ragged_async instead of adding up 48000 floats per source and frame on the host.  The squared-peak
 * ring is then independent of the audio rings' positions; wf_hip_tick recomputes every stream's m_input_rms as above.
 * The two forms are mutually exclusive on a handle. */
int wf_hip_enable_input_rms(wf_hip *h, int feed);
/* sq: page-locked [count][max_frames] squared peaks, oldest first; frames[count] values are valid per stream (0: that
 * stream's sync_rms_buffer had nothing to consume).  max_frames <= sample_rate & -16.  Shares the ingest slots of
 * wf_hip_push_audio*_async: wf_hip_ingest_done(slot) says when `sq` may be written again. */
int wf_hip_push_rms_ragged_async(wf_hip *h, uint32_t first, uint32_t count, const float *pinned_sq, const uint32_t *frames,
                                 uint32_t max_frames, uint32_t slot);
/* ---- loudness (ITU-R BS.1770-4 / EBU R128, EBU Tech 3341 / 3342) --------------------------------------------------------
 * An opt-in producer that follows the audio rings: once enabled, every frame any push appends to a stream (wf_hip_push_audio*,
 * wf_hip_push_synth, wf_hip_push_pcm, and the wf_hip_multi_push_* calls through their shards) is measured exactly once, in
 * push order, by one kernel launch per push.  Definitions (per stream):
 *   channels     the captured channels (1 or 2), each with weight 1.0 (a mono handle reads 3.01 LU below the same signal
 *                captured as dual-mono stereo)
 *   K-weighting  the BS.1770-4 shelf, then the RLB high-pass: bilinear transforms (pre-warped) of the analogue prototypes
 *                behind Tables 1 and 2, derived on the host for the batch's rate (equal to the tables at 48 kHz); float64
 *   loudness     L = -0.691 + 10 log10(sum over channels of the mean square)
 *   sub-blocks   100 ms = sample_rate / 10 frames, counted from enable / reset; momentary = the last 4 complete sub-blocks,
 *                short-term = the last 30.  At every completed sub-block, once 4 exist, the 400 ms block enters the integrated
 *                set; once 30 exist, the 3 s block enters the range set (a 100 ms hop for both)
 *   gating sets  two histograms per stream of 800 bins of 0.1 LU from -70 LUFS: bin b holds blocks with
 *                -70 + 0.1 b <= L < -70 + 0.1 (b + 1) (blocks above +10 LUFS go to the last bin), each bin a count and a float64
 *                energy sum.  Only blocks with L > -70 LUFS (the absolute gate) enter.  A bin passes a relative gate when its
 *                centre (-70 + 0.1 (b + 0.5)) lies above the gate.
 *   integrated   the mean energy of the bins above the relative gate (-10 LU below the mean of the set)
 *   range        EBU Tech 3342: over the bins above -20 LU below the mean of the range set, the nearest-rank P95 minus P10,
 *                each taken as its bin's centre
 *   true peak    BS.1770-4 Annex 2 style: 4x oversampling by a 48-tap linear-phase polyphase FIR (4 phases of 12 taps, a
 *                Kaiser-windowed sinc, beta 7, cut-off at the input's Nyquist frequency, each phase scaled to unit DC gain),
 *                the largest |value| of the oversampled signal and of the samples themselves, since enable / reset.  The
 *                last 11 samples of every channel are kept, so a packet boundary changes nothing.
 * Determinism: no float atomics, fixed-order reductions; the same frames in the same packets give bit-identical readings. */
typedef struct wf_hip_loudness {
    float momentary;   /* LUFS, the last 400 ms */
    float short_term;  /* LUFS, the last 3 s */
    float integrated;  /* LUFS, gated (-70 LUFS absolute, -10 LU relative) */
    float range;       /* LU, EBU Tech 3342 (-70 LUFS absolute, -20 LU relative, P95 - P10) */
    float true_peak;   /* dBTP, the largest since enable / reset */
    uint32_t reserved; /* 0 */
    uint64_t frames;   /* frames measured since enable / reset */
} wf_hip_loudness;
/* A value with nothing to report is -INFINITY (a window not yet filled since enable / reset, an empty gated set, digital
 * silence, a silent true peak); `range` is then 0. */
/* (re)starts the measurement of streams [first, first+count) from the next push on: filter state, sub-blocks, histograms,
 * true peak and frames start afresh.  The first call turns the producer on and allocates the state of every stream of the
 * batch (the others start measuring too).  One entry point for enable and reset keeps the release ABI within its 75 exports.
 * WF_HIP_ERR_INVALID when cfg.sample_rate % 10 != 0 (the 100 ms step must be whole frames).  Spectrum, meter and waveform
 * batches alike.  wf_hip_reset leaves the loudness state alone (a settings change does not restart an integration).  While
 * the producer is on, a push of more frames than the ring holds (wf_hip_ring_frames) is refused with WF_HIP_ERR_INVALID
 * before anything is enqueued.  A multi-device group: call it on each shard (wf_hip_multi_shard) with local indices;
 * WF_HIP_OUT_LOUDNESS is read through wf_hip_multi_read. */
int wf_hip_enable_loudness(wf_hip *h, uint32_t first, uint32_t count);

/* waits for everything the handle has issued.  With WF_HIP_CANARY=1 in the environment of wf_hip_create every device block of the
 * handle ends in guard bytes, which this call then reads back: a kernel that wrote past a buffer makes it return
 * WF_HIP_ERR_RUNTIME with the block named in wf_hip_last_error (a debugging aid: one small copy per block and sync) */
int wf_hip_sync(wf_hip *h);

/* ---- results ----------------------------------------------------------------------------- */
/* What a tick leaves per stream.  One synchronous reader and one pipelined one serve all of them (ABI 13; ABI 12 had a function
 * per output and per form).  Shapes per stream, in the order the reference's members hold them: */
typedef enum wf_hip_output {
    WF_HIP_OUT_DECIBELS = 0,   /* float [output_channels][fft_size/2]        m_decibels (dBFS); not on meter batches */
    WF_HIP_OUT_BARS,           /* float [display_channels][num_bars]         bar tops / curve points in pixels: m_interp_bufs after the optional
                                  Gaussian filter, the dB->y mapping and the mirror of render_bars (src/source.cpp:1535-1564) or
                                  render_curve (:1396-1424) */
    WF_HIP_OUT_PREMIRROR,      /* float [display_channels]                   cfg.mirror_freq_axis displays: render_bars / render_curve take the
                                  row's smallest y for the shader (miny / minpos; gradient and pulse render modes) BEFORE the outputs
                                  above the middle are replaced by images of the lower ones (src/source.cpp:1548-1567, :1411-1424).
                                  Without the Gaussian filter every output above the middle sits on the clamped top position and has one
                                  and the same value: that value (output num_bars / 2 + 1 before the mirror).  With it and the BARS rows
                                  the host finds the reference's miny / minpos without interpolating the row itself.  (With the filter on
                                  the outputs next to the middle are blends and the value is not enough: the plugin binding keeps the
                                  reference's own loops for that combination.) */
    WF_HIP_OUT_VERTICES,       /* float [display_channels][num_vertices][4]  cfg.vertices: x, y, z, w as libobs' vec3 holds them (z = w = 0), the
                                  vertices render_bars / render_curve write into their vertex buffer (src/source.cpp:1576-1659,
                                  :1436-1461), produced by every tick from the bars / curve points of that tick */
    WF_HIP_OUT_VERTEX_COUNTS,  /* uint32 [display_channels]                  stepped bars (cfg.vertices == 3): num_vertices is the buffer's capacity
                                  per channel (num_bars * 6 * max_steps, create_vbuf src/source.cpp:988-1000); how many of them a tick's
                                  draw call uses -- gs_draw(GS_TRIS, 0, vertpos), :1663; vertices beyond it are whatever earlier ticks
                                  left, as in the reference's buffer */
    WF_HIP_OUT_LAST_SILENT,    /* uint8                                      m_last_silent */
    WF_HIP_OUT_TSMOOTH,        /* float [capture_channels][fft_size/2]       m_tsmooth_buf (spectrum batches) */
    WF_HIP_OUT_METER,          /* float [capture_channels]                   meter batches: m_meter_val (dBFS) */
    WF_HIP_OUT_INPUT_RMS,      /* float                                      m_input_rms as of the last tick (wf_hip_enable_input_rms) */
    WF_HIP_OUT_WAVEFORM_TS,    /* uint64                                     waveform batches: m_waveform_ts (src/source.hpp:135, the timestamp of
                                  the next point the sweep will draw, ns) -- what a source needs to continue the sweep on the host
                                  (src/source_generic.cpp:318-353) when it leaves a batch */
    WF_HIP_OUT_LOUDNESS,       /* wf_hip_loudness                            the loudness producer's readings (wf_hip_enable_loudness) as of the
                                  pushes issued so far; 0 bytes while the producer is off */
    WF_HIP_OUT_PEAKS,          /* wf_hip_peaks [output_channels]             the strongest peaks of each m_decibels row as of the newest tick
                                  (spectrum batches; definition below) */
    WF_HIP_OUT_SIGNAL,         /* wf_hip_signal                              level, DC, clipping and stereo phase of the newest
                                  wf_hip_fft_size() frames in the rings as of the pushes issued so far (spectrum and meter
                                  batches; definition below) */
    WF_HIP_OUT_PITCH,          /* wf_hip_pitch                               fundamental frequency (YIN) of the newest
                                  min(wf_hip_fft_size(), 4096) frames in the rings as of the pushes issued so far (spectrum
                                  and meter batches; definition below) */
    WF_HIP_OUT_BANDS,          /* wf_hip_bands [output_channels]             third-octave band levels and the Z / A / C weighted level
                                  of each m_decibels row as of the newest tick (spectrum batches; definition below) */
    WF_HIP_OUT_STEREO,         /* wf_hip_stereo                              correlation, coherence, phase and balance per third-octave
                                  band between captured channels 0 and 1, over the newest frames in the rings as of the pushes
                                  issued so far (spectrum and meter batches with two captured channels; definition below) */
    WF_HIP_OUT_CQ,             /* wf_hip_cq                                  constant-Q spectrum: one level per semitone and captured
                                  channel, each over its own Q periods of the newest frames in the rings as of the pushes issued
                                  so far (spectrum and meter batches; definition below) */
    WF_HIP_OUT_SCOPE,          /* wf_hip_scope                               oscilloscope: the smallest and largest sample per display
                                  column of a triggered view of the newest min(wf_hip_fft_size(), 8192) frames in the rings as of
                                  the pushes issued so far (spectrum and meter batches; definition below) */
    WF_HIP_OUT_GONIO,          /* wf_hip_gonio                               vectorscope: how many of the newest
                                  min(wf_hip_fft_size(), 8192) frames in the rings, as of the pushes issued so far, fall into each
                                  cell of a 64 x 64 side / mid picture that a power of two magnifies to the peak (spectrum and
                                  meter batches with two captured channels; definition below) */
    WF_HIP_OUT_SONO,           /* wf_hip_sono                                sonogram: the level in 64 bands of an eighth of an
                                  octave of up to 64 windows of 1024 frames, 256 frames apart and anchored to the sample counter,
                                  of the audio in the rings as of the pushes issued so far (spectrum and meter batches with a ring
                                  of at least 2048 frames; definition below) */
    WF_HIP_OUT_BITS,           /* wf_hip_bits                                bit statistics: per captured channel the histogram of
                                  sample values, how often each bit of the sample on a 32-bit grid is set, the word length, the
                                  over-range count and the longest run of identical samples of the newest
                                  min(wf_hip_fft_size(), 8192) frames in the rings as of the pushes issued so far (spectrum and
                                  meter batches; definition below) */
    WF_HIP_OUT_THD,            /* wf_hip_thd                                 distortion: per captured channel the fundamental, the
                                  harmonics 2 .. 10, THD, THD+N, SNR, SFDR and the noise floor of the newest P frames in the
                                  rings as of the pushes issued so far, P the largest power of two <= min(wf_hip_fft_size(),
                                  8192) (spectrum and meter batches of at least 512 frames; definition below) */
    WF_HIP_OUT_DELAY,          /* wf_hip_delay                               inter-channel delay: the lag in frames and the
                                  polarity of captured channel 0 against channel 1, with the correlation curve around the peak, of
                                  the newest P frames in the rings as of the pushes issued so far, P the largest power of two <=
                                  min(wf_hip_fft_size(), 4096) (spectrum and meter batches with two captured channels; definition
                                  below) */
    WF_HIP_OUT_ONSET,          /* wf_hip_onset                               onsets: the onset strength of the newest up to 128
                                  columns of 256 frames in the rings as of the pushes issued so far, in total and in three
                                  frequency groups, and the onsets picked from them (spectrum and meter batches whose ring holds at
                                  least 8192 frames; definition below) */
    WF_HIP_OUT_XFER,           /* wf_hip_xfer                                transfer function: gain, phase and coherence per bin
                                  of captured channel 0 (measured) against channel 1 (reference), averaged over K segments of P
                                  frames in the rings as of the pushes issued so far, with the integer delay between them found
                                  and taken out (spectrum and meter batches of at least 256 frames with two captured channels;
                                  definition below) */
    WF_HIP_OUT_IMPULSE,        /* wf_hip_impulse                             impulse response: the response over time of captured
                                  channel 0 (measured) against channel 1 (reference) from the same K segments of P frames, L = P / 4
                                  frames before the delay taken out and 3 L behind it, its envelope in dB and the up to 8 strongest
                                  arrivals (spectrum and meter batches of at least 256 frames with two captured channels;
                                  definition below) */
    WF_HIP_OUT_CLICK,          /* wf_hip_click                               clicks: per captured channel the clicks, pops and
                                  splices of the newest min(wf_hip_fft_size(), 8192) frames in the rings as of the pushes issued so
                                  far, the frames a linear predictor fitted to the window cannot account for, as a count, a rate
                                  and the up to 8 strongest events (spectrum and meter batches of at least 256 frames; definition
                                  below) */
    WF_HIP_OUT_IMD,            /* wf_hip_imd                                 intermodulation: per captured channel the two tones
                                  of a twin-tone stimulus, their 20 products of orders 2 .. 5, total IMD, DFD, modulation
                                  distortion, distortion + noise and the noise floor of the newest P frames in the rings as of the
                                  pushes issued so far, P as WF_HIP_OUT_THD's (spectrum and meter batches of at least 512 frames;
                                  definition below) */
    WF_HIP_OUT_TEMPO,          /* wf_hip_tempo                               tempo: the onset strength of the newest up to 2048
                                  columns of 256 frames in the rings as of the pushes issued so far, its autocorrelation, the tempo
                                  and a second candidate, and the frame of the last and the next beat on the sample counter
                                  (spectrum and meter batches with a ring of at least 131072 frames; definition below) */
    WF_HIP_OUT_HUM             /* wf_hip_hum                                 mains hum: per captured channel the family (50 or
                                  60 Hz), the mains frequency, the qualified harmonics 1 .. 8 with their levels, the hum's level
                                  against the total and the noise floor of the newest N <= 32768 frames in the rings as of the
                                  pushes issued so far (spectrum and meter batches with a ring of at least sample_rate / 3 frames;
                                  definition below) */
} wf_hip_output;
/* ---- spectral peaks (WF_HIP_OUT_PEAKS) ------------------------------------------------------------------------------------
 * Per stream and output channel, let d[0..M-1] be the row exactly as WF_HIP_OUT_DECIBELS returns it, M = fft_size / 2.
 *   candidate      bin k with 1 <= k <= M-2, d[k] > d[k-1], d[k] >= d[k+1] and d[k] > cfg.floor_db
 *   order          d[k] descending, equal values lower k first; the first WF_HIP_MAX_PEAKS are kept.  Selection and order use
 *                  the row's values only, so a host that holds the row reproduces them exactly.
 *   interpolation  the parabola through a = d[k-1], b = d[k], c = d[k+1]: p = 0.5 (a - c) / (a - 2b + c) (the denominator is
 *                  strictly negative, so -0.5 < p <= 0.5), hz = (k + p) sample_rate / fft_size, db = b - 0.25 (a - c) p;
 *                  computed in float64 from the float32 row and rounded to float32 once.
 * The peaks describe the rows the batch displays, after slope, smoothing, volume normalisation and roll-off, and the search
 * covers the whole row, not only the cutoff range.  A stream whose row holds no candidate -- hidden, freshly created or
 * reset (rows at DB_MIN), silent with rows at or below the floor -- has count 0.  After WF_HIP_TICK_NO_DECIBELS ticks the
 * peaks are as stale as the rows.  The peaks are computed when read, by one kernel behind the ticks issued so far, into a
 * block the first read allocates: a handle whose peaks are never read pays nothing.  Meter and waveform batches: wf_hip_read
 * returns WF_HIP_ERR_INVALID and wf_hip_output_bytes 0.  A multi-device group reads them through wf_hip_multi_read. */
#define WF_HIP_MAX_PEAKS 8
typedef struct wf_hip_peak {
    float hz;
    float db;
} wf_hip_peak;
typedef struct wf_hip_peaks {
    uint32_t count;                     /* valid entries, 0..WF_HIP_MAX_PEAKS */
    uint32_t reserved;                  /* 0 */
    wf_hip_peak peak[WF_HIP_MAX_PEAKS]; /* strongest first; unused entries: hz 0, db -INFINITY */
} wf_hip_peaks;                         /* 72 bytes */
/* ---- signal statistics (WF_HIP_OUT_SIGNAL) --------------------------------------------------------------------------------
 * Per stream, over a window of W = wf_hip_fft_size() frames: the newest W frames of each captured channel's ring, positions
 * (wpos - W .. wpos - 1) mod the ring's capacity of the stream's write position.  Every push issued before the read counts,
 * whatever its path (blocking, async / pinned, ragged, device, synth, muted, wf_hip_push_pcm); the A/V-sync delay is not
 * applied.  W is one analysis window on spectrum batches and the meter buffer on meter batches.  After create and
 * wf_hip_reset the rings hold zeros, and a window not yet filled by pushes counts those zeros: a host that keeps a
 * zero-prefixed history of what it pushed reproduces the read.
 *   sums           taken in float64 over the float32 samples, l and r being captured channels 0 and 1:
 *                  S1 = sum x, S2 = sum x^2, Slr = sum l r, Smid = sum ((l + r) / 2)^2, Sside = sum ((l - r) / 2)^2
 *                  (l + r and l - r of two float32 values are exact in float64, so l = -r gives Smid exactly 0).  The
 *                  reduction order is fixed and uses no atomics: the same ring contents read bit-identically.  Each field
 *                  is computed in float64 from the sums and rounded to float32 once.
 *   rms_db         10 log10(S2 / W) (dBFS: a full-scale sine reads -3.01)
 *   peak_db        20 log10(max |x|)
 *   dc             S1 / W
 *   clipped        samples with |x| >= WF_HIP_FULL_SCALE (32767 / 32768: s16's positive extreme counts, u8's 127/128 does not)
 *   correlation    Slr / sqrt(S2l S2r) clamped to [-1, 1]; 0 when S2l or S2r is 0
 *   balance_db     10 log10(S2r / S2l), positive when the right channel is louder; 0 when both are 0, +-INFINITY when one is
 *   mid_db         10 log10(Smid / W)
 *   side_db        10 log10(Sside / W)
 * Every dB field is -INFINITY when its sum or maximum is 0.  With one captured channel ch[1] reads {-INFINITY, -INFINITY,
 * 0, 0}, correlation and balance_db 0, mid_db and side_db -INFINITY.  Computed when read, by one kernel on the handle's
 * stream behind the pushes issued so far, into a block the first read allocates: a handle that never reads it allocates and
 * launches nothing new.  Waveform batches: wf_hip_read returns WF_HIP_ERR_INVALID and wf_hip_output_bytes 0.  A
 * multi-device group reads it through wf_hip_multi_read. */
#define WF_HIP_FULL_SCALE 0.999969482421875f /* 32767 / 32768, exact in float32 */
typedef struct wf_hip_channel_signal {
    float rms_db;     /* 10 log10(S2 / W), dBFS */
    float peak_db;    /* 20 log10(max |x|) */
    float dc;         /* S1 / W */
    uint32_t clipped; /* samples with |x| >= WF_HIP_FULL_SCALE */
} wf_hip_channel_signal;                       /* 16 bytes */
typedef struct wf_hip_signal {
    wf_hip_channel_signal ch[2]; /* captured channels 0 and 1 */
    float correlation;           /* Slr / sqrt(S2l S2r), clamped to [-1, 1] */
    float balance_db;            /* 10 log10(S2r / S2l): positive means right is louder */
    float mid_db;                /* 10 log10(Smid / W), mid  = (l + r) / 2 */
    float side_db;               /* 10 log10(Sside / W), side = (l - r) / 2 */
} wf_hip_signal;                               /* 48 bytes */
/* ---- pitch (WF_HIP_OUT_PITCH) ----------------------------------------------------------------------------------------------
 * Per stream, the fundamental frequency by YIN (de Cheveigne and Kawahara, "YIN, a fundamental frequency estimator for speech
 * and music", JASA 111 (4), 2002, steps 1 to 5).  sr = cfg.sample_rate, W = wf_hip_fft_size().
 *   window         P = min(W, WF_HIP_PITCH_MAX_WINDOW) frames, H = P / 2 (integer division): the newest P frames of each
 *                  captured channel's ring, positions (wpos - P .. wpos - 1) mod the ring's capacity, with the rules of
 *                  WF_HIP_OUT_SIGNAL: every push issued before the read counts whatever its path, the A/V-sync delay is not
 *                  applied, the zeros of create and wf_hip_reset count as samples.
 *   signal         x[i], i < P, in float64: the sample of a one-channel capture, (l + r) / 2 of a two-channel capture (exact
 *                  in float64, and a value of at most 25 bits, so every product of two of them is exact as well).
 *   difference     the paper's eq. 7 for tau = 0 .. H:
 *                      r(tau) = sum_{j<H} x[j] x[j+tau],  e(tau) = sum_{j<H} x[j+tau]^2,
 *                      d(tau) = max(e(0) + e(tau) - 2 r(tau), 0),  d(0) = 0.
 *                  r(tau) and e(tau) are direct sums per lag in float64, both added in the order of j: every product is
 *                  exact and only the additions round, in an order fixed by the window and the same for every lag.  So
 *                  d(tau) is exactly 0 wherever x[j+tau] == x[j] for all j < H (a constant; a period of whole frames), and
 *                  the same ring contents read bit-identically; there are no atomics.
 *   normalisation  d'(0) = 1, d'(tau) = d(tau) tau / sum_{t=1..tau} d(t), and 1 where that running sum is 0 (the cumulative
 *                  mean normalised difference).
 *   search         over tau in [WF_HIP_PITCH_MIN_LAG, H - 1], so hz <= sr / 8 (6 kHz at 48 kHz) and the lowest pitch that
 *                  can be reported is about sr / (H - 1) (23.4 Hz at 48 kHz with P = 4096).  The first tau with
 *                  d'(tau) < WF_HIP_PITCH_THRESHOLD, then forward while tau + 1 <= H - 1 and d'(tau + 1) < d'(tau): that
 *                  lag, voiced = 1.  If no lag is under the threshold: the lag of the smallest d' in the range, the lower
 *                  lag on ties, voiced = 0 (a best guess: noise, a chord, a pitch outside the range).
 *   interpolation  a = d'(lag - 1), b = d'(lag), c = d'(lag + 1); den = a - 2 b + c;
 *                  p = den > 0 ? clamp(0.5 (a - c) / den, -0.5, 0.5) : 0; hz = sr / (lag + p); clarity = clamp(1 - b, 0, 1);
 *                  in float64, each rounded to float32 once.
 *   nothing to report   when sum_{t=1..H} d(t) == 0 (digital silence, a constant, a stereo pair with l = -r):
 *                  hz = 0, clarity = 0, lag = 0, voiced = 0.
 * Accuracy is the estimator's: the parabola through d' reads high at short lags.  Pure sines at 48 kHz with P = 4096 read
 * within 0.0002 % up to 110 Hz, +0.004 % at 440 Hz (lag 109), +0.02 % at 1 kHz (lag 48), +0.19 % at 3 kHz (lag 16) and
 * +0.7 % at 6 kHz (lag 8).  There is no state between reads: smoothing, octave-error correction and note names are the
 * host's.  Computed when read, by one kernel on the handle's stream behind the pushes issued so far (about H^2 float64
 * multiply-adds per stream for r and as many for e: compute-bound, unlike the other outputs; INTEGRATION.md, "Pitch"), into a
 * block the first read allocates: a handle that never reads it allocates and launches nothing new.  Handles with W < 64 and
 * waveform batches: wf_hip_read returns WF_HIP_ERR_INVALID and wf_hip_output_bytes 0.  A multi-device group reads it
 * through wf_hip_multi_read. */
#define WF_HIP_PITCH_MIN_LAG 8
#define WF_HIP_PITCH_THRESHOLD 0.15
#define WF_HIP_PITCH_MAX_WINDOW 4096
typedef struct wf_hip_pitch {
    float hz;        /* sr / (lag + p); 0: nothing to report */
    float clarity;   /* 1 - d'(lag): 1 = perfectly periodic */
    uint32_t lag;    /* the integer lag chosen, frames */
    uint32_t voiced; /* 1: a lag under the threshold was found; 0: the best guess, or nothing */
} wf_hip_pitch;      /* 16 bytes */
/* ---- band levels (WF_HIP_OUT_BANDS) ---------------------------------------------------------------------------------------
 * Per stream and output channel, the levels a real-time analyser shows: 31 third-octave bands and the broadband level
 * unweighted (Z), A-weighted and C-weighted.  sr = cfg.sample_rate, N = wf_hip_fft_size(), M = N / 2, d[0..M-1] the row exactly
 * as WF_HIP_OUT_DECIBELS returns it.  Everything below is float64 unless it says otherwise.
 *   power          P[k] = 10^(d[k] / 10) from the float32 value; P[k] = 0 where d[k] <= wf_hip_db_min(); P[0] = 0 (the DC bin is
 *                  left out: its magnitude carries the factor 2 of the one-sided spectrum, and no band reaches it).
 *   ENBW           the window's equivalent noise bandwidth in bins, N sum(w^2) / (sum w)^2, both sums over the float32 table
 *                  WF_HIP_TABLE_WINDOW in index order; 1 for WF_WINDOW_NONE (an empty table).  Computed on the host.  The
 *                  rows hold |X| 2 / window_sum, so a sine of amplitude A has the power sum A^2 ENBW over its main lobe
 *                  wherever it falls between bins (Parseval); dividing by ENBW makes every level below read 20 log10 A for a
 *                  sine of amplitude A, the convention of the rows themselves.
 *   band grid      IEC 61260-1, base ten: band b = 0 .. WF_HIP_NUM_BANDS - 1 has the centre 1000 * 10^((b - 17) / 10) Hz
 *                  (nominal 20 Hz .. 20 kHz) and lies between the edges e[b] and e[b + 1],
 *                  e[j] = 1000 * 10^((2 (j - 17) - 1) / 20) Hz, j = 0 .. 31.  In bins: E[j] = e[j] N / sr.
 *   bin to band    bin k >= 1 stands for the interval [k - 0.5, k + 0.5] in bins.  Its weight in band b is the length of the
 *                  overlap of that interval with [E[b], E[b + 1]]:
 *                  weight(b, k) = max(min(k + 0.5, E[b + 1]) - max(k - 0.5, E[b]), 0), 0 to 1.  A bin an edge cuts is shared by
 *                  the two bands, its two weights adding to 1.
 *                  band power(b) = sum_k weight(b, k) P[k] / ENBW, band_db[b] = 10 log10(band power), rounded to float32 once.
 *   covered        bit b is set when E[b] >= 0.5 and E[b + 1] <= M - 0.5: the band lies wholly inside the row's frequency
 *                  range.  A band only partly inside still reports what lies inside; a band with no overlap, or with power
 *                  0, reads -INFINITY.  Bit 31 is 0.  `covered` depends on N and sr alone, never on the row.
 *   totals         total = sum_{k=1..M-1} P[k] / ENBW; a and c are the same sum with P[k] multiplied by the squared
 *                  IEC 61672-1 weighting at f = k sr / N, normalised to exactly 1 at 1000 Hz (not the rounded +2.00 / +0.06 dB):
 *                  RA(f) = 12194^2 f^4 / ((f^2 + 20.6^2) sqrt((f^2 + 107.7^2) (f^2 + 737.9^2)) (f^2 + 12194^2)),
 *                  RC(f) = 12194^2 f^2 / ((f^2 + 20.6^2) (f^2 + 12194^2)), weight (R(f) / R(1000))^2.
 *                  Each total is 10 log10 of its sum, -INFINITY for 0, rounded to float32 once.
 *   determinism    no atomics; the order of every sum depends on M and the edges alone, never on the data or on timing: the
 *                  same rows read bit-identically.  A host that restates the sums in another order, or with another exp10,
 *                  differs by rounding only: below 2e-11 dB before the one rounding to float32, so by at most one float32 ulp.
 * The levels describe the rows the batch displays: after slope, smoothing, volume normalisation and roll-off, over the whole
 * row and not only the cutoff range.  A host that wants calibrated levels configures slope 0, no volume normalisation and no
 * roll-off.  Rows at DB_MIN -- hidden, freshly created or reset streams -- read -INFINITY in every level, with `covered` as
 * always.  After WF_HIP_TICK_NO_DECIBELS ticks the levels are as stale as the rows.  Every legal FFT size and sample rate is
 * served; a short FFT simply leaves the low bands uncovered.  Octave bands are the sums of three third-octave powers.
 * Computed when read, by one kernel behind the ticks issued so far, into a block the first read allocates together with
 * the tables of the band edges and of the bins' A and C weights: a handle whose bands are never read allocates and launches nothing new.  Meter and waveform batches:
 * wf_hip_read returns WF_HIP_ERR_INVALID and wf_hip_output_bytes 0.  A multi-device group reads them through
 * wf_hip_multi_read. */
#define WF_HIP_NUM_BANDS 31
typedef struct wf_hip_bands {
    float band_db[WF_HIP_NUM_BANDS]; /* third-octave band levels, band 0 = 20 Hz ... band 30 = 20 kHz */
    uint32_t covered;                /* bit b set: band b lies wholly inside the row's frequency range */
    float total_db;                  /* Z (unweighted) level of the whole row */
    float a_db;                      /* A-weighted level of the whole row (IEC 61672-1) */
    float c_db;                      /* C-weighted level of the whole row */
    uint32_t reserved;               /* 0 */
} wf_hip_bands;                      /* 144 bytes */
/* ---- stereo image (WF_HIP_OUT_STEREO) ---------------------------------------------------------------------------------------
 * Per stream, what a correlation meter by band shows: how captured channels 0 (l) and 1 (r) relate in each of the 31
 * third-octave bands.  WF_HIP_OUT_SIGNAL's one broadband correlation cannot tell a bass that cancels in mono from a wide reverb
 * tail, and the tick keeps magnitudes only, so the output takes a complex transform of its own when read.  sr = cfg.sample_rate,
 * W = wf_hip_fft_size().  Everything below is float64 unless it says otherwise.
 *   window         P = the largest power of two <= min(W, WF_HIP_STEREO_MAX_WINDOW) frames: the newest P frames of both rings,
 *                  positions (wpos - P .. wpos - 1) mod the ring's capacity, with the rules of WF_HIP_OUT_SIGNAL: every push
 *                  issued before the read counts whatever its path, the A/V-sync delay is not applied, the zeros of create and
 *                  wf_hip_reset count as samples.  Hidden and paused streams are read like any other.
 *   transform      w[i] = 0.5 - 0.5 cos(2 pi i / P) (periodic Hann; a table made on the host), z[i] = w[i] (l[i] + j r[i]) from
 *                  the float32 samples, Z = the forward DFT of z with the kernel e^(-j 2 pi i k / P), twiddles from a host-made
 *                  table of cos / sin.  For k = 1 .. P/2 - 1:
 *                      L[k] = (Z[k] + conj Z[P - k]) / 2,   R[k] = (Z[k] - conj Z[P - k]) / (2j):
 *                  one complex transform serves both channels.
 *   per bin        Pll = |L|^2, Prr = |R|^2, C = L conj(R): the phase of C is positive when the left channel leads.
 *   bands          the grid, the edges e[j] and the bin-to-band overlap weights of WF_HIP_OUT_BANDS with N replaced by P:
 *                  E[j] = e[j] P / sr, weight(b, k) = max(min(k + 0.5, E[b + 1]) - max(k - 0.5, E[b]), 0).  For band b,
 *                      A = sum_k weight Pll,  B = sum_k weight Prr,  X = sum_k weight C     (k = 1 .. P/2 - 1).
 *                  `covered` is defined as there, with M = P / 2.
 *   fields         per band, each rounded to float32 once:
 *                  correlation[b] = Re X / sqrt(A B), clamped to [-1, 1]: +1 mono, 0 unrelated or in quadrature, -1 out of phase
 *                  coherence[b]   = |X| / sqrt(A B), clamped to [0, 1]: 1 where one fixed phase and gain relate the channels
 *                                   over the band, small where the phase wanders (decorrelated: reverb, independent sources)
 *                  phase_deg[b]   = atan2(Im X, Re X) 180 / pi, in (-180, 180]; a rounded -180 is reported as +180
 *                  balance_db[b]  = 10 log10(B / A), positive when the right channel is louder
 *                  When A or B is 0, or the band has no overlap with the bins: correlation, coherence and phase read 0, and
 *                  balance_db reads 0 if both are 0 and +-INFINITY if one is (wf_hip_signal's rule).  L and R come out of one
 *                  transform, so a channel of exact zeros leaves a sum of the other's rounding errors, some 310 dB under it,
 *                  not 0: a sum below WF_HIP_STEREO_DEAD_RATIO (2^-80, -240.8 dB) times the other counts as 0, so that a dead
 *                  channel reads as one.  No pair of float32 signals that means anything lies that far apart.
 *   determinism    no atomics; the order of every sum depends on P and the edges alone: the same ring contents read
 *                  bit-identically.  A host that restates the transform with another FFT differs by float64 rounding only,
 *                  below 1e-12 in every field before the one rounding to float32 (phase: wherever coherence >= 0.01; below
 *                  that the phase of a sum that nearly cancels is not a number to rely on).
 * A short window leaves the low bands uncovered (`covered`); no state is kept between reads: averaging over time is the
 * host's.  Computed when read, by one kernel on the handle's stream behind the pushes issued so far (one workgroup per stream,
 * the transform in 16 P bytes of LDS), into a block the first read allocates together with the window, twiddle and edge
 * tables: a handle that never reads it allocates and launches nothing new.  Measured on an MI355X, 4096 stereo streams at FFT
 * 4096: 0.275 ms per read, against 2.36 ms to copy the windows to the host (profiles/stereo_kernel_stats.json; INTEGRATION.md,
 * "Stereo image").  Spectrum and meter batches with two captured
 * channels are served whatever cfg.stereo says (a mono mixdown still captures two).  One captured channel, W < 64 and
 * waveform batches: wf_hip_read returns WF_HIP_ERR_INVALID and wf_hip_output_bytes 0.  A multi-device group reads it through
 * wf_hip_multi_read. */
#define WF_HIP_STEREO_MAX_WINDOW 4096
#define WF_HIP_STEREO_DEAD_RATIO 8.271806125530277e-25 /* 2^-80, exact */
typedef struct wf_hip_stereo {
    float correlation[WF_HIP_NUM_BANDS]; /* Re X / sqrt(A B), -1 .. 1 */
    float coherence[WF_HIP_NUM_BANDS];   /* |X| / sqrt(A B), 0 .. 1 */
    float phase_deg[WF_HIP_NUM_BANDS];   /* phase of X in degrees, (-180, 180]: positive when the left channel leads */
    float balance_db[WF_HIP_NUM_BANDS];  /* 10 log10(B / A): positive means right is louder */
    uint32_t covered;                    /* as wf_hip_bands::covered, for P and sr */
    uint32_t window;                     /* P */
} wf_hip_stereo;                         /* 504 bytes */
/* ---- constant-Q spectrum (WF_HIP_OUT_CQ) -------------------------------------------------------------------------------------
 * Per stream and captured channel, one level per semitone: the "notes" display, from which hosts sum chroma, chord and key
 * displays.  Every other spectral output is a view of the tick's rows and has their one resolution, sr / fft_size per bin --
 * 11.7 Hz at FFT 4096 and 48 kHz, where semitones lie 6 Hz apart at 100 Hz -- so this one analyses the audio in the rings
 * itself, with a window of Q periods per note: long in the bass, short in the treble, the same relative resolution everywhere.
 * sr = cfg.sample_rate.  Everything below is float64 unless it says otherwise.
 *   bins           WF_HIP_CQ_BINS = 120 semitones; bin b has the centre f_b = 440 * 2^((b - 57) / 12) Hz: b = 0 is C0
 *                  (16.35 Hz), b = 57 is A4, b = 119 is B9 (15 804 Hz); bin b is MIDI note 12 + b.  Q = 1 / (2^(1/12) - 1), about
 *                  16.817.
 *   windows        Lmax = min(wf_hip_ring_frames(), WF_HIP_CQ_MAX_WINDOW), L_b = min(ceil(Q sr / f_b), Lmax).  Bin b analyses
 *                  the newest L_b frames of each captured channel's ring, positions (wpos - L_b .. wpos - 1) mod the ring's
 *                  capacity: all bins end at the newest frame.  The rules are WF_HIP_OUT_SIGNAL's: every push issued before
 *                  the read counts whatever its path, the A/V-sync delay is not applied, the zeros of create and wf_hip_reset
 *                  count as samples.  Hidden and paused streams are read like any other.
 *   value          w_b[n] = 0.5 - 0.5 cos(2 pi n / L_b) (periodic Hann), x[n] frame n of the window as float32,
 *                      S_b = sum_{n < L_b} w_b[n] x[n] e^(-j 2 pi f_b n / sr),   a_b = 4 |S_b| / L_b,
 *                  db = 20 log10 a_b, rounded to float32 once; -INFINITY when a_b is 0.  A sine of amplitude A at f_b reads
 *                  20 log10 A, the convention of the rows and of WF_HIP_OUT_BANDS; its semitone neighbours read about 6 dB
 *                  lower, the usual overlap of a Hann constant-Q bank.
 *   covered        bin b is covered when f_b 2^(1/24) < sr / 2: its upper edge lies under the Nyquist frequency.  The covered
 *                  bins are a prefix, `end_covered` is their count; the others read -INFINITY and are not computed.
 *   resolved       `first_resolved` is the lowest b with ceil(Q sr / f_b) <= Lmax (WF_HIP_CQ_BINS when there is none).  Bins
 *                  below it use Lmax frames and are wider than a semitone; a host that wants resolved notes further down
 *                  creates the handle with a larger `ring_frames` (16384 frames at 48 kHz resolve from G#1, 51.9 Hz).  Both
 *                  fields depend on sr and the ring alone, never on the audio.
 *   channels       db[c] is captured channel c; with one captured channel db[1] reads -INFINITY throughout.
 *   determinism    no atomics; every sum in an order fixed by L_b alone: the same ring contents read bit-identically, across
 *                  push paths, repeated reads, slices and shards.  On the device the carrier and the window's phasor start from
 *                  float64 values made on the host for the first 64 frames and advance by a complex multiplication per 64
 *                  frames, at most 256 times.  A host that restates the sums directly differs by float64 rounding: phase
 *                  rounding of 2 pi f_b n / sr (at most 2 pi Q, 106 rad), the 256-step recurrence and the order of the sums,
 *                  about 1e-11 of the window's largest |x| in a_b by derivation; the tests hold it to 1e-10 of that, and to two
 *                  float32 ulps of db wherever a_b is at least 1e-3 of it.  Measured on an MI355X over the tests' shapes: every
 *                  such bin equal to the restatement's float32, every other covered bin within two ulps of it.
 * No state is kept between reads: smoothing over time is the host's.  Computed when read, by one kernel on the handle's stream
 * behind the pushes issued so far (one workgroup per stream, the newest Lmax frames of each channel staged in LDS, one
 * wavefront per bin), into a block the first read allocates together with the per-bin constants (about 250 KB): a handle that
 * never reads it allocates and launches nothing new.  Measured on an MI355X, 4096 stereo streams at FFT 4096: 1.28 ms per read at
 * Lmax 8192 against 4.71 ms to copy the windows to the host, 2.24 ms against 11.28 ms at Lmax 16384 (profiles/cq_kernel_stats.json;
 * INTEGRATION.md, "Constant-Q spectrum").  Spectrum and meter batches are served; on waveform batches wf_hip_read
 * returns WF_HIP_ERR_INVALID and wf_hip_output_bytes 0.  A multi-device group reads it through wf_hip_multi_read. */
#define WF_HIP_CQ_BINS 120
#define WF_HIP_CQ_MAX_WINDOW 16384
typedef struct wf_hip_cq {
    float db[2][WF_HIP_CQ_BINS]; /* captured channels 0 and 1 */
    uint32_t end_covered;        /* covered bins: b < end_covered */
    uint32_t first_resolved;     /* lowest bin with its full Q sr / f window */
    uint32_t max_window;         /* Lmax */
    uint32_t reserved;           /* 0 */
} wf_hip_cq;                     /* 976 bytes */
/* ---- oscilloscope (WF_HIP_OUT_SCOPE) ------------------------------------------------------------------------------------------
 * Per stream, the wave itself against time: a min/max trace of WF_HIP_SCOPE_COLUMNS columns per captured channel, over a view
 * that starts at a trigger point, so that a periodic signal stands still from read to read.  W = wf_hip_fft_size().  Everything
 * below consists of comparisons, exact float64 operations and single correctly rounded IEEE operations: a host that restates it
 * reproduces every field bit for bit.
 *   window         P = min(W, WF_HIP_SCOPE_MAX_WINDOW) frames: the newest P frames of each captured channel's ring, positions
 *                  (wpos - P .. wpos - 1) mod the ring's capacity, with the rules of WF_HIP_OUT_SIGNAL: every push issued before
 *                  the read counts whatever its path, the A/V-sync delay is not applied, the zeros of create and wf_hip_reset
 *                  count as samples.  Hidden and paused streams are read like any other.  x_c[i], i < P, is the float32 sample
 *                  of channel c.
 *   view           V = P / 2 (integer division) frames are drawn, in K = min(WF_HIP_SCOPE_COLUMNS, V) columns.
 *   trigger signal in float64: t[i] = x_0[i] with one captured channel, x_0[i] + x_1[i] with two (exact).
 *   level          an automatic 50 % trigger, so that a DC offset does not stop the scope from triggering: tmax = max t and
 *                  tmin = min t over all P frames, level = (tmax + tmin) * 0.5, hyst = (tmax - tmin) * 0.125,
 *                  u[i] = t[i] - level; each one IEEE float64 operation followed by an exact scaling.
 *   classes        frame i is LOW when u[i] <= -hyst and HIGH when u[i] >= 0; otherwise it is neither.
 *   triggers       walk i upwards from 0, starting unarmed: a LOW frame arms, a HIGH frame met while armed is a trigger and
 *                  disarms.  So i is a trigger iff it is HIGH and the nearest earlier frame that is LOW or HIGH is LOW; then
 *                  i >= 1 and u[i-1] < 0 <= u[i].  The hysteresis rejects the extra zero crossings of a harmonic-rich wave whose
 *                  excursion stays within an eighth of the swing.
 *   selection      `start` is the largest trigger with start <= P - V, so that the view [start, start + V) lies inside the
 *                  window; triggered = 1; period = start - j with j the largest trigger below start, 0 when there is none;
 *                  frac = u[start-1] / (u[start-1] - u[start]), computed in float64 and rounded to float32 once, in (0, 1]: the
 *                  interpolated crossing lies at start - 1 + frac, and a host draws frame start + k at x = k + (1 - frac), the
 *                  crossing at x = 0, for a picture that is steady to less than a sample.  If tmax == tmin (silence, a constant, l = -r) or no trigger lies at or
 *                  below P - V: start = P - V, triggered = 0, period = 0, frac = 0 -- the scope free-runs on the newest V frames.
 *   trace          column c < K covers frames start + floor(c V / K) .. start + floor((c + 1) V / K) - 1 (never empty, K <= V);
 *                  lo[ch][c] and hi[ch][c] are the smallest and largest x_ch among them, as float32.  Columns c >= K and the rows
 *                  of a channel that is not captured read 0.  Behaviour for non-finite samples is not defined.
 *   determinism    no atomics; the result depends on the ring contents alone and reads bit-identically across push paths,
 *                  repeated reads, slices and shards.
 * sample_rate / period is the scope's "frequency" read-out; the time base is the FFT size's (V = fft_size / 2 frames across the
 * picture) and is capped at WF_HIP_SCOPE_MAX_WINDOW frames.  No state is kept between reads.  Computed when read, by one kernel on
 * the handle's stream behind the pushes issued so far (one workgroup per stream, the window of each channel staged in LDS once,
 * the trigger search as a scan over ballots of 64 frames), into a block the first read allocates: a handle that never reads it
 * allocates and launches nothing new.  Cost on an MI355X, 4096 stereo streams: unmeasured (tools/scope_bench.py measures it against
 * copying the windows to the host; INTEGRATION.md, "Oscilloscope").  Spectrum and meter batches are served; on waveform
 * batches and on handles with W < 64, wf_hip_read returns WF_HIP_ERR_INVALID and wf_hip_output_bytes 0.  A multi-device group
 * reads it through wf_hip_multi_read. */
#define WF_HIP_SCOPE_MAX_WINDOW 8192
#define WF_HIP_SCOPE_COLUMNS 256
typedef struct wf_hip_scope {
    float lo[2][WF_HIP_SCOPE_COLUMNS]; /* captured channels 0 and 1: the smallest sample of each column */
    float hi[2][WF_HIP_SCOPE_COLUMNS]; /* the largest */
    uint32_t window;                   /* P */
    uint32_t view;                     /* V */
    uint32_t columns;                  /* K */
    uint32_t start;     /* first frame of the view inside the window; the view ends P - start - V frames before the newest */
    uint32_t triggered; /* 1: start is a trigger; 0: free run */
    uint32_t period;    /* frames back to the trigger before, 0: none (sample_rate / period is a scope's "frequency" read-out) */
    float frac;         /* see above */
    uint32_t reserved;  /* 0 */
} wf_hip_scope;         /* 4128 bytes */
/* ---- vectorscope (WF_HIP_OUT_GONIO) ------------------------------------------------------------------------------------------
 * Per stream, the goniometer of a metering suite: the L/R Lissajous picture, turned so that mid points up and side to the right, as
 * an image of G x G cells that count frames.  W = wf_hip_fft_size(); l and r are captured channels 0 and 1.  Everything below
 * consists of comparisons, integer counting, exact float64 operations and single correctly rounded IEEE operations: a host that
 * restates it reproduces every field bit for bit (tests/gonio_ref.py does).
 *   window         P = min(W, WF_HIP_GONIO_MAX_WINDOW) frames: the newest P frames of both rings, positions
 *                  (wpos - P .. wpos - 1) mod the ring's capacity, with the rules of WF_HIP_OUT_SIGNAL: every push issued before
 *                  the read counts whatever its path, the A/V-sync delay is not applied, the zeros of create and wf_hip_reset
 *                  count as samples.  Hidden and paused streams are read like any other.
 *   peak           A = the largest |l[i]|, |r[i]| over the window, as float32.
 *   zoom           an automatic range, by a power of two so that it is exact.  If A == 0 then e = 0; otherwise A = f 2^e with
 *                  0.5 <= f < 1 (frexp), and e is raised to at least WF_HIP_GONIO_MIN_EXP.  zoom = -e: the picture is magnified
 *                  by 2^zoom, and the loudest sample lies between half and full deflection for every level from -144 dBFS up to
 *                  above full scale.  No state is kept between reads: a host that dislikes the range flipping while the peak
 *                  hovers at a power of two applies its own hysteresis when drawing ("Vectorscope").
 *   coordinates    in float64: x = (r - l) * 0.5 is the side signal, y = (l + r) * 0.5 the mid signal -- the left channel points
 *                  up-left and the right channel up-right, the usual orientation --, u = x * 2^-e and v = y * 2^-e.  The
 *                  subtraction and the addition are one IEEE float64 operation each; every scaling is exact.
 *   cell           G = WF_HIP_GONIO_GRID.  ix = (int) min(max(floor((u + 1.0) * (G / 2)), 0.0), G - 1.0), and iy the same from
 *                  v: an addition, then an exact multiplication.  Without the clamp of e every index is in range by construction
 *                  (|u|, |v| < 1); with it the clamped indices collect on the border.  The min / max is taken in floating point
 *                  before the conversion to integer, so that whatever the samples hold, no index leaves the grid.  Behaviour
 *                  for non-finite samples is otherwise not defined.
 *   image          cell[iy][ix] is the number of frames of the window that fall into the cell (P <= 8192: a uint16 cannot
 *                  overflow).  Row 0 is v = -1, the bottom of the picture.  The cells always add up to P.
 *   scalars        window = P; peak = A; mid_peak = max |y| and side_peak = max |x|, each taken in float64 and rounded to
 *                  float32 once; in_phase = frames with l and r both > 0 or both < 0, out_phase = frames where one is > 0 and the
 *                  other < 0 (sign comparisons, not a product: a zero sample counts in neither); occupied = the number of
 *                  non-zero cells.
 *   determinism    the only accumulation is integer counting, which commutes: the same ring contents read bit-identically
 *                  across push paths, repeated reads, slices and shards.
 * Cell (ix, iy) covers side in [(ix - G/2) / (G/2), (ix - G/2 + 1) / (G/2)) * 2^-zoom and mid likewise from iy.  Computed when
 * read, by one kernel on the handle's stream behind the pushes issued so far (one workgroup per stream, the window of both
 * channels staged in LDS once, the count by integer LDS atomics that neighbouring lanes of equal cell share), into a block the first
 * read allocates: a handle that never reads it allocates and launches nothing new.  Cost on an MI355X, 4096 stereo streams, read
 * into page-locked memory (33.7 MB back): 0.69 / 0.70 / 0.66 ms at W = 4096 for independent noise / a mono source / silence against
 * 2.36 ms for copying the windows to the host, 0.76 / 0.80 / 0.70 ms against 4.71 ms at W = 16384; into pageable memory the read's
 * own copy takes about 3 ms (tools/gonio_bench.py, profiles/gonio_kernel_stats.json; INTEGRATION.md, "Vectorscope").
 * Spectrum and meter batches with two captured channels are served, whatever cfg.stereo says (a mono mixdown still captures two),
 * and there is no lower limit on W; with one captured channel and on waveform batches wf_hip_read returns WF_HIP_ERR_INVALID and
 * wf_hip_output_bytes 0.  A multi-device group reads it through wf_hip_multi_read. */
#define WF_HIP_GONIO_GRID 64
#define WF_HIP_GONIO_MAX_WINDOW 8192
#define WF_HIP_GONIO_MIN_EXP (-24)
typedef struct wf_hip_gonio {
    uint16_t cell[WF_HIP_GONIO_GRID][WF_HIP_GONIO_GRID]; /* [iy][ix] */
    uint32_t window;    /* P */
    int32_t  zoom;      /* the picture is magnified by 2^zoom */
    float    peak;      /* A */
    float    mid_peak;  /* max |(l + r) / 2| */
    float    side_peak; /* max |(r - l) / 2| */
    uint32_t in_phase, out_phase, occupied;
} wf_hip_gonio;         /* 8224 bytes, a multiple of 16 */
/* ---- sonogram (WF_HIP_OUT_SONO) ---------------------------------------------------------------------------------------------
 * Per stream, the spectrogram of a metering suite: level against time and frequency, from the audio the rings hold.  Every other
 * spectral output is a view of one tick's rows, with the tick's time step (a video frame, about 800 frames of audio) and its smear
 * (one FFT window, 85 ms at 4096); this one has a step of 256 frames and a window of 1024, so that a consonant, a click, a
 * drop-out or a drum hit shows.  sr = cfg.sample_rate; everything is float64 unless it says otherwise.
 *   constants      P = WF_HIP_SONO_WINDOW = 1024 frames, H = WF_HIP_SONO_HOP = 256 frames, WF_HIP_SONO_COLUMNS = 64,
 *                  WF_HIP_SONO_BANDS = 64.
 *   columns        wpos is the stream's uint32 write counter as of the pushes issued so far, with the rules of WF_HIP_OUT_SIGNAL:
 *                  every push counts whatever its path, the A/V-sync delay is not applied, the zeros of create and wf_hip_reset
 *                  count as samples, hidden and paused streams are read like any other.  newest = wpos / H (integer division) is
 *                  the absolute index of the newest complete column, and column index n covers counter frames [n H - P, n H), at
 *                  ring positions masked by the capacity: columns are anchored to the counter, not to "now", so column n covers
 *                  the same frames whenever it is read.  All of this arithmetic is uint32 and wraps with the counter; H and the
 *                  capacity divide 2^32, so nothing breaks at the wrap.  columns = T = min(64, (ring_cap - P) / H): the oldest
 *                  column read starts at most (T - 1) H + P + (H - 1) < ring_cap frames back and is always still in the ring.  T
 *                  depends on the ring alone: 28 for the default ring of 8192 frames, 64 from 32768 up (wf_hip_create's
 *                  ring_frames).  The entry is indexed by age: db[c][a][b] with a = 0 column `newest` and a < T column
 *                  newest - a; columns a >= T read -INFINITY.  A host that keeps a waterfall of any length appends the
 *                  (newest_now - newest_before) mod 2^32 / H new columns of each read, at whatever rate it reads.
 *   transform      the window is w[i] = 0.5 - 0.5 cos(2 pi i / P), a host-made table.  With two captured channels
 *                  z[i] = w[i] (l[i] + j r[i]) and Z is its forward DFT with the kernel e^(-j 2 pi i k / P); L[k] and R[k] are
 *                  separated as WF_HIP_OUT_STEREO does it, L = (Z[k] + conj Z[P - k]) / 2, R = (Z[k] - conj Z[P - k]) / 2j, so
 *                  that one complex transform serves both channels.  With one captured channel z = w x and X = Z.  Twiddles
 *                  come from a host-made table.
 *   bands          the band edges are e[j] = 62.5 * 2^(j / 8) Hz, j = 0 .. 64: eight bands to the octave from 62.5 Hz to 16 kHz;
 *                  in bins E[j] = e[j] P / sr.  weight(b, k) = max(min(k + 0.5, E[b+1]) - max(k - 0.5, E[b]), 0) for
 *                  k = 1 .. P/2 - 1, the overlap rule of WF_HIP_OUT_BANDS, and B_c[b] = sum_k weight(b, k) |X_c[k]|^2.  A band
 *                  narrower than a bin takes its share of that bin: at 48 kHz a bin is 46.9 Hz wide and the bands below about
 *                  400 Hz are narrower, so the bottom of the picture is blurred by the 21 ms window, not by the grid.
 *   cell           db = 10 log10(B_c[b] * 32 / (3 P^2)), rounded to float32 once; -INFINITY when the power is 0.  The factor is
 *                  the periodic Hann's coherent gain 1/2 and its noise bandwidth of exactly 1.5 bins: a sine of amplitude A whose
 *                  main lobe lies inside the band range reads 20 log10 A, summed over the bands of a column as powers (0.5 at
 *                  1 kHz and at 5 kHz: -6.0206 dB to 1e-8).  With two channels a band power below WF_HIP_STEREO_DEAD_RATIO times
 *                  the other channel's in the same band and column counts as 0, the stereo image's rule for a dead channel and
 *                  for the same reason.  With one captured channel db[1] reads -INFINITY throughout.
 *   covered        first_covered is the lowest b with E[b] >= 0.5, end_covered the count of bands with E[b+1] <= P/2 - 0.5; both
 *                  depend on sr alone (0 and 64 at 48000 and 44100, 0 and 47 at 8000, 5 and 64 at 192000).  A band partly inside
 *                  the spectrum reports what lies inside; a band with no overlap reads -INFINITY.
 *   determinism    there are no atomics and every sum runs in an order fixed by P and the edges: the same column index reads
 *                  bit-identically across reads, push paths, slices and shards for as long as its frames are in the ring.
 * Resolution: a column is 21.3 ms of audio at 48 kHz and columns are 5.3 ms apart; 64 columns span 0.34 s, 28 columns 0.15 s.
 * Computed when read, by one kernel on the handle's stream behind the pushes issued so far (one wavefront per column, four columns
 * to a workgroup, a float64 transform in LDS), into a block the first read allocates together with its tables: a handle that never
 * reads it allocates and launches nothing new, and no state is kept between reads -- averaging, peak hold and a longer history are
 * the host's, and `newest` makes them exact.  Cost on an MI355X, 4096 stereo streams at FFT 4096 read into page-locked memory
 * (134.3 MB back, whatever T): 3.42 ms with the default ring (T = 28) against 4.71 ms for copying the 268.4 MB of both rings that
 * the columns span to the host, 3.86 ms with ring_frames = 32768 (T = 64) against 10.00 ms for its 570.4 MB; into pageable memory
 * the read's own copy takes 12 to 13 ms and loses to either (tools/sono_bench.py, profiles/sono_kernel_stats.json;
 * INTEGRATION.md, "Sonogram").
 * Spectrum and meter batches with one or two captured channels and any FFT size are served; on waveform batches and on handles
 * whose ring holds fewer than 2048 frames (T would be below 4) wf_hip_read returns WF_HIP_ERR_INVALID and wf_hip_output_bytes 0.
 * A multi-device group reads it through wf_hip_multi_read. */
#define WF_HIP_SONO_WINDOW 1024
#define WF_HIP_SONO_HOP 256
#define WF_HIP_SONO_COLUMNS 64
#define WF_HIP_SONO_BANDS 64
typedef struct wf_hip_sono {
    float db[2][WF_HIP_SONO_COLUMNS][WF_HIP_SONO_BANDS]; /* [channel][age][band] */
    uint32_t columns;        /* T */
    uint32_t newest;         /* wpos / H: the absolute index of the column of age 0 */
    uint32_t first_covered, end_covered;
    uint32_t window, hop;    /* P, H */
    uint32_t reserved[2];    /* 0 */
} wf_hip_sono;               /* 32800 bytes, a multiple of 16 */
/* ---- bit statistics (WF_HIP_OUT_BITS) ---------------------------------------------------------------------------------------
 * Per stream and captured channel, the bit meter of a metering suite: how many bits the audio really carries, whether a bit is
 * stuck, whether the signal is clipped into flat tops, whether a drop-out left a run of identical samples, and whether codes are
 * missing from the value histogram because the audio was requantised.  W = wf_hip_fft_size().  Every step below is a comparison,
 * an exact operation or an integer operation: a host that restates it reproduces every field bit for bit (tests/bits_ref.py
 * does).
 *   window         P = min(W, WF_HIP_BITS_MAX_WINDOW) frames: the newest P frames of each captured channel's ring, positions
 *                  (wpos - P .. wpos - 1) mod the ring's capacity, with the rules of WF_HIP_OUT_SIGNAL: every push issued before
 *                  the read counts whatever its path, the A/V-sync delay is not applied, the zeros of create and wf_hip_reset
 *                  count as samples.  Hidden and paused streams are read like any other.  x[i], i < P, is the float32 sample
 *                  and bits[i] its 32-bit pattern.
 *   code           the sample on a 32-bit two's-complement grid.  y = (double)x * 2^31, which is exact.  over <=> y >= 2^31 or
 *                  y < -2^31, that is x >= 1 or x < -1: -1.0 fits and +1.0 does not.  v = (int32) min(max(floor(y), -2^31),
 *                  2^31 - 1).  fine <=> not over and floor(y) != y: only a float32 below 2^-8 in magnitude can be fine, a sample
 *                  with bits below 2^-31, which no integer PCM format of up to 32 bits produces.  s(v) = v for v >= 0 and ~v for
 *                  v < 0, and m(v) is the number of significant bits of s(v): 0 for s = 0, else 32 - clz(s); 0 .. 31.  The
 *                  device derives v from the sign, the exponent and the mantissa with integer shifts, so nothing depends on how
 *                  the hardware treats denormals.  +-INFINITY follow the rules above (over, clamped); for a NaN nothing is
 *                  promised except that no index leaves its table.
 *   hist           hist[(v >> 24) + 128], an arithmetic shift: bin h counts the frames with x in [(h - 128) / 128,
 *                  (h - 127) / 128), and over-range frames land in bin 0 or 255.  The linear sample-value histogram: clipping
 *                  shows as spikes at the ends, asymmetry as a lopsided shape, requantised audio as a comb.
 *   ones           ones[b] = the frames whose v has bit b set; b = 0 is the least significant bit (2^-31), b = 31 the sign.  A
 *                  bit with ones == 0 or ones == P inside the used range is stuck.
 *   mag            mag[m(v)]: a level histogram in steps of 6.02 dB; mag[31] is |x| in [0.5, 1), mag[0] is v = 0 or v = -1.
 *   word_length    0 if every v is 0, else 32 - ctz(the OR of all v): 8 for u8 audio, 16 for s16, 24 for 24-bit audio, and 32
 *                  for float audio, where fine > 0 says that there is more below the grid.
 *   magnitude_bits the largest m(v): the headroom is 31 - magnitude_bits bits.
 *   over, fine     the counts of the frames that are over and fine.
 *   repeats        the frames i >= 1 with bits[i] == bits[i - 1].  Patterns are compared, so +0 and -0 differ; the frame in
 *                  front of the window does not count.
 *   runs           a run is a maximal stretch of equal patterns inside the window.  max_run is the longest run's length (>= 1),
 *                  max_run_start the window index of the first frame of the first run of that length, and max_run_value its
 *                  sample.  A long run at 0 is a drop-out, one at the peak a flat top.
 *   invariants     sum(hist) = sum(mag) = P, and ones[31] = the frames with v < 0.  P <= 8192: no uint16 overflows.
 *   determinism    the accumulations are integer counts, ORs and a maximum with a fixed tie-break: the same ring contents read
 *                  bit-identically across push paths, repeated reads, slices and shards.
 * Computed when read, by one kernel on the handle's stream behind the pushes issued so far (one workgroup per stream, the window of
 * every captured channel staged in LDS once, ballots and popcounts for the bits, integer LDS atomics that neighbouring lanes of equal
 * bin share for the histogram), into a block the first read allocates: a handle that never reads it allocates and launches nothing
 * new, and no state is kept between reads -- averaging and peak hold are the host's.
 * Cost on an MI355X, 4096 stereo streams, read into page-locked memory (5.57 MB back): 0.53 / 0.52 / 0.50 ms at W = 4096 for
 * independent noise / a 100 Hz sine / silence against 2.36 ms for copying the 134.2 MB of windows to the host, and 1.28 / 1.29 /
 * 1.17 ms against 4.71 ms at W = 16384 (P = 8192): the read wins at both shapes and for every kind, 4.5 to 4.8 times at W = 4096
 * and 3.7 to 4.0 times at the cap.  Into a fresh pageable numpy array (the Python reader) a read takes 0.50 to 1.33 ms and wins as
 * well.  The kernel's own time without its copy is unmeasured (tools/bits_bench.py, profiles/bits_kernel_stats.json;
 * INTEGRATION.md, "Bit meter").
 * Spectrum and meter batches with one or two captured channels are served, and there is no lower limit on W; on waveform batches
 * wf_hip_read returns WF_HIP_ERR_INVALID and wf_hip_output_bytes 0.  A multi-device group reads it through wf_hip_multi_read. */
#define WF_HIP_BITS_MAX_WINDOW 8192
typedef struct wf_hip_bits_channel {
    uint16_t hist[256];      /* [(v >> 24) + 128] */
    uint16_t ones[32];       /* [bit of v] */
    uint16_t mag[32];        /* [m(v)] */
    uint32_t word_length, magnitude_bits, over, fine, repeats, max_run, max_run_start;
    float max_run_value;
} wf_hip_bits_channel;       /* 672 bytes */
typedef struct wf_hip_bits {
    wf_hip_bits_channel ch[2]; /* captured channels 0 and 1; with one captured channel ch[1] is all zero bytes */
    uint32_t window;         /* P */
    uint32_t reserved[3];    /* 0 */
} wf_hip_bits;               /* 1360 bytes, a multiple of 16 */
/* ---- distortion (WF_HIP_OUT_THD) --------------------------------------------------------------------------------------------
 * Per stream and captured channel, the distortion analyser of a metering suite: the level and frequency of a test tone, the level
 * of its harmonics 2 .. 10, THD, THD+N (SINAD is its negative), SNR, SFDR, the noise floor and the effective number of bits.  No
 * other output can stand in for it: the tick's rows are float32 and Hann-class windowed, with a leakage floor far above a -100 dB
 * harmonic.  W = wf_hip_fft_size(), sr = cfg.sample_rate; everything is float64 unless it says otherwise.
 *   window         P = the largest power of two <= min(W, WF_HIP_THD_MAX_WINDOW = 8192): the newest P frames of each captured
 *                  channel's ring, positions (wpos - P .. wpos - 1) mod the ring's capacity, with the rules of WF_HIP_OUT_SIGNAL:
 *                  every push issued before the read counts whatever its path, the A/V-sync delay is not applied, the zeros of
 *                  create and wf_hip_reset count as samples.  Hidden and paused streams are read like any other.
 *   taper          w[i] = sum_{m = 0 .. 6} (-1)^m a_m cos(2 pi m i / P), the periodic 7-term Blackman-Harris window, a host-made
 *                  table, with a = 0.27105140069342, 0.43329793923448, 0.21812299954311, 0.06592544638803, 0.01081174209837,
 *                  0.00077658482522, 0.00001388721735.  Its side lobes are about -180 dB and its main lobe is +-7 bins;
 *                  H = WF_HIP_THD_LOBE = 8 is the half-width of every region below.
 *   spectrum       per captured channel c, X_c = DFT_P(w x_c) with the kernel e^(-j 2 pi i k / P) and p[k] = |X_c[k]|^2 for
 *                  1 <= k < M = P / 2.  With two captured channels both come out of one complex transform of w (x_0 + j x_1),
 *                  separated as WF_HIP_OUT_STEREO does it; with one the imaginary part is 0 and ch[1] is all zero bytes.  A
 *                  channel whose P frames are all +-0 has p = 0 exactly, whatever the other channel holds (the device sets it
 *                  so: the shared transform's rounding would otherwise leave it some 1e-32 of the other channel's power), and a
 *                  NaN or an infinity in either channel's window spoils the shared transform: both channels then read valid = 0.
 *                  S = P sum w[i]^2 / 4: a sine of amplitude A well inside the band has a lobe power of A^2 S.
 *   fundamental    k0 = the argmax of p over k in [2H + 1, M - H - 1]: the search starts from (k = 2H + 1, best = 0) and only a
 *                  strictly greater value wins, so the lowest index wins a tie and a NaN never wins.  F = the sum of p[k] over
 *                  |k - k0| <= H and f0 = (sum k p[k]) / F over the same bins, in bins of P.  If F is not a finite number > 0
 *                  (silence; a NaN or an infinity in the window) valid = 0 and every other field of the channel is 0.
 *   harmonics      for h = 2 .. 10 (WF_HIP_THD_HARMONICS = 9) k_h = floor(h f0 + 0.5).  Harmonic h is in band iff
 *                  k_h + H <= M - 1; then H_h = the sum of p[k] over |k - k_h| <= H and bit h - 2 of `harmonics` is set.
 *                  Harmonics beyond the band are not folded back.
 *   residue        D = the sum of p[k] over H < k < M with |k - k0| > H, summed directly and never as a difference.  N = the sum
 *                  over those of these bins that lie in no in-band harmonic region, n their count, and
 *                  N_s = N (M - 3H - 2) / n fills the removed bins back in.  k_s = the argmax, lowest index on ties, of p over
 *                  the bins of D: the strongest spur, a harmonic included.
 *   levels         dB(x, y) = 10 log10(x / y); -INFINITY where x is 0, else +INFINITY where y is 0.  Each float32 field is
 *                  rounded once from float64.
 *                    fundamental_hz (double) f0 sr / P          fundamental_db   dB(F, S): a sine of amplitude A reads 20 log10 A
 *                    harmonic_db[h - 2]      dB(H_h, F), dBc; -INFINITY when harmonic h is not in band
 *                    thd_db                  dB(sum H_h, F); -INFINITY when no harmonic is in band
 *                    thdn_db                 dB(D, F)           snr_db           dB(F, N_s)
 *                    noise_db                dB(N_s, 2S): white noise of variance s^2 reads 10 log10 s^2
 *                    sfdr_db                 dB(p[k0], p[k_s])  spur_hz          k_s sr / P
 *                    enob                    (-thdn_db - 1.76) / 6.02, from the float64 thdn_db
 *                    fundamental_bin k0, spur_bin k_s, harmonics, valid (uint32)
 *                  Nothing reads NaN while valid is 1.
 *   determinism    the order of every sum follows from P, k0 and the k_h alone and there are no atomics: the same ring contents
 *                  read bit-identically across push paths, repeated reads, slices and shards.
 * Resolution: a bin is 5.9 Hz wide at P = 8192 and 48 kHz, and the fundamental must lie at least 17 bins up, about 100 Hz.
 * Computed when read, by one kernel on the handle's stream behind the pushes issued so far (one workgroup of 512 threads per stream,
 * a float64 transform of P points in up to 128 KB of LDS, so one workgroup to a CU at the cap), into a block the first read
 * allocates together with its tables: a handle that never reads it allocates and launches nothing new, and no state is kept between
 * reads -- averaging is the host's.
 * Cost on an MI355X, 4096 stereo streams, read into page-locked memory (0.85 MB back): 0.29 ms at W = 4096 against 2.37 ms for
 * copying the 134.2 MB of windows to the host, and 0.63 ms against 5.62 ms at W = 16384 (P = 8192): 8.1 and 8.9 times.  Into a fresh
 * pageable numpy array (the Python reader) a read takes 0.32 and 0.66 ms.  The kernel's own time without its copy is unmeasured
 * (tools/thd_bench.py, profiles/thd_kernel_stats.json; INTEGRATION.md, "Distortion").
 * Spectrum and meter batches with one or two captured channels and W >= 512 are served (the analysis needs 17 bins below the
 * fundamental and room for the regions above it); on waveform batches and below 512 frames wf_hip_read returns WF_HIP_ERR_INVALID
 * and wf_hip_output_bytes 0.  A multi-device group reads it through wf_hip_multi_read. */
#define WF_HIP_THD_MAX_WINDOW 8192
#define WF_HIP_THD_LOBE 8
#define WF_HIP_THD_HARMONICS 9
typedef struct wf_hip_thd_channel {
    double fundamental_hz;
    float fundamental_db, thd_db, thdn_db, snr_db, noise_db, sfdr_db, spur_hz, enob;
    float harmonic_db[WF_HIP_THD_HARMONICS]; /* [h - 2], dBc */
    uint32_t fundamental_bin, spur_bin;
    uint32_t harmonics;      /* bit h - 2: harmonic h is in band */
    uint32_t valid;
    uint32_t reserved;       /* 0 */
} wf_hip_thd_channel;        /* 96 bytes */
typedef struct wf_hip_thd {
    wf_hip_thd_channel ch[2]; /* captured channels 0 and 1; with one captured channel ch[1] is all zero bytes */
    uint32_t window;         /* P */
    uint32_t reserved[3];    /* 0 */
} wf_hip_thd;                /* 208 bytes, a multiple of 16 */
/* ---- inter-channel delay (WF_HIP_OUT_DELAY) -------------------------------------------------------------------------------------
 * Per stream, the delay finder of a metering suite: by how many frames one captured channel lags the other, and whether one of
 * them is inverted -- two microphones on one voice, a desktop capture behind a microphone, a lead wired out of phase.  No other
 * output can stand in for it: WF_HIP_OUT_SIGNAL and WF_HIP_OUT_STEREO report the correlation at lag 0 only, where a negative
 * reading cannot tell a polarity flip from a 0.3 ms offset.  W = wf_hip_fft_size(), sr = cfg.sample_rate; everything is float64
 * unless it says otherwise.
 *   window         P = the largest power of two <= min(W, WF_HIP_DELAY_MAX_WINDOW = 4096): the newest P frames of both captured
 *                  channels' rings, positions (wpos - P .. wpos - 1) mod the ring's capacity, with the rules of WF_HIP_OUT_SIGNAL:
 *                  every push issued before the read counts whatever its path, the A/V-sync delay is not applied, the zeros of
 *                  create and wf_hip_reset count as samples.  Hidden and paused streams are read like any other.  M = P / 2 and
 *                  L = P / 4, the range of lags.
 *   taper          w[i] = 0.5 - 0.5 cos(2 pi i / P), the periodic Hann window, a host-made table.
 *   spectra        X_c = DFT_P(w x_c) with the kernel e^(-j 2 pi i k / P); on the device both come out of one complex transform
 *                  of w (x_0 + j x_1), separated as WF_HIP_OUT_STEREO does it.  Only the bins 1 <= k < M are used: DC and Nyquist
 *                  are not.
 *   cross spectrum G[k] = X_0[k] conj X_1[k], g = max_k |G[k]|, E_c = sum_k |X_c[k]|^2.
 *   weighting      PHAT with a floor: u[k] = |G[k]| / max(|G[k]|, b g) and A[k] = G[k] / max(|G[k]|, b g) with b = 1e-3.  A bin
 *                  more than 60 dB under the strongest cross-power fades out in proportion instead of entering with unit weight
 *                  and a phase made of rounding noise, which is what plain PHAT gives it.
 *   correlations   for integer n, circular over P:
 *                    R[n] = (1 / (M - 1)) sum_k Re(A[k] e^(j 2 pi k n / P))    a pure broadband delay reads close to 1
 *                    C[n] = sum_k Re(G[k] e^(j 2 pi k n / P)) / sqrt(E_0 E_1)  the ordinary normalised cross-correlation of the
 *                                                                              tapered windows, in [-1, 1]
 *   lag            n0 = the argmax of |R[n]| over -L <= n <= L: the scan runs from n = -L upwards and only a strictly greater
 *                  value wins.  polarity = +1 if R[n0] > 0, else -1.  A positive lag means that channel 0 is the later one:
 *                  x_0(t) = x_1(t - d).
 *   fraction       from the slope of the phase, not by interpolating the peak (parabolic interpolation of a sinc-shaped peak is
 *                  biased: it reads 5.07 to 5.18 for a true 5.3): B[k] = polarity A[k] e^(j 2 pi ((k n0) mod P) / P),
 *                  phi[k] = atan2(Im B[k], Re B[k]), f = -(P / 2 pi) sum_k u[k] k phi[k] / sum_k u[k] k^2, clamped to [-0.5, 0.5]
 *                  and 0 where the denominator is 0.  With the integer lag taken out |phi| stays under pi / 2 for coherent bins,
 *                  so nothing is unwrapped.
 *   fields         each float32 field is rounded once from float64.
 *                    delay_frames (double)  n0 + f              delay_ms     1000 delay_frames / sr
 *                    peak                   R[n0], signed       corr         C[n0]           corr_zero   C[0]
 *                    ambiguity              the largest |R[n]| over -L <= n <= L with |n - n0| > 2, over |R[n0]| (0 where
 *                                           R[n0] is 0): near 0 one clear arrival, near 1 a tone or unrelated channels -- the
 *                                           delay is not to be trusted
 *                    lag (int32) n0, polarity (int32), valid, window = P (uint32)
 *                    curve[i]               R[n0 - 32 + i], i < WF_HIP_DELAY_CURVE = 65: the picture a delay finder draws around
 *                                           its peak.  The index is circular and may leave +-L.
 *   validity       valid = 0, and every other field but `window` 0, when either channel's window is all +-0, when either holds a
 *                  NaN or an infinity, or when g is not a finite number > 0.  valid = 1 says "computed", not "reliable":
 *                  reliability is `peak` against `ambiguity`, for the host to judge.
 *   determinism    no atomics, and every sum and every max runs in an order that follows from P alone: the same ring contents
 *                  read bit-identically across push paths, repeated reads, slices and shards.
 * Limits: the correlation is circular over tapered windows, so the peak shrinks as |d| approaches L (to about 0.55 at |d| = L), and
 * delays beyond L read as noise with a high `ambiguity`.  At 48 kHz and P = 4096 L is 21 ms, a path of 7 m.  At P = 128 a delay
 * of a few frames is found to about 0.03 frame and one beyond P / 8 to about 0.16; from P = 1024 up to 0.01.
 * Computed when read, by one kernel on the handle's stream behind the pushes issued so far (one workgroup of 256 threads per
 * stream, two float64 transforms of P points in two LDS regions, 128 KB at the cap, so one workgroup to a CU there), into a block
 * the first read allocates together with its tables: a handle that never reads it allocates and launches nothing new, and no state
 * is kept between reads -- smoothing over reads is the host's.
 * Cost on an MI355X, 4096 stereo streams, read into page-locked memory (1.31 MB back): 0.44 ms at W = 4096 and at W = 16384 (P =
 * 4096 at both) against 2.36 ms for copying the 134.2 MB of windows to the host: 5.4 times.  Into a fresh pageable numpy array (the
 * Python reader) a read takes 0.44 ms as well.  The kernel's own time without its copy is unmeasured (tools/delay_bench.py,
 * profiles/delay_kernel_stats.json; INTEGRATION.md, "Inter-channel delay").
 * Spectrum and meter batches with two captured channels are served, at every legal W; with one captured channel and on waveform
 * batches wf_hip_read returns WF_HIP_ERR_INVALID and wf_hip_output_bytes 0.  A multi-device group reads it through
 * wf_hip_multi_read. */
#define WF_HIP_DELAY_MAX_WINDOW 4096
#define WF_HIP_DELAY_CURVE 65
typedef struct wf_hip_delay {
    double delay_frames;     /* n0 + f: positive when channel 0 is the later one */
    float delay_ms, peak, corr, corr_zero, ambiguity;
    int32_t lag;             /* n0 */
    int32_t polarity;        /* +1, or -1: one channel is inverted */
    uint32_t valid;
    uint32_t window;         /* P */
    uint32_t reserved;       /* 0 */
    float curve[WF_HIP_DELAY_CURVE]; /* R[n0 - 32 + i] */
    uint32_t reserved2[3];   /* 0 */
} wf_hip_delay;              /* 320 bytes, a multiple of 16 */
/* ---- onsets (WF_HIP_OUT_ONSET) -----------------------------------------------------------------------------------------------
 * Per stream, when something starts: a kick, a note, a consonant, a cut.  No other output says so -- the levels say how loud it
 * is, and the tick's time step (a video frame, about 800 frames of audio, under an 85 ms window) is too coarse to tell.  This
 * output is the positive change of a compressed band level from one sonogram column to the next (spectral flux), in total and in
 * three frequency groups, and the onsets picked from each of the four curves by one fixed rule.  sr = cfg.sample_rate; everything is
 * float64 unless it says otherwise.
 *   constants      P = WF_HIP_ONSET_WINDOW = 1024 frames, H = WF_HIP_ONSET_HOP = 256 frames, WF_HIP_ONSET_COLUMNS = 128,
 *                  WF_HIP_ONSET_BANDS = 64, the sonogram's filterbank, in three groups: low = bands 0 .. 15 (62.5 to 250 Hz),
 *                  mid = 16 .. 39 (250 Hz to 2 kHz), high = 40 .. 63 (2 to 16 kHz).
 *   columns        the sonogram's: wpos is the stream's uint32 write counter as of the pushes issued so far, with the rules of
 *                  WF_HIP_OUT_SIGNAL (every push counts whatever its path, the A/V-sync delay is not applied, the zeros of create
 *                  and wf_hip_reset count as samples, hidden and paused streams are read like any other); newest = wpos / H, and
 *                  spectral column n covers counter frames [n H - P, n H) at ring positions masked by the capacity.  The
 *                  arithmetic is uint32 and wraps with the counter.  Ts = min(129, (ring_cap - P) / H) spectral columns are
 *                  always in the ring and give T = Ts - 1 strength columns: 27 for a ring of 8192 frames, 59 for 16384, 123 for
 *                  32768, 128 from 65536 up (wf_hip_create's ring_frames).  Every array is indexed by age: age a is column
 *                  newest - a; ages >= T read 0 with flags 0.
 *   transform      exactly the sonogram's: the periodic Hann window, both captured channels through one complex transform and
 *                  separated from Z[k] and conj Z[P - k], the 64 eighth-octave bands from 62.5 Hz with the same overlap weights.
 *                  The band power is B[n][b] = B_0[n][b] + B_1[n][b], the sum over the captured channels; there is no
 *                  dead-channel rule here.
 *   level          a[n][b] = sqrt(B[n][b] * 32 / (3 P^2 capture_channels)), the rms amplitude a sine would need, and
 *                  S[n][b] = log1p(100 a[n][b]) / ln 10: linear below the knee at -40 dBFS, logarithmic above it, so that neither
 *                  the noise floor's flutter nor level alone decides.  A column of zeros gives S = 0 exactly.
 *   strength       d[n][b] = max(S[n][b] - S[n-1][b], 0); low, mid and high are the sums of d over the group's bands, each in
 *                  ascending band order, and strength[n] = (low + mid) + high.  Each of the four is rounded to float32 once.
 *   picking        on the float32 values alone, by comparisons, float64 additions and one division -- no product, so that no
 *                  compiler can contract anything -- and with the same constants for the total and for each group.  Column n is
 *                  decided when the columns n - 16 .. n + 3 are all among the T returned: ages 3 .. T - 17.  A decided column
 *                  of the curve o is an onset if and only if
 *                    o[n] >  o[m] for m = n - 6 .. n - 1,
 *                    o[n] >= o[m] for m = n + 1 .. n + 3, and
 *                    o[n] >= mean + 2.0 with mean = (o[n - 16] + ... + o[n + 3]) / 20, summed oldest first in float64.
 *                  A decision depends on 20 columns anchored to the counter: once decided, a column's flags never change, and
 *                  read the same bits at any later read while the column is in view.  With the smallest ring ages 3 .. 10 are
 *                  decided, 2048 frames: a reader at 24 Hz or faster sees every column decided.  The latency is 3 hops, 16 ms at
 *                  48 kHz.
 *   flags          bit 0: onset of the total; bits 1, 2, 3: onset of low, mid, high; bit 7: decided.
 *   summary        columns = T, newest, decided_first = 3, decided_end = T - 16 (0 if no column is decided), window = P,
 *                  hop = H; onsets = the decided columns in view with bit 0; last_age = the age of the newest of them (0xFFFFFFFF
 *                  if there is none, and last_frame and last_strength are then 0), last_frame = n H - 384 of that column (uint32,
 *                  wraps with the counter): the column's end less 3 P / 8, where the start of the event lies to within about a
 *                  hop; last_strength = its strength.
 *   determinism    no atomics, and every sum runs in a fixed order: the same column reads bit-identically across reads, push
 *                  paths, slices and shards for as long as its frames and its predecessor's are in the ring.
 * The constants -- the knee 100, the margin 2.0, the windows 6 / 3 / 16 -- were chosen with a numpy prototype on synthetic audio:
 * over 4 s each they find every event of 60 Hz kicks over noise at -40 dB, of noise bursts over noise at -30 dB and of legato note
 * changes at equal level, and flag nothing on stationary noise at -20 and -60 dBFS or on a steady sine.  They are definitional, as
 * a library's defaults are, and have not been tuned on recorded music.  Tempo, smoothing and any longer history are the host's:
 * `newest` makes appending exact.
 * Computed when read, by one kernel on the handle's stream behind the pushes issued so far (one workgroup of 256 threads per
 * stream, one wavefront per spectral column, float64 transforms in LDS), into a block the first read allocates together with its
 * tables: a handle that never reads it allocates and launches nothing new, nothing is added to the tick, and no state is kept
 * between reads.  Cost on an MI355X, 4096 stereo streams at FFT 4096 read into page-locked memory (9.18 MB back): 0.86 ms with the
 * default ring (T = 27) against 4.72 ms for copying the 268.4 MB of both rings that the columns span to the host, 3.29 ms with
 * ring_frames = 65536 (T = 128) against 19.64 ms for its 1115.7 MB.  The kernel's own time without its copy is unmeasured
 * (tools/onset_bench.py, profiles/onset_kernel_stats.json; INTEGRATION.md, "Onsets").
 * Spectrum and meter batches with one or two captured channels and any FFT size are served; on waveform batches and on handles
 * whose ring holds fewer than 8192 frames (no column would be decided) wf_hip_read returns WF_HIP_ERR_INVALID and
 * wf_hip_output_bytes 0.  A multi-device group reads it through wf_hip_multi_read. */
#define WF_HIP_ONSET_WINDOW 1024
#define WF_HIP_ONSET_HOP 256
#define WF_HIP_ONSET_COLUMNS 128
#define WF_HIP_ONSET_BANDS 64
typedef struct wf_hip_onset {
    float strength[WF_HIP_ONSET_COLUMNS];  /* [age] (low + mid) + high */
    float group[3][WF_HIP_ONSET_COLUMNS];  /* [low, mid, high][age] */
    uint8_t flags[WF_HIP_ONSET_COLUMNS];   /* [age] */
    uint32_t columns;        /* T */
    uint32_t newest;         /* wpos / H: the absolute index of the column of age 0 */
    uint32_t decided_first, decided_end; /* the ages [3, T - 16) carry bit 7 */
    uint32_t window, hop;    /* P, H */
    uint32_t onsets;         /* decided columns in view with bit 0 */
    uint32_t last_age;       /* of the newest of them; 0xFFFFFFFF: none */
    uint32_t last_frame;     /* its counter position, (newest - last_age) H - 384 */
    float last_strength;
    uint32_t reserved[6];    /* 0 */
} wf_hip_onset;              /* 2240 bytes, a multiple of 16 */
/* ---- transfer function (WF_HIP_OUT_XFER) ---------------------------------------------------------------------------------------
 * Per stream, the third instrument of a dual-channel analyser: the frequency response between the two captured channels with the
 * programme itself as the stimulus -- magnitude, phase and coherence against frequency, what Smaart, REW and ARTA call the transfer
 * function: a microphone chain against its dry feed, a return against its send.  No other output can stand in for it:
 * WF_HIP_OUT_STEREO reads one window, so its coherence means something only across a band, and it reports no gain and no phase of a
 * system; WF_HIP_OUT_DELAY reads one window and reports one number.  A transfer function needs an average over several segments, and
 * the ring holds them, so nothing is kept between reads.  W = wf_hip_fft_size(), R = wf_hip_ring_frames(), sr = cfg.sample_rate;
 * everything is float64 unless it says otherwise.
 *   roles          captured channel 1 is the reference (what went in), channel 0 the measured signal (what came out): the
 *                  convention of WF_HIP_OUT_DELAY, where a positive lag means that channel 0 is the later one, x_0(t) = x_1(t - d),
 *                  a causal system.  The other direction costs the host nothing: H_01[k] = coherence[k] / H_10[k].
 *   segments       P = the largest power of two <= min(W, WF_HIP_XFER_MAX_WINDOW = 2048, R / 8); M = P / 2 bins, the hop H = P / 2
 *                  (50 % overlap) and L = P / 4, the range of lags.  K = min(WF_HIP_XFER_MAX_SEGMENTS = 32, 2 R / P - 3) segments,
 *                  at least 13.  They are anchored to the stream's uint32 write counter wpos as the sonogram's columns are:
 *                  E = wpos - (wpos mod H) - L, and segment a (its age, 0 the newest) of channel 0 covers the counter frames
 *                  E - a H - P .. E - a H - 1, in uint32 arithmetic that wraps with the counter, at ring positions masked by the
 *                  capacity.  The span is the frames E - (K - 1) H - P - L .. E + L - 1 of both channels, the segments with the L
 *                  frames on either side that the alignment may reach into: (K - 1) H + P + 2 L frames, and with the up to H - 1
 *                  frames behind the anchor at most R - 1, so it is in the ring wherever in a hop the counter stands.  The rules
 *                  are WF_HIP_OUT_SIGNAL's: every push issued before the read counts whatever its path, the A/V-sync delay is not
 *                  applied, the zeros of create and wf_hip_reset count as samples, hidden and paused streams are read like any
 *                  other.
 *   taper          w[i] = 0.5 - 0.5 cos(2 pi i / P), the periodic Hann window, the host-made table of WF_HIP_OUT_DELAY at this P.
 *   spectra        for segment a and a shift n, X_0,a = DFT_P(w x_0) over the segment's frames and X_1,a^(n) = DFT_P(w x_1(. - n)):
 *                  channel 1 is read n frames earlier.  The kernel is e^(-j 2 pi i k / P); on the device both come out of one
 *                  complex transform of w (x_0 + j x_1^(n)), separated as WF_HIP_OUT_STEREO does it.  Only the bins 1 <= k < M are
 *                  used.  Two properties of separate transforms are kept to the bit: a segment of a channel that is all +-0 has the
 *                  spectrum 0, and a segment whose two channels are the same bits has X_0 = X_1 (the device takes such a
 *                  segment's spectra from Z[k] alone instead of separating them).  A muted measured channel therefore reads
 *                  Syy = 0, and dual mono reads gain_db 0, phase 0 and coherence 1, exactly.  With Sxx[k] = sum_a |X_1,a^(n)[k]|^2, Syy[k] = sum_a |X_0,a[k]|^2 and
 *                  Sxy[k] = sum_a conj(X_1,a^(n)[k]) X_0,a[k], every sum over the segments oldest first:
 *   pass 1         n = 0.  G[k] = Sxy[k] (which is sum_a X_0,a conj X_1,a), g = max_k |G[k]|, and the floored PHAT weighting of
 *                  WF_HIP_OUT_DELAY, A[k] = G[k] / max(|G[k]|, b g) with b = 1e-3; r[n] = (1 / (M - 1)) sum_k Re(A[k] e^(j 2 pi k n
 *                  / P)).  n0 = the argmax of |r[n]| over -L <= n <= L: the scan runs from n = -L upwards and only a strictly
 *                  greater value wins.  lag_peak = r[n0].  Where g is 0 -- no cross power in any bin -- n0 = 0 and lag_peak = 0.
 *   pass 2         n = n0 (where n0 is 0 the sums of pass 1 are the result, bit for bit).  Hk = Sxy[k] / Sxx[k] and
 *                  coherence[k] = min(|Sxy[k]|^2 / (Sxx[k] Syy[k]), 1).
 *   fields         each float32 field is rounded once from float64.
 *                    gain_db[k]     10 log10(|Sxy[k]|^2 / Sxx[k]^2)
 *                    phase[k]       atan2(Im Hk, Re Hk): the system's phase with `lag` frames of delay taken out; a host that
 *                                   wants the raw one adds -2 pi k lag / P
 *                    coherence[k]
 *                    valid, window = P, hop = H, segments = K, lag = n0 (int32), newest = (E + L) / H = wpos / H, lag_peak,
 *                    mean_coherence = sum_k Sxx[k] coherence[k] / sum_k Sxx[k] over the live bins (0 where there is none); the
 *                    reserved words are 0.  Bin k lies at k sr / P Hz.
 *   dead bins      a bin with Sxx[k] <= WF_HIP_STEREO_DEAD_RATIO max_k Sxx is dead: the reference has nothing there, and what is
 *                  left is the transform's rounding.  It reads gain_db = 0, phase = 0, coherence = 0.  A live bin with Syy[k] == 0
 *                  reads gain_db = -INFINITY, phase = 0, coherence = 0.  Index 0 and the indices M .. WF_HIP_XFER_BINS - 1 are
 *                  written as zeros on every read.
 *   validity       valid = 0, and everything but window, hop and segments 0, when the span of either channel is all +-0 or when
 *                  the span of either channel holds a NaN or an infinity.  valid = 1 says "computed", not "reliable": reliability
 *                  is `coherence`.
 *   determinism    no atomics, and every sum and every max runs in an order that follows from P and K alone: the same ring
 *                  contents read bit-identically across push paths, repeated reads, slices and shards -- and, because of the
 *                  anchor, so do any two reads within one hop.
 * Limits: a delay beyond L is not found and biases the coherence down by about (1 - |d| / P)^2; a fractional delay stays in `phase`
 * as a linear slope; with K = 13 segments two independent channels read a coherence near 1 / K and not 0 -- the half overlap makes
 * it somewhat more: the numpy restatement reads a mean of 0.081 at K = 13 and 0.033 at K = 32 on white noise (tests/test_xfer_cpu.py).
 * The response against time is WF_HIP_OUT_IMPULSE (below); smoothing to fractional octaves and averaging across reads are the
 * host's; `newest` says when a read brings new segments.
 * Computed when read, by one kernel on the handle's stream behind the pushes issued so far (one workgroup of 256 threads per
 * stream; K float64 transforms of P points per pass, one behind the other in one LDS region, every thread keeping the running sums
 * of its own bins in registers; the lag search as one more transform of the weighted cross spectrum held in half a region beside
 * it: 48 KB at the cap, two workgroups to a CU; a second pass of K transforms only where the lag is not 0), into a block the first read allocates together
 * with its tables: a handle that never reads it allocates and launches nothing new, nothing is added to the tick, and no state is
 * kept between reads.
 * Cost on an MI355X, 4096 stereo streams at FFT 4096 read into page-locked memory (50.53 MB back): 1.88 ms with the default ring
 * (P = 1024, K = 13) where the lag is not 0 and both passes run, 1.50 ms where it is 0, against 4.71 ms for copying the 268.4 MB of
 * both rings that the segments span to the host; 4.85 and 3.28 ms with ring_frames = 65536 (P = 2048, K = 32) against 22.9 and 20.6
 * ms for its 1174.4 MB.  Into a fresh pageable numpy array (the Python reader) a read takes 5.14 and 8.42 ms, most of it the copy of
 * the 12 KB entries.  The kernel's own time without its copy is unmeasured (tools/xfer_bench.py, profiles/xfer_kernel_stats.json;
 * INTEGRATION.md, "Transfer function").
 * Spectrum and meter batches with two captured channels and W >= 256 are served; with one captured channel, with W < 256, with a
 * ring under 512 frames (W = 256 and ring_frames <= 256: P would fall under the transform's 64 points) and on waveform batches
 * wf_hip_read returns WF_HIP_ERR_INVALID and wf_hip_output_bytes 0.  A multi-device group reads it through wf_hip_multi_read. */
#define WF_HIP_XFER_MAX_WINDOW 2048
#define WF_HIP_XFER_MAX_SEGMENTS 32
#define WF_HIP_XFER_BINS 1024
typedef struct wf_hip_xfer {
    uint32_t valid;
    uint32_t window, hop;    /* P, H */
    uint32_t segments;       /* K */
    int32_t lag;             /* n0: by how many frames channel 0 is the later one, taken out of `phase` */
    uint32_t newest;         /* wpos / H: the absolute index of the newest segment's anchor */
    float lag_peak;          /* r[n0], signed */
    float mean_coherence;
    uint32_t reserved[4];    /* 0 */
    float gain_db[WF_HIP_XFER_BINS];   /* [k], 1 <= k < P / 2; 0 elsewhere */
    float phase[WF_HIP_XFER_BINS];     /* radians */
    float coherence[WF_HIP_XFER_BINS];
} wf_hip_xfer;               /* 12336 bytes, a multiple of 16 */
/* ---- impulse response (WF_HIP_OUT_IMPULSE) ----------------------------------------------------------------------------------------
 * Per stream, the fourth view of the dual-channel analyser: the response of the measured channel against the reference over *time*,
 * what such analysers show beside the transfer function as the "live IR" with its energy-time curve.  It answers what the others
 * cannot: is there an echo, how late and how loud is it, is it inverted -- a monitor bleeding into a microphone, a doubled route
 * through a mixer, a room reflection.  A host cannot make it from WF_HIP_OUT_XFER: that output's curves are float32, its dead bins
 * are forced to 0 and ring in the time domain, and at 4096 streams the host would pull 50.5 MB per read and run 4096 inverse
 * transforms.  Everything is float64 unless it says otherwise.
 *   sums           roles, P, M = H = P / 2, L = P / 4, K, the anchor E, the span, the taper, the spectra, pass 1, the lag n0 and
 *                  pass 2 are WF_HIP_OUT_XFER's (above), taken by the same code: Sxx[k], Syy[k] and Sxy[k] = sum_a conj(X_1) X_0 for
 *                  1 <= k < M are the bits that output holds, and so are valid, window, hop, segments, lag, newest, lag_peak and
 *                  mean_coherence.  The validity rule and everything a zero record carries (window, hop, segments; all else 0) are
 *                  that output's too.
 *   response       lambda = WF_HIP_IMPULSE_REG (1e-6) max_k Sxx[k]; Hr[k] = Sxy[k] / (Sxx[k] + lambda) for 1 <= k < M, the real and
 *                  the imaginary part each divided by the real sum, and Hr[0] = Hr[M] = 0.  There are no dead bins: the
 *                  regulariser takes their place smoothly, so the response does not ring.  (Where Sxx[k] + lambda is 0 -- a
 *                  reference whose only samples lie in the slack beside the segments -- Hr[k] = 0.)
 *   ir             h[n] = (1 / P) sum_{k < P} Hext[k] e^(+j 2 pi k n / P) with Hext the Hermitian extension of Hr, Hext[P - k] =
 *                  conj Hr[k]: one forward transform read at (-n) mod P, as the lag search reads its own.  ir[i] = (float) h[i - L]
 *                  for 0 <= i < P, negative n taken mod P: L frames before the arrival that was taken out and 3 L behind it.  Index i
 *                  lies lag + i - L frames behind the reference.  The indices P .. WF_HIP_IMPULSE_FRAMES - 1 read 0.
 *   envelope       the energy-time curve: a[n] = (1 / P) sum_{1 <= k < M} 2 T[k] Hr[k] e^(+j 2 pi k n / P), the analytic signal of
 *                  the response under the taper T[k] = 1 - cos(2 pi k / M) = 2 w[2 k], a Hann window across frequency with the mean
 *                  1 (without it the Hilbert part of a single tap decays only as 1 / n, and every odd index would be a local
 *                  maximum).  env[i] = |a[i - L]| and etc_db[i] = (float)(20 log10 env[i]), -INFINITY where env[i] == 0; the indices
 *                  from P up read 0.  A unit tap reads about 0 dB; the taper's side lobes lie 5 frames to either side of a tap, 31 to
 *                  33 dB under it.
 *   arrivals       the peak is the argmax of env over 0 <= i < P: the larger value, the lower index of equal ones.  Candidates are
 *                  the interior local maxima, env[i] > env[i - 1] && env[i] >= env[i + 1], 1 <= i <= P - 2.  arrivals[0] is the
 *                  peak; then, up to WF_HIP_IMPULSE_ARRIVALS = 8 in all, the strongest candidate (the lower index of equal ones)
 *                  that lies more than WF_HIP_IMPULSE_GUARD = 8 indices from every arrival taken so far and has env[i] >=
 *                  WF_HIP_IMPULSE_ARRIVAL_RATIO env[peak] (-30 dB), until there is none.  Of the arrival at index i:
 *                    frames     (float)(lag + i - L + frac): frac = 0.5 (l - r) / ((l - c) + (r - c)) with l, c, r = env[i - 1],
 *                               env[i], env[i + 1], the vertex of the parabola through them, clamped to +-0.5; 0 where the divisor
 *                               is not negative and at i == 0 and i == P - 1
 *                    level_db   (float)(20 log10(env[i] / env[peak])): the peak reads 0
 *                    polarity   +1 where Re a[i - L] >= 0, else -1
 *                  The slots not used are zeros, and so is every `reserved`.
 *   scalars        count, the number of arrivals; peak_index; peak_db = 20 log10 env[peak]; delay_ms, the peak's float64 `frames`
 *                  times 1000 / sr; energy_db = 10 log10 sum_{i < P} h[i - L]^2 and direct_db, the same sum over |i - peak_index| <=
 *                  WF_HIP_IMPULSE_DIRECT = 16 (the host subtracts the two for direct-to-rest); -INFINITY where a sum is 0.  Each
 *                  float32 field is rounded once from float64.
 *   no response    env[peak] == 0 -- a measured channel that is +-0 under every segment while the span is not silent: valid = 1,
 *                  count = 0, ir all +0, etc_db all -INFINITY up to P, and the peak fields, energy_db and direct_db 0.
 *   determinism    as WF_HIP_OUT_XFER's: no atomics, every sum and every max in an order that follows from P and K alone, so the
 *                  same ring contents read bit-identically across push paths, repeated reads, slices, shards and any two reads
 *                  within one hop.
 * Limits: an arrival d frames behind the one taken out is scaled by the overlap of the Hann segments, rho(d) = sum_n w[n] w[n + d] /
 * sum_n w[n]^2 -- -0.22 dB at P / 16, -3.62 dB at P / 4 and -3.9 dB at P / 4 + 11 frames of P = 1024 --, so later arrivals read low, and one beyond the view (more than
 * 3 L behind or L before the lag) is noise.  Around rho the estimate scatters with the K segments: over eight seeds of white noise
 * through taps of +1, -0.5 and +0.25 the numpy restatement stayed within 0.016 of the first tap in ir, 0.54 dB in level and 0.062 frames
 * in place of g rho(d) at P = 256, K = 13, and within 0.003, 0.05 dB and 0.01 frames at P = 2048, K = 32 (tests/test_impulse_cpu.py).  DC
 * and Nyquist are not part of the response.  With K = 13 and noise as strong as the signal in the measured channel, the floor's
 * maxima stand 22.9 to 26.2 dB under the peak on the restatement (29.3 to 32.4 dB with K = 32): they can pass the -30 dB rule, and mean_coherence says when they do.
 * Computed when read, by one kernel on the handle's stream behind the pushes issued so far (one workgroup of 256 threads per
 * stream: the transfer function's passes, then two more of the shared float64 transforms in the same LDS, 48 KB at the cap), into
 * a block the first read allocates together with its tables: a handle that never reads it allocates and launches nothing new,
 * nothing is added to the tick, and no state is kept between reads.
 * Cost on an MI355X, 4096 stereo streams at FFT 4096 read into page-locked memory (67.9 MB back): 2.39 ms with the default ring
 * (P = 1024, K = 13) where the lag is not 0 and both passes run, 1.95 ms where it is 0, against 4.71 ms for copying the 268.4 MB of
 * both rings that the segments span to the host; 5.43 and 3.79 ms with ring_frames = 65536 (P = 2048, K = 32) against 20.6 ms for
 * its 1174.4 MB.  Into a fresh pageable numpy array (the Python reader) a read takes 7.52 and 10.35 ms, most of it the copy of the
 * 16 KB entries.
 * The kernel's own time without its copy is unmeasured (tools/impulse_bench.py, profiles/impulse_kernel_stats.json; INTEGRATION.md,
 * "Impulse response").
 * The refusals are WF_HIP_OUT_XFER's: with one captured channel, with W < 256, with a ring under 512 frames and on waveform batches
 * wf_hip_read returns WF_HIP_ERR_INVALID and wf_hip_output_bytes 0.  A multi-device group reads it through wf_hip_multi_read. */
#define WF_HIP_IMPULSE_FRAMES 2048
#define WF_HIP_IMPULSE_ARRIVALS 8
#define WF_HIP_IMPULSE_GUARD 8
#define WF_HIP_IMPULSE_DIRECT 16
#define WF_HIP_IMPULSE_REG 1e-6
#define WF_HIP_IMPULSE_ARRIVAL_RATIO 0.031622776601683794 /* 10^(-30 / 20) */
typedef struct wf_hip_impulse_arrival {
    float frames;            /* behind the reference; lag + i - L + frac */
    float level_db;          /* against the peak: 0 for arrivals[0] */
    int32_t polarity;        /* +1 or -1 */
    uint32_t reserved;       /* 0 */
} wf_hip_impulse_arrival;
typedef struct wf_hip_impulse {
    uint32_t valid;
    uint32_t window, hop;    /* P, H */
    uint32_t segments;       /* K */
    int32_t lag;             /* n0, as wf_hip_xfer's */
    uint32_t newest;         /* wpos / H */
    float lag_peak;
    float mean_coherence;
    uint32_t count;          /* arrivals listed */
    uint32_t peak_index;     /* into ir and etc_db */
    float peak_db;           /* 20 log10 env[peak] */
    float delay_ms;          /* arrivals[0].frames in milliseconds */
    float energy_db;         /* 10 log10 sum h^2 */
    float direct_db;         /* the same within WF_HIP_IMPULSE_DIRECT indices of the peak */
    uint32_t reserved[2];    /* 0 */
    wf_hip_impulse_arrival arrivals[WF_HIP_IMPULSE_ARRIVALS]; /* the peak, then by falling level */
    float ir[WF_HIP_IMPULSE_FRAMES];     /* [i], 0 <= i < P: h[i - L]; 0 elsewhere */
    float etc_db[WF_HIP_IMPULSE_FRAMES]; /* [i], 0 <= i < P: 20 log10 |a[i - L]|; 0 elsewhere */
} wf_hip_impulse;            /* 16576 bytes, a multiple of 16 */
/* ---- clicks (WF_HIP_OUT_CLICK) -----------------------------------------------------------------------------------------------------
 * Per stream and captured channel, the click detector of a QC monitor: the clicks of an interface that drops buffers, the splice
 * where a block was skipped or repeated, the pop of a bad cable.  The programme is predictable from its own recent past and a click
 * is not: a linear predictor is fitted to the window, and the frames whose residual stands far above the residual's own robust level
 * are the clicks.  Let W = wf_hip_fft_size() and sr = cfg.sample_rate.  Everything is float64 unless it says otherwise, and every
 * product and every sum is rounded on its own (no fused multiply-add, except where it is named).
 *   window         P = min(W, WF_HIP_CLICK_MAX_WINDOW) frames: the newest P frames of the channel's ring.  WF_HIP_OUT_SIGNAL's rules:
 *                  every push issued before the read counts, the A/V-sync delay is not applied, the zeros of create and reset count,
 *                  hidden and paused streams are read like any other.  x[n], 0 <= n < P, is the float32 sample widened exactly;
 *                  A = the largest |x[n]|.
 *   predictor      of order p = WF_HIP_CLICK_ORDER = 16.  r[k] = sum_{n=k}^{P-1} x[n] x[n-k] for k = 0 .. p, the biased
 *                  autocorrelation, which keeps Levinson stable.  The order of the sum is fixed: partial t, 0 <= t < 256, is the
 *                  fused sum over n = t, t + 256, ... in ascending n (a product of two float32 values is exact in float64: the fused
 *                  sum is the plain one); then, within each 64 consecutive partials, six rounds v[t] += v[t ^ 32], ^ 16, ^ 8, ^ 4,
 *                  ^ 2, ^ 1; then ((s_0 + s_1) + s_2) + s_3 of the four groups.  The same frames therefore give the same bits, and
 *                  a host that restates the order reproduces them (tests/click_ref.py does).  Levinson-Durbin on r'[0] = r[0] (1 +
 *                  1e-9), r'[k] = r[k]: E = r'[0]; for i = 1 .. p: acc = r[i], acc = acc - a[j] r[i-j] for j = 1 .. i-1 ascending,
 *                  k = acc / E, a'[j] = a[j] - k a[i-j] for j < i, a'[i] = k, E = E (1 - k k).  It gives a[1..p] and the error power
 *                  E.  e[n] = x[n] - acc for p <= n < P, acc = 0, acc = acc + a[k] x[n-k] for k = 1 .. p ascending; the frames n < p
 *                  are not judged.  d[n] = (float) |e[n]|.
 *   scale          blocks of B = 256 judged frames: nb = max(1, (P - p) / B); block b covers [p + b B, p + (b+1) B), the last one
 *                  runs to P (up to 511 frames).  m_b = the element of rank len_b / 2 (0-based, ascending) of the block's d;
 *                  g = the element of rank (P - p) / 2 of all judged d: exact order statistics of float32 values.
 *                  s_b = 1.4826 max(m_{b-1}, m_b, m_{b+1}, 0.25 g, 2^-24 A) over the neighbours that exist.  The neighbours keep a
 *                  signal that starts inside the window from reading as clicks; the last term lets a lone click in digital silence
 *                  read as one (141 dB) instead of 0 / 0.  A window of one block (nb = 1: P - p < 512) has no neighbours, and half
 *                  the medians of its two halves stand in for them: h = p + (P - p) / 2, m_lo and m_hi the elements of rank len / 2
 *                  of d over [p, h) and [h, P), s_0 = 1.4826 max(m_0, 0.5 m_lo, 0.5 m_hi, 0.25 g, 2^-24 A).  Without them zeros
 *                  followed by noise at P = 256 read 1 to 3 events on 18 of 24 seeds of the restatement; with them none does, and a
 *                  block of one kind reads the same bits as without, half a half's median lying under the block's own.
 *   hits           frame n of block b is a hit when d[n] / s_b > WF_HIP_CLICK_THRESHOLD = 16 (24.1 dB).  A Laplacian residual exceeds
 *                  it with probability exp(-1.028 * 16) = 7e-8 per frame, 6e-4 per window.
 *   events         hits whose gaps are at most WF_HIP_CLICK_GAP = 32 frames form one event: start (its first hit), length (last
 *                  hit - first + 1), peak (the hit of the largest ratio, the lower index of equal ones), strength_db = 20 log10 of
 *                  that ratio, amplitude = (float) e[peak], signed.
 *   list           the up to WF_HIP_CLICK_MAX_EVENTS = 8 strongest events, strength_db (the float32) descending, then start
 *                  ascending; the slots behind them are zero bytes.
 *   validity       valid = 0 when r[0] == 0 or the window holds a NaN or an infinity; every other field of that channel is then 0
 *                  and peak_db, floor_db and prediction_gain_db are -INFINITY.
 * Limits.  Hard clipping reads as long events: the flat tops are unpredictable, and WF_HIP_OUT_SIGNAL's clip count says why.  A
 * source that is an impulse train through a resonator with no noise under it (a synthetic voice) reads its own pulses.  A window of
 * 800 frames or fewer leaves a pure sine too much residual for a 0.01 click on a 0.5 sine to be found; at 4096 and 8192 it reads 36
 * and 43 dB.  A signal that starts in the last quarter of a window of one block, or in the last 128 frames of a longer one, has no later
 * block or half to lean on and reads as events until the next read.  The constants were chosen on synthetic noise, tones, notes and splices, not on recorded programme.  The host can raise
 * the threshold on strength_db; it cannot lower it.
 * Computed when read, by one kernel on the handle's stream behind the pushes issued so far (one workgroup of 256 threads per stream
 * and captured channel, the window and the residual in LDS, about 73 KB at the cap), into a block the first read allocates: a handle
 * that never reads it allocates and launches nothing new, nothing is added to the tick, and no state is kept between reads (a host
 * that polls tells an event it has seen by `frame`).
 * Cost on an MI355X, 4096 stereo streams read into page-locked memory (1.9 MB back): 980 us on noise, 1002 us on a sine with a click
 * and 272 us on silence at FFT 4096, against 2361 us for copying the windows to the host; 2277, 2307 and 597 us at FFT 16384 (P =
 * 8192) against 4890 us.  The kernel's own time without its copy is unmeasured (tools/click_bench.py,
 * profiles/click_kernel_stats.json; INTEGRATION.md, "Clicks").
 * On waveform batches and with W < 256 wf_hip_read returns WF_HIP_ERR_INVALID and wf_hip_output_bytes 0.  A multi-device group reads
 * it through wf_hip_multi_read; the pipelined readback (wf_hip_read_async) carries the tick's outputs only. */
#define WF_HIP_CLICK_MAX_WINDOW 8192
#define WF_HIP_CLICK_ORDER 16
#define WF_HIP_CLICK_GAP 32
#define WF_HIP_CLICK_MAX_EVENTS 8
#define WF_HIP_CLICK_THRESHOLD 16.0
typedef struct wf_hip_click_event {
    uint32_t start, length, peak;   /* indices into the window */
    uint32_t frame;                 /* counter position of `start`: wpos - P + start (mod 2^32), as WF_HIP_OUT_ONSET's last_frame */
    float strength_db, amplitude;
} wf_hip_click_event;               /* 24 bytes */
typedef struct wf_hip_click_channel {
    uint32_t valid, events, hit_frames, listed;   /* events in the window; frames that are hits; min(events, 8) */
    float rate;              /* events * sr / (P - p): clicks per second */
    float peak_db;           /* 20 log10 of the largest d[n] / s_b over all judged frames, hit or not: the "crackle meter" */
    float floor_db;          /* 20 log10(1.4826 g): the residual's robust level, dBFS */
    float prediction_gain_db;/* 10 log10(r[0] / E) */
    wf_hip_click_event ev[WF_HIP_CLICK_MAX_EVENTS];
} wf_hip_click_channel;      /* 224 bytes */
typedef struct wf_hip_click {
    wf_hip_click_channel ch[2];   /* captured channels 0 and 1; with one captured channel ch[1] is all zero bytes */
    uint32_t window, order, reserved[2];   /* P, p, 0 */
} wf_hip_click;              /* 464 bytes, a multiple of 16 */
/* ---- intermodulation (WF_HIP_OUT_IMD) ---------------------------------------------------------------------------------------------
 * Per stream and captured channel, the measurement that stands beside THD on an audio analyser: intermodulation distortion from a
 * two-tone stimulus.  WF_HIP_OUT_THD cannot stand in for it: at 48 kHz a tone above 8 kHz has every harmonic from the third up
 * beyond Nyquist, so the top octave and a half of a codec, a resampler, an interface or a limiter is measured on one harmonic or on
 * none, while a twin tone at 19 + 20 kHz puts its products at 1, 18 and 21 kHz, in band; and a low tone with a high one shows the
 * modulation a limiter or a class-D stage adds (the DIN / SMPTE method).  No host can make it from the tick's rows: they are
 * float32 behind a Hann-class window, with a leakage floor far above a product at -100 dB.  W = wf_hip_fft_size(),
 * sr = cfg.sample_rate; everything is float64 unless it says otherwise.
 *   window, taper, spectrum   exactly WF_HIP_OUT_THD's: P the largest power of two <= min(W, WF_HIP_THD_MAX_WINDOW = 8192), the newest
 *                  P frames with the rules of WF_HIP_OUT_SIGNAL, the periodic 7-term Blackman-Harris taper, H = WF_HIP_THD_LOBE = 8,
 *                  M = P / 2, p[k] = |X_c[k]|^2 for 1 <= k < M, S = P sum w^2 / 4.  With two captured channels both come out of
 *                  one complex transform; a channel of all zeros has p = 0 exactly; a NaN or an infinity in either window makes
 *                  both channels read valid = 0; with one captured channel ch[1] is all zero bytes.
 *   tones          k_a = the argmax of p over k in [2H + 1, M - H - 1]: the search starts from best = 0 and only a strictly
 *                  greater value wins, so the lowest index wins a tie and a NaN never wins.  F_a = the sum of p[k] over
 *                  |k - k_a| <= H and f_a = (sum k p[k]) / F_a over the same bins.  If F_a is not a finite number > 0: tones = 0,
 *                  valid = 0 and every other field of the channel is 0.  k_b = the same argmax over the bins with
 *                  |k - k_a| > 2H, so the two regions share no bin, and F_b, f_b from it.  If no such bin has p > 0, or F_b is
 *                  not finite, or F_b < WF_HIP_IMD_MIN_RATIO F_a (1e-3: 30 dB): tones = 1, valid = 0 and every other field is 0.
 *                  Otherwise tones = 2 and valid = 1.  lo is the tone of the lower f and hi the other; T = F_lo + F_hi.
 *   products       q = 0 .. 19 (WF_HIP_IMD_PRODUCTS = 20) enumerates the orders o = 2 .. 5, within an order m = 1 .. o - 1 (the
 *                  multiple of f_hi) with n = o - m, and for each (m, n) first |m f_hi - n f_lo|, then m f_hi + n f_lo:
 *                  q0 = f_hi - f_lo, q1 = f_hi + f_lo, q2 = |f_hi - 2 f_lo|, q3 = f_hi + 2 f_lo, q4 = 2 f_hi - f_lo,
 *                  q5 = 2 f_hi + f_lo, q6 = |f_hi - 3 f_lo| ... q18 = 4 f_hi - f_lo, q19 = 4 f_hi + f_lo.  k_q = floor(f + 0.5).
 *                  Product q is clear iff k_q >= 2H + 1, k_q + H <= M - 1, |k_q - k_lo| > 2H and |k_q - k_hi| > 2H; then
 *                  R_q = the sum of p[k] over |k - k_q| <= H and bit q of `products` is set.  Products beyond the band are not
 *                  folded back.
 *   harmonics      for h = 2 .. 5 of each tone k = floor(h f + 0.5); the harmonic is in band iff k + H <= M - 1.  Their regions
 *                  are only kept out of the noise estimate.
 *   residue        one pass over H < k < M outside both tones' regions.  D sums every such bin.  A bin in the region of any clear
 *                  product goes to I, once however many regions hold it; otherwise a bin in an in-band harmonic's region goes
 *                  nowhere else; otherwise it goes to N, and n counts it.  N_s = N (M - 5H - 3) / n, or 0 when n = 0.
 *   levels         dB(x, y) is WF_HIP_OUT_THD's.  Each float32 field is rounded once from float64.
 *                    lo_hz, hi_hz (double)   f sr / P           lo_db, hi_db     dB(F, S): a sine of amplitude A reads 20 log10 A
 *                    ratio_db                dB(F_hi, F_lo)
 *                    product_db[q]           dB(R_q, T); -INFINITY when product q is not clear
 *                    order_db[o - 2]         dB(the sum of the clear R_q of order o, q ascending, T); -INFINITY when none is clear
 *                    imd_db                  dB(I, T); -INFINITY when no product is clear
 *                    dfd2_db                 20 log10(sqrt R_0 / (sqrt F_lo + sqrt F_hi)), the difference-frequency distortion of
 *                                            IEC 60268-3, second order; -INFINITY when q0 is not clear
 *                    dfd3_db                 the same with sqrt R_2 + sqrt R_4 over the clear ones; -INFINITY when neither is clear
 *                    mod_db                  dB(the sum of the clear R_q of q in {0, 1, 2, 3, 6, 7, 12, 13}, F_hi): the modulation
 *                                            distortion of the DIN / SMPTE method, the sidebands f_hi +- n f_lo for n = 1 .. 4
 *                                            against the upper tone
 *                    tdn_db                  dB(D, T)           noise_db         dB(N_s, 2S): white noise of variance s^2 reads
 *                                                                                10 log10 s^2
 *                    lo_bin k_lo, hi_bin k_hi, products, tones, valid (uint32)
 *                  Nothing reads NaN while valid is 1.
 *   determinism    the order of every sum follows from P, the two bins and the k_q alone and there are no atomics: the same ring
 *                  contents read bit-identically across push paths, repeated reads, slices and shards.
 * What follows from the definition.  A tone must lie at least 17 bins up: about 100 Hz at P = 8192 and 48 kHz, so SMPTE's 60 Hz is
 * out of reach at 48 kHz and DIN's 250 Hz + 8 kHz is not.  With one tone and a loud harmonic (above -30 dBc), the harmonic is taken
 * for the second tone.  Two tones an exact octave apart have q0 on the lower tone, not clear.
 * Computed when read, by one kernel on the handle's stream behind the pushes issued so far (one workgroup of 512 threads per stream,
 * the distortion analyser's transform of P points in up to 128 KB of LDS), into a block the first read allocates; the tables are
 * WF_HIP_OUT_THD's, built by whichever of the two outputs is read first.  A handle that never reads it allocates and launches
 * nothing new, nothing is added to the tick, and no state is kept between reads.
 * Cost on an MI355X, 4096 stereo streams, read into page-locked memory (1.5 MB back): 0.35 ms at W = 4096 against 0.29 ms for a
 * WF_HIP_OUT_THD read in the same process and 2.36 ms for copying the 134.2 MB of windows to the host, and 0.71 ms against 0.63 and
 * 4.71 ms at W = 16384 (P = 8192): 1.23 and 1.14 times the THD read's time, which it loses to, and 6.7 and 6.6 times faster than
 * the copy.  Into a fresh pageable numpy array (the Python reader) a read takes 0.36 and 0.72 ms.  The kernel's own time without its
 * copy is unmeasured (tools/imd_bench.py, profiles/imd_kernel_stats.json; INTEGRATION.md, "Intermodulation").
 * Spectrum and meter batches with one or two captured channels and W >= 512 are served; on waveform batches and below 512 frames
 * wf_hip_read returns WF_HIP_ERR_INVALID and wf_hip_output_bytes 0.  A multi-device group reads it through wf_hip_multi_read. */
#define WF_HIP_IMD_PRODUCTS 20
#define WF_HIP_IMD_MIN_RATIO 1e-3
typedef struct wf_hip_imd_channel {
    double lo_hz, hi_hz;
    float lo_db, hi_db, ratio_db, imd_db;
    float order_db[4];       /* [o - 2] */
    float dfd2_db, dfd3_db, mod_db, tdn_db, noise_db;
    float product_db[WF_HIP_IMD_PRODUCTS]; /* [q], against T */
    uint32_t lo_bin, hi_bin;
    uint32_t products;       /* bit q: product q is clear */
    uint32_t tones;          /* 0, 1 or 2 tones found */
    uint32_t valid;
    uint32_t reserved[2];    /* 0 */
} wf_hip_imd_channel;        /* 176 bytes */
typedef struct wf_hip_imd {
    wf_hip_imd_channel ch[2]; /* captured channels 0 and 1; with one captured channel ch[1] is all zero bytes */
    uint32_t window;         /* P */
    uint32_t reserved[3];    /* 0 */
} wf_hip_imd;                /* 368 bytes, a multiple of 16 */
/* ---- tempo (WF_HIP_OUT_TEMPO) ------------------------------------------------------------------------------------------------
 * Per stream, how fast the beat is and where it falls: the onset strength of WF_HIP_OUT_ONSET over seconds instead of 0.68 s, the
 * periodicity of that curve, and the beat phase on the sample counter, so that a host can schedule the next beat instead of
 * learning about the last.  sr = cfg.sample_rate; every sum is float64 in the order stated, on the float32 strengths.
 *   columns        WF_HIP_OUT_ONSET's, bit for bit: P = WF_HIP_TEMPO_WINDOW = 1024, H = WF_HIP_TEMPO_HOP = 256, the same window,
 *                  transform, bands, level S and strength (low + mid) + high rounded to float32 once; only the total is used.
 *                  T = min(WF_HIP_TEMPO_COLUMNS, (ring_cap - P) / H - 1) strength columns: 507 for a ring of 131072 frames, 1019
 *                  for 2^18, 2043 for 2^19, 2048 from 2^20 up (wf_hip_create's ring_frames).  strength[age], age 0 the newest,
 *                  column newest - age with newest = wpos / H; ages >= T read 0.  Where WF_HIP_OUT_ONSET exists, strength[0 .. 127]
 *                  is what it returns from the same handle at the same moment.  Below, o[n] is the curve oldest first,
 *                  o[n] = strength[T - 1 - n].
 *   lags           lag_lo = ceil(60 sr / (240 H)), lag_hi = min(floor(60 sr / (40 H)), T / 4, WF_HIP_TEMPO_MAX_LAG = 287) columns:
 *                  240 down to 40 BPM where the ring and the rate allow it (47 .. 126 at 48 kHz with T = 507, which cannot read
 *                  60 BPM; 47 .. 254 with T = 1019; 47 .. 281 from T = 2043 on).  Both are returned.
 *   mean           mean = (o[0] + o[1] + ... + o[T - 1]) / T, added oldest first; e[n] = (double)o[n] - mean.
 *   acf            r[L] = (sum over n = L .. T - 1 ascending of e[n] e[n - L]) / (T - L) for L = 0 .. 2 lag_hi + 1, each product
 *                  rounded before it is added; acf[L] = r[L] / r[0], returned as float32, 0 from 2 lag_hi + 2 on.
 *   salience       c[L] = (acf[L] + 0.5 acf[2 L]) w[L] for lag_lo <= L <= lag_hi, with w[L] = exp(-0.5 log2(bpm(L) / 120)^2) and
 *                  bpm(L) = 60 sr / (H L): a preference of one octave's width around 120 BPM, which settles the octave question
 *                  by a stated rule (w is a float64 table made by the host).
 *   best           lag = the L with the largest c, the lowest on ties.  For lag_lo < lag < lag_hi the parabola through
 *                  a = c[lag - 1], b = c[lag], g = c[lag + 1]: p = 0.5 (a - g) / (a - 2 b + g) when that denominator is
 *                  negative, else 0; at either end of the range p = 0.  period = rint(16 (lag + p)) / 16 columns,
 *                  bpm = 60 sr / (H (lag + p)), period_frames = period H (a whole number of frames), confidence = acf[lag],
 *                  salience = c[lag].
 *   second         among the L with lag_lo < L < lag_hi, c[L] > c[L - 1], c[L] >= c[L + 1] and |L - lag| > max(2, lag / 16)
 *                  (integer division) the one with the largest c, the lowest on ties: lag2, bpm2 = 60 sr / (H lag2),
 *                  salience2 = c[lag2], ambiguity = salience2 / salience (0 unless salience > 0); all 0 if there is none.  A
 *                  bare pulse train is as much 87 as 174 BPM: this is where the entry says so.
 *   phase          phi[k] = sum over j = 0, 1, ... of e[T - 1 - k - rint(j period)] while that index is >= 0, ascending j, for
 *                  k = 0 .. ceil(period) - 1 (j period is exact in float64; rint rounds ties to even).  beat_age = the k with the
 *                  largest phi, the lowest on ties; last_beat_frame = (newest - beat_age) H - 3 P / 8, WF_HIP_OUT_ONSET's
 *                  convention for where an event starts (uint32, wraps with the counter); next_beat_frame = last_beat_frame +
 *                  period_frames.
 *   validity       valid = 1 if and only if every strength is finite, r[0] > 0 and the largest strength is at least
 *                  WF_HIP_TEMPO_MARGIN = 2.0, the onset rule's margin: a curve that stays below it holds no onset by this
 *                  library's own definition (a steady sine peaks at 0.007, noise at -60 dBFS at 0.06, noise at -20 dBFS at 3.3
 *                  and reads valid with a confidence below 0.2).  With valid = 0 acf and every field but strength, columns,
 *                  newest, lag_lo, lag_hi, window and hop are 0.  strength_max and strength_mean are the largest strength and
 *                  `mean`.
 *   determinism    no atomics, and every sum runs in a fixed order: the same frames read bit-identically across reads, push paths,
 *                  slices and shards.
 * What it reads on synthetic pulse trains (tests/tempo_ref.py, 48 kHz; 60 Hz kicks and 50 ms noise bursts over noise at -40 dBFS):
 * 90, 120, 128 and 150 BPM at T = 507 and 60, 72.5, 90, 120, 128 and 150 BPM at T = 1019 and 2043 within 0.13 % (119.84 for 120)
 * with a confidence of 0.80 or more and last_beat_frame within 432 frames of a true beat.  Not recovered: 174 BPM reads 87 from
 * T = 1019 on (bpm2 reads 173); 200 BPM bursts read 100 (bpm2 201); 60 BPM at T = 507 reads 120.  The prior and the onset constants
 * were chosen on synthetic signals and have not been tuned on recorded music.  Nothing is kept between reads: smoothing the tempo
 * over time, time signatures and downbeats are the host's.
 * Computed when read, by two kernels on the handle's stream behind the pushes issued so far -- the columns spread over the grid
 * in chunks of 64 (256 threads, one wavefront per spectral column, float64 transforms in LDS) into a scratch block of 8 KB per
 * stream, then one workgroup per stream for the rule -- into blocks the first read allocates together with its tables.  Cost on an
 * MI355X: unmeasured (tools/tempo_bench.py).
 * Spectrum and meter batches with one or two captured channels and any FFT size are served; on waveform batches, on handles
 * whose ring holds fewer than WF_HIP_TEMPO_MIN_RING = 131072 frames and at sample rates for which lag_hi < lag_lo + 2 wf_hip_read
 * returns WF_HIP_ERR_INVALID and wf_hip_output_bytes 0.  A multi-device group reads it through wf_hip_multi_read. */
#define WF_HIP_TEMPO_WINDOW 1024
#define WF_HIP_TEMPO_HOP 256
#define WF_HIP_TEMPO_COLUMNS 2048
#define WF_HIP_TEMPO_LAGS 576
#define WF_HIP_TEMPO_MAX_LAG 287
#define WF_HIP_TEMPO_MIN_RING 131072
#define WF_HIP_TEMPO_MARGIN 2.0
typedef struct wf_hip_tempo {
    float strength[WF_HIP_TEMPO_COLUMNS]; /* [age] */
    float acf[WF_HIP_TEMPO_LAGS];         /* [L] */
    float bpm, period;       /* of the best lag: beats per minute, and columns in sixteenths */
    float confidence;        /* acf[lag] */
    float salience;          /* c[lag] */
    float bpm2, salience2;   /* of the second candidate */
    float ambiguity;         /* salience2 / salience */
    float strength_max, strength_mean;
    uint32_t valid;
    uint32_t columns;        /* T */
    uint32_t newest;         /* wpos / H: the absolute index of the column of age 0 */
    uint32_t lag_lo, lag_hi;
    uint32_t lag, lag2;
    uint32_t beat_age;       /* the age of the column the newest beat falls into */
    uint32_t period_frames;  /* period H */
    uint32_t last_beat_frame, next_beat_frame; /* on the sample counter, uint32 */
    uint32_t window, hop;    /* P, H */
    uint32_t reserved[2];    /* 0 */
} wf_hip_tempo;              /* 10592 bytes, a multiple of 16 */
/* ---- mains hum (WF_HIP_OUT_HUM) ----------------------------------------------------------------------------------------------
 * Per captured channel, "is it humming": whether a line at 50 or 60 Hz and its harmonics stand above the programme -- a ground
 * loop, a bad DI box, a dimmer beside a cable -- which family it is, the mains frequency, and how strong the hum is against the
 * total.  sr = cfg.sample_rate; everything is float64; every sum runs in ascending harmonic order.
 *   plan           D = the largest power of two with 1280 D <= sr (the decimation), N = min(ring_cap, WF_HIP_HUM_MAX_WINDOW,
 *                  1024 D) the newest frames read, M = N / D (512 or 1024), hz = sr / N, K = ceil(8 * 60.5 / hz) + 22 bins.  48 kHz:
 *                  N = 16384 and 2.93 Hz with a ring of 16384 frames, 32768 and 1.46 Hz from a ring of 32768 on.  fft_size plays
 *                  no part.
 *   spectrum       with x the newest N frames of the channel, float32 taken to float64, X[k] for k = -1 .. K is the N-point
 *                  transform of x, formed exactly from D / 2 complex M-point transforms of the branches x[r], x[r + D], ... in
 *                  pairs; H[k] = (0.5 X[k] - 0.25 (X[k - 1] + X[k + 1])) 4 / N for k = 0 .. K - 1, the transform of x through
 *                  the periodic Hann window: a sine of amplitude A at a bin centre reads |H| = A.  p[k] = |H[k]|^2.
 *   lines          for each family fam = 50, 60 and harmonic h = 1 .. WF_HIP_HUM_HARMONICS = 8:
 *                  1. the bins lo = max(ceil(h (fam - 0.5) / hz - 0.5), 6) .. hi = floor(h (fam + 0.5) / hz + 0.5), in exact
 *                     integer arithmetic; k = the bin of the largest |H| in it, the lowest on ties; none if hi < lo.
 *                  2. it must be a local maximum: |H[k]| > |H[k - 1]| and |H[k]| >= |H[k + 1]|.
 *                  3. alpha = the larger neighbour / |H[k]|, d = (2 alpha - 1) / (alpha + 1) held to [0, 0.5];
 *                     amp = |H[k]| (1 - d^2) pi d / sin(pi d) (amp = |H[k]| at d = 0); f = (k + d) hz / h, k - d where the lower
 *                     neighbour is the larger.
 *                  4. |f - fam| <= WF_HIP_HUM_TOL_HZ = 0.5, else it is not mains (no equal-tempered note at A = 440 Hz falls
 *                     inside either range: G1 = 49.0, G#1 = 51.9, A#1 = 58.3, B1 = 61.7 Hz).
 *                  5. the local floor: the powers p of the bins [max(2, k - 20), max(2, k - 3)) and [k + 4, k + 21)
 *                     (WF_HIP_HUM_FLOOR_SPAN = 20, WF_HIP_HUM_FLOOR_GUARD = 3), n of them, sorted; the one of rank n / 2 (integer
 *                     division), divided by ln 2, which turns the median of an exponential distribution into its mean; at least
 *                     1e-300.
 *                  6. snr_db = 10 log10(amp^2 / floor); the line qualifies at snr_db >= WF_HIP_HUM_MARGIN_DB = 15.0.
 *   family         per family: f0 = the mean of the qualified f weighted by (h amp)^2; lines with |f - f0| h > hz are dropped;
 *                  hum = the sum of amp^2 / 2 over the rest.  The family with the larger hum wins, 50 on a tie; with no line in
 *                  either, family = 0 and mains_hz, hum_db, ratio_db, odd_db, even_db, lines, mask and the three arrays are 0.
 *                  A lone line at 300 Hz is the 6th harmonic of 50 and the 5th of 60 Hz alike: it reads 50, by the tie rule.
 *   fields         mains_hz = the winner's f0; lines and mask (bit h - 1) its remaining harmonics; hz[h - 1] = f,
 *                  level_db[h - 1] = 10 log10(amp^2) (dB re full scale, a sine of amplitude 1 reads 0), snr_db[h - 1], 0 where
 *                  the mask bit is clear; hum_db = 10 log10(hum); total_db = 10 log10 of the mean square of the N frames (each
 *                  thread of 256 adds the squares of frames t, t + 256, ... ascending, the 64 lanes of a wavefront combine at
 *                  distances 32, 16 .. 1, the four wavefronts are added in ascending order); ratio_db = hum_db - total_db;
 *                  odd_db and even_db = 10 log10 of the sums of amp^2 / 2 over the remaining harmonics 3, 5, 7 and 2, 4, 6, 8
 *                  (0 where there is none): a rectifier's buzz and a transformer's hum read differently; noise_db = the rule of
 *                  step 5 over the bins ceil(20 / hz) .. floor(8 * 60.5 / hz) outside +-3 bins of every remaining line, in
 *                  level_db's scale: with nothing found, a line would have had to reach about noise_db + 15 to be seen.
 *   validity       valid = 0 and every other field of the channel 0 for a window of zeros and for one that holds a NaN or an
 *                  infinity.  A channel the batch does not capture reads zeros.
 *   determinism    no atomics, and every sum runs in a fixed order: the same frames read bit-identically across reads, push
 *                  paths, slices and shards.
 * What it sees is hum that stands above the programme's density in its bin: in pauses, under speech, on idle lines.  On the numpy
 * restatement (tests/hum_ref.py) lines at -40 / -46 / -43 / -52 dBFS on harmonics 1, 2, 3, 5 of 50 or 60 +- 0.2 Hz under white
 * noise at -40 dBFS are found in every one of 30 seeds per plan, exactly those four, mains_hz within 0.027 Hz at N = 16384 and
 * 0.011 Hz at N = 32768 / 48 kHz, levels within 1.43 dB; noise alone finds nothing in 200 seeds per plan.  White noise at -30 dBFS
 * hides a -50 dBFS hum at N = 16384, and bass-heavy music hides more: no detection is promised under it.
 * Computed when read, by one workgroup of 256 threads per stream and captured channel on the handle's stream behind the pushes
 * issued so far: the window staged branch-major in LDS (128 KB at N = 32768), D / 2 transforms in a 16 KB region, the lines on
 * sixteen lanes, the medians by exact selection.  Cost on an MI355X at 4096 stereo streams and 48 kHz, the copy to the host included:
 * 2.27 ms per read with a ring of 16384 frames, 6.05 ms with 32768 (tools/hum_bench.py).
 * Spectrum and meter batches with one or two captured channels and any FFT size are served; on waveform batches, on handles whose
 * ring holds fewer than sample_rate / 3 frames (the default ring at 48 kHz: 5.9 Hz bins), and at sample rates under 2560 Hz or so
 * high that no ring serves (above 3 * 32768 Hz) wf_hip_read returns WF_HIP_ERR_INVALID and wf_hip_output_bytes 0.  A multi-device
 * group reads it through wf_hip_multi_read. */
#define WF_HIP_HUM_HARMONICS 8
#define WF_HIP_HUM_MARGIN_DB 15.0
#define WF_HIP_HUM_TOL_HZ 0.5
#define WF_HIP_HUM_FLOOR_SPAN 20
#define WF_HIP_HUM_FLOOR_GUARD 3
#define WF_HIP_HUM_MAX_WINDOW 32768
typedef struct wf_hip_hum_channel {
    float mains_hz;          /* f0 of the winning family */
    float hum_db;            /* 10 log10 of the sum of amp^2 / 2 over its lines */
    float total_db;          /* 10 log10 of the mean square of the N frames */
    float ratio_db;          /* hum_db - total_db */
    float odd_db, even_db;   /* over harmonics 3, 5, 7 and 2, 4, 6, 8 */
    float noise_db;          /* the floor between the lines, in level_db's scale */
    uint32_t valid;
    uint32_t family;         /* 0, 50 or 60 */
    uint32_t lines;          /* how many bits mask has */
    uint32_t mask;           /* bit h - 1: harmonic h qualified */
    float hz[WF_HIP_HUM_HARMONICS];       /* the line's frequency over h */
    float level_db[WF_HIP_HUM_HARMONICS]; /* 10 log10(amp^2) */
    float snr_db[WF_HIP_HUM_HARMONICS];   /* over the local floor */
    uint32_t reserved;       /* 0 */
} wf_hip_hum_channel;        /* 144 bytes */
typedef struct wf_hip_hum {
    wf_hip_hum_channel ch[2];
    uint32_t window;         /* N */
    uint32_t decimation;     /* D */
    float resolution_hz;     /* sr / N */
    uint32_t reserved;       /* 0 */
} wf_hip_hum;                /* 304 bytes, a multiple of 16 */
/* bytes per stream of an output of this batch (0: the batch has no such output) */
size_t wf_hip_output_bytes(const wf_hip *h, wf_hip_output what);
/* `what` of streams [first, first+count) as the ticks issued so far leave it, into `out` ([count] x the shape above); waits for
 * those ticks.  WF_HIP_ERR_INVALID when the batch has no such output (wf_hip_last_error says why). */
int wf_hip_read(wf_hip *h, wf_hip_output what, uint32_t first, uint32_t count, void *out);
/* m_tsmooth_buf written back (state restore; layout of WF_HIP_OUT_TSMOOTH) */
int wf_hip_write_tsmooth(wf_hip *h, uint32_t first, uint32_t count, const float *in);
/* Pipelined readback: what the ticks issued so far leave for streams [first, first+count) is copied into page-locked memory
 * (wf_hip_host_alloc) on the handle's readback stream, without waiting; the following ticks run meanwhile.  `slot` (0 or 1) names
 * the copy for wf_hip_readback_done, which blocks until everything of it has landed.  Every destination is [count] x the shape
 * of the output of that name; a NULL pointer leaves that output out.  Three combinations:
 *  - rows (+ last_silent, both required) and any of bars / premirror / vertices / vertex_counts / input_rms behind them: the
 *    plugin binding's frame (its render() override draws from them one frame later).  The copies read the handle's own
 *    buffers: the next wf_hip_tick waits (on the device, not the host) for a copy still in flight before it overwrites them.
 *  - bars alone: the device keeps one snapshot per slot (a device copy of a few MB at most behind the ticks), so a later tick
 *    neither waits for nor disturbs a copy in flight (bench.py's host-fed leg).
 *  - meter + last_silent (meter batches; both required): snapshots as well -- the plugin's batched mode reads every source's
 *    level one video frame late. */
typedef struct wf_hip_readback {
    float *rows;             /* WF_HIP_OUT_DECIBELS */
    uint8_t *last_silent;    /* WF_HIP_OUT_LAST_SILENT */
    float *bars;             /* WF_HIP_OUT_BARS */
    float *premirror;        /* WF_HIP_OUT_PREMIRROR */
    float *vertices;         /* WF_HIP_OUT_VERTICES */
    uint32_t *vertex_counts; /* WF_HIP_OUT_VERTEX_COUNTS */
    float *input_rms;        /* WF_HIP_OUT_INPUT_RMS */
    float *meter;            /* WF_HIP_OUT_METER */
} wf_hip_readback;
int wf_hip_read_async(wf_hip *h, uint32_t first, uint32_t count, const wf_hip_readback *dst, uint32_t slot);
int wf_hip_readback_done(wf_hip *h, uint32_t slot);
/* The bars copied device-to-device into `d_out` (a buffer on the handle's device, e.g. the send buffer of an RCCL all-gather;
 * [count][display_channels][num_bars]) without waiting: the copy is enqueued behind the ticks issued so far (every lane of a large batch copies the bars
 * of its own slice: the tick's concurrent launches are not joined) and `consumer_stream` (a hipStream_t of the caller, e.g.
 * the stream its RCCL all-gather runs on) is made to wait for it; the handle goes on with the next tick meanwhile.  The
 * caller keeps `d_out` untouched by anything else until its consumer has run (wf_hip_wait_event orders a reuse). */
int wf_hip_copy_bars_device_async(wf_hip *h, uint32_t first, uint32_t count, void *d_out, void *consumer_stream);
/* Zero-copy form of the above (ABI 13): from the next tick on, every tick ALSO leaves the bars of the whole batch -- the ones it
 * finishes and, copied over, the ones it leaves as they are (paused, hidden, silent streams) -- in caller-owned device memory of
 * the same shape ([num_streams][display_channels][num_bars] floats): the send buffer of an all-gather is written by the tick
 * kernel itself, nothing is enqueued behind the tick.  Two SETS of n <= 8 buffers each; every tick writes every buffer of the
 * current write set.  The buffers may be memory of peer devices this device can address (hipDeviceEnablePeerAccess must have
 * SUCCEEDED for the pair: a kernel store to an unmapped peer address faults): a shard then leaves its slice in every device's
 * gathered result itself, and the exchange of BASELINE configs[4] needs no copy and no collective kernel at all (the C ABI's
 * multi-device group, peer transport).  n = 0 turns it off.  The call waits for the ticks in flight (they write the old
 * buffers) before it replaces the sets: the caller may free the old buffers when it returns.
 * Power-of-two fft sizes up to 32768 whose display the tick kernel finishes itself ONLY: WF_HIP_ERR_UNSUPPORTED for the sizes that
 * are not powers of two (Bluestein / mixed-radix instantiations run at their register caps), for the sizes beyond a CU's LDS and
 * for filtered displays that do not fit the tick kernel's staging -- those keep wf_hip_copy_bars_device_async (wf_hip_multi_* and
 * waveform_amd.dist.BarsGather pick the path per handle).  WF_HIP_ERR_INVALID for level-meter and waveform batches. */
int wf_hip_set_bars_mirrors(wf_hip *h, uint32_t n, void *const *set0, void *const *set1);
/* Hand-over: `consumer_stream` is made to wait for the newest tick (every lane); *d_out = buffer 0 of the set that tick wrote,
 * and the OTHER set becomes the write set -- ticks issued after this call leave the handed-over set alone until the next
 * hand-over makes it the write set again.  (The write set changes here and only here: ticks between two hand-overs rewrite the
 * same set, a tick that fails changes nothing.)  If no tick has written the set since it became the write set, the call fills it
 * from the handle's own bars first (a device copy per buffer, behind the ticks issued so far).  Nothing waits on the host.
 * The caller's side of the protocol: whatever still reads the set that now becomes the write set (the consumer of the hand-over
 * before last) must have run before the next tick is issued -- an event of its own behind that consumer, a tick old by then:
 * hipEventSynchronize returns at once (a device-side wait in front of every tick instead cost 4 % of the tick rate). */
int wf_hip_bars_mirror_ready(wf_hip *h, void *consumer_stream, void **d_out);
/* everything the handle issues after this call (on all of its internal streams) waits, on the device, for `event` (a
 * hipEvent_t of the caller, recorded before the call) -- e.g. "the gather that read the buffer the next
 * wf_hip_copy_bars_device_async overwrites has run".  Does not wait on the host. */
int wf_hip_wait_event(wf_hip *h, void *event);
/* device pointers for zero-copy consumers on the same device (e.g. an RCCL all-gather of
 * the bars, or a renderer): valid until wf_hip_destroy */
float *wf_hip_decibels_device(wf_hip *h);
float *wf_hip_bars_device(wf_hip *h);
void *wf_hip_stream(wf_hip *h); /* hipStream_t */

/* ---- host tables (what update() precomputes), for tests and for hosts that render themselves */
typedef enum wf_hip_table_id {
    WF_HIP_TABLE_WINDOW = 0,     /* float [fft_size]   m_window_coefficients (src/source.cpp:1190-1226) */
    WF_HIP_TABLE_WINDOW_SUM,     /* float [1]          m_window_sum (:1228-1234) */
    WF_HIP_TABLE_SLOPE,          /* float [fft_size/2] m_slope_modifiers (:1283-1290); empty when cfg.slope <= 0 */
    WF_HIP_TABLE_ROLLOFF,        /* float [fft_size/2] m_rolloff_modifiers (:898-918) */
    WF_HIP_TABLE_INTERP_INDICES, /* float []           m_interp_indices (init_interp, :837-896) */
    WF_HIP_TABLE_BAND_WIDTHS,    /* int   [num_bars]   m_band_widths */
    WF_HIP_TABLE_INTERP_WEIGHTS, /* float [][taps]     m_interp_kernel's weights, one row per sample position */
    WF_HIP_TABLE_INTERP_SHAPE    /* int   [2]          {radius, taps} of the interpolation kernel */
} wf_hip_table_id;
/* number of elements; *out (may be NULL) = the table, owned by the handle, NULL when empty */
size_t wf_hip_table(const wf_hip *h, wf_hip_table_id which, const void **out);
float wf_hip_gravity(const wf_hip *h, float seconds); /* get_gravity(), src/source.hpp:301-312 */
/* vertex fill (cfg.vertices; WF_HIP_OUT_VERTICES / WF_HIP_OUT_VERTEX_COUNTS): vertices per displayed channel, 0 when cfg.vertices is off */
uint32_t wf_hip_num_vertices(const wf_hip *h);
const float *wf_hip_vertices_device(wf_hip *h); /* [n_streams][display_channels][num_vertices][4], device pointer */

float wf_hip_db_min(void);                            /* DB_MIN, src/source.cpp:43 */

/* ---- measurement ---------------------------------------------------------------------------- */
/* Runs `ticks` ticks back to back, each `hop` frames further into audio that must already be in the rings
 * (delay_frames = first_delay - i*hop; a walk that has reached the newest sample starts over at first_delay: the same work
 * per tick on the same resident audio, with no host synchronisation in between), and returns the average device time per
 * tick in milliseconds, measured with hipEvents on the handle's stream around all of the ticks' launches. */
int wf_hip_time_ticks(wf_hip *h, const wf_hip_tick_params *p, uint32_t ticks, uint32_t hop, float *avg_kernel_ms);
/* The same measurement around calls of the host's choosing: wf_hip_time_begin records a hipEvent on the handle's stream,
 * wf_hip_time_end joins everything issued since (ticks on every lane, copies), records the second event, waits for it and
 * returns the elapsed device time in milliseconds. */
int wf_hip_time_begin(wf_hip *h);
int wf_hip_time_end(wf_hip *h, float *elapsed_ms);
const char *wf_hip_kernel_name(const wf_hip *h);
/* launches of the fused kernel one wf_hip_tick issues (lanes: slices of the batch on their own HIP streams, running
 * concurrently; a profiler's per-launch average is then not the time a tick takes) */
uint32_t wf_hip_launches_per_tick(const wf_hip *h);
/* algorithmic HBM bytes one tick moves: per spectrum 4N in + state r/w + dB out */
uint64_t wf_hip_algorithmic_bytes_per_tick(const wf_hip *h, uint32_t flags);


/* ---- one batch over several devices (BASELINE.json configs[4]) ----------------------------------
 * The reference has nothing distributed: its sources share nothing (one WAVSource per OBS source, src/source.cpp:87-102), so
 * a batch shards embarrassingly.  A wf_hip_multi is ONE batch of `streams_total` streams split into contiguous shards over
 * n devices of one node -- shard i = streams [first_i, first_i + count_i), sizes differing by at most one, the first
 * (streams_total % n) shards holding one more -- each shard a plain wf_hip handle on its device, driven by its own host
 * thread (single process; the calls below fan out to the threads and return when every device has *enqueued* its part, as
 * wf_hip_tick does).  There is no collective on the data path.  The one exchange is the result the north star asks for:
 * wf_hip_multi_allgather_bars leaves the bar heights of ALL streams on EVERY device ([streams_total][display_channels]
 * [num_bars] floats, global stream order) for a combined render -- by ncclAllGather of a dlopen()ed librccl.so over xGMI
 * (transport "rccl"; shards of unequal size are padded to the largest and compacted on the device), or, where RCCL is
 * absent or refuses the device list (e.g. the same device named twice, which this library allows), by direct peer copies
 * (hipMemcpyPeerAsync, transport "peer"); WF_HIP_MULTI_TRANSPORT=rccl|peer forces one.  The gather is asynchronous and
 * double-buffered: it is enqueued on a side stream of every device behind the ticks issued so far, the next tick runs
 * meanwhile, and a result stays valid until the FIRST TICK AFTER THE NEXT GATHER (where the tick kernels write the send
 * buffers -- or, one device / peer access everywhere, the results -- themselves, that tick's kernels rewrite the buffer; the
 * copying paths keep it until the second-next gather, but no caller should count on which path a size takes).  Ticks between
 * two gathers, on the group or on a shard handle, and ticks that fail on one shard do not move the buffers: the pair is
 * switched by the gather, on every shard together.  wf_hip_set_bars_mirrors / wf_hip_bars_mirror_ready must not be called on a
 * shard handle (the group owns its shards' mirror buffers; a gather that finds the shards disagreeing fails).
 * A gather that fails on one device (the others may have their half in flight) takes the exchange out of service for the
 * group: the failing call returns the error, the RCCL communicators are aborted (ncclCommAbort -- no device keeps waiting for
 * a rank that never joined), every later gather returns WF_HIP_ERR_RUNTIME, and everything else -- ticks, reads,
 * wf_hip_multi_sync, wf_hip_multi_destroy -- keeps working.
 * A wf_hip_multi is used by one thread at a time, like a handle.  Shard handles may be used directly (shard-local stream
 * indices) between multi calls -- every wf_hip_* entry point works on them. */
typedef struct wf_hip_multi wf_hip_multi;
int wf_hip_multi_create(const wf_config *cfg, const int *devices, uint32_t n_devices, uint32_t streams_total, uint32_t ring_frames,
                        wf_hip_multi **out);
void wf_hip_multi_destroy(wf_hip_multi *m);
/* text of the last error on this group (or of the last failed wf_hip_multi_create when m == NULL).  Right after a successful
 * wf_hip_multi_create: why the group did not get the transport it would have picked by itself, or "".  RCCL's reason where it was
 * wanted and not to be had ("librccl.so not loadable: ...", "librccl.so lacks nccl...", "ncclCommInitAll failed: ..."); otherwise,
 * on the peer transport, why the tick kernels do not store into every device's result themselves, each ending in ": the bars
 * travel by hipMemcpyPeerAsync" -- "peer access is not enabled from device I to device J" (the first such ordered pair, HIP device
 * numbers), "N devices: a tick kernel stores into the results of at most 8 (wf_hip_set_bars_mirrors)", or
 * "WF_HIP_MULTI_MIRROR=send asks for no direct stores into the other devices' results" (=0 likewise) */
const char *wf_hip_multi_last_error(const wf_hip_multi *m);
uint32_t wf_hip_multi_num_devices(const wf_hip_multi *m);
uint32_t wf_hip_multi_num_streams(const wf_hip_multi *m);
/* "rccl", "peer" or "local" (one shard: the gather is a device copy) */
const char *wf_hip_multi_transport(const wf_hip_multi *m);
/* shard i: its handle, its HIP device, its first global stream and its stream count (any out pointer may be NULL) */
wf_hip *wf_hip_multi_shard(wf_hip_multi *m, uint32_t i, int *device, uint32_t *first, uint32_t *count);
/* wf_hip_push_audio / wf_hip_push_synth / wf_hip_set_hidden / wf_hip_reset with global stream indices (a range may span
 * shards; stream s of wf_hip_multi_push_synth receives wf_synth_noise(seed, stream_id0 + s, ..): the same audio whatever
 * the number of devices) */
int wf_hip_multi_push_audio(wf_hip_multi *m, uint32_t first, uint32_t count, const float *samples, uint32_t frames);
int wf_hip_multi_push_synth(wf_hip_multi *m, uint32_t first, uint32_t count, uint64_t seed, uint32_t stream_id0, uint64_t index0, uint32_t frames);
/* wf_hip_push_pcm with global stream indices: the packet is split at the shard boundaries (stream i's block at
 * i * channels * frames * bytes_per_sample).  WF_HIP_PCM_HOST packets without frames_per_stream only. */
int wf_hip_multi_push_pcm(wf_hip_multi *m, uint32_t first, uint32_t count, const wf_hip_pcm *pcm);
int wf_hip_multi_set_hidden(wf_hip_multi *m, uint32_t first, uint32_t count, const uint8_t *mask);
int wf_hip_multi_reset(wf_hip_multi *m, uint32_t first, uint32_t count);
/* WAVSource*::tick_spectrum for every stream of every shard (wf_hip_tick on each device, issued concurrently by the
 * devices' host threads) */
int wf_hip_multi_tick(wf_hip_multi *m, const wf_hip_tick_params *p);
int wf_hip_multi_sync(wf_hip_multi *m); /* every device's streams, the gather streams included */
/* results with global stream indices, as wf_hip_read (any output of the batch) */
int wf_hip_multi_read(wf_hip_multi *m, wf_hip_output what, uint32_t first, uint32_t count, void *out);
/* the exchange (see above); needs cfg.bars or cfg.curve */
int wf_hip_multi_allgather_bars(wf_hip_multi *m);
/* device i's copy of the newest gathered result: a pointer on that device (valid until the first tick after the next gather; ordered behind
 * the gather on wf_hip_multi_gather_stream(m, i)), or copied to the host after waiting for it */
const float *wf_hip_multi_gathered_device(wf_hip_multi *m, uint32_t i);
void *wf_hip_multi_gather_stream(wf_hip_multi *m, uint32_t i); /* hipStream_t */
int wf_hip_multi_read_gathered(wf_hip_multi *m, uint32_t i, float *out);
/* measurement: `ticks` ticks back to back on every device as wf_hip_time_ticks does (each device's host thread runs its own
 * loop), with an all-gather of the bars behind every tick when gather != 0; returns the largest per-device average device
 * time per tick (ms) and, in per_device_ms[n_devices] when not NULL, each device's own */
int wf_hip_multi_time_ticks(wf_hip_multi *m, const wf_hip_tick_params *p, uint32_t ticks, uint32_t hop, int gather, float *avg_ms,
                            float *per_device_ms);


/* ---- test aids (development builds only: -DWF_DEV_BUILD, libwaveform_hip_dev.so; the release library exports neither) ---- */
#ifdef WF_DEV_BUILD
/* Moves the 32-bit sample counters of streams [first, first+count) on by `frames` (a multiple of the ring capacity), as
 * if that much audio had been captured before what the rings hold: tests reach the 2^32-sample wrap-around (a day at
 * 48 kHz; the reference's deques have no such counter) without feeding a day of audio. */
int wf_hip_debug_age(wf_hip *h, uint32_t first, uint32_t count, uint32_t frames);
/* Shard `shard` of the group reports a failure in its half of the next gather (wf_hip_multi_allgather_bars or a gathering
 * wf_hip_multi_time_ticks) before it enqueues anything -- what a failed wait or copy on one device looks like to the others,
 * which have their collective / copies in flight by then.  Tests use it to check that the group survives: the call returns
 * the error, the communicators are aborted, later gathers are refused, ticks, reads, sync and destroy go on working. */
int wf_hip_multi_debug_fail_next_gather(wf_hip_multi *m, uint32_t shard);
#endif

#ifdef __cplusplus
}
#endif
#endif
