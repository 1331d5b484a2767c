"""ctypes binding of libwaveform_hip.so (include/wf_hip.h).  Thin by design: argument
marshalling only, no numerics and no fallbacks."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
_LIB = None

WINDOW = dict(none=0, hann=1, hamming=2, blackman=3, blackman_harris=4, power_of_sine=5)
TSMOOTH = dict(none=0, exponential=1, tvexponential=2)
INTERP = dict(point=0, lanczos=1, catrom=2)


class WfHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"wf_hip error {code}: {msg}")
        self.code = code


class Config(C.Structure):
    """struct wf_config (include/wf_config.h)."""
    _fields_ = [
        ("fft_size", C.c_uint32), ("sample_rate", C.c_uint32), ("capture_channels", C.c_uint32), ("stereo", C.c_uint32),
        ("window", C.c_int32), ("sine_exponent", C.c_int32), ("tsmoothing", C.c_int32), ("gravity", C.c_float),
        ("fast_peaks", C.c_uint32), ("slope", C.c_float), ("rolloff_q", C.c_float), ("rolloff_rate", C.c_float),
        ("cutoff_low", C.c_int32), ("cutoff_high", C.c_int32), ("floor_db", C.c_int32), ("ceiling_db", C.c_int32),
        ("normalize_volume", C.c_uint32), ("volume_target", C.c_float), ("max_gain", C.c_float),
        ("bars", C.c_uint32), ("interp_mode", C.c_int32), ("log_scale", C.c_uint32), ("mirror_freq_axis", C.c_uint32),
        ("width", C.c_uint32), ("height", C.c_uint32), ("bar_width", C.c_int32), ("bar_gap", C.c_int32),
        ("channel_spacing", C.c_int32), ("min_bar_height", C.c_int32), ("rounded_caps", C.c_uint32),
        ("curve", C.c_uint32), ("filter_mode", C.c_int32), ("filter_radius", C.c_float),
        ("meter", C.c_uint32), ("meter_rms", C.c_uint32), ("meter_ms", C.c_int32),
        ("waveform", C.c_uint32), ("vertices", C.c_uint32), ("step_width", C.c_int32), ("step_gap", C.c_int32),
        ("radial", C.c_uint32),
    ]

    @classmethod
    def defaults(cls, **overrides) -> "Config":
        cfg = cls()
        lib().wf_config_defaults(C.byref(cfg))
        for k, v in overrides.items():
            if not hasattr(cfg, k):
                raise AttributeError(f"wf_config has no field {k!r}")
            setattr(cfg, k, v)
        return cfg


class TickParams(C.Structure):
    _fields_ = [("seconds", C.c_float), ("delay_frames", C.c_uint32), ("input_rms", C.c_float), ("flags", C.c_uint32),
                ("audio_ts_ns", C.c_uint64)]


TICK_NO_DECIBELS = 1


# wf_hip_output / wf_hip_table_id (include/wf_hip.h)
OUT_DECIBELS, OUT_BARS, OUT_PREMIRROR, OUT_VERTICES, OUT_VERTEX_COUNTS, OUT_LAST_SILENT, OUT_TSMOOTH, OUT_METER, OUT_INPUT_RMS, OUT_WAVEFORM_TS, \
    OUT_LOUDNESS, OUT_PEAKS, OUT_SIGNAL, OUT_PITCH, OUT_BANDS, OUT_STEREO, OUT_CQ, OUT_SCOPE, OUT_GONIO, OUT_SONO, OUT_BITS, OUT_THD, OUT_DELAY, OUT_ONSET, \
    OUT_XFER, OUT_IMPULSE, OUT_CLICK, OUT_IMD, OUT_TEMPO, OUT_HUM = range(30)
(TABLE_WINDOW, TABLE_WINDOW_SUM, TABLE_SLOPE, TABLE_ROLLOFF, TABLE_INTERP_INDICES, TABLE_BAND_WIDTHS, TABLE_INTERP_WEIGHTS,
 TABLE_INTERP_SHAPE) = range(8)


# wf_hip_pcm_format / wf_hip_pcm_memory: libobs' enum audio_format, by numpy dtype (the planar format is the interleaved one + 4)
PCM_FORMAT = {np.dtype(np.uint8): 1, np.dtype(np.int16): 2, np.dtype(np.int32): 3, np.dtype(np.float32): 4}
PCM_HOST, PCM_PINNED, PCM_DEVICE = 0, 1, 2
# wf_hip_wire_format: what libobs has no name for, by name (the planar format is the interleaved one + 8), and a sample's bytes
WIRE_FORMAT = {"s24": 16, "s24_be": 17, "s16_be": 18, "ulaw": 19, "alaw": 20}
WIRE_BYTES = {"s24": 3, "s24_be": 3, "s16_be": 2, "ulaw": 1, "alaw": 1}


class Pcm(C.Structure):
    """struct wf_hip_pcm (include/wf_hip.h): one packet in any libobs sample format or wire format"""
    _fields_ = [("data", C.c_void_p), ("format", C.c_uint32), ("channels", C.c_uint32), ("channel_base", C.c_uint32),
                ("frames", C.c_uint32), ("frames_per_stream", C.POINTER(C.c_uint32)), ("memory", C.c_uint32), ("slot", C.c_uint32)]


def _pcm(samples, interleaved: bool, channel_base: int, frames, slot, wire: str | None = None):
    """(wf_hip_pcm, count, keep-alive) for a numpy array, a PinnedBuffer or a torch tensor on the device.  Shape
    [count, frames, channels] interleaved, [count, channels, frames] planar; `frames`: None, or the per-stream frame counts of
    a ragged push (the shape's frame axis is then max_frames).  wire: a key of WIRE_FORMAT; the array is then uint8 with one
    more axis, the WIRE_BYTES[wire] bytes of a sample."""
    keep = []
    if isinstance(samples, PinnedBuffer):
        if slot is None:
            raise ValueError("a pinned buffer needs a slot (0 / 1)")
        ptr, memory, shape, dtype = samples.ptr, PCM_PINNED, samples.array.shape, samples.array.dtype
    elif hasattr(samples, "data_ptr") and getattr(samples, "is_cuda", False):
        if not samples.is_contiguous():
            raise ValueError("a device tensor must be contiguous")
        ptr, memory, shape = samples.data_ptr(), PCM_DEVICE, tuple(samples.shape)
        dtype = np.dtype(str(samples.dtype).replace("torch.", ""))
    else:
        arr = np.ascontiguousarray(samples)
        keep.append(arr)
        ptr, memory, shape, dtype = arr.ctypes.data, PCM_HOST, arr.shape, arr.dtype
    if wire is None:
        if dtype not in PCM_FORMAT or len(shape) != 3:
            raise ValueError(f"expected a [count, frames, channels] / [count, channels, frames] array of uint8, int16, int32 or float32, "
                             f"got {dtype} {shape}")
        fmt = PCM_FORMAT[dtype] + (0 if interleaved else 4)
    else:
        if wire not in WIRE_FORMAT:
            raise ValueError(f"wire format {wire!r}: expected one of {', '.join(WIRE_FORMAT)}")
        if dtype != np.uint8 or len(shape) != 4 or shape[3] != WIRE_BYTES[wire]:
            raise ValueError(f"{wire}: expected a uint8 [count, frames, channels, {WIRE_BYTES[wire]}] / [count, channels, frames, "
                             f"{WIRE_BYTES[wire]}] array, got {dtype} {shape}")
        fmt = WIRE_FORMAT[wire] + (0 if interleaved else 8)
    count = shape[0]
    block_frames, channels = (shape[1], shape[2]) if interleaved else (shape[2], shape[1])
    pcm = Pcm(data=ptr, format=fmt, channels=channels, channel_base=channel_base,
              frames=block_frames, memory=memory, slot=0 if slot is None else slot)
    if frames is not None:
        f = np.ascontiguousarray(frames, dtype=np.uint32)
        assert f.shape == (count,), f.shape
        keep.append(f)
        pcm.frames_per_stream = f.ctypes.data_as(C.POINTER(C.c_uint32))
    return pcm, count, keep


class Loudness(C.Structure):
    """struct wf_hip_loudness (include/wf_hip.h): one stream's loudness readings."""
    _fields_ = [("momentary", C.c_float), ("short_term", C.c_float), ("integrated", C.c_float), ("range", C.c_float),
                ("true_peak", C.c_float), ("reserved", C.c_uint32), ("frames", C.c_uint64)]


LOUDNESS_DTYPE = np.dtype({"names": [n for n, _ in Loudness._fields_],
                           "formats": [np.float32] * 5 + [np.uint32, np.uint64],
                           "offsets": [getattr(Loudness, n).offset for n, _ in Loudness._fields_],
                           "itemsize": C.sizeof(Loudness)})


# struct wf_hip_peaks (include/wf_hip.h): the strongest peaks of one m_decibels row
MAX_PEAKS = 8
PEAKS_DTYPE = np.dtype([("count", np.uint32), ("reserved", np.uint32),
                        ("peak", np.dtype([("hz", np.float32), ("db", np.float32)]), (MAX_PEAKS,))])


# struct wf_hip_signal (include/wf_hip.h): level, DC, clipping and stereo phase of one stream's newest fft_size frames
FULL_SCALE = np.float32(0.999969482421875)  # WF_HIP_FULL_SCALE, 32767 / 32768: |x| at or above it counts as clipped
CHANNEL_SIGNAL_DTYPE = np.dtype([("rms_db", np.float32), ("peak_db", np.float32), ("dc", np.float32), ("clipped", np.uint32)])
SIGNAL_DTYPE = np.dtype([("ch", CHANNEL_SIGNAL_DTYPE, (2,)), ("correlation", np.float32), ("balance_db", np.float32),
                         ("mid_db", np.float32), ("side_db", np.float32)])


# struct wf_hip_pitch (include/wf_hip.h): YIN over one stream's newest min(fft_size, PITCH_MAX_WINDOW) frames
PITCH_MIN_LAG = 8  # WF_HIP_PITCH_MIN_LAG: the shortest lag searched, so hz <= sample_rate / 8
PITCH_THRESHOLD = 0.15  # WF_HIP_PITCH_THRESHOLD: the first lag whose normalised difference is under it is voiced
PITCH_MAX_WINDOW = 4096  # WF_HIP_PITCH_MAX_WINDOW
PITCH_DTYPE = np.dtype([("hz", np.float32), ("clarity", np.float32), ("lag", np.uint32), ("voiced", np.uint32)])


# struct wf_hip_bands (include/wf_hip.h): third-octave band levels and the Z / A / C weighted level of one m_decibels row
NUM_BANDS = 31  # WF_HIP_NUM_BANDS
BANDS_DTYPE = np.dtype([("band_db", np.float32, (NUM_BANDS,)), ("covered", np.uint32), ("total_db", np.float32), ("a_db", np.float32),
                        ("c_db", np.float32), ("reserved", np.uint32)])
BAND_CENTRES_HZ = 1000.0 * 10.0 ** ((np.arange(NUM_BANDS) - 17) / 10.0)  # IEC 61260-1, base ten: 19.95 Hz .. 19.95 kHz

# struct wf_hip_stereo (include/wf_hip.h): correlation, coherence, phase and balance between captured channels 0 and 1 in each
# third-octave band, over one stream's newest window of at most STEREO_MAX_WINDOW frames
STEREO_MAX_WINDOW = 4096  # WF_HIP_STEREO_MAX_WINDOW
STEREO_DTYPE = np.dtype([("correlation", np.float32, (NUM_BANDS,)), ("coherence", np.float32, (NUM_BANDS,)),
                         ("phase_deg", np.float32, (NUM_BANDS,)), ("balance_db", np.float32, (NUM_BANDS,)), ("covered", np.uint32),
                         ("window", np.uint32)])

# struct wf_hip_cq (include/wf_hip.h): the constant-Q spectrum, one level per semitone (bin b: MIDI note 12 + b) and captured
# channel, each over its own Q periods of the newest frames in the ring, at most CQ_MAX_WINDOW of them
CQ_BINS = 120  # WF_HIP_CQ_BINS
CQ_MAX_WINDOW = 16384  # WF_HIP_CQ_MAX_WINDOW
CQ_DTYPE = np.dtype([("db", np.float32, (2, CQ_BINS)), ("end_covered", np.uint32), ("first_resolved", np.uint32),
                     ("max_window", np.uint32), ("reserved", np.uint32)])
CQ_CENTRES_HZ = 440.0 * 2.0 ** ((np.arange(CQ_BINS) - 57) / 12.0)  # C0 16.35 Hz .. B9 15.8 kHz

# struct wf_hip_scope (include/wf_hip.h): the oscilloscope, the smallest and largest sample per column and captured channel of a
# triggered view of V = P / 2 frames inside the newest P = min(fft_size, SCOPE_MAX_WINDOW) frames of the ring
SCOPE_MAX_WINDOW = 8192  # WF_HIP_SCOPE_MAX_WINDOW
SCOPE_COLUMNS = 256  # WF_HIP_SCOPE_COLUMNS
SCOPE_DTYPE = np.dtype([("lo", np.float32, (2, SCOPE_COLUMNS)), ("hi", np.float32, (2, SCOPE_COLUMNS)), ("window", np.uint32),
                        ("view", np.uint32), ("columns", np.uint32), ("start", np.uint32), ("triggered", np.uint32),
                        ("period", np.uint32), ("frac", np.float32), ("reserved", np.uint32)])

# struct wf_hip_gonio (include/wf_hip.h): the vectorscope, how many of the newest P = min(fft_size, GONIO_MAX_WINDOW) frames of
# captured channels 0 and 1 fall into each cell [iy][ix] of a GONIO_GRID x GONIO_GRID picture of side (x) against mid (y), which
# 2^zoom magnifies so that the loudest sample lies between half and full deflection
GONIO_GRID = 64  # WF_HIP_GONIO_GRID
GONIO_MAX_WINDOW = 8192  # WF_HIP_GONIO_MAX_WINDOW
GONIO_MIN_EXP = -24  # WF_HIP_GONIO_MIN_EXP: zoom <= 24
GONIO_DTYPE = np.dtype([("cell", np.uint16, (GONIO_GRID, GONIO_GRID)), ("window", np.uint32), ("zoom", np.int32), ("peak", np.float32),
                        ("mid_peak", np.float32), ("side_peak", np.float32), ("in_phase", np.uint32), ("out_phase", np.uint32),
                        ("occupied", np.uint32)])

# struct wf_hip_sono (include/wf_hip.h): the sonogram, db[channel][age][band] = the level in band b (SONO_EDGES_HZ[b] to [b + 1]) of
# the window of SONO_WINDOW frames that ends at counter frame (newest - age) * SONO_HOP, for age < columns; -inf beyond
SONO_WINDOW = 1024  # WF_HIP_SONO_WINDOW
SONO_HOP = 256  # WF_HIP_SONO_HOP
SONO_COLUMNS = 64  # WF_HIP_SONO_COLUMNS
SONO_BANDS = 64  # WF_HIP_SONO_BANDS
SONO_EDGES_HZ = 62.5 * np.exp2(np.arange(SONO_BANDS + 1, dtype=np.float64) / 8.0)  # eight bands to the octave, 62.5 Hz to 16 kHz
SONO_DTYPE = np.dtype([("db", np.float32, (2, SONO_COLUMNS, SONO_BANDS)), ("columns", np.uint32), ("newest", np.uint32),
                       ("first_covered", np.uint32), ("end_covered", np.uint32), ("window", np.uint32), ("hop", np.uint32),
                       ("reserved", np.uint32, (2,))])

# struct wf_hip_bits (include/wf_hip.h): the bit meter, per captured channel the histogram of sample values, how often each bit of the
# sample on a 32-bit two's-complement grid is set, the level histogram in bits, the word length, the over-range and below-the-grid
# counts and the longest run of identical samples of the newest P = min(fft_size, BITS_MAX_WINDOW) frames of the ring
BITS_MAX_WINDOW = 8192  # WF_HIP_BITS_MAX_WINDOW
BITS_CHANNEL_DTYPE = np.dtype([("hist", np.uint16, (256,)), ("ones", np.uint16, (32,)), ("mag", np.uint16, (32,)),
                               ("word_length", np.uint32), ("magnitude_bits", np.uint32), ("over", np.uint32), ("fine", np.uint32),
                               ("repeats", np.uint32), ("max_run", np.uint32), ("max_run_start", np.uint32),
                               ("max_run_value", np.float32)])
BITS_DTYPE = np.dtype([("ch", BITS_CHANNEL_DTYPE, (2,)), ("window", np.uint32), ("reserved", np.uint32, (3,))])

# struct wf_hip_thd (include/wf_hip.h): the distortion analyser, per captured channel the fundamental of a test tone, its harmonics
# 2 .. 10 in dBc, THD, THD+N, SNR, SFDR, the noise floor and the strongest spur of the newest P frames of the ring through a 7-term
# Blackman-Harris taper, P the largest power of two <= min(fft_size, THD_MAX_WINDOW)
THD_MAX_WINDOW = 8192  # WF_HIP_THD_MAX_WINDOW
THD_LOBE = 8  # WF_HIP_THD_LOBE
THD_HARMONICS = 9  # WF_HIP_THD_HARMONICS
THD_CHANNEL_DTYPE = np.dtype([("fundamental_hz", np.float64), ("fundamental_db", np.float32), ("thd_db", np.float32),
                              ("thdn_db", np.float32), ("snr_db", np.float32), ("noise_db", np.float32), ("sfdr_db", np.float32),
                              ("spur_hz", np.float32), ("enob", np.float32), ("harmonic_db", np.float32, (THD_HARMONICS,)),
                              ("fundamental_bin", np.uint32), ("spur_bin", np.uint32), ("harmonics", np.uint32), ("valid", np.uint32),
                              ("reserved", np.uint32)])
THD_DTYPE = np.dtype([("ch", THD_CHANNEL_DTYPE, (2,)), ("window", np.uint32), ("reserved", np.uint32, (3,))])

# struct wf_hip_delay (include/wf_hip.h): the delay finder, by how many frames captured channel 0 lags channel 1 (positive: channel 0
# is the later one) and whether one of them is inverted, from the floored-PHAT cross-correlation of the newest P frames of both
# rings, P the largest power of two <= min(fft_size, DELAY_MAX_WINDOW), with the correlation curve around the peak
DELAY_MAX_WINDOW = 4096  # WF_HIP_DELAY_MAX_WINDOW
DELAY_CURVE = 65  # WF_HIP_DELAY_CURVE
DELAY_DTYPE = np.dtype([("delay_frames", np.float64), ("delay_ms", np.float32), ("peak", np.float32), ("corr", np.float32),
                        ("corr_zero", np.float32), ("ambiguity", np.float32), ("lag", np.int32), ("polarity", np.int32),
                        ("valid", np.uint32), ("window", np.uint32), ("reserved", np.uint32), ("curve", np.float32, (DELAY_CURVE,)),
                        ("reserved2", np.uint32, (3,))])

# struct wf_hip_onset (include/wf_hip.h): the onset detector, strength[age] and group[low, mid, high][age] = the positive change of
# the compressed level in the sonogram's 64 bands between the columns that end at counter frames (newest - age - 1) and
# (newest - age) * ONSET_HOP, for age < columns; flags[age] (ONSET_FLAG_*) say which of the four curves has an onset there and
# whether the column is decided; 0 beyond
ONSET_WINDOW = 1024  # WF_HIP_ONSET_WINDOW
ONSET_HOP = 256  # WF_HIP_ONSET_HOP
ONSET_COLUMNS = 128  # WF_HIP_ONSET_COLUMNS
ONSET_BANDS = 64  # WF_HIP_ONSET_BANDS
ONSET_FLAG_TOTAL, ONSET_FLAG_LOW, ONSET_FLAG_MID, ONSET_FLAG_HIGH, ONSET_FLAG_DECIDED = 1, 2, 4, 8, 0x80
ONSET_NONE = 0xFFFFFFFF  # last_age when no decided column in view is an onset
ONSET_DTYPE = np.dtype([("strength", np.float32, (ONSET_COLUMNS,)), ("group", np.float32, (3, ONSET_COLUMNS)),
                        ("flags", np.uint8, (ONSET_COLUMNS,)), ("columns", np.uint32), ("newest", np.uint32),
                        ("decided_first", np.uint32), ("decided_end", np.uint32), ("window", np.uint32), ("hop", np.uint32),
                        ("onsets", np.uint32), ("last_age", np.uint32), ("last_frame", np.uint32), ("last_strength", np.float32),
                        ("reserved", np.uint32, (6,))])

# struct wf_hip_xfer (include/wf_hip.h): the transfer function of captured channel 0 (measured) against channel 1 (reference),
# gain_db[k], phase[k] and coherence[k] at bin k (k sample_rate / window Hz, 1 <= k < window / 2; 0 elsewhere), averaged over
# `segments` half-overlapped segments of `window` frames anchored to the sample counter, with `lag` frames of delay taken out
XFER_MAX_WINDOW = 2048  # WF_HIP_XFER_MAX_WINDOW
XFER_MAX_SEGMENTS = 32  # WF_HIP_XFER_MAX_SEGMENTS
XFER_BINS = 1024  # WF_HIP_XFER_BINS
XFER_DTYPE = np.dtype([("valid", np.uint32), ("window", np.uint32), ("hop", np.uint32), ("segments", np.uint32), ("lag", np.int32),
                       ("newest", np.uint32), ("lag_peak", np.float32), ("mean_coherence", np.float32), ("reserved", np.uint32, (4,)),
                       ("gain_db", np.float32, (XFER_BINS,)), ("phase", np.float32, (XFER_BINS,)),
                       ("coherence", np.float32, (XFER_BINS,))])

# struct wf_hip_impulse (include/wf_hip.h): the impulse response of captured channel 0 (measured) against channel 1 (reference), ir[i]
# and its envelope etc_db[i] at lag + i - window / 4 frames behind the reference (0 <= i < window; 0 elsewhere), from the transfer
# function's segments, and the up to IMPULSE_ARRIVALS strongest arrivals, the peak first
IMPULSE_FRAMES = 2048  # WF_HIP_IMPULSE_FRAMES
IMPULSE_ARRIVALS = 8  # WF_HIP_IMPULSE_ARRIVALS
IMPULSE_GUARD = 8  # WF_HIP_IMPULSE_GUARD
IMPULSE_DIRECT = 16  # WF_HIP_IMPULSE_DIRECT
IMPULSE_REG = 1e-6  # WF_HIP_IMPULSE_REG
IMPULSE_ARRIVAL_RATIO = 0.031622776601683794  # WF_HIP_IMPULSE_ARRIVAL_RATIO: -30 dB
IMPULSE_ARRIVAL_DTYPE = np.dtype([("frames", np.float32), ("level_db", np.float32), ("polarity", np.int32), ("reserved", np.uint32)])
IMPULSE_DTYPE = np.dtype([("valid", np.uint32), ("window", np.uint32), ("hop", np.uint32), ("segments", np.uint32), ("lag", np.int32),
                          ("newest", np.uint32), ("lag_peak", np.float32), ("mean_coherence", np.float32), ("count", np.uint32),
                          ("peak_index", np.uint32), ("peak_db", np.float32), ("delay_ms", np.float32), ("energy_db", np.float32),
                          ("direct_db", np.float32), ("reserved", np.uint32, (2,)), ("arrivals", IMPULSE_ARRIVAL_DTYPE, (IMPULSE_ARRIVALS,)),
                          ("ir", np.float32, (IMPULSE_FRAMES,)), ("etc_db", np.float32, (IMPULSE_FRAMES,))])

# struct wf_hip_click (include/wf_hip.h): the click detector, per captured channel the clicks, pops and splices of the newest
# P = min(fft_size, CLICK_MAX_WINDOW) frames of the ring -- the frames a linear predictor of order CLICK_ORDER fitted to the window
# cannot account for -- as a count, a rate and the up to CLICK_MAX_EVENTS strongest events
CLICK_MAX_WINDOW = 8192  # WF_HIP_CLICK_MAX_WINDOW
CLICK_ORDER = 16  # WF_HIP_CLICK_ORDER
CLICK_GAP = 32  # WF_HIP_CLICK_GAP
CLICK_MAX_EVENTS = 8  # WF_HIP_CLICK_MAX_EVENTS
CLICK_THRESHOLD = 16.0  # WF_HIP_CLICK_THRESHOLD
CLICK_EVENT_DTYPE = np.dtype([("start", np.uint32), ("length", np.uint32), ("peak", np.uint32), ("frame", np.uint32),
                              ("strength_db", np.float32), ("amplitude", np.float32)])
CLICK_CHANNEL_DTYPE = np.dtype([("valid", np.uint32), ("events", np.uint32), ("hit_frames", np.uint32), ("listed", np.uint32),
                                ("rate", np.float32), ("peak_db", np.float32), ("floor_db", np.float32), ("prediction_gain_db", np.float32),
                                ("ev", CLICK_EVENT_DTYPE, (CLICK_MAX_EVENTS,))])
CLICK_DTYPE = np.dtype([("ch", CLICK_CHANNEL_DTYPE, (2,)), ("window", np.uint32), ("order", np.uint32), ("reserved", np.uint32, (2,))])

# struct wf_hip_imd (include/wf_hip.h): the two-tone intermodulation analyser, per captured channel the two tones of a twin-tone
# stimulus, their IMD_PRODUCTS sum and difference products of orders 2 .. 5 against the two tones' power, total IMD, the
# difference-frequency (IEC 60268-3) and modulation (DIN / SMPTE) distortion, distortion + noise and the noise floor of the newest P
# frames of the ring through the distortion analyser's taper, P as THD's
IMD_PRODUCTS = 20  # WF_HIP_IMD_PRODUCTS
IMD_MIN_RATIO = 1e-3  # WF_HIP_IMD_MIN_RATIO
IMD_ORDERS = 4  # orders 2 .. 5
IMD_CHANNEL_DTYPE = np.dtype([("lo_hz", np.float64), ("hi_hz", np.float64), ("lo_db", np.float32), ("hi_db", np.float32),
                              ("ratio_db", np.float32), ("imd_db", np.float32), ("order_db", np.float32, (IMD_ORDERS,)),
                              ("dfd2_db", np.float32), ("dfd3_db", np.float32), ("mod_db", np.float32), ("tdn_db", np.float32),
                              ("noise_db", np.float32), ("product_db", np.float32, (IMD_PRODUCTS,)), ("lo_bin", np.uint32),
                              ("hi_bin", np.uint32), ("products", np.uint32), ("tones", np.uint32), ("valid", np.uint32),
                              ("reserved", np.uint32, (2,))])
IMD_DTYPE = np.dtype([("ch", IMD_CHANNEL_DTYPE, (2,)), ("window", np.uint32), ("reserved", np.uint32, (3,))])

# struct wf_hip_tempo (include/wf_hip.h): tempo and beat phase, strength[age] = the onset detector's total strength of the column
# that ends at counter frame (newest - age) * TEMPO_HOP, for age < columns (0 beyond); acf[L] its autocorrelation at a lag of L
# columns; the best lag as bpm and period, a second candidate, and the frames of the last and the next beat on the sample counter
TEMPO_WINDOW = 1024  # WF_HIP_TEMPO_WINDOW
TEMPO_HOP = 256  # WF_HIP_TEMPO_HOP
TEMPO_COLUMNS = 2048  # WF_HIP_TEMPO_COLUMNS
TEMPO_LAGS = 576  # WF_HIP_TEMPO_LAGS
TEMPO_MAX_LAG = 287  # WF_HIP_TEMPO_MAX_LAG
TEMPO_MIN_RING = 131072  # WF_HIP_TEMPO_MIN_RING
TEMPO_MARGIN = 2.0  # WF_HIP_TEMPO_MARGIN
TEMPO_DTYPE = np.dtype([("strength", np.float32, (TEMPO_COLUMNS,)), ("acf", np.float32, (TEMPO_LAGS,)), ("bpm", np.float32),
                        ("period", np.float32), ("confidence", np.float32), ("salience", np.float32), ("bpm2", np.float32),
                        ("salience2", np.float32), ("ambiguity", np.float32), ("strength_max", np.float32),
                        ("strength_mean", np.float32), ("valid", np.uint32), ("columns", np.uint32), ("newest", np.uint32),
                        ("lag_lo", np.uint32), ("lag_hi", np.uint32), ("lag", np.uint32), ("lag2", np.uint32), ("beat_age", np.uint32),
                        ("period_frames", np.uint32), ("last_beat_frame", np.uint32), ("next_beat_frame", np.uint32),
                        ("window", np.uint32), ("hop", np.uint32), ("reserved", np.uint32, (2,))])

# struct wf_hip_hum (include/wf_hip.h): mains hum, per captured channel the family (0 / 50 / 60), the mains frequency, the
# qualified harmonics (mask bit h - 1; hz, level_db and snr_db at [h - 1], 0 where the bit is clear) and the hum's level against
# the total, from the newest `window` frames at a resolution of resolution_hz
HUM_HARMONICS = 8  # WF_HIP_HUM_HARMONICS
HUM_MARGIN_DB = 15.0  # WF_HIP_HUM_MARGIN_DB
HUM_TOL_HZ = 0.5  # WF_HIP_HUM_TOL_HZ
HUM_FLOOR_SPAN = 20  # WF_HIP_HUM_FLOOR_SPAN
HUM_FLOOR_GUARD = 3  # WF_HIP_HUM_FLOOR_GUARD
HUM_MAX_WINDOW = 32768  # WF_HIP_HUM_MAX_WINDOW
HUM_CHANNEL_DTYPE = np.dtype([("mains_hz", np.float32), ("hum_db", np.float32), ("total_db", np.float32), ("ratio_db", np.float32),
                              ("odd_db", np.float32), ("even_db", np.float32), ("noise_db", np.float32), ("valid", np.uint32),
                              ("family", np.uint32), ("lines", np.uint32), ("mask", np.uint32), ("hz", np.float32, (HUM_HARMONICS,)),
                              ("level_db", np.float32, (HUM_HARMONICS,)), ("snr_db", np.float32, (HUM_HARMONICS,)),
                              ("reserved", np.uint32)])
HUM_DTYPE = np.dtype([("ch", HUM_CHANNEL_DTYPE, (2,)), ("window", np.uint32), ("decimation", np.uint32), ("resolution_hz", np.float32),
                      ("reserved", np.uint32)])


# the measurement outputs (csrc/wf_hip_measure.hip, MEASURES): reader -> (output, the dtype of an entry, one entry per m_decibels
# row -- output_channels per stream -- rather than one per stream)
MEASURES = {
    "loudness": (OUT_LOUDNESS, LOUDNESS_DTYPE, False),
    "peaks": (OUT_PEAKS, PEAKS_DTYPE, True),
    "signal": (OUT_SIGNAL, SIGNAL_DTYPE, False),
    "pitch": (OUT_PITCH, PITCH_DTYPE, False),
    "bands": (OUT_BANDS, BANDS_DTYPE, True),
    "stereo": (OUT_STEREO, STEREO_DTYPE, False),
    "cq": (OUT_CQ, CQ_DTYPE, False),
    "scope": (OUT_SCOPE, SCOPE_DTYPE, False),
    "gonio": (OUT_GONIO, GONIO_DTYPE, False),
    "sono": (OUT_SONO, SONO_DTYPE, False),
    "bits": (OUT_BITS, BITS_DTYPE, False),
    "thd": (OUT_THD, THD_DTYPE, False),
    "delay": (OUT_DELAY, DELAY_DTYPE, False),
    "onset": (OUT_ONSET, ONSET_DTYPE, False),
    "xfer": (OUT_XFER, XFER_DTYPE, False),
    "impulse": (OUT_IMPULSE, IMPULSE_DTYPE, False),
    "click": (OUT_CLICK, CLICK_DTYPE, False),
    "imd": (OUT_IMD, IMD_DTYPE, False),
    "tempo": (OUT_TEMPO, TEMPO_DTYPE, False),
    "hum": (OUT_HUM, HUM_DTYPE, False),
}


def _read_measure(batch, name: str, first: int, count: int | None) -> np.ndarray:
    """the reader `name` of a SpectrumBatch or MultiBatch: [count] or [count, output_channels] entries"""
    what, dtype, per_row = MEASURES[name]
    return batch._read(what, first, count, (batch.output_channels,) if per_row else (), dtype)


class Readback(C.Structure):
    """wf_hip_readback: the page-locked destinations of one wf_hip_read_async (NULL leaves an output out)"""
    _fields_ = [("rows", C.c_void_p), ("last_silent", C.c_void_p), ("bars", C.c_void_p), ("premirror", C.c_void_p), ("vertices", C.c_void_p),
                ("vertex_counts", C.c_void_p), ("input_rms", C.c_void_p), ("meter", C.c_void_p)]


def library_path() -> Path:
    # WF_HIP_LIB: development aid for A/B-ing kernel builds; the default is the in-tree library
    import os
    override = os.environ.get("WF_HIP_LIB")
    return Path(override) if override else _HERE / "libwaveform_hip.so"


def lib():
    """Loads libwaveform_hip.so; raises if it has not been built (no fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    p = library_path()
    if not p.exists():
        raise FileNotFoundError(f"{p} not built: run `make -C waveform_amd/csrc` (or __graft_entry__.build())")
    L = C.CDLL(str(p))
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    fp = C.POINTER(C.c_float)
    L.wf_config_defaults.argtypes = [C.POINTER(Config)]
    L.wf_hip_abi_version.restype = C.c_int
    L.wf_hip_device_count.restype = C.c_int
    L.wf_hip_last_error.restype = C.c_char_p
    L.wf_hip_last_error.argtypes = [vp]
    L.wf_hip_create.argtypes = [C.POINTER(Config), C.c_int, u32, u32, C.POINTER(vp)]
    L.wf_hip_destroy.argtypes = [vp]
    L.wf_hip_reset.argtypes = [vp, u32, u32]
    for n in ("fft_size", "num_streams", "capture_channels", "output_channels", "display_channels", "num_bars", "ring_frames"):
        f = getattr(L, "wf_hip_" + n)
        f.restype = u32
        f.argtypes = [vp]
    L.wf_hip_push_audio.argtypes = [vp, u32, u32, fp, u32]
    L.wf_hip_push_audio_device.argtypes = [vp, u32, u32, vp, u32]
    L.wf_hip_push_audio_async.argtypes = [vp, u32, u32, vp, u32, u32]
    L.wf_hip_ingest_done.argtypes = [vp, u32]
    L.wf_hip_read_async.argtypes = [vp, u32, u32, C.POINTER(Readback), u32]
    L.wf_hip_readback_done.argtypes = [vp, u32]
    L.wf_hip_host_alloc.restype = vp
    L.wf_hip_host_alloc.argtypes = [C.c_size_t]
    L.wf_hip_host_free.argtypes = [vp]
    L.wf_hip_push_synth.argtypes = [vp, u32, u32, u64, u32, u64, u32]
    L.wf_hip_push_audio_ragged_async.argtypes = [vp, u32, u32, vp, C.POINTER(u32), u32, u32]
    L.wf_hip_push_pcm.argtypes = [vp, u32, u32, C.POINTER(Pcm)]
    L.wf_hip_multi_push_pcm.argtypes = [vp, u32, u32, C.POINTER(Pcm)]
    L.wf_hip_push_audio_muted.argtypes = [vp, u32, u32, fp, u32]
    L.wf_hip_enable_input_rms.argtypes = [vp, C.c_int]
    L.wf_hip_push_rms_ragged_async.argtypes = [vp, u32, u32, vp, C.POINTER(u32), u32, u32]
    L.wf_hip_enable_loudness.argtypes = [vp, u32, u32]
    L.wf_hip_tick.argtypes = [vp, C.POINTER(TickParams)]
    L.wf_hip_set_hidden.argtypes = [vp, u32, u32, C.POINTER(C.c_uint8)]
    L.wf_hip_set_input_rms.argtypes = [vp, u32, u32, fp]
    L.wf_hip_set_stream_delay.argtypes = [vp, u32, u32, C.POINTER(C.c_uint32)]
    L.wf_hip_set_stream_audio_ts.argtypes = [vp, u32, u32, C.POINTER(C.c_uint64)]
    L.wf_hip_sync.argtypes = [vp]
    L.wf_hip_read.argtypes = [vp, C.c_int, u32, u32, vp]
    L.wf_hip_output_bytes.restype = C.c_size_t
    L.wf_hip_output_bytes.argtypes = [vp, C.c_int]
    L.wf_hip_num_vertices.restype = u32
    L.wf_hip_num_vertices.argtypes = [vp]
    L.wf_hip_copy_bars_device_async.argtypes = [vp, u32, u32, vp, vp]
    L.wf_hip_wait_event.argtypes = [vp, vp]
    L.wf_hip_time_begin.argtypes = [vp]
    L.wf_hip_time_end.argtypes = [vp, fp]
    L.wf_hip_write_tsmooth.argtypes = [vp, u32, u32, fp]
    for n in ("decibels_device", "bars_device", "stream"):
        f = getattr(L, "wf_hip_" + n)
        f.restype = vp
        f.argtypes = [vp]
    L.wf_hip_table.restype = C.c_size_t
    L.wf_hip_table.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.wf_hip_gravity.restype = C.c_float
    L.wf_hip_gravity.argtypes = [vp, C.c_float]
    L.wf_hip_db_min.restype = C.c_float
    L.wf_hip_time_ticks.argtypes = [vp, C.POINTER(TickParams), u32, u32, fp]
    L.wf_hip_kernel_name.restype = C.c_char_p
    L.wf_hip_kernel_name.argtypes = [vp]
    if hasattr(L, "wf_hip_debug_age"):  # development builds only (libwaveform_hip_dev.so, -DWF_DEV_BUILD)
        L.wf_hip_debug_age.argtypes = [vp, u32, u32, u32]
    L.wf_hip_launches_per_tick.restype = u32
    L.wf_hip_launches_per_tick.argtypes = [vp]
    L.wf_hip_algorithmic_bytes_per_tick.restype = u64
    L.wf_hip_algorithmic_bytes_per_tick.argtypes = [vp, u32]
    L.wf_hip_set_bars_mirrors.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(vp)]
    L.wf_hip_bars_mirror_ready.argtypes = [vp, vp, C.POINTER(vp)]
    # one batch over several devices (wf_hip_multi_*)
    L.wf_hip_multi_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_int), u32, u32, u32, C.POINTER(vp)]
    L.wf_hip_multi_destroy.argtypes = [vp]
    L.wf_hip_multi_last_error.restype = C.c_char_p
    L.wf_hip_multi_last_error.argtypes = [vp]
    L.wf_hip_multi_transport.restype = C.c_char_p
    L.wf_hip_multi_transport.argtypes = [vp]
    for n in ("num_devices", "num_streams"):
        f = getattr(L, "wf_hip_multi_" + n)
        f.restype = u32
        f.argtypes = [vp]
    L.wf_hip_multi_shard.restype = vp
    L.wf_hip_multi_shard.argtypes = [vp, u32, C.POINTER(C.c_int), C.POINTER(u32), C.POINTER(u32)]
    L.wf_hip_multi_push_audio.argtypes = [vp, u32, u32, fp, u32]
    L.wf_hip_multi_push_synth.argtypes = [vp, u32, u32, u64, u32, u64, u32]
    L.wf_hip_multi_set_hidden.argtypes = [vp, u32, u32, C.POINTER(C.c_uint8)]
    L.wf_hip_multi_reset.argtypes = [vp, u32, u32]
    L.wf_hip_multi_tick.argtypes = [vp, C.POINTER(TickParams)]
    L.wf_hip_multi_sync.argtypes = [vp]
    L.wf_hip_multi_read.argtypes = [vp, C.c_int, u32, u32, vp]
    L.wf_hip_multi_allgather_bars.argtypes = [vp]
    L.wf_hip_multi_gathered_device.restype = vp
    L.wf_hip_multi_gathered_device.argtypes = [vp, u32]
    L.wf_hip_multi_gather_stream.restype = vp
    L.wf_hip_multi_gather_stream.argtypes = [vp, u32]
    L.wf_hip_multi_read_gathered.argtypes = [vp, u32, fp]
    L.wf_hip_multi_time_ticks.argtypes = [vp, C.POINTER(TickParams), u32, u32, C.c_int, fp, fp]
    if hasattr(L, "wf_hip_multi_debug_fail_next_gather"):  # development builds only
        L.wf_hip_multi_debug_fail_next_gather.argtypes = [vp, u32]
    _LIB = L
    return L


def device_count() -> int:
    return int(lib().wf_hip_device_count())


def db_min() -> float:
    return float(lib().wf_hip_db_min())


def _copy(ptr, n, dtype=np.float32):
    if not ptr or n == 0:
        return None
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True)


class _MeasureReaders:
    """The readers of the measurement outputs (MEASURES), shared by SpectrumBatch and MultiBatch: each goes through the batch's own
    _read."""

    def loudness(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count] structured array with the fields of wf_hip_loudness (LOUDNESS_DTYPE)"""
        return _read_measure(self, "loudness", first, count)

    def peaks(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count, output_channels] structured array of wf_hip_peaks (PEAKS_DTYPE): the strongest peaks of each m_decibels row
        as of the newest tick, found on the device when read"""
        return _read_measure(self, "peaks", first, count)

    def signal(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count] structured array of wf_hip_signal (SIGNAL_DTYPE): level, DC, clipping and stereo phase of each stream's
        newest fft_size frames as of the pushes issued so far, measured on the device when read"""
        return _read_measure(self, "signal", first, count)

    def pitch(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count] structured array of wf_hip_pitch (PITCH_DTYPE): fundamental frequency, clarity, lag and voiced flag of each
        stream's newest min(fft_size, PITCH_MAX_WINDOW) frames as of the pushes issued so far, by YIN on the device when read"""
        return _read_measure(self, "pitch", first, count)

    def bands(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count, output_channels] structured array of wf_hip_bands (BANDS_DTYPE): the third-octave band levels and the Z / A / C
        weighted level of each m_decibels row as of the newest tick, summed on the device when read"""
        return _read_measure(self, "bands", first, count)

    def stereo(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count] structured array of wf_hip_stereo (STEREO_DTYPE): correlation, coherence, phase and balance between captured
        channels 0 and 1 in each third-octave band, over each stream's newest window (the largest power of two <=
        min(fft_size, STEREO_MAX_WINDOW) frames) as of the pushes issued so far, transformed on the device when read"""
        return _read_measure(self, "stereo", first, count)

    def cq(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count] structured array of wf_hip_cq (CQ_DTYPE): the constant-Q spectrum, db[channel][semitone] from C0 to B9, each
        bin over the newest min(ceil(Q sr / f), ring_frames, CQ_MAX_WINDOW) frames of the ring as of the pushes issued so far,
        correlated on the device when read"""
        return _read_measure(self, "cq", first, count)

    def scope(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count] structured array of wf_hip_scope (SCOPE_DTYPE): the oscilloscope, lo / hi[channel][column] over a view of
        fft_size / 2 frames that starts at the last rising 50 % crossing of the newest min(fft_size, SCOPE_MAX_WINDOW) frames of the
        ring as of the pushes issued so far, with the trigger's position, sub-sample fraction and period; made on the device
        when read"""
        return _read_measure(self, "scope", first, count)

    def gonio(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count] structured array of wf_hip_gonio (GONIO_DTYPE): the vectorscope, cell[iy][ix] = how many of the newest
        min(fft_size, GONIO_MAX_WINDOW) frames of captured channels 0 and 1, as of the pushes issued so far, fall into each cell
        of the side (x) / mid (y) picture magnified by 2^zoom, with the peaks, the phase counts and the number of occupied cells;
        counted on the device when read (batches with two captured channels)"""
        return _read_measure(self, "gonio", first, count)

    def sono(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count] structured array of wf_hip_sono (SONO_DTYPE): the sonogram, db[channel][age][band] = the level in dB of band
        `band` (SONO_EDGES_HZ) in the Hann window of SONO_WINDOW frames that ends at frame (newest - age) * SONO_HOP of the stream's
        sample counter, for age < columns (which the ring decides: 28 by default, 64 from ring_frames = 32768 up); -inf beyond,
        for silence, and for channel 1 of a capture of one channel.  Columns are anchored to the counter: the same column reads
        the same bits whenever it is read, and (newest - newest of the last read) mod 2^24 columns are new.  Transformed in float64
        on the device when read, from the rings as of the pushes issued so far (batches whose ring holds at least 2048 frames)"""
        return _read_measure(self, "sono", first, count)

    def bits(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count] structured array of wf_hip_bits (BITS_DTYPE): the bit meter, per captured channel ch[c] the sample-value
        histogram hist[256], ones[b] = the frames whose code on a 32-bit two's-complement grid has bit b set, the level histogram
        mag[32], word_length (8 / 16 / 24 for integer PCM, 32 with fine > 0 for float audio), magnitude_bits, the over-range count
        and the longest run of identical samples (max_run, max_run_start, max_run_value) with the count of repeats, over the
        newest min(fft_size, BITS_MAX_WINDOW) frames of the ring as of the pushes issued so far; counted on the device when read.
        With one captured channel ch[1] is all zero"""
        return _read_measure(self, "bits", first, count)

    def thd(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count] structured array of wf_hip_thd (THD_DTYPE): the distortion analyser, per captured channel ch[c] the fundamental
        of a test tone (fundamental_hz, fundamental_db, fundamental_bin), harmonic_db[h - 2] of the harmonics 2 .. 10 in dBc with
        the mask `harmonics` of those in band, thd_db, thdn_db (SINAD is its negative), snr_db, noise_db, sfdr_db with the strongest
        spur (spur_hz, spur_bin), enob and valid (0 for silence or a window holding a NaN: every field 0), over the newest P frames
        of the ring as of the pushes issued so far, P = `window` the largest power of two <= min(fft_size, THD_MAX_WINDOW);
        transformed in float64 through a 7-term Blackman-Harris taper on the device when read (batches of at least 512 frames).
        With one captured channel ch[1] is all zero"""
        return _read_measure(self, "thd", first, count)

    def delay(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count] structured array of wf_hip_delay (DELAY_DTYPE): the delay finder, delay_frames / delay_ms by which captured
        channel 0 lags channel 1 (positive: channel 0 is the later one; lag is its integer part, found within +-window / 4), polarity
        (-1: one channel is inverted), peak (the floored-PHAT correlation at the lag, signed; close to +-1 for one broadband
        arrival) against ambiguity (the second peak over the first: near 1 for a tone or unrelated channels, the delay is not to
        be trusted), corr and corr_zero (the ordinary normalised cross-correlation at the lag and at lag 0), curve (the PHAT
        correlation at lag - 32 .. lag + 32) and valid (0 for silence in either channel or a window holding a NaN: every field 0),
        over the newest P frames of both rings as of the pushes issued so far, P = `window` the largest power of two <=
        min(fft_size, DELAY_MAX_WINDOW); in float64 on the device when read (batches with two captured channels)"""
        return _read_measure(self, "delay", first, count)

    def onset(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count] structured array of wf_hip_onset (ONSET_DTYPE): the onset detector.  strength[age] and group[g][age] (g = low,
        mid, high: 62.5 to 250 Hz, to 2 kHz, to 16 kHz) are the onset strength -- the positive change of the compressed level in
        the sonogram's bands from one column to the next -- of the column that ends at frame (newest - age) * ONSET_HOP of the
        stream's sample counter, for age < columns (which the ring decides: 27 by default, 128 from ring_frames = 65536 up); 0
        beyond.  flags[age]: ONSET_FLAG_TOTAL / _LOW / _MID / _HIGH = an onset of that curve (a strict maximum of the 6 columns
        before, no less than the 3 after, and 2.0 above the mean of the 20 around it), ONSET_FLAG_DECIDED = the column's 20 columns
        are all in view (ages decided_first .. decided_end - 1); once decided a column's flags never change.  onsets counts the
        decided onsets of the total in view; last_age (ONSET_NONE: none), last_frame (the counter position where it started, to
        about a hop) and last_strength describe the newest.  Columns are anchored to the counter: (newest - newest of the last
        read) mod 2^24 columns are new.  In float64 on the device when read, from the rings as of the pushes issued so far
        (batches whose ring holds at least 8192 frames)"""
        return _read_measure(self, "onset", first, count)

    def xfer(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count] structured array of wf_hip_xfer (XFER_DTYPE): the transfer function of a dual-channel analyser with the programme
        as the stimulus, captured channel 0 (measured, what came out) against channel 1 (reference, what went in).  gain_db[k],
        phase[k] (radians, with `lag` frames of delay taken out: add -2 pi k lag / window for the raw one) and coherence[k] (0 .. 1:
        how far the reading at that bin is to be trusted) at bin k = k sample_rate / window Hz for 1 <= k < window / 2, 0 elsewhere;
        averaged over `segments` (13 .. 32, the ring decides) segments of `window` frames (the largest power of two <=
        min(fft_size, XFER_MAX_WINDOW, ring_frames / 8)) `hop` = window / 2 frames apart and anchored to the stream's sample counter:
        reads within one hop are bit-identical, and `newest` = the counter / hop says when a read brings a new segment.  lag is the
        delay of channel 0 behind channel 1 in whole frames, found within +-window / 4 by the floored PHAT of the averaged cross
        spectrum, lag_peak its correlation there; mean_coherence is weighted by the reference's power.  A bin where the reference
        has nothing reads 0 / 0 / 0; valid = 0 (silence in either channel or a NaN in the span) leaves everything but window, hop
        and segments 0.  In float64 on the device when read, from the rings as of the pushes issued so far (batches with two
        captured channels and fft_size >= 256)"""
        return _read_measure(self, "xfer", first, count)

    def impulse(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count] structured array of wf_hip_impulse (IMPULSE_DTYPE): the impulse response of a dual-channel analyser with the
        programme as the stimulus, captured channel 0 (measured) against channel 1 (reference), from the segments xfer() averages
        (window, hop, segments, lag, newest, lag_peak, mean_coherence and valid are its fields, bit for bit).  ir[i] is the response
        and etc_db[i] its envelope in dB (the energy-time curve; -inf where it is 0) lag + i - window / 4 frames behind the
        reference, 0 <= i < window: window / 4 frames before the delay that was taken out and 3 window / 4 behind it; 0 elsewhere.
        arrivals[:count] are the strongest local maxima of the envelope, the peak first and then by falling level, at least
        IMPULSE_GUARD + 1 indices apart and no more than 30 dB under the peak: frames (behind the reference, to a fraction),
        level_db (against the peak) and polarity (+1 / -1).  peak_index, peak_db and delay_ms describe the peak; energy_db is the
        power of the whole response and direct_db that within IMPULSE_DIRECT indices of the peak.  A later arrival reads low by the
        overlap of the segments (-3.9 dB at window / 4).  valid = 0 as xfer(); valid = 1 with count = 0 where the measured channel
        is silent under every segment.  In float64 on the device when read, from the rings as of the pushes issued so far (batches
        with two captured channels and fft_size >= 256)"""
        return _read_measure(self, "impulse", first, count)

    def click(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count] structured array of wf_hip_click (CLICK_DTYPE): the click detector, per captured channel ch[c] the clicks, pops
        and splices of the newest min(fft_size, CLICK_MAX_WINDOW) frames of the ring as of the pushes issued so far -- the frames
        whose residual under a linear predictor of order CLICK_ORDER, fitted to the window, stands more than CLICK_THRESHOLD times
        above the residual's robust level around them -- as events (hits at most CLICK_GAP frames apart), hit_frames, rate in
        clicks per second, peak_db (the largest ratio, hit or not), floor_db, prediction_gain_db and ev[:listed], the up to
        CLICK_MAX_EVENTS strongest events with start, length, peak, frame (the counter position of start: what a polling host tells
        an event it has seen by), strength_db and amplitude; valid = 0 for digital silence, a NaN or an infinity.  Fitted in float64
        on the device when read (batches of at least 256 frames).  With one captured channel ch[1] is all zero"""
        return _read_measure(self, "click", first, count)

    def imd(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count] structured array of wf_hip_imd (IMD_DTYPE): the two-tone intermodulation analyser, per captured channel ch[c]
        the two strongest tones of the newest P = `window` frames of the ring as of the pushes issued so far (lo_hz, hi_hz, lo_db,
        hi_db, ratio_db, lo_bin, hi_bin; `tones` = 0, 1 or 2 found, valid = 1 with two at most 30 dB apart), their IMD_PRODUCTS
        products |m f_hi -+ n f_lo| of orders 2 .. 5 against the two tones' power (product_db[q], order_db[o - 2], the mask `products`
        of those clear of the band's ends and of the tones; -inf otherwise), imd_db over all clear products, dfd2_db and dfd3_db
        (IEC 60268-3), mod_db (DIN / SMPTE: the sidebands of the upper tone against it), tdn_db and noise_db.  P and the taper are
        thd()'s; in float64 on the device when read (batches of at least 512 frames).  With one captured channel ch[1] is all zero"""
        return _read_measure(self, "imd", first, count)

    def tempo(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count] structured array of wf_hip_tempo (TEMPO_DTYPE): tempo and beat phase.  strength[age] is onset()'s total strength
        over the newest `columns` = up to TEMPO_COLUMNS columns of TEMPO_HOP frames in the ring as of the pushes issued so far (507
        with ring_frames = 131072, 2043 with 2^19; 0 beyond), acf[L] its autocorrelation at a lag of L columns.  With valid = 1:
        `lag` (of lag_lo .. lag_hi, 240 down to 40 BPM where the ring allows it) is the lag of the largest salience
        (acf[L] + 0.5 acf[2 L]) w[L] under a preference of one octave around 120 BPM, bpm and period (columns) its parabolic
        refinement, period_frames = period * TEMPO_HOP, confidence = acf[lag]; lag2, bpm2, salience2 and ambiguity =
        salience2 / salience the second candidate (0: none); beat_age the age of the column of the newest beat, last_beat_frame
        and next_beat_frame = last_beat_frame + period_frames its place on the uint32 sample counter.  valid = 0 (a non-finite
        strength, a flat curve, or no strength of at least TEMPO_MARGIN) leaves everything but strength, columns, newest, lag_lo,
        lag_hi, window and hop 0.  In float64 on the device when read (rings of at least TEMPO_MIN_RING frames)"""
        return _read_measure(self, "tempo", first, count)

    def hum(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count] structured array of wf_hip_hum (HUM_DTYPE): mains hum.  Per captured channel ch[c] of the newest `window` = N
        frames in the ring as of the pushes issued so far (N = 16384 at 48 kHz with ring_frames = 16384, 32768 from 32768 on;
        resolution_hz = sample_rate / N): `family` 50 or 60 where lines at h times 50 +- 0.5 or 60 +- 0.5 Hz, h = 1 .. HUM_HARMONICS,
        stand HUM_MARGIN_DB above the local floor and agree on one mains frequency, else 0; `mask` (bit h - 1) and `lines` the
        harmonics found, hz[h - 1] each line's frequency over h, level_db[h - 1] its level (a sine of amplitude 1 reads 0) and
        snr_db[h - 1] its height over the floor, 0 where the bit is clear; mains_hz their weighted mean; hum_db the lines' power,
        total_db the window's mean square, ratio_db = hum_db - total_db; odd_db and even_db the harmonics 3, 5, 7 and 2, 4, 6, 8
        (0: none); noise_db the floor between the lines: with nothing found, a line would have had to reach about noise_db + 15.
        valid = 0 (a window of zeros, a NaN or an infinity) leaves the channel 0, as is a channel the batch does not capture.  A
        lone 300 Hz line reads as the 6th of 50 Hz.  It sees hum above the programme's density in its bin -- pauses, speech, idle
        lines -- and promises nothing under bass-heavy music.  In float64 on the device when read (rings of at least
        sample_rate / 3 frames)"""
        return _read_measure(self, "hum", first, count)


class SpectrumBatch(_MeasureReaders):
    """A batch of `streams` independent sources sharing one configuration, resident on one GPU."""

    def __init__(self, cfg: Config, streams: int, device: int = 0, ring_frames: int = 0):
        self.L = lib()
        self.cfg = cfg
        h = C.c_void_p()
        rc = self.L.wf_hip_create(C.byref(cfg), device, streams, ring_frames, C.byref(h))
        if rc != 0:
            raise WfHipError(rc, self.L.wf_hip_last_error(None).decode())
        self.h = h
        self.streams = streams
        self.fft_size = self.L.wf_hip_fft_size(h)
        self.bins = self.fft_size if cfg.waveform else self.fft_size // 2  # floats per m_decibels row
        self.capture_channels = self.L.wf_hip_capture_channels(h)
        self.output_channels = self.L.wf_hip_output_channels(h)
        self.display_channels = self.L.wf_hip_display_channels(h)
        self.num_bars = self.L.wf_hip_num_bars(h)
        self.ring_frames = self.L.wf_hip_ring_frames(h)

    # -- plumbing -----------------------------------------------------------------
    def _ck(self, rc):
        if rc != 0:
            raise WfHipError(rc, self.L.wf_hip_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.wf_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- audio ----------------------------------------------------------------------
    def push_audio(self, samples: np.ndarray, first: int = 0):
        """samples: float32 [count, capture_channels, frames]"""
        s = np.ascontiguousarray(samples, dtype=np.float32)
        assert s.ndim == 3 and s.shape[1] == self.capture_channels, s.shape
        self._ck(self.L.wf_hip_push_audio(self.h, first, s.shape[0], s.ctypes.data_as(C.POINTER(C.c_float)), s.shape[2]))

    def push_audio_muted(self, samples: np.ndarray, first: int = 0):
        """muted packet: zeros into the rings, `samples` into the device RMS producer"""
        s = np.ascontiguousarray(samples, dtype=np.float32)
        assert s.ndim == 3 and s.shape[1] == self.capture_channels, s.shape
        self._ck(self.L.wf_hip_push_audio_muted(self.h, first, s.shape[0], s.ctypes.data_as(C.POINTER(C.c_float)), s.shape[2]))

    def enable_input_rms(self, feed: bool = False):
        """update_input_rms on the device from now on (cfg.normalize_volume); feed: the squared peaks come from
        push_rms_ragged_async instead of the pushed audio"""
        self._ck(self.L.wf_hip_enable_input_rms(self.h, 1 if feed else 0))

    def push_rms_ragged_async(self, pinned: "PinnedBuffer", frames, max_frames: int, slot: int, first: int = 0):
        """wf_hip_push_rms_ragged_async: pinned [count, max_frames] float32 squared peaks, frames[count] per stream"""
        f = np.ascontiguousarray(frames, dtype=np.uint32)
        self._ck(self.L.wf_hip_push_rms_ragged_async(self.h, first, len(f), C.c_void_p(pinned.ptr), f.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                      max_frames, slot))

    def input_rms(self, first: int = 0, count: int | None = None) -> np.ndarray:
        return self._read(OUT_INPUT_RMS, first, count, (), np.float32)

    def enable_loudness(self):
        """BS.1770-4 / EBU R128 loudness and true peak of every stream, measured from the next push on"""
        self._ck(self.L.wf_hip_enable_loudness(self.h, 0, self.streams))

    def reset_loudness(self, first: int = 0, count: int | None = None):
        """restarts the measurement of streams [first, first+count) (the producer must be on)"""
        count = self.streams - first if count is None else count
        if int(self.L.wf_hip_output_bytes(self.h, OUT_LOUDNESS)) == 0:
            raise WfHipError(-1, "the loudness producer is not enabled (enable_loudness)")
        self._ck(self.L.wf_hip_enable_loudness(self.h, first, count))

    def push_audio_async(self, pinned: "PinnedBuffer", count: int, frames: int, slot: int, first: int = 0):
        """pipelined ingest from page-locked memory (see wf_hip_push_audio_async); does not wait"""
        self._ck(self.L.wf_hip_push_audio_async(self.h, first, count, C.c_void_p(pinned.ptr), frames, slot))

    def read_bars_async(self, pinned: "PinnedBuffer", slot: int, first: int = 0, count: int | None = None):
        """bars of the ticks enqueued so far -> page-locked memory, without waiting (wf_hip_read_async, the bars alone)"""
        count = self.streams - first if count is None else count
        dst = Readback(bars=pinned.ptr)
        self._ck(self.L.wf_hip_read_async(self.h, first, count, C.byref(dst), slot))

    def read_async(self, slot: int, first: int = 0, count: int | None = None, **pinned: "PinnedBuffer"):
        """wf_hip_read_async without waiting: `pinned` names the destinations by Readback field (rows, last_silent, bars,
        premirror, vertices, vertex_counts, input_rms, meter); readback_done(slot) waits for them"""
        count = self.streams - first if count is None else count
        dst = Readback(**{k: v.ptr for k, v in pinned.items()})
        self._ck(self.L.wf_hip_read_async(self.h, first, count, C.byref(dst), slot))

    def readback_done(self, slot: int):
        self._ck(self.L.wf_hip_readback_done(self.h, slot))

    def ingest_done(self, slot: int):
        self._ck(self.L.wf_hip_ingest_done(self.h, slot))

    def push_audio_device(self, dev_ptr: int, count: int, frames: int, first: int = 0):
        self._ck(self.L.wf_hip_push_audio_device(self.h, first, count, C.c_void_p(dev_ptr), frames))

    def push_pcm(self, samples, *, interleaved: bool, channel_base: int = 0, frames=None, slot: int | None = None, first: int = 0,
                 wire: str | None = None):
        """wf_hip_push_pcm: a packet in its own sample format, converted and channel-picked on the device.  The format comes
        from the dtype (uint8, int16, int32, float32); shape [count, frames, channels] interleaved, [count, channels, frames]
        planar.  A numpy array is copied before the call returns; a PinnedBuffer goes through the pipelined form (`slot`,
        ingest_done); a torch tensor on the handle's device is read in place.  frames: per-stream frame counts (ragged,
        PinnedBuffer only).
        wire: None, or a wf_hip_wire_format by name ("s24", "s24_be", "s16_be", "ulaw", "alaw": packed 24-bit, big-endian and
        G.711 samples).  `samples` is then a uint8 array, PinnedBuffer or device tensor whose last axis holds the bytes of one
        sample as they lie in memory: [count, frames, channels, B] interleaved, [count, channels, frames, B] planar,
        B = WIRE_BYTES[wire]; anything else raises ValueError.  Without it nothing changes."""
        pcm, count, keep = _pcm(samples, interleaved, channel_base, frames, slot, wire)
        self._ck(self.L.wf_hip_push_pcm(self.h, first, count, C.byref(pcm)))
        del keep

    def push_audio_ragged_async(self, pinned: "PinnedBuffer", frames, max_frames: int, slot: int, first: int = 0):
        """wf_hip_push_audio_ragged_async: pinned [count, capture_channels, max_frames] float32, frames[count] per stream"""
        f = np.ascontiguousarray(frames, dtype=np.uint32)
        self._ck(self.L.wf_hip_push_audio_ragged_async(self.h, first, len(f), C.c_void_p(pinned.ptr), f.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                        max_frames, slot))

    def push_synth(self, seed: int, index0: int, frames: int, first: int = 0, count: int | None = None, stream_id0: int = 0):
        count = self.streams - first if count is None else count
        self._ck(self.L.wf_hip_push_synth(self.h, first, count, seed, stream_id0, index0, frames))

    def push_silence(self, frames: int, first: int = 0, count: int | None = None):
        count = self.streams - first if count is None else count
        self._ck(self.L.wf_hip_push_audio_muted(self.h, first, count, None, frames))  # a packet without data: zeros

    def reset(self, first: int = 0, count: int | None = None):
        count = self.streams - first if count is None else count
        self._ck(self.L.wf_hip_reset(self.h, first, count))

    # -- tick -------------------------------------------------------------------------
    def tick(self, seconds: float = 1.0 / 60.0, delay_frames: int = 0, input_rms: float = 0.0, flags: int = 0, audio_ts_ns: int = 0):
        p = TickParams(seconds, delay_frames, input_rms, flags, audio_ts_ns)
        self._ck(self.L.wf_hip_tick(self.h, C.byref(p)))

    def set_hidden(self, mask, first: int = 0):
        """mask: uint8[count]; non-zero = hidden (1) / capture timed out (2) (reset branch of tick_spectrum; tick_meter
        tells the two apart)"""
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        self._ck(self.L.wf_hip_set_hidden(self.h, first, len(m), m.ctypes.data_as(C.POINTER(C.c_uint8))))

    def set_stream_delay(self, delay_frames, first: int = 0):
        """delay_frames: uint32[count], A/V-sync delay of streams first.. in frames (added to the tick's delay_frames)"""
        d = np.ascontiguousarray(delay_frames, dtype=np.uint32)
        self._ck(self.L.wf_hip_set_stream_delay(self.h, first, len(d), d.ctypes.data_as(C.POINTER(C.c_uint32))))

    def set_stream_audio_ts(self, audio_ts_ns, first: int = 0):
        """waveform batches: m_audio_ts per stream (ns) instead of TickParams.audio_ts_ns (wf_hip_set_stream_audio_ts)"""
        d = np.ascontiguousarray(audio_ts_ns, dtype=np.uint64)
        self._ck(self.L.wf_hip_set_stream_audio_ts(self.h, first, len(d), d.ctypes.data_as(C.POINTER(C.c_uint64))))

    def set_input_rms(self, rms, first: int = 0):
        """rms: float32[count], m_input_rms of streams first.. (per-stream volume normalisation)"""
        r = np.ascontiguousarray(rms, dtype=np.float32)
        self._ck(self.L.wf_hip_set_input_rms(self.h, first, len(r), r.ctypes.data_as(C.POINTER(C.c_float))))

    def sync(self):
        self._ck(self.L.wf_hip_sync(self.h))

    def time_ticks(self, ticks: int, hop: int, first_delay: int, seconds: float = 1.0 / 60.0, flags: int = 0) -> float:
        """average fused-kernel duration in ms over `ticks` back-to-back ticks (hipEvents on the handle's stream)"""
        p = TickParams(seconds, first_delay, 0.0, flags, 0)
        ms = C.c_float(0.0)
        self._ck(self.L.wf_hip_time_ticks(self.h, C.byref(p), ticks, hop, C.byref(ms)))
        return float(ms.value)

    # -- results ------------------------------------------------------------------------
    def decibels(self, first: int = 0, count: int | None = None) -> np.ndarray:
        return self._read(OUT_DECIBELS, first, count, (self.output_channels, self.bins), np.float32)

    def _read(self, what: int, first: int, count: int | None, shape, dtype) -> np.ndarray:
        """wf_hip_read: output `what` of streams [first, first+count) as [count, *shape]"""
        count = self.streams - first if count is None else count
        out = np.empty((count,) + tuple(shape), dtype)
        per = int(self.L.wf_hip_output_bytes(self.h, what))
        assert per == 0 or per * count == out.nbytes, (what, per, out.shape)  # (0: the call below reports why the batch has none)
        self._ck(self.L.wf_hip_read(self.h, what, first, count, out.ctypes.data_as(C.c_void_p)))
        return out

    def bars(self, first: int = 0, count: int | None = None) -> np.ndarray:
        return self._read(OUT_BARS, first, count, (self.display_channels, self.num_bars), np.float32)

    def premirror(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """mirrored displays: the one value the outputs above the middle had before the mirror, [count, display_channels]"""
        return self._read(OUT_PREMIRROR, first, count, (self.display_channels,), np.float32)

    def copy_bars_to_device_async(self, dev_ptr: int, consumer_stream: int, first: int = 0, count: int | None = None):
        """the same without waiting: `consumer_stream` (a hipStream_t handle, e.g. torch.cuda.Stream.cuda_stream) is made
        to wait for the copy; the handle goes on with its next tick"""
        count = self.streams - first if count is None else count
        self._ck(self.L.wf_hip_copy_bars_device_async(self.h, first, count, C.c_void_p(dev_ptr), C.c_void_p(consumer_stream)))

    def set_bars_mirrors(self, set0, set1):
        """from the next tick on every tick also leaves the whole batch's bars in every buffer of the current write set (set0 /
        set1: sequences of up to 8 device pointers each -- buffers of [streams][display_channels][num_bars] floats owned by the
        caller); bars_mirror_ready() hands the write set over and switches to the other.  Empty sequences turn it off (the call
        waits for the ticks in flight: the old buffers may be freed afterwards).  Raises WfHipError (code -2,
        WF_HIP_ERR_UNSUPPORTED) for fft sizes that are not powers of two and for batches whose display comes from a kernel of
        its own."""
        n = len(set0)
        assert n == len(set1) and n <= 8
        a0 = (C.c_void_p * max(n, 1))(*set0)
        a1 = (C.c_void_p * max(n, 1))(*set1)
        self._ck(self.L.wf_hip_set_bars_mirrors(self.h, n, a0, a1))

    def bars_mirror_ready(self, consumer_stream: int) -> int:
        """hand-over: `consumer_stream` waits for the newest tick; returns the device pointer of buffer 0 of the set the ticks
        have written (filled from the handle's own bars if no tick has); the other set becomes the ticks' target"""
        out = C.c_void_p(0)
        self._ck(self.L.wf_hip_bars_mirror_ready(self.h, C.c_void_p(consumer_stream), C.byref(out)))
        return out.value

    def time_begin(self):
        self._ck(self.L.wf_hip_time_begin(self.h))

    def time_end(self) -> float:
        """device milliseconds since time_begin (everything the handle issued in between, on every lane)"""
        ms = C.c_float(0.0)
        self._ck(self.L.wf_hip_time_end(self.h, C.byref(ms)))
        return float(ms.value)

    def meter(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """meter batches: m_meter_val in dBFS, [count, capture_channels]"""
        count = self.streams - first if count is None else count
        return self._read(OUT_METER, first, count, (self.capture_channels,), np.float32)

    def tsmooth(self, first: int = 0, count: int | None = None) -> np.ndarray:
        return self._read(OUT_TSMOOTH, first, count, (self.capture_channels, self.bins), np.float32)

    def set_tsmooth(self, state: np.ndarray, first: int = 0):
        s = np.ascontiguousarray(state, dtype=np.float32)
        self._ck(self.L.wf_hip_write_tsmooth(self.h, first, s.shape[0], s.ctypes.data_as(C.POINTER(C.c_float))))

    def last_silent(self, first: int = 0, count: int | None = None) -> np.ndarray:
        return self._read(OUT_LAST_SILENT, first, count, (), np.uint8).astype(bool)

    def waveform_ts(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """m_waveform_ts per stream (ns) as the last enqueued tick leaves it (waveform batches)"""
        return self._read(OUT_WAVEFORM_TS, first, count, (), np.uint64)

    def decibels_device_ptr(self) -> int:
        return int(self.L.wf_hip_decibels_device(self.h) or 0)

    def vertices(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count, display_channels, num_vertices, 4]: what render_bars / render_curve hand to gs_draw (cfg.vertices)"""
        n = int(self.L.wf_hip_num_vertices(self.h))
        return self._read(OUT_VERTICES, first, count, (self.display_channels, n, 4), np.float32)

    def vertex_counts(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count, display_channels]: vertices each row's draw call uses (constant unless the bars are stepped)"""
        return self._read(OUT_VERTEX_COUNTS, first, count, (self.display_channels,), np.uint32)

    def bars_device_ptr(self) -> int:
        return int(self.L.wf_hip_bars_device(self.h) or 0)

    def stream_ptr(self) -> int:
        return int(self.L.wf_hip_stream(self.h) or 0)

    # -- tables / measurement ---------------------------------------------------------------
    def _table(self, which: int, ctype, dtype):
        p = C.c_void_p()
        n = int(self.L.wf_hip_table(self.h, which, C.byref(p)))
        return _copy(C.cast(p, C.POINTER(ctype)), n, dtype) if p.value else None

    def table_window(self):
        return self._table(TABLE_WINDOW, C.c_float, np.float32), float(self._table(TABLE_WINDOW_SUM, C.c_float, np.float32)[0])

    def table(self, name: str):
        if name == "band_widths":
            return self._table(TABLE_BAND_WIDTHS, C.c_int, np.int32)
        if name == "interp_weights":
            r, t = self._table(TABLE_INTERP_SHAPE, C.c_int, np.int32)
            return self._table(TABLE_INTERP_WEIGHTS, C.c_float, np.float32), int(r), int(t)
        which = {"slope": TABLE_SLOPE, "rolloff": TABLE_ROLLOFF, "interp_indices": TABLE_INTERP_INDICES}[name]
        return self._table(which, C.c_float, np.float32)

    def gravity(self, seconds: float) -> float:
        return float(self.L.wf_hip_gravity(self.h, seconds))

    def kernel_name(self) -> str:
        return self.L.wf_hip_kernel_name(self.h).decode()

    def launches_per_tick(self) -> int:
        return int(self.L.wf_hip_launches_per_tick(self.h))

    def algorithmic_bytes_per_tick(self, flags: int = 0) -> int:
        return int(self.L.wf_hip_algorithmic_bytes_per_tick(self.h, flags))


class PinnedBuffer:
    """page-locked host memory (wf_hip_host_alloc) viewed as a numpy array (float32 unless `dtype` says otherwise)"""

    def __init__(self, shape, dtype=np.float32):
        self.L = lib()
        dt = np.dtype(dtype)
        n = int(np.prod(shape))
        self.ptr = self.L.wf_hip_host_alloc(max(n * dt.itemsize, 1))
        if not self.ptr:
            raise MemoryError("wf_hip_host_alloc failed")
        raw = np.ctypeslib.as_array(C.cast(self.ptr, C.POINTER(C.c_uint8)), shape=(n * dt.itemsize,))
        self.array = raw.view(dt).reshape(shape)

    def close(self):
        if getattr(self, "ptr", None):
            self.array = None
            self.L.wf_hip_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiBatch(_MeasureReaders):
    """One batch of `streams` sources sharded contiguously over several devices of one node, single process, one host thread
    per device (wf_hip_multi_*); all stream indices are global.  allgather_bars() leaves every stream's bars on every device."""

    def __init__(self, cfg: Config, streams: int, devices, ring_frames: int = 0):
        self.L = lib()
        self.cfg = cfg
        devs = (C.c_int * len(devices))(*devices)
        m = C.c_void_p()
        rc = self.L.wf_hip_multi_create(C.byref(cfg), devs, len(devices), streams, ring_frames, C.byref(m))
        if rc != 0:
            raise WfHipError(rc, self.L.wf_hip_multi_last_error(None).decode())
        self.m = m
        self.streams = streams
        self.n_devices = int(self.L.wf_hip_multi_num_devices(m))
        self.transport = self.L.wf_hip_multi_transport(m).decode()
        self.transport_note = self.L.wf_hip_multi_last_error(m).decode()  # why not the transport it would have picked ("" if it did)
        self.shards = []
        for i in range(self.n_devices):
            dev, first, count = C.c_int(0), C.c_uint32(0), C.c_uint32(0)
            h = self.L.wf_hip_multi_shard(m, i, C.byref(dev), C.byref(first), C.byref(count))
            self.shards.append((C.c_void_p(h), int(dev.value), int(first.value), int(count.value)))
        h0 = self.shards[0][0]
        self.fft_size = self.L.wf_hip_fft_size(h0)
        self.bins = self.fft_size // 2
        self.capture_channels = self.L.wf_hip_capture_channels(h0)
        self.output_channels = self.L.wf_hip_output_channels(h0)
        self.display_channels = self.L.wf_hip_display_channels(h0)
        self.num_bars = self.L.wf_hip_num_bars(h0)

    def _ck(self, rc):
        if rc != 0:
            raise WfHipError(rc, self.L.wf_hip_multi_last_error(self.m).decode())

    def close(self):
        if getattr(self, "m", None):
            self.L.wf_hip_multi_destroy(self.m)
            self.m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def push_audio(self, samples: np.ndarray, first: int = 0):
        s = np.ascontiguousarray(samples, dtype=np.float32)
        assert s.ndim == 3 and s.shape[1] == self.capture_channels, s.shape
        self._ck(self.L.wf_hip_multi_push_audio(self.m, first, s.shape[0], s.ctypes.data_as(C.POINTER(C.c_float)), s.shape[2]))

    def push_pcm(self, samples, *, interleaved: bool, channel_base: int = 0, frames=None, slot: int | None = None, first: int = 0,
                 wire: str | None = None):
        """wf_hip_multi_push_pcm: SpectrumBatch.push_pcm with global stream indices (host numpy arrays only; `wire` as there:
        a uint8 array whose last axis holds a sample's bytes)"""
        if frames is not None or slot is not None or not isinstance(samples, np.ndarray):
            raise ValueError("a group takes host numpy packets without per-stream frame counts")
        pcm, count, keep = _pcm(samples, interleaved, channel_base, None, None, wire)
        self._ck(self.L.wf_hip_multi_push_pcm(self.m, first, count, C.byref(pcm)))
        del keep

    def push_synth(self, seed: int, index0: int, frames: int, first: int = 0, count: int | None = None, stream_id0: int = 0):
        count = self.streams - first if count is None else count
        self._ck(self.L.wf_hip_multi_push_synth(self.m, first, count, seed, stream_id0, index0, frames))

    def set_hidden(self, mask, first: int = 0):
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        self._ck(self.L.wf_hip_multi_set_hidden(self.m, first, len(m), m.ctypes.data_as(C.POINTER(C.c_uint8))))

    def reset(self, first: int = 0, count: int | None = None):
        count = self.streams - first if count is None else count
        self._ck(self.L.wf_hip_multi_reset(self.m, first, count))

    def tick(self, seconds: float = 1.0 / 60.0, delay_frames: int = 0, input_rms: float = 0.0, flags: int = 0):
        p = TickParams(seconds, delay_frames, input_rms, flags, 0)
        self._ck(self.L.wf_hip_multi_tick(self.m, C.byref(p)))

    def sync(self):
        self._ck(self.L.wf_hip_multi_sync(self.m))

    def _read(self, what: int, first: int, count: int | None, shape, dtype) -> np.ndarray:
        """wf_hip_multi_read: output `what` of streams [first, first+count) as [count, *shape]"""
        count = self.streams - first if count is None else count
        out = np.empty((count,) + tuple(shape), dtype)
        self._ck(self.L.wf_hip_multi_read(self.m, what, first, count, out.ctypes.data_as(C.c_void_p)))
        return out

    def decibels(self, first: int = 0, count: int | None = None) -> np.ndarray:
        return self._read(OUT_DECIBELS, first, count, (self.output_channels, self.bins), np.float32)

    def bars(self, first: int = 0, count: int | None = None) -> np.ndarray:
        return self._read(OUT_BARS, first, count, (self.display_channels, self.num_bars), np.float32)

    def _loudness_on_shards(self, first: int, count: int):
        """wf_hip_enable_loudness on every shard the global range overlaps, with local indices"""
        for h, _, s0, n in self.shards:
            lo, hi = max(first, s0), min(first + count, s0 + n)
            if lo < hi and self.L.wf_hip_enable_loudness(h, lo - s0, hi - lo) != 0:
                raise WfHipError(-1, self.L.wf_hip_last_error(h).decode())

    def enable_loudness(self):
        self._loudness_on_shards(0, self.streams)

    def reset_loudness(self, first: int = 0, count: int | None = None):
        count = self.streams - first if count is None else count
        if int(self.L.wf_hip_output_bytes(self.shards[0][0], OUT_LOUDNESS)) == 0:
            raise WfHipError(-1, "the loudness producer is not enabled (enable_loudness)")
        self._loudness_on_shards(first, count)

    def last_silent(self, first: int = 0, count: int | None = None) -> np.ndarray:
        return self._read(OUT_LAST_SILENT, first, count, (), np.uint8).astype(bool)

    def allgather_bars(self):
        """asynchronous: enqueued behind the ticks so far on every device's gather stream"""
        self._ck(self.L.wf_hip_multi_allgather_bars(self.m))

    def gathered(self, device_index: int) -> np.ndarray:
        """device `device_index`'s copy of the newest gathered result: [streams, display_channels, num_bars]"""
        out = np.empty((self.streams, self.display_channels, self.num_bars), np.float32)
        self._ck(self.L.wf_hip_multi_read_gathered(self.m, device_index, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def time_ticks(self, ticks: int, hop: int, first_delay: int, gather: bool = False, seconds: float = 1.0 / 60.0, flags: int = 0):
        """(largest per-device average device ms per tick, [per-device ms])"""
        p = TickParams(seconds, first_delay, 0.0, flags, 0)
        ms = C.c_float(0.0)
        per = (C.c_float * self.n_devices)()
        self._ck(self.L.wf_hip_multi_time_ticks(self.m, C.byref(p), ticks, hop, 1 if gather else 0, C.byref(ms), per))
        return float(ms.value), [float(x) for x in per]

    def algorithmic_bytes_per_tick(self, flags: int = 0) -> int:
        return sum(int(self.L.wf_hip_algorithmic_bytes_per_tick(h, flags)) for h, _, _, _ in self.shards)
