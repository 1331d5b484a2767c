"""Spectral peaks on the device (WF_HIP_OUT_PEAKS): exact against the float64 restatement (tests/peaks_ref.py) of the rows
decibels() returns after the same tick, over every FFT family, channel layout, window and row transform; sines against
analytic truth; empty rows; slices; refusals; nothing else moving; bars-only ticks; a three-shard group."""
import ctypes as C

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import peaks_ref as ref
from tools import synth

pytestmark = pytest.mark.gpu
ERR_INVALID = -1
SEED = 20251015


def _audio(rng, streams, channels, frames, fs, n):
    """noise under a few sines per (stream, channel) at random non-integer bins"""
    t = np.arange(frames) / fs
    x = 0.01 * rng.standard_normal((streams, channels, frames))
    for s in range(streams):
        for c in range(channels):
            for level in (-6.0, -18.0, -30.0):
                f = rng.uniform(3.0, n / 2 - 3.0) * fs / n
                x[s, c] += 10.0 ** (level / 20.0) * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
    return x.astype(np.float32)


def _check(b, rows=None, peaks=None):
    """peaks() against peaks_ref of decibels(), both read after the same tick"""
    rows = b.decibels() if rows is None else rows
    got = b.peaks() if peaks is None else peaks
    cfg = b.cfg
    count, k, hz, db = ref.peaks(rows, _floor(b), cfg.sample_rate, b.fft_size)
    assert got.shape == rows.shape[:2]
    assert np.array_equal(got["count"], count), np.argwhere(got["count"] != count)[:5]
    assert np.all(got["reserved"] == 0)
    bin_hz = cfg.sample_rate / b.fft_size
    ghz = got["peak"]["hz"].astype(np.float64)
    gdb = got["peak"]["db"].astype(np.float64)
    used = np.arange(ref.MAX_PEAKS) < count[..., None]
    # 1e-3 bin pins the bin k; the float32 result itself carries up to half an ulp of hz on top (1.3e-3 bin at 24 kHz, FFT 65536)
    tol_hz = 1e-3 * bin_hz + np.spacing(np.abs(hz).astype(np.float32)).astype(np.float64)
    bad = used & ~(np.abs(ghz - hz) <= tol_hz)
    assert not bad.any(), (np.argwhere(bad)[:5], ghz[bad][:5], hz[bad][:5], k[bad][:5])
    with np.errstate(invalid="ignore"):  # (-inf - -inf in the unused entries, checked below)
        bad = used & ~(np.abs(gdb - db) <= 1e-4)
    assert not bad.any(), (np.argwhere(bad)[:5], gdb[bad][:5], db[bad][:5])
    assert np.all(ghz[~used] == 0.0) and np.all(np.isneginf(gdb[~used]))
    return count


def _floor(b):
    return b.cfg.floor_db  # (every configuration here leaves ceiling - floor >= 1, so the batch keeps this floor)


CASES = [  # (fft, capture channels, stereo, overrides)
    (128, 2, 1, dict(window=wf.WINDOW["hann"])),
    (1024, 2, 1, dict(window=wf.WINDOW["blackman"], slope=1.0)),
    (4096, 2, 0, dict(window=wf.WINDOW["hamming"], tsmoothing=wf.TSMOOTH["exponential"], gravity=0.6)),  # mono mixdown
    (16384, 1, 0, dict(window=wf.WINDOW["blackman_harris"], rolloff_q=0.5, rolloff_rate=0.35)),           # mono capture
    (800, 2, 1, dict(window=wf.WINDOW["power_of_sine"], sine_exponent=3, normalize_volume=1, volume_target=-12.0, max_gain=20.0)),
    (4800, 2, 1, dict(window=wf.WINDOW["none"], tsmoothing=wf.TSMOOTH["tvexponential"], fast_peaks=1, slope=0.5)),
    (32768, 2, 1, dict(window=wf.WINDOW["hann"], slope=1.0, tsmoothing=wf.TSMOOTH["exponential"])),
    (65536, 2, 0, dict(window=wf.WINDOW["hann"], rolloff_q=0.6, rolloff_rate=0.5, normalize_volume=1)),
]


@pytest.mark.parametrize("fft,cap,stereo,kw", CASES, ids=[f"n{c[0]}_cap{c[1]}_st{c[2]}" for c in CASES])
def test_peaks_equal_the_reference_of_the_rows(fft, cap, stereo, kw):
    fs, streams, hop, ticks = 48000, 3, 800, 4
    cfg = wf.Config.defaults(**{**dict(fft_size=fft, sample_rate=fs, capture_channels=cap, stereo=stereo, slope=0.0, floor_db=-70), **kw})
    rng = np.random.default_rng(fft + cap)
    x = _audio(rng, streams, cap, fft + hop * ticks, fs, fft)
    with wf.SpectrumBatch(cfg, streams, ring_frames=fft + hop * ticks) as b:
        b.push_audio(np.ascontiguousarray(x[:, :, :fft]))
        for t in range(ticks):
            b.push_audio(np.ascontiguousarray(x[:, :, fft + t * hop:fft + (t + 1) * hop]))
            b.tick(input_rms=0.05)
            count = _check(b)
        assert b.peaks().shape == (streams, b.output_channels)
        assert np.all(count[:, 0] >= 3) and (not stereo or np.all(count[:, 1] >= 3)), count  # the sines at least


def test_headline_shape_every_row():
    """4096 stereo streams, FFT 4096, slope: all 8192 rows"""
    cfg = wf.Config.defaults(fft_size=4096, stereo=1, slope=1.0, bars=1, floor_db=-70)
    streams, hop = 4096, 800
    with wf.SpectrumBatch(cfg, streams, ring_frames=4096 + 2 * hop) as b:
        b.push_synth(SEED, 0, 4096 + 2 * hop)
        b.tick(delay_frames=hop)
        b.tick()
        count = _check(b)
    assert count.shape == (streams, 2) and np.all(count == ref.MAX_PEAKS)


def test_sines_against_analytic_truth():
    """Three sines at non-integer bins (Hann, no smoothing, slope 0): the float64 reference on the exact spectrum of the same
    signal lands within 0.016 bin and 0.32 dB for these cases (the parabola through dB values of a Hann main lobe), so
    0.1 bin and 0.5 dB bound the device with margin."""
    fs, n = 48000, 4096
    cfg = wf.Config.defaults(fft_size=n, sample_rate=fs, capture_channels=1, stereo=0, slope=0.0, window=wf.WINDOW["hann"],
                             tsmoothing=wf.TSMOOTH["none"], floor_db=-70)
    fracs = np.linspace(0.0, 0.95, 8)
    t = np.arange(2 * n)
    x = np.zeros((len(fracs), 1, 2 * n), np.float64)
    truth = []
    for s, frac in enumerate(fracs):
        tones = [(200.0 + frac, -6.0), (300.37 + frac / 2, -20.0), (517.71 - frac / 3, -40.0)]
        for i, (bn, lv) in enumerate(tones):
            x[s, 0] += 10.0 ** (lv / 20.0) * np.sin(2 * np.pi * bn / n * t + 0.7 * i)
        truth.append(tones)
    with wf.SpectrumBatch(cfg, len(fracs)) as b:
        b.push_audio(x.astype(np.float32))
        b.tick()
        got = b.peaks()
        _check(b, peaks=got)
    for s, tones in enumerate(truth):
        g = got[s, 0]
        assert g["count"] >= 3, g
        for j, (bn, lv) in enumerate(tones):  # strongest first: the tones in level order
            assert abs(g["peak"]["hz"][j] * n / fs - bn) < 0.1, (s, j, g["peak"][j], bn)
            assert abs(g["peak"]["db"][j] - lv) < 0.5, (s, j, g["peak"][j], lv)


def _empty(p):
    return np.all(p["count"] == 0) and np.all(p["peak"]["hz"] == 0.0) and np.all(np.isneginf(p["peak"]["db"]))


def test_silent_hidden_and_reset_streams_have_none():
    cfg = wf.Config.defaults(fft_size=1024, stereo=1, slope=1.0, floor_db=-70)
    rng = np.random.default_rng(7)
    with wf.SpectrumBatch(cfg, 4) as b:
        assert _empty(b.peaks())  # freshly created: rows at DB_MIN
        x = _audio(rng, 4, 2, 2048, 48000, 1024)
        x[0] = 0.0  # stream 0 silent
        b.push_audio(x)
        b.tick()
        p = b.peaks()
        assert _empty(p[0]) and np.all(p["count"][1:] > 0)
        b.set_hidden(np.array([0, 1, 0, 0], np.uint8))
        b.push_audio(x[:, :, :800])
        b.tick()
        p = b.peaks()
        assert _empty(p[1]) and np.all(p["count"][2:] > 0)
        b.reset(2, 1)
        p = b.peaks()
        assert _empty(p[2]) and np.all(p["count"][3] > 0)
        _check(b, peaks=p)


def test_slice_equals_the_full_read():
    cfg = wf.Config.defaults(fft_size=2048, stereo=1, slope=1.0, floor_db=-70)
    rng = np.random.default_rng(11)
    with wf.SpectrumBatch(cfg, 9) as b:
        b.push_audio(_audio(rng, 9, 2, 4096, 48000, 2048))
        b.tick()
        part = b.peaks(3, 5)  # the first read is a slice: the block is allocated whole
        full = b.peaks()
        assert part.tobytes() == full[3:8].tobytes()
        assert b.peaks(8, 1).tobytes() == full[8:].tobytes()
        _check(b, peaks=full)


def test_meter_waveform_and_null_are_refused():
    L = wf.lib()
    for kw in (dict(meter=1), dict(waveform=1, stereo=1, width=640, meter_ms=100)):
        with wf.SpectrumBatch(wf.Config.defaults(**kw), 2) as b:
            assert L.wf_hip_output_bytes(b.h, binding.OUT_PEAKS) == 0
            with pytest.raises(wf.WfHipError) as e:
                b.peaks()
            assert e.value.code == ERR_INVALID
    with wf.SpectrumBatch(wf.Config.defaults(fft_size=1024, stereo=1), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_PEAKS) == 2 * 72  # before the first read
        assert L.wf_hip_read(b.h, binding.OUT_PEAKS, 0, 1, None) == ERR_INVALID
        out = np.empty((3, 2), binding.PEAKS_DTYPE)
        assert L.wf_hip_read(b.h, binding.OUT_PEAKS, 0, 3, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID  # past the batch


def test_nothing_else_moves(monkeypatch):
    """twin handles for 50 ticks, one read every tick: decibels, bars and tsmooth stay bit-identical; guard bytes intact"""
    monkeypatch.setenv("WF_HIP_CANARY", "1")
    cfg = wf.Config.defaults(fft_size=4096, stereo=1, slope=1.0, bars=1, tsmoothing=wf.TSMOOTH["exponential"], floor_db=-70)
    streams, hop = 16, 800
    with wf.SpectrumBatch(cfg, streams) as a, wf.SpectrumBatch(cfg, streams) as b:
        for t in range(50):
            x = synth.block(SEED, 0, streams, 2, t * hop, hop)
            a.push_audio(x)
            b.push_audio(x)
            a.tick()
            b.tick()
            b.peaks()
        b.sync()
        a.sync()
        for name in ("decibels", "bars", "tsmooth"):
            assert getattr(a, name)().tobytes() == getattr(b, name)().tobytes(), name
        _check(b)


def test_bars_only_ticks_leave_the_peaks_as_stale_as_the_rows():
    cfg = wf.Config.defaults(fft_size=4096, stereo=1, slope=1.0, bars=1, floor_db=-70)
    streams, hop = 8, 800
    with wf.SpectrumBatch(cfg, streams) as b:
        for t in range(6):
            b.push_audio(synth.block(SEED, 0, streams, 2, t * hop, hop))
            b.tick(flags=0 if t < 3 else wf.TICK_NO_DECIBELS)
            _check(b)


def test_three_shards_match_one_handle():
    cfg = wf.Config.defaults(fft_size=2048, stereo=1, slope=1.0, floor_db=-70)
    streams, hop = 7, 800
    with wf.SpectrumBatch(cfg, streams) as one, wf.MultiBatch(cfg, streams, [0, 0, 0]) as m:
        for t in range(5):
            x = synth.block(SEED, 0, streams, 2, t * hop, hop)
            one.push_audio(x)
            m.push_audio(x)
            one.tick()
            m.tick()
        m.sync()
        assert m.peaks().tobytes() == one.peaks().tobytes()
        assert m.peaks(2, 4).tobytes() == one.peaks()[2:6].tobytes()
        _check(one)
