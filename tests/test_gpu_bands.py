"""Band levels on the device (WF_HIP_OUT_BANDS) against the float64 restatement (tests/bands_ref.py) of the rows decibels()
returns after the same tick, over every FFT family, channel layout, window, row transform and three sample rates; the headline
shape; sines against analytic truth; rows at DB_MIN; slices; refusals; nothing else moving; bars-only ticks; a three-shard group.

The bound against the restatement is derived, not measured (include/wf_hip.h, "determinism"): both sides work in float64 from the
same float32 row and differ in exp10 and in the order of at most 32768 positive additions, below 2e-11 dB before the one
rounding to float32.  So |got - want| <= max(1 float32 ulp of want, 1e-9 dB), -INFINITY exactly where the restatement has it,
`covered` and `reserved` equal (bands_ref.mismatches)."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import bands_ref as ref
from test_gpu_peaks import CASES, _audio
from tools import synth
from measure_common import check_abi_refusals

pytestmark = pytest.mark.gpu
ERR_INVALID = -1
SEED = 20251015


def _check(b, rows=None, bands=None):
    """bands() against bands_ref of decibels(), both read after the same tick"""
    rows = b.decibels() if rows is None else rows
    got = b.bands() if bands is None else bands
    want = ref.bands(rows, b.table_window()[0], b.cfg.sample_rate, b.fft_size)
    assert got.shape == rows.shape[:2] and got.dtype == binding.BANDS_DTYPE
    worst = 0
    for name in ("band_db", "total_db", "a_db", "c_db"):
        fin = np.isfinite(want[name])
        if fin.any():
            worst = max(worst, int(ref.ulps(got[name][fin], want[name][fin]).max()))
    print(f"fft {b.fft_size} sr {b.cfg.sample_rate}: {rows.shape[0] * rows.shape[1]} rows, worst distance {worst} float32 ulp, "
          f"covered {int(want['covered'].flat[0]):#010x}")
    bad = ref.mismatches(got, want)
    assert not bad, bad[:8]
    return got


@pytest.mark.parametrize("sr", [48000, 44100, 96000])
@pytest.mark.parametrize("fft,cap,stereo,kw", CASES, ids=[f"n{c[0]}_cap{c[1]}_st{c[2]}" for c in CASES])
def test_bands_equal_the_reference_of_the_rows(fft, cap, stereo, kw, sr):
    streams, hop, ticks = 3, 800, 4
    cfg = wf.Config.defaults(**{**dict(fft_size=fft, sample_rate=sr, capture_channels=cap, stereo=stereo, slope=0.0, floor_db=-70), **kw})
    rng = np.random.default_rng(fft + cap)
    x = _audio(rng, streams, cap, fft + hop * ticks, sr, fft)
    with wf.SpectrumBatch(cfg, streams, ring_frames=fft + hop * ticks) as b:
        b.push_audio(np.ascontiguousarray(x[:, :, :fft]))
        for t in range(ticks):
            b.push_audio(np.ascontiguousarray(x[:, :, fft + t * hop:fft + (t + 1) * hop]))
            b.tick(input_rms=0.05)
            got = _check(b)
        assert got.shape == (streams, b.output_channels)
        assert np.all(got["covered"] == ref.covered(sr, fft))
        # (a mono mixdown of two captured channels leaves its second row at DB_MIN: -INFINITY there, as the restatement has it)
        live = slice(None) if stereo or cap == 1 else 0
        assert np.all(np.isfinite(got["total_db"][:, live]))


def test_headline_shape_every_row():
    """4096 stereo streams, FFT 4096, slope: all 8192 rows"""
    cfg = wf.Config.defaults(fft_size=4096, stereo=1, slope=1.0, bars=1, floor_db=-70)
    streams, hop = 4096, 800
    with wf.SpectrumBatch(cfg, streams, ring_frames=4096 + 2 * hop) as b:
        b.push_synth(SEED, 0, 4096 + 2 * hop)
        b.tick(delay_frames=hop)
        b.tick()
        got = _check(b)
    assert got.shape == (streams, 2) and np.all(got["covered"] == 0x7fffffff) and np.all(np.isfinite(got["band_db"]))


def test_sines_against_analytic_truth():
    """Hann, no smoothing, slope 0, N = 4096, 48 kHz, one sine of amplitude 0.5 per stream at bins 85.0, 85.37, 200.5 and
    1000.25 (each at least three bins inside its band: 17, 17, 21, 28).  The restatement on the exact spectrum reads total_db and
    the sine's band = 20 log10(0.5) within 2e-6 dB whatever the offset between bins, and a_db - total_db = -0.012, +0.001,
    +1.265, -3.702 dB (tests/test_bands_cpu.py); 0.01 dB covers the tick's float32 transform with a wide margin."""
    fs, n, amp = 48000, 4096, 0.5
    bins, holds = (85.0, 85.37, 200.5, 1000.25), (17, 17, 21, 28)
    cfg = wf.Config.defaults(fft_size=n, sample_rate=fs, capture_channels=1, stereo=0, slope=0.0, window=wf.WINDOW["hann"],
                             tsmoothing=wf.TSMOOTH["none"], floor_db=-70)
    t = np.arange(2 * n)
    x = np.stack([amp * np.sin(2 * np.pi * bn / n * t + 0.3) for bn in bins])[:, None, :]
    with wf.SpectrumBatch(cfg, len(bins)) as b:
        b.push_audio(x.astype(np.float32))
        b.tick()
        got = _check(b)
    truth = 20.0 * np.log10(amp)
    for s, (bn, band) in enumerate(zip(bins, holds)):
        g = got[s, 0]
        f = bn * fs / n
        da, dc = 10.0 * np.log10(ref.a_weight(f)), 10.0 * np.log10(ref.c_weight(f))
        print(f"bin {bn}: total {g['total_db']:.5f} band {g['band_db'][band]:.5f} a-total {g['a_db'] - g['total_db']:.5f} ({da:.5f}) "
              f"c-total {g['c_db'] - g['total_db']:.5f} ({dc:.5f})")
        assert abs(g["total_db"] - truth) < 0.01 and abs(g["band_db"][band] - truth) < 0.01, (bn, g)
        assert abs((g["a_db"] - g["total_db"]) - da) < 0.01 and abs((g["c_db"] - g["total_db"]) - dc) < 0.01, (bn, g)
        assert np.argmax(g["band_db"]) == band


def _empty(p, covered):
    return (np.all(np.isneginf(p["band_db"])) and np.all(np.isneginf(p["total_db"])) and np.all(np.isneginf(p["a_db"]))
            and np.all(np.isneginf(p["c_db"])) and np.all(p["covered"] == covered) and np.all(p["reserved"] == 0))


def test_rows_at_db_min_read_minus_infinity():
    cfg = wf.Config.defaults(fft_size=1024, stereo=1, slope=1.0, floor_db=-70)
    cov = ref.covered(cfg.sample_rate, 1024)
    rng = np.random.default_rng(7)
    with wf.SpectrumBatch(cfg, 4) as b:
        assert cov != 0 and _empty(b.bands(), cov)  # freshly created: rows at DB_MIN
        x = _audio(rng, 4, 2, 2048, 48000, 1024)
        b.push_audio(x)
        b.tick()
        p = b.bands()
        assert np.all(np.isfinite(p["total_db"]))
        b.set_hidden(np.array([0, 1, 0, 0], np.uint8))
        b.push_audio(x[:, :, :800])
        b.tick()
        p = b.bands()
        assert _empty(p[1], cov) and np.all(np.isfinite(p["total_db"][[0, 2, 3]]))
        b.reset(2, 1)
        p = b.bands()
        assert _empty(p[2], cov) and np.all(np.isfinite(p["total_db"][[0, 3]]))
        _check(b, bands=p)


def test_slice_equals_the_full_read():
    cfg = wf.Config.defaults(fft_size=2048, stereo=1, slope=1.0, floor_db=-70)
    rng = np.random.default_rng(11)
    with wf.SpectrumBatch(cfg, 9) as b:
        b.push_audio(_audio(rng, 9, 2, 4096, 48000, 2048))
        b.tick()
        part = b.bands(3, 5)  # the first read is a slice: the block is allocated whole
        full = b.bands()
        assert part.tobytes() == full[3:8].tobytes()
        assert b.bands(8, 1).tobytes() == full[8:].tobytes()
        assert b.bands().tobytes() == full.tobytes()  # the same rows read bit-identically
        _check(b, bands=full)


def test_meter_waveform_and_bad_arguments_are_refused():
    L = wf.lib()
    for kw in (dict(meter=1), dict(waveform=1, stereo=1, width=640, meter_ms=100)):
        with wf.SpectrumBatch(wf.Config.defaults(**kw), 2) as b:
            assert L.wf_hip_output_bytes(b.h, binding.OUT_BANDS) == 0
            with pytest.raises(wf.WfHipError) as e:
                b.bands()
            assert e.value.code == ERR_INVALID and "band levels" in str(e.value)
    with wf.SpectrumBatch(wf.Config.defaults(fft_size=1024, stereo=1), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_BANDS) == 2 * 144  # before the first read
        check_abi_refusals(b, binding.OUT_BANDS, np.dtype((binding.BANDS_DTYPE, (2,))), 2)  # (an entry is both channels' rows)


def test_nothing_else_moves(monkeypatch):
    """twin handles for 50 ticks, one read every tick: every other output stays bit-identical; guard bytes intact"""
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
            b.bands()
        b.sync()
        a.sync()
        for name in ("decibels", "bars", "tsmooth", "last_silent", "peaks", "signal", "pitch"):
            assert np.asarray(getattr(a, name)()).tobytes() == np.asarray(getattr(b, name)()).tobytes(), name
        first = b.bands()
        assert b.bands().tobytes() == first.tobytes()
        assert a.bands().tobytes() == first.tobytes()  # a handle's first read equals another's fifty-first
        _check(b, bands=first)


def test_bars_only_ticks_leave_the_bands_as_stale_as_the_rows():
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
        assert m.bands().tobytes() == one.bands().tobytes()
        assert m.bands(2, 4).tobytes() == one.bands()[2:6].tobytes()  # a range that spans the shards
        _check(one)


def test_device_memory_path():
    """rows of audio pushed from a torch tensor in place: a fresh child process (torch brings its own HIP runtime)"""
    child = Path(__file__).resolve().parent / "bands_device_child.py"
    r = subprocess.run([sys.executable, str(child)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bands device ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
