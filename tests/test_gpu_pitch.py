"""Pitch on the device (WF_HIP_OUT_PITCH): analytic cases through real pushes, a fuzz against the float64 restatement
(tests/pitch_ref.py) of the frames pushed -- the scripts of tests/pitch_cases.py: windows not yet filled, ragged pushes,
packets longer than the ring, a reset in the middle, every FFT family (P < W among them), ring capacities, meter batches --,
determinism, every push path, nothing else moving, slices, refusals, a three-shard group and the headline shape.

The device is compared with the reference only, never with the truth.  Per stream: if the reference's two orders of addition
agree (well conditioned), lag and voiced are equal and hz, clarity within 2 float32 ulps; otherwise the stream is left out
and counted, at most 0.5 % of the streams of a test.  tests/test_pitch_cpu.py shows that the committed seeds leave out none."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import pitch_cases as cases
import pitch_ref as ref
from signal_ref import History
from pcm_convert import captured, random_packet
from tools import synth

pytestmark = pytest.mark.gpu
ERR_INVALID = -1
SR = cases.SR


def _cfg(fft=4096, cap=2, **kw):
    return wf.Config.defaults(**{**dict(fft_size=fft, sample_rate=SR, capture_channels=cap, stereo=1 if cap == 2 else 0, slope=1.0,
                                        bars=1, floor_db=-70), **kw})


class Tally:
    """streams compared and streams left out over one test"""

    def __init__(self):
        self.streams = self.skipped = 0

    def check(self, got, window, what=""):
        want, well = ref.evaluate(window, SR)
        bad, skipped = ref.compare(got, want, well)
        self.streams += len(got)
        self.skipped += skipped
        assert len(bad) == 0, (what, bad, got[bad], want[bad])
        return want

    def close(self):
        print(f"pitch: {self.streams} streams compared, {self.skipped} skipped")
        assert self.skipped <= 0.005 * self.streams, (self.skipped, self.streams)


# ---- analytic cases --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [1, 2])
def test_analytic_cases_through_pushes(cap):
    P = 4096
    c = cases.analytic(P)
    names = list(c)
    mono = np.stack([c[k] for k in names])
    if cap == 1:
        x = mono[:, None]
    else:  # the second channel: the same tone quieter, so the mix keeps the pitch
        x = np.stack([mono, (0.5 * mono).astype(np.float32)], axis=1)
        x = np.concatenate([x, np.stack([c["sine440"], -c["sine440"]])[None]])  # l = -r: nothing to report
        names.append("inverted")
    tally = Tally()
    with wf.SpectrumBatch(_cfg(P, cap), len(x)) as b:
        b.push_audio(x)
        got = b.pitch()
    tally.check(got, x, names)
    tally.close()
    g = dict(zip(names, got))
    for hz, lag in ((55.0, 873), (110.0, 436), (440.0, 109), (997.3, 48), (3000.0, 16)):
        r = g[f"sine{hz:g}"]
        assert r["voiced"] == 1 and r["lag"] == lag and r["clarity"] > 0.99, (hz, r)
    assert g["sine3000"]["clarity"] == 1.0  # a period of whole frames: d(16) is exactly 0
    assert g["missing_fundamental"]["lag"] == 218 and g["missing_fundamental"]["voiced"] == 1
    assert g["noise"]["voiced"] == 0
    zero = np.zeros(1, binding.PITCH_DTYPE)[0]
    for k in ("silence", "constant") + (("inverted",) if cap == 2 else ()):
        assert g[k] == zero, (k, g[k])


# ---- fuzz against the reference ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fft,cap,kw,ring", cases.FUZZ, ids=cases.FUZZ_IDS)
def test_fuzz_against_the_reference(fft, cap, kw, ring):
    streams = cases.FUZZ_STREAMS
    steps = cases.fuzz_script(fft, cap, kw, ring)
    tally = Tally()
    with wf.SpectrumBatch(_cfg(fft, cap, **kw), streams, ring_frames=ring) as b:
        assert b.fft_size == fft and b.ring_frames == cases.ring_capacity(fft, ring)
        hist = History(streams, cap, ref.window_frames(fft))

        def on_read(i):
            tally.check(b.pitch(), hist.window(), f"read {i}")
            if i % 3 == 2:
                assert b.pitch(1, 2).tobytes() == b.pitch()[1:3].tobytes()
        assert cases.replay(steps, hist, on_read, b, lambda shape: wf.PinnedBuffer(shape)) == 9
    tally.close()


# ---- determinism ------------------------------------------------------------------------------------------------------------

def test_reads_repeat_and_packet_sizes_do_not_matter():
    streams, cap, total = 8, 2, 9000
    x = cases.bank(5, streams, cap, total)
    with wf.SpectrumBatch(_cfg(4096), streams) as a, wf.SpectrumBatch(_cfg(4096), streams) as b:
        a.push_audio(x)
        rng = np.random.default_rng(6)
        at = 0
        while at < total:
            n = min(int(rng.integers(1, 700)), total - at)
            b.push_audio(x[:, :, at:at + n])
            at += n
        first = a.pitch()
        assert a.pitch().tobytes() == first.tobytes()
        a.tick()
        assert a.pitch().tobytes() == first.tobytes()  # a tick does not move the rings
        assert b.pitch().tobytes() == first.tobytes()
    assert first["voiced"].any() and not first["voiced"].all()


# ---- every push path, nothing else moving -----------------------------------------------------------------------------------

def test_push_paths_match_a_twin_fed_float32():
    streams, cap, frames, W = 5, 2, 800, 1024
    rng = np.random.default_rng(3)

    def twin_of(feed, cfg=None):
        cfg = cfg or _cfg(W)
        with wf.SpectrumBatch(cfg, streams) as b, wf.SpectrumBatch(cfg, streams) as twin:
            for pkts in feed(b):
                for p in pkts:
                    twin.push_audio(p)
            b.sync()
            got, want = b.pitch(), twin.pitch()
        assert got.tobytes() == want.tobytes(), (feed.__name__, got, want)
        assert got["lag"].any(), feed.__name__
        return got

    def feed_blocking(b):
        p = cases.bank(1, streams, cap, 3000)
        b.push_audio(p)
        return [[p[:, :, :1234], p[:, :, 1234:]]]
    got = twin_of(feed_blocking)
    assert got["voiced"].any()

    def feed_async(b):
        pin = [wf.PinnedBuffer((streams, cap, frames)), wf.PinnedBuffer((streams, cap, frames))]
        src = cases.bank(2, streams, cap, 4 * frames)
        out = []
        for t in range(4):
            b.ingest_done(t & 1)
            pin[t & 1].array[...] = src[:, :, t * frames:(t + 1) * frames]
            b.push_audio_async(pin[t & 1], streams, frames, t & 1)
            out.append([pin[t & 1].array.copy()])
        b.sync()
        for p in pin:
            p.close()
        return out
    twin_of(feed_async)

    # ragged from pinned memory against per-stream pushes
    with wf.SpectrumBatch(_cfg(W), streams) as b, wf.SpectrumBatch(_cfg(W), streams) as twin:
        pin = wf.PinnedBuffer((streams, cap, frames))
        src = cases.bank(4, streams, cap, frames)
        counts = rng.integers(frames // 2, frames + 1, streams).astype(np.uint32)
        b.ingest_done(0)
        pin.array[...] = src
        b.push_audio_ragged_async(pin, counts, frames, 0)
        b.sync()
        pin.close()
        for s in range(streams):
            twin.push_audio(src[s:s + 1, :, :counts[s]], first=s)
        assert b.pitch().tobytes() == twin.pitch().tobytes() and b.pitch()["lag"].all()

    def feed_muted(b):
        out = []
        for _ in range(2):
            p = rng.uniform(-1, 1, (streams, cap, frames)).astype(np.float32)
            b.push_audio(p)
            b.push_audio_muted(p[:, :, :100])
            out.append([p, np.zeros_like(p[:, :, :100])])
        return out
    twin_of(feed_muted)

    def feed_synth(b):
        out = []
        for t in range(3):
            b.push_synth(synth.DEFAULT_SEED, t * frames, frames)
            out.append([synth.block(synth.DEFAULT_SEED, 0, streams, cap, t * frames, frames)])
        return out
    twin_of(feed_synth)

    def feed_pcm_s16(b):
        out = []
        for _ in range(2):
            pkt = random_packet(rng, np.int16, streams, cap, frames + 3, True)
            b.push_pcm(pkt, interleaved=True)
            out.append([captured(pkt, True, 0, cap)])
        return out
    twin_of(feed_pcm_s16)


def test_device_memory_path():
    """wf_hip_push_audio_device in a child process (torch brings its own HIP runtime and has to be imported before
    libwaveform_hip.so is loaded)"""
    pytest.importorskip("torch")
    child = Path(__file__).resolve().parent / "pitch_device_child.py"
    r = subprocess.run([sys.executable, str(child)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "pitch device ok" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


def test_nothing_else_moves(monkeypatch):
    """twin handles for 20 ticks, one of them read every tick: rows, bars, signal statistics, peaks and loudness stay
    bit-identical, before and after a read and against the twin that never read the pitch; guard bytes intact"""
    monkeypatch.setenv("WF_HIP_CANARY", "1")
    cfg = _cfg(4096, tsmoothing=wf.TSMOOTH["exponential"])
    streams, hop = 16, 800
    names = ("decibels", "bars", "tsmooth", "peaks", "signal", "loudness", "last_silent")
    tally = Tally()
    with wf.SpectrumBatch(cfg, streams) as a, wf.SpectrumBatch(cfg, streams) as b:
        a.enable_loudness()
        b.enable_loudness()
        hist = History(streams, 2, 4096)
        for t in range(20):
            x = synth.block(cases.SEED, 0, streams, 2, t * hop, hop)
            a.push_audio(x)
            b.push_audio(x)
            hist.push(x)
            a.tick()
            b.tick()
            if t in (0, 7, 19):
                before = {n: getattr(b, n)().tobytes() for n in names}
                tally.check(b.pitch(), hist.window(), f"tick {t}")
                for n in names:
                    assert getattr(b, n)().tobytes() == before[n], (t, n)
            else:
                b.pitch()
        b.sync()
        a.sync()
        for n in names:
            assert getattr(a, n)().tobytes() == getattr(b, n)().tobytes(), n
        b.sync()
    tally.close()


# ---- slices, refusals, groups -------------------------------------------------------------------------------------------------

def test_slices_and_refusals(monkeypatch):
    monkeypatch.setenv("WF_HIP_CANARY", "1")
    L = wf.lib()
    with wf.SpectrumBatch(_cfg(2048), 9) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_PITCH) == 16  # before the first read
        b.push_audio(cases.bank(9, 9, 2, 3001))
        part = b.pitch(3, 5)  # the first read is a slice: the block is allocated whole
        full = b.pitch()
        assert part.tobytes() == full[3:8].tobytes()
        assert b.pitch(8, 1).tobytes() == full[8:].tobytes()
        assert full["lag"].all()
        assert L.wf_hip_read(b.h, binding.OUT_PITCH, 0, 1, None) == ERR_INVALID
        out = np.empty(10, binding.PITCH_DTYPE)
        assert L.wf_hip_read(b.h, binding.OUT_PITCH, 0, 10, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID  # past the batch
        assert L.wf_hip_read(b.h, binding.OUT_PITCH, 9, 1, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID
        assert L.wf_hip_read(b.h, binding.OUT_PITCH, 0, 0, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID
        b.sync()  # (checks the guard bytes)
    with wf.SpectrumBatch(wf.Config.defaults(waveform=1, stereo=1, width=640, meter_ms=100), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_PITCH) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.pitch()
        assert e.value.code == ERR_INVALID
    with wf.SpectrumBatch(_cfg(1024, meter=1, bars=0, meter_ms=1), 2) as b:  # a meter buffer of 48 frames: under 64
        assert b.fft_size == 48 and L.wf_hip_output_bytes(b.h, binding.OUT_PITCH) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.pitch()
        assert e.value.code == ERR_INVALID
        assert L.wf_hip_output_bytes(b.h, binding.OUT_SIGNAL) == 48  # (the signal statistics have no such floor)


def test_three_shards_match_one_handle():
    cfg = _cfg(2048)
    streams, total = 7, 4005
    x = cases.bank(12, streams, 2, total)
    with wf.SpectrumBatch(cfg, streams) as one, wf.MultiBatch(cfg, streams, [0, 0, 0]) as m:
        for t in range(5):
            p = x[:, :, t * 801:(t + 1) * 801]
            one.push_audio(p)
            m.push_audio(p)
            one.tick()
            m.tick()
        m.sync()
        assert m.pitch().tobytes() == one.pitch().tobytes()
        assert m.pitch(2, 4).tobytes() == one.pitch()[2:6].tobytes()
        assert m.pitch().shape == (streams,) and m.pitch()["lag"].all()


def test_headline_shape():
    """all 4096 stereo streams at FFT 4096, the window wrapping round the ring at an odd offset; the first and the last 32
    streams against the reference"""
    streams, n = 4096, 4096
    with wf.SpectrumBatch(_cfg(n), streams) as b:
        b.push_synth(cases.SEED, 0, n + 800)
        b.tick()
        b.push_synth(cases.SEED, n + 800, 801)
        got = b.pitch()
    assert got.shape == (streams,)
    idx = list(range(32)) + list(range(streams - 32, streams))
    w = np.concatenate([synth.block(cases.SEED, s, 1, 2, 1601, n) for s in idx])  # frames [5697 - 4096, 5697)
    tally = Tally()
    tally.check(got[idx], w)
    tally.close()
    assert got["lag"].all()
