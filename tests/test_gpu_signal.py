"""Signal statistics on the device (WF_HIP_OUT_SIGNAL): analytic cases (integer-period sines, DC, polarity inversion, a dead
channel, full scale in float and integer PCM), a fuzz against the float64 restatement (tests/signal_ref.py) of the frames
pushed -- ragged hops, packets longer than the ring, windows not yet filled after create and after a reset, reads between
ticks, every FFT family, mono and stereo capture, meter batches --, bit identity across every push path, nothing else moving,
slices, refusals, repeated reads, a three-shard group and the headline shape."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import signal_ref as ref
from pcm_convert import captured, random_packet
from tools import synth

pytestmark = pytest.mark.gpu
ERR_INVALID = -1
SEED = 20251016


def _cfg(fft=4096, cap=2, **kw):
    return wf.Config.defaults(**{**dict(fft_size=fft, sample_rate=48000, capture_channels=cap, stereo=1 if cap == 2 else 0, slope=1.0,
                                        bars=1, floor_db=-70), **kw})


def _check(got, want, what=""):
    """got: SIGNAL_DTYPE [streams]; want: ref.signal(...); the bound is signal_ref.mismatches'"""
    bad = ref.mismatches(got, want)
    assert not bad, (what, bad[:8])


def _sig_of(b, hist):
    got = b.signal()
    _check(got, ref.signal(hist.window()))
    return got


# ---- analytic cases --------------------------------------------------------------------------------------------------------

def test_integer_period_sines_dc_inversion_and_a_dead_channel():
    W = 4096
    n = np.arange(W)
    a, bb = 0.5, 0.25
    l = (a * np.sin(2 * np.pi * 5 * n / W)).astype(np.float32)
    r = (bb * np.sin(2 * np.pi * 11 * n / W + 0.3)).astype(np.float32)
    cases = [np.stack([l, r]),                                     # two sines at different whole periods: uncorrelated
             np.stack([np.full(W, 0.25, np.float32), np.full(W, -0.5, np.float32)]),  # DC
             np.stack([l, -l]),                                    # polarity inversion
             np.stack([l, np.zeros(W, np.float32)]),               # right channel dead
             np.stack([l, l])]                                     # identical
    x = np.stack(cases)
    with wf.SpectrumBatch(_cfg(W), len(cases)) as b:
        b.push_audio(x)
        got = b.signal()
    _check(got, ref.signal(x))
    g = got
    assert abs(g["ch"]["rms_db"][0, 0] - (20 * np.log10(a) - 3.0103)) < 1e-4
    assert abs(g["ch"]["rms_db"][0, 1] - (20 * np.log10(bb) - 3.0103)) < 1e-4
    assert abs(g["correlation"][0]) < 1e-6 and abs(g["ch"]["dc"][0, 0]) < 1e-7
    assert abs(g["balance_db"][0] - 20 * np.log10(bb / a)) < 1e-4
    assert g["ch"]["dc"][1, 0] == 0.25 and g["ch"]["dc"][1, 1] == -0.5 and g["correlation"][1] == -1.0
    assert g["ch"]["peak_db"][1, 0] == np.float32(20 * np.log10(0.25))
    assert g["correlation"][2] == -1.0 and np.isneginf(g["mid_db"][2]) and g["balance_db"][2] == 0.0
    assert g["side_db"][2] == g["ch"]["rms_db"][2, 0]
    assert g["correlation"][3] == 0.0 and g["balance_db"][3] == -np.inf
    assert np.isneginf(g["ch"]["rms_db"][3, 1]) and np.isneginf(g["ch"]["peak_db"][3, 1]) and g["ch"]["dc"][3, 1] == 0.0
    assert g["correlation"][4] == 1.0 and np.isneginf(g["side_db"][4]) and g["balance_db"][4] == 0.0
    assert np.all(g["ch"]["clipped"] == 0)


def test_full_scale_in_float_and_integer_pcm():
    W = 1024
    with wf.SpectrumBatch(_cfg(W), 1) as b:
        sq = np.where(np.arange(W) % 2 == 0, 1.0, -1.0).astype(np.float32)
        b.push_audio(np.stack([sq, -sq])[None])
        g = b.signal()[0]
        assert np.all(g["ch"]["clipped"] == W) and np.all(g["ch"]["peak_db"] == 0.0) and np.all(g["ch"]["rms_db"] == 0.0)
        assert g["correlation"] == -1.0 and np.isneginf(g["mid_db"]) and g["side_db"] == 0.0
        # the integer formats: alternating extremes, interleaved [1, frames, 2]
        for dtype, lo, hi, clipped in ((np.int16, -32768, 32767, W),           # 32767/32768 is the threshold itself
                                       (np.int32, -2 ** 31, 2 ** 31 - 1, W),   # (float)(2^31 - 1) rounds to 2^31: 1.0
                                       (np.uint8, 0, 255, W // 2)):            # 127/128 stays below it
            pkt = np.empty((1, W, 2), dtype)
            pkt[0, 0::2, :] = hi
            pkt[0, 1::2, :] = lo
            b.push_pcm(pkt, interleaved=True)
            g = b.signal()[0]
            assert np.all(g["ch"]["clipped"] == clipped), (dtype, g)
            want = ref.signal(captured(pkt, True, 0, 2))
            _check(b.signal(), want, str(dtype))


# ---- fuzz against the reference ----------------------------------------------------------------------------------------------

FUZZ = [  # (fft, capture channels, overrides)
    (128, 2, {}), (800, 2, {}), (800, 1, {}), (4096, 2, {}), (16384, 1, {}), (48000, 2, dict(stereo=0)), (65536, 2, {}),
    (1024, 2, dict(meter=1, bars=0)), (1024, 1, dict(meter=1, bars=0, meter_rms=1)),
]


@pytest.mark.parametrize("fft,cap,kw", FUZZ, ids=[f"n{f}_cap{c}" + ("_meter" if k.get("meter") else "") for f, c, k in FUZZ])
def test_fuzz_against_the_reference(fft, cap, kw):
    rng = np.random.default_rng(fft * 3 + cap + (7 if kw.get("meter") else 0))
    streams = 5
    with wf.SpectrumBatch(_cfg(fft, cap, **kw), streams) as b:
        W, ring = b.fft_size, b.ring_frames
        hist = ref.History(streams, cap, W)
        _sig_of(b, hist)  # freshly created: zeros
        pin = [wf.PinnedBuffer((streams, cap, W + 3)), wf.PinnedBuffer((streams, cap, W + 3))]
        try:
            for step in range(14):
                kind = rng.integers(0, 4) if step else 0
                scale = float(rng.choice([0.01, 0.5, 1.0, 1.2]))
                if step == 6:  # a packet longer than the ring: only its newest frames survive
                    n = ring + int(rng.integers(1, 300))
                    x = rng.uniform(-scale, scale, (streams, cap, n)).astype(np.float32)
                    b.push_audio(x)
                    hist.push(x)
                elif step == 9:  # reset of a slice: its window is zeros again, filled partially by the next push
                    b.reset(1, 2)
                    hist.reset(1, 2)
                    x = rng.uniform(-scale, scale, (streams, cap, int(rng.integers(1, W // 2 + 1)))).astype(np.float32)
                    b.push_audio(x)
                    hist.push(x)
                elif kind == 0:  # one packet for every stream, any length (a partial window after create: step 0)
                    n = int(rng.integers(1, min(W // 3, 4000) + 1)) if step == 0 else int(rng.integers(1, 2 * W + 1))
                    x = rng.uniform(-scale, scale, (streams, cap, n)).astype(np.float32)
                    b.push_audio(x)
                    hist.push(x)
                elif kind == 1:  # ragged: every stream its own count, through the pinned slot
                    slot = step & 1
                    b.ingest_done(slot)
                    frames = rng.integers(0, W + 4, streams).astype(np.uint32)
                    pin[slot].array[...] = rng.uniform(-scale, scale, (streams, cap, W + 3)).astype(np.float32)
                    b.push_audio_ragged_async(pin[slot], frames, W + 3, slot)
                    hist.push(pin[slot].array.copy(), frames=frames)
                    b.sync()
                elif kind == 2:  # small odd hops to one slice of streams
                    for _ in range(3):
                        f0 = int(rng.integers(0, streams))
                        x = rng.uniform(-scale, scale, (streams - f0, cap, int(rng.integers(1, 8)))).astype(np.float32)
                        b.push_audio(x, first=f0)
                        hist.push(x, first=f0)
                else:  # a tick: the rings do not move
                    b.tick()
                _sig_of(b, hist)
                if step % 4 == 3:
                    b.tick()
                    _check(b.signal(1, 3), {k: v[1:4] for k, v in ref.signal(hist.window()).items()}, "slice after a tick")
        finally:
            for p in pin:
                p.close()


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
            got, want = b.signal(), twin.signal()
        assert got.tobytes() == want.tobytes(), (feed.__name__, got, want)
        return got

    def feed_async(b):
        pin = [wf.PinnedBuffer((streams, cap, frames)), wf.PinnedBuffer((streams, cap, frames))]
        out = []
        for t in range(4):
            b.ingest_done(t & 1)
            pin[t & 1].array[...] = rng.uniform(-1, 1, (streams, cap, frames)).astype(np.float32)
            b.push_audio_async(pin[t & 1], streams, frames, t & 1)
            out.append([pin[t & 1].array.copy()])
        b.sync()
        for p in pin:
            p.close()
        return out
    twin_of(feed_async)

    def feed_muted(b):
        out = []
        for _ in range(2):
            p = rng.uniform(-1, 1, (streams, cap, frames)).astype(np.float32)
            b.push_audio(p)
            b.push_audio_muted(p)
            out.append([p, np.zeros_like(p)])
        return out
    twin_of(feed_muted)

    def feed_synth(b):
        out = []
        for t in range(3):
            b.push_synth(synth.DEFAULT_SEED, t * frames, frames)
            out.append([synth.block(synth.DEFAULT_SEED, 0, streams, cap, t * frames, frames)])
        return out
    twin_of(feed_synth)

    for dtype in (np.uint8, np.int16, np.int32, np.float32):
        for inter in (True, False):
            def feed_pcm(b, dtype=dtype, inter=inter):
                out = []
                for _ in range(2):
                    pkt = random_packet(rng, dtype, streams, 3, frames + 3, inter)  # three channels, capture 0 and 1
                    b.push_pcm(pkt, interleaved=inter)
                    out.append([captured(pkt, inter, 0, cap)])
                return out
            twin_of(feed_pcm)

    # push_pcm ragged from pinned memory against per-stream float32 pushes
    with wf.SpectrumBatch(_cfg(W), streams) as b, wf.SpectrumBatch(_cfg(W), streams) as twin:
        pin = wf.PinnedBuffer((streams, frames, cap), np.int16)
        for slot in (0, 1, 0):
            b.ingest_done(slot)
            pin.array[...] = random_packet(rng, np.int16, streams, cap, frames, True)
            counts = rng.integers(0, frames + 1, streams).astype(np.uint32)
            b.push_pcm(pin, interleaved=True, frames=counts, slot=slot)
            b.sync()
            conv = captured(pin.array, True, 0, cap)
            for s in range(streams):
                if counts[s]:
                    twin.push_audio(conv[s:s + 1, :, :counts[s]], first=s)
        pin.close()
        assert b.signal().tobytes() == twin.signal().tobytes()

    # a meter batch reads what a spectrum batch does
    def feed_audio(b):
        p = rng.uniform(-1, 1, (streams, cap, 3000)).astype(np.float32)
        b.push_audio(p)
        return [[p]]
    twin_of(feed_audio, _cfg(W, meter=1, bars=0))


def test_device_memory_paths():
    """_device and push_pcm from device memory, in a child process (torch brings its own HIP runtime and has to be imported
    before libwaveform_hip.so is loaded)"""
    pytest.importorskip("torch")
    child = Path(__file__).resolve().parent / "signal_device_child.py"
    r = subprocess.run([sys.executable, str(child)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "signal device ok" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


def test_nothing_else_moves(monkeypatch):
    """twin handles for 30 ticks, one of them read every tick: decibels, bars, peaks and loudness stay bit-identical; guard
    bytes intact"""
    monkeypatch.setenv("WF_HIP_CANARY", "1")
    cfg = _cfg(4096, tsmoothing=wf.TSMOOTH["exponential"])
    streams, hop = 16, 800
    with wf.SpectrumBatch(cfg, streams) as a, wf.SpectrumBatch(cfg, streams) as b:
        a.enable_loudness()
        b.enable_loudness()
        hist = ref.History(streams, 2, 4096)
        for t in range(30):
            x = synth.block(SEED, 0, streams, 2, t * hop, hop)
            a.push_audio(x)
            b.push_audio(x)
            hist.push(x)
            a.tick()
            b.tick()
            _sig_of(b, hist)
        b.sync()
        a.sync()
        for name in ("decibels", "bars", "tsmooth", "peaks", "loudness", "last_silent"):
            assert getattr(a, name)().tobytes() == getattr(b, name)().tobytes(), name
        b.sync()


# ---- slices, refusals, repeated reads, groups ---------------------------------------------------------------------------------

def test_slices_refusals_and_repeated_reads():
    L = wf.lib()
    rng = np.random.default_rng(11)
    with wf.SpectrumBatch(_cfg(2048), 9) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_SIGNAL) == 48  # before the first read
        b.push_audio(rng.uniform(-1, 1, (9, 2, 3001)).astype(np.float32))
        part = b.signal(3, 5)  # the first read is a slice: the block is allocated whole
        full = b.signal()
        assert part.tobytes() == full[3:8].tobytes()
        assert b.signal(8, 1).tobytes() == full[8:].tobytes()
        for _ in range(3):
            assert b.signal().tobytes() == full.tobytes()
        b.tick()
        assert b.signal().tobytes() == full.tobytes()  # a tick does not move the rings
        assert L.wf_hip_read(b.h, binding.OUT_SIGNAL, 0, 1, None) == ERR_INVALID
        out = np.empty(10, binding.SIGNAL_DTYPE)
        assert L.wf_hip_read(b.h, binding.OUT_SIGNAL, 0, 10, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID  # past the batch
        assert L.wf_hip_read(b.h, binding.OUT_SIGNAL, 9, 1, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID
        assert L.wf_hip_read(b.h, binding.OUT_SIGNAL, 0, 0, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID
    with wf.SpectrumBatch(wf.Config.defaults(waveform=1, stereo=1, width=640, meter_ms=100), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_SIGNAL) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.signal()
        assert e.value.code == ERR_INVALID
    with wf.SpectrumBatch(_cfg(1024, meter=1, bars=0), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_SIGNAL) == 48
        assert b.signal().shape == (2,)


def test_three_shards_match_one_handle():
    cfg = _cfg(2048)
    streams, hop = 7, 801
    with wf.SpectrumBatch(cfg, streams) as one, wf.MultiBatch(cfg, streams, [0, 0, 0]) as m:
        for t in range(5):
            x = synth.block(SEED, 0, streams, 2, t * hop, hop)
            one.push_audio(x)
            m.push_audio(x)
            one.tick()
            m.tick()
        m.sync()
        assert m.signal().tobytes() == one.signal().tobytes()
        assert m.signal(2, 4).tobytes() == one.signal()[2:6].tobytes()
        assert m.signal().shape == (streams,)


def test_headline_shape():
    """all 4096 stereo streams at FFT 4096, the window wrapping round the ring at an odd offset"""
    streams, n = 4096, 4096
    with wf.SpectrumBatch(_cfg(n), streams) as b:
        b.push_synth(SEED, 0, n + 800)
        b.tick()
        b.push_synth(SEED, n + 800, 801)
        got = b.signal()
    assert got.shape == (streams,)
    _check(got, ref.signal(synth.block(SEED, 0, streams, 2, 1601, n)))  # frames [5697 - 4096, 5697)
