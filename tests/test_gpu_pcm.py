"""wf_hip_push_pcm / wf_hip_multi_push_pcm on the device: every case drives a handle with a packet in its own sample format and
a twin handle with the converted, channel-picked float32 planar packet (tests/pcm_convert.py) through the float entry points
that the rest of the suite checks against the reference.  After every tick the two must agree bit for bit in every output
the handle has (decibels, tsmooth, bars, meter, input RMS).  Two cases also go against the reference itself."""
import ctypes as C

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
from oracle import wfref
from helpers import ref_settings, assert_db_close
from pcm_convert import DTYPES, captured, random_packet

pytestmark = pytest.mark.gpu

# (packet channels, capture channels, channel_base): mono of a mono packet, mono picked from 5.1, stereo, stereo of 5.1
CAPTURES = [(1, 1, 0), (6, 1, 3), (2, 2, 0), (6, 2, 0)]
ERR_INVALID = -1


def _cfg(cap, **kw):
    return wf.Config.defaults(**{**dict(fft_size=1024, capture_channels=cap, stereo=1 if cap == 2 else 0, bars=1, slope=1.0), **kw})


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_same(b, twin, what):
    cfg = b.cfg
    outs = []
    if cfg.meter:
        outs.append(("meter", b.meter, twin.meter))
    else:
        outs.append(("decibels", b.decibels, twin.decibels))
        if not cfg.waveform:
            outs.append(("tsmooth", b.tsmooth, twin.tsmooth))
        if cfg.bars and not cfg.waveform:
            outs.append(("bars", b.bars, twin.bars))
    if cfg.normalize_volume:
        outs.append(("input_rms", b.input_rms, twin.input_rms))
    for name, got, want in outs:
        g, w = got(), want()
        assert g.shape == w.shape
        bad = np.flatnonzero(_bits(g) != _bits(w))
        assert bad.size == 0, f"{what}: {name} differs at {bad.size} values, first {g.flat[bad[0]]} vs {w.flat[bad[0]]}"


def _run(b, twin, dtype, interleaved, channels, base, frames, steps, seed=1, first=0, count=None):
    rng = np.random.default_rng(seed)
    count = b.streams - first if count is None else count
    for t in range(steps):
        pkt = random_packet(rng, dtype, count, channels, frames, interleaved)
        b.push_pcm(pkt, interleaved=interleaved, channel_base=base, first=first)
        twin.push_audio(captured(pkt, interleaved, base, b.capture_channels), first=first)
        b.tick()
        twin.tick()
        _assert_same(b, twin, f"{np.dtype(dtype)} {'interleaved' if interleaved else 'planar'} {channels}ch base {base} frames {frames} step {t}")


@pytest.fixture(scope="module")
def pairs():
    made = {cap: (wf.SpectrumBatch(_cfg(cap), 5), wf.SpectrumBatch(_cfg(cap), 5)) for cap in (1, 2)}
    yield made
    for b, t in made.values():
        b.close()
        t.close()


@pytest.mark.parametrize("frames", [1, 3, 800, 801])
@pytest.mark.parametrize("capture", CAPTURES, ids=["mono1", "mono_of_6_base3", "stereo2", "stereo_of_6"])
@pytest.mark.parametrize("interleaved", [True, False], ids=["interleaved", "planar"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "s16", "s32", "f32"])
def test_formats_layouts_captures(pairs, dtype, interleaved, capture, frames):
    channels, cap, base = capture
    b, twin = pairs[cap]
    b.reset()
    twin.reset()
    _run(b, twin, dtype, interleaved, channels, base, frames, steps=3 if frames > 3 else 6, seed=frames * 31 + channels)


@pytest.mark.parametrize("dtype,interleaved,capture", [(np.int16, True, (2, 2, 0)), (np.uint8, False, (6, 1, 3)), (np.int32, True, (6, 2, 0)),
                                                       (np.float32, False, (6, 2, 0))])
def test_pinned_async_two_slots(dtype, interleaved, capture):
    channels, cap, base = capture
    streams, frames = 7, 800
    shape = (streams, frames, channels) if interleaved else (streams, channels, frames)
    rng = np.random.default_rng(5)
    with wf.SpectrumBatch(_cfg(cap), streams) as b, wf.SpectrumBatch(_cfg(cap), streams) as twin:
        pin = [wf.PinnedBuffer(shape, dtype), wf.PinnedBuffer(shape, dtype)]
        for t in range(10):
            slot = t & 1
            b.ingest_done(slot)  # the slot's buffer is free again: refill it
            pin[slot].array[...] = random_packet(rng, dtype, streams, channels, frames, interleaved)
            b.push_pcm(pin[slot], interleaved=interleaved, channel_base=base, slot=slot)
            twin.push_audio(captured(pin[slot].array, interleaved, base, cap))
            b.tick()
            twin.tick()
            _assert_same(b, twin, f"pinned step {t}")
        b.sync()
        for p in pin:
            p.close()


def test_device_tensor():
    """WF_HIP_PCM_DEVICE from torch tensors (every sample type, interleaved and planar, channel picks): in a child process,
    tests/pcm_device_child.py -- torch brings its own HIP runtime and has to be imported before libwaveform_hip.so is loaded"""
    import subprocess
    import sys
    from pathlib import Path
    pytest.importorskip("torch")
    child = Path(__file__).resolve().parent / "pcm_device_child.py"
    r = subprocess.run([sys.executable, str(child)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "pcm device ok" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


@pytest.mark.parametrize("dtype,interleaved,capture", [(np.int16, True, (2, 2, 0)), (np.uint8, False, (6, 1, 3)), (np.int16, False, (6, 2, 0)),
                                                       (np.uint8, True, (6, 1, 3))])
def test_ragged_async(dtype, interleaved, capture):
    channels, cap, base = capture
    streams, max_frames = 6, 803
    shape = (streams, max_frames, channels) if interleaved else (streams, channels, max_frames)
    rng = np.random.default_rng(11)
    with wf.SpectrumBatch(_cfg(cap), streams) as b, wf.SpectrumBatch(_cfg(cap), streams) as twin:
        pin = [wf.PinnedBuffer(shape, dtype), wf.PinnedBuffer(shape, dtype)]
        fpin = [wf.PinnedBuffer((streams, cap, max_frames)), wf.PinnedBuffer((streams, cap, max_frames))]
        for t in range(8):
            slot = t & 1
            frames = rng.integers(0, max_frames + 1, streams).astype(np.uint32)
            frames[t % streams] = 0
            frames[(t + 1) % streams] = max_frames
            b.ingest_done(slot)
            twin.ingest_done(slot)
            pin[slot].array[...] = random_packet(rng, dtype, streams, channels, max_frames, interleaved)
            fpin[slot].array[...] = captured(pin[slot].array, interleaved, base, cap)
            b.push_pcm(pin[slot], interleaved=interleaved, channel_base=base, frames=frames, slot=slot)
            twin.push_audio_ragged_async(fpin[slot], frames, max_frames, slot)
            b.tick()
            twin.tick()
            _assert_same(b, twin, f"ragged step {t}")
        b.sync()
        twin.sync()
        for p in pin + fpin:
            p.close()


@pytest.mark.parametrize("entry", ["float", "pcm"])
def test_one_slot_grows_while_in_use(entry):
    """The ordering rule of an ingest slot, on its own: every push goes through slot 0 and none waits for the one before.  A
    small plain push, a ragged push with more streams and more frames (the staging block is outgrown and the frame counts
    appear while the plain push may still read the slot), a small plain push, a ragged push beyond 64 streams (both blocks are
    outgrown, the page-locked counts are rewritten) and a small plain push again; a tick behind each.  Every push has a host
    buffer of its own, so wf_hip_ingest_done is not needed in between.  The twin takes the same frames through wf_hip_push_audio."""
    streams, cap = 100, 2
    steps = [(2, 64, False), (40, 300, True), (2, 64, False), (streams, 403, True), (3, 65, False)]  # (count, frames, ragged)
    rng = np.random.default_rng(29)
    with wf.SpectrumBatch(_cfg(cap), streams) as b, wf.SpectrumBatch(_cfg(cap), streams) as twin:
        pins, counts = [], []
        for count, frames, ragged in steps:
            pin = wf.PinnedBuffer((count, cap, frames))
            pin.array[...] = random_packet(rng, np.float32, count, cap, frames, False)
            f = rng.integers(0, frames + 1, count).astype(np.uint32) if ragged else np.full(count, frames, np.uint32)
            if ragged:
                f[0], f[1] = frames, 0
            pins.append(pin)
            counts.append(f)
        for (count, frames, ragged), pin, f in zip(steps, pins, counts):
            if entry == "pcm":
                b.push_pcm(pin, interleaved=False, frames=f if ragged else None, slot=0)
            elif ragged:
                b.push_audio_ragged_async(pin, f, frames, 0)
            else:
                b.push_audio_async(pin, count, frames, 0)
            b.tick()
        for pin, f in zip(pins, counts):
            for s in np.flatnonzero(f):
                twin.push_audio(pin.array[s:s + 1, :, :f[s]], first=int(s))
            twin.tick()
        _assert_same(b, twin, f"one slot, {entry} entry points")
        b.sync()
        for p in pins:
            p.close()


def test_volume_normalisation_and_ragged_refused():
    streams, frames = 4, 800
    cfg = _cfg(2, normalize_volume=1)
    rng = np.random.default_rng(13)
    with wf.SpectrumBatch(cfg, streams) as b, wf.SpectrumBatch(cfg, streams) as twin:
        b.enable_input_rms()
        twin.enable_input_rms()
        for t, dtype in enumerate([np.int16, np.uint8, np.int32, np.float32] * 2):
            interleaved = t % 2 == 0
            pkt = random_packet(rng, dtype, streams, 2, frames, interleaved)
            pkt = (pkt // (t + 1)).astype(dtype) if dtype != np.float32 else pkt * np.float32(0.1 * (t + 1))  # a level that moves
            b.push_pcm(pkt, interleaved=interleaved)
            twin.push_audio(captured(pkt, interleaved, 0, 2))
            b.tick()
            twin.tick()
            _assert_same(b, twin, f"normalised step {t}")
        pin = wf.PinnedBuffer((streams, frames, 2), np.int16)
        with pytest.raises(wf.WfHipError) as e:
            b.push_pcm(pin, interleaved=True, frames=np.full(streams, frames), slot=0)
        assert e.value.code == ERR_INVALID
        b.tick()
        twin.tick()
        _assert_same(b, twin, "after the refused ragged push")
        pin.close()


def test_packet_longer_than_the_ring():
    streams = 3
    cfg = _cfg(2)
    with wf.SpectrumBatch(cfg, streams, ring_frames=4096) as b, wf.SpectrumBatch(cfg, streams, ring_frames=4096) as twin:
        assert b.ring_frames == 4096
        _run(b, twin, np.int16, True, 6, 0, 4096 + 1203, steps=2)
        _run(b, twin, np.uint8, False, 2, 0, 9001, steps=2, seed=3)


def test_more_streams_than_one_slice():
    streams = 16384 + 300
    cfg = wf.Config.defaults(fft_size=512, capture_channels=1, stereo=0, bars=0)
    with wf.SpectrumBatch(cfg, streams) as b, wf.SpectrumBatch(cfg, streams) as twin:
        _run(b, twin, np.int16, True, 6, 3, 257, steps=2)
        _run(b, twin, np.uint8, False, 2, 1, 64, steps=1, seed=2)


@pytest.mark.parametrize("kind", ["meter", "waveform"])
def test_meter_and_waveform_handles(kind):
    cfg = wf.Config.defaults(meter=1, meter_ms=50) if kind == "meter" else wf.Config.defaults(waveform=1, stereo=1, width=640, meter_ms=100)
    streams = 4
    with wf.SpectrumBatch(cfg, streams) as b, wf.SpectrumBatch(cfg, streams) as twin:
        _run(b, twin, np.int16, True, 6, 0, 801, steps=4)
        _run(b, twin, np.uint8, False, 2, 0, 800, steps=2, seed=9)


def test_fft_size_800():
    streams = 3
    cfg = wf.Config.defaults(fft_size=800, capture_channels=2, stereo=1, bars=1)
    with wf.SpectrumBatch(cfg, streams) as b, wf.SpectrumBatch(cfg, streams) as twin:
        _run(b, twin, np.int16, True, 2, 0, 801, steps=4)
        _run(b, twin, np.int32, False, 6, 0, 800, steps=2, seed=4)


@pytest.mark.parametrize("dtype,channels,base,cap", [(np.int16, 2, 0, 2), (np.uint8, 6, 2, 1)], ids=["s16_stereo", "u8_mono_of_5.1"])
def test_against_the_reference(dtype, channels, base, cap):
    if not wfref.available():
        pytest.skip("oracle/_ref/libwfref.so not built")
    cfg = wf.Config.defaults(fft_size=2048, capture_channels=cap, stereo=1 if cap == 2 else 0, slope=1.0)
    streams, hop = 3, 800
    refs = [wfref.RefSource(ref_settings(cfg), channels=cap) for _ in range(streams)]
    rng = np.random.default_rng(17)
    with wf.SpectrumBatch(cfg, streams) as b:
        assert b.capture_channels == refs[0].capture_channels
        for t in range(6):
            pkt = random_packet(rng, dtype, streams, channels, hop, True)
            b.push_pcm(pkt, interleaved=True, channel_base=base)
            b.tick()
            got = b.decibels()
            audio = captured(pkt, True, base, cap)
            for s, r in enumerate(refs):
                r.feed_and_tick(audio[s, 0], audio[s, 1] if cap > 1 else None)
                for c in range(b.output_channels):
                    assert_db_close(got[s, c], r.decibels(c), f"tick {t} stream {s} ch {c}", deep=True)


def test_multi_group_splits_the_packet_at_shard_boundaries():
    streams, frames = 11, 800
    cfg = _cfg(2)
    have = wf.device_count()
    rng = np.random.default_rng(19)
    with wf.MultiBatch(cfg, streams, [i % have for i in range(3)]) as m, wf.SpectrumBatch(cfg, streams) as one:
        assert m.n_devices == 3 and all(s[3] < streams for s in m.shards)
        for t, (dtype, interleaved) in enumerate([(np.int16, True), (np.uint8, False), (np.int32, True), (np.float32, False)]):
            first, count = (1, 9) if t % 2 else (0, streams)  # a range that starts and ends inside shards
            pkt = random_packet(rng, dtype, count, 6, frames, interleaved)
            m.push_pcm(pkt, interleaved=interleaved, first=first)
            one.push_pcm(pkt, interleaved=interleaved, first=first)
            m.tick()
            one.tick()
            m.sync()
            assert np.array_equal(_bits(m.decibels()), _bits(one.decibels())), f"step {t}"
            assert np.array_equal(_bits(m.bars()), _bits(one.bars())), f"step {t}"


def test_invalid_calls_are_refused_before_anything_is_enqueued():
    streams, frames = 3, 800
    cfg = _cfg(1)
    L = wf.lib()
    pkt = random_packet(np.random.default_rng(23), np.int16, streams, 6, frames, True)
    good = dict(data=pkt.ctypes.data, format=2, channels=6, channel_base=3, frames=frames, memory=binding.PCM_HOST, slot=0)
    bad = [dict(format=0), dict(format=9), dict(channels=0), dict(channels=9), dict(channel_base=6), dict(channel_base=0xFFFFFFFF),
           dict(data=None), dict(memory=3), dict(memory=binding.PCM_PINNED, slot=2)]
    with wf.SpectrumBatch(cfg, streams) as b, wf.SpectrumBatch(cfg, streams) as twin, wf.SpectrumBatch(_cfg(2), streams) as b2:
        for change in bad:
            pcm = binding.Pcm(**{**good, **change})
            assert L.wf_hip_push_pcm(b.h, 0, streams, C.byref(pcm)) == ERR_INVALID, change
        assert L.wf_hip_push_pcm(b.h, 0, streams, None) == ERR_INVALID
        assert L.wf_hip_push_pcm(b.h, 1, streams, C.byref(binding.Pcm(**good))) == ERR_INVALID  # range
        ragged = binding.Pcm(**{**good, "memory": binding.PCM_HOST})
        counts = np.full(streams, frames, np.uint32)
        ragged.frames_per_stream = counts.ctypes.data_as(C.POINTER(C.c_uint32))
        assert L.wf_hip_push_pcm(b.h, 0, streams, C.byref(ragged)) == ERR_INVALID  # ragged needs pinned memory
        # a stereo capture: channel_base must be 0, and the packet needs two channels
        assert L.wf_hip_push_pcm(b2.h, 0, streams, C.byref(binding.Pcm(**{**good, "channel_base": 1}))) == ERR_INVALID
        assert L.wf_hip_push_pcm(b2.h, 0, streams, C.byref(binding.Pcm(**{**good, "channels": 1, "channel_base": 0}))) == ERR_INVALID
        # the handle has seen none of it
        b.push_pcm(pkt, interleaved=True, channel_base=3)
        twin.push_audio(captured(pkt, True, 3, 1))
        b.tick()
        twin.tick()
        _assert_same(b, twin, "after the refused calls")
        with wf.MultiBatch(cfg, streams, [0, 0]) as m:
            pinned = binding.Pcm(**{**good, "memory": binding.PCM_PINNED})
            assert L.wf_hip_multi_push_pcm(m.m, 0, streams, C.byref(pinned)) == ERR_INVALID
            assert L.wf_hip_multi_push_pcm(m.m, 0, streams, C.byref(binding.Pcm(**{**good, "format": 0}))) == ERR_INVALID
            assert L.wf_hip_multi_push_pcm(m.m, 0, streams, C.byref(binding.Pcm(**{**good, "channel_base": 6}))) == ERR_INVALID
