"""The wire formats of wf_hip_push_pcm / wf_hip_multi_push_pcm on the device (packed 24-bit in either byte order, big-endian
int16, G.711 mu-law and A-law), by the method of tests/test_gpu_pcm.py: a handle is fed the packet in its own bytes, a twin the
decoded, channel-picked float32 planar packet (tests/wire_convert.py) through the float entry points.  After every tick the two
must agree bit for bit in every output the handle has.  One case goes against the reference itself."""
import ctypes as C

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
from oracle import wfref
from helpers import ref_settings, assert_db_close
from test_gpu_pcm import CAPTURES, ERR_INVALID, _assert_same, _bits, _cfg
from wire_convert import BYTES, WIRES, captured, random_packet

pytestmark = pytest.mark.gpu

CAPTURE_IDS = ["mono1", "mono_of_6_base3", "stereo2", "stereo_of_6"]


def _layout(interleaved):
    return "interleaved" if interleaved else "planar"


def _run(b, twin, wire, interleaved, channels, base, frames, steps, seed=1, first=0, count=None):
    rng = np.random.default_rng(seed)
    count = b.streams - first if count is None else count
    for t in range(steps):
        pkt = random_packet(rng, wire, count, channels, frames, interleaved)
        b.push_pcm(pkt, interleaved=interleaved, channel_base=base, first=first, wire=wire)
        twin.push_audio(captured(pkt, wire, interleaved, base, b.capture_channels), first=first)
        b.tick()
        twin.tick()
        _assert_same(b, twin, f"{wire} {_layout(interleaved)} {channels}ch base {base} frames {frames} step {t}")


@pytest.fixture(scope="module")
def pairs():
    made = {cap: (wf.SpectrumBatch(_cfg(cap), 5), wf.SpectrumBatch(_cfg(cap), 5)) for cap in (1, 2)}
    yield made
    for b, t in made.values():
        b.close()
        t.close()


@pytest.mark.parametrize("frames", [1, 3, 800, 801])
@pytest.mark.parametrize("capture", CAPTURES, ids=CAPTURE_IDS)
@pytest.mark.parametrize("interleaved", [True, False], ids=["interleaved", "planar"])
@pytest.mark.parametrize("wire", WIRES)
def test_formats_layouts_captures(pairs, wire, interleaved, capture, frames):
    channels, cap, base = capture
    b, twin = pairs[cap]
    b.reset()
    twin.reset()
    _run(b, twin, wire, interleaved, channels, base, frames, steps=3 if frames > 3 else 6, seed=frames * 31 + channels)


# one frame on either side of a tile of 8192 bytes: 8192 // 6 = 1365 frames of s24 stereo, 8192 // 3 = 2730 samples of an s24
# plane, 8192 // 18 = 455 frames of 5.1 s24, 8192 // 6 = 1365 frames of 5.1 mu-law
@pytest.mark.parametrize("wire,interleaved,capture,frames", [
    ("s24", True, (2, 2, 0), 1365), ("s24", True, (2, 2, 0), 1366), ("s24", False, (2, 2, 0), 2730), ("s24", False, (2, 2, 0), 2731),
    ("s24", True, (6, 2, 0), 455), ("s24", True, (6, 2, 0), 456), ("ulaw", True, (6, 1, 3), 1365), ("ulaw", True, (6, 1, 3), 1366)])
def test_tile_edges(pairs, wire, interleaved, capture, frames):
    channels, cap, base = capture
    b, twin = pairs[cap]
    b.reset()
    twin.reset()
    _run(b, twin, wire, interleaved, channels, base, frames, steps=2, seed=frames)


def test_every_start_alignment_from_one_host_packet():
    """17 blocks of 801 packed 24-bit frames: block i starts at byte i * 2403, and 2403 = 3 (mod 16), so the blocks' start
    addresses take every value mod 16 (the staged copy on the device is 16-B aligned: there block i starts at 3 i mod 16)"""
    streams, frames = 17, 801
    rng = np.random.default_rng(41)
    with wf.SpectrumBatch(_cfg(1), streams) as b, wf.SpectrumBatch(_cfg(1), streams) as twin:
        for t in range(3):
            pkt = random_packet(rng, "s24", streams, 1, frames, True)
            assert pkt.flags.c_contiguous
            starts = {(pkt.ctypes.data + i * frames * 3) % 16 for i in range(streams)}
            assert starts == set(range(16)) == {(i * frames * 3) % 16 for i in range(streams)}
            b.push_pcm(pkt, interleaved=True, wire="s24")
            twin.push_audio(captured(pkt, "s24", True, 0, 1))
            b.tick()
            twin.tick()
            _assert_same(b, twin, f"17 x 801 s24 step {t}")


def test_device_tensor_at_every_byte_offset():
    """WF_HIP_PCM_DEVICE from torch tensors whose data pointer is advanced by 0..15 bytes (s24_be planar), the other formats
    once each, and s16_be at an odd address refused: in a child process, tests/wire_device_child.py -- torch brings its own HIP
    runtime and has to be imported before libwaveform_hip.so is loaded"""
    import subprocess
    import sys
    from pathlib import Path
    pytest.importorskip("torch")
    child = Path(__file__).resolve().parent / "wire_device_child.py"
    r = subprocess.run([sys.executable, str(child)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "wire device ok" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


@pytest.mark.parametrize("wire,interleaved,capture", [("s24", True, (2, 2, 0)), ("alaw", False, (6, 1, 3))], ids=["s24_stereo", "alaw_mono_of_6"])
def test_pinned_async_two_slots(wire, interleaved, capture):
    channels, cap, base = capture
    streams, frames = 7, 800
    shape = ((streams, frames, channels) if interleaved else (streams, channels, frames)) + (BYTES[wire],)
    rng = np.random.default_rng(5)
    with wf.SpectrumBatch(_cfg(cap), streams) as b, wf.SpectrumBatch(_cfg(cap), streams) as twin:
        pin = [wf.PinnedBuffer(shape, np.uint8), wf.PinnedBuffer(shape, np.uint8)]
        for t in range(10):
            slot = t & 1
            b.ingest_done(slot)  # the slot's buffer is free again: refill it
            pin[slot].array[...] = random_packet(rng, wire, streams, channels, frames, interleaved)
            b.push_pcm(pin[slot], interleaved=interleaved, channel_base=base, slot=slot, wire=wire)
            twin.push_audio(captured(pin[slot].array, wire, interleaved, base, cap))
            b.tick()
            twin.tick()
            _assert_same(b, twin, f"pinned {wire} step {t}")
        b.sync()
        for p in pin:
            p.close()


@pytest.mark.parametrize("wire,interleaved,capture", [("s24", True, (2, 2, 0)), ("ulaw", False, (6, 1, 3))], ids=["s24_stereo", "ulaw_mono_of_6"])
def test_ragged_async(wire, interleaved, capture):
    channels, cap, base = capture
    streams, max_frames = 6, 803
    shape = ((streams, max_frames, channels) if interleaved else (streams, channels, max_frames)) + (BYTES[wire],)
    rng = np.random.default_rng(11)
    with wf.SpectrumBatch(_cfg(cap), streams) as b, wf.SpectrumBatch(_cfg(cap), streams) as twin:
        pin = [wf.PinnedBuffer(shape, np.uint8), wf.PinnedBuffer(shape, np.uint8)]
        fpin = [wf.PinnedBuffer((streams, cap, max_frames)), wf.PinnedBuffer((streams, cap, max_frames))]
        for t in range(8):
            slot = t & 1
            frames = rng.integers(0, max_frames + 1, streams).astype(np.uint32)
            frames[t % streams] = 0
            frames[(t + 1) % streams] = max_frames
            b.ingest_done(slot)
            twin.ingest_done(slot)
            pin[slot].array[...] = random_packet(rng, wire, streams, channels, max_frames, interleaved)
            fpin[slot].array[...] = captured(pin[slot].array, wire, interleaved, base, cap)
            b.push_pcm(pin[slot], interleaved=interleaved, channel_base=base, frames=frames, slot=slot, wire=wire)
            twin.push_audio_ragged_async(fpin[slot], frames, max_frames, slot)
            b.tick()
            twin.tick()
            _assert_same(b, twin, f"ragged {wire} step {t}")
        b.sync()
        twin.sync()
        for p in pin + fpin:
            p.close()


def test_volume_normalisation_and_ragged_refused():
    streams, frames = 4, 800
    cfg = _cfg(2, normalize_volume=1)
    rng = np.random.default_rng(13)
    with wf.SpectrumBatch(cfg, streams) as b, wf.SpectrumBatch(cfg, streams) as twin:
        b.enable_input_rms()
        twin.enable_input_rms()
        for t, wire in enumerate(WIRES * 2):
            interleaved = t % 2 == 0
            pkt = random_packet(rng, wire, streams, 2, frames, interleaved)
            if wire == "s24" and t >= len(WIRES):
                pkt[..., 2] = np.where(pkt[..., 2] & 0x80, 0xFF, 0x00)  # a level that moves: 16 bits of the 24
            b.push_pcm(pkt, interleaved=interleaved, wire=wire)
            twin.push_audio(captured(pkt, wire, interleaved, 0, 2))
            b.tick()
            twin.tick()
            _assert_same(b, twin, f"normalised {wire} step {t}")
        pin = wf.PinnedBuffer((streams, frames, 2, 3), np.uint8)
        with pytest.raises(wf.WfHipError) as e:
            b.push_pcm(pin, interleaved=True, frames=np.full(streams, frames), slot=0, wire="s24")
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
        _run(b, twin, "s24", True, 6, 0, 4096 + 1203, steps=2)
        _run(b, twin, "ulaw", False, 2, 0, 9001, steps=2, seed=3)
        _run(b, twin, "s24_be", False, 2, 0, 4096 + 2731, steps=1, seed=4)


@pytest.mark.parametrize("kind", ["meter", "waveform"])
def test_meter_and_waveform_handles(kind):
    cfg = wf.Config.defaults(meter=1, meter_ms=50) if kind == "meter" else wf.Config.defaults(waveform=1, stereo=1, width=640, meter_ms=100)
    streams = 4
    with wf.SpectrumBatch(cfg, streams) as b, wf.SpectrumBatch(cfg, streams) as twin:
        if kind == "meter":
            _run(b, twin, "s24_be", True, 6, 0, 801, steps=4)
        else:
            _run(b, twin, "alaw", False, 2, 0, 800, steps=3, seed=9)


def test_multi_group_splits_the_packet_inside_it():
    streams, frames = 11, 801
    cfg = _cfg(2)
    rng = np.random.default_rng(19)
    with wf.MultiBatch(cfg, streams, [0, 0, 0]) as m, wf.SpectrumBatch(cfg, streams) as one:
        assert m.n_devices == 3 and all(s[3] < streams for s in m.shards)
        for t, (wire, interleaved) in enumerate([("s24", True), ("s24_be", False), ("s16_be", True), ("ulaw", False), ("alaw", True)]):
            first, count = (1, 9) if t % 2 else (0, streams)  # a range that starts and ends inside shards
            pkt = random_packet(rng, wire, count, 6, frames, interleaved)
            m.push_pcm(pkt, interleaved=interleaved, first=first, wire=wire)
            one.push_audio(captured(pkt, wire, interleaved, 0, 2), first=first)
            m.tick()
            one.tick()
            m.sync()
            assert np.array_equal(_bits(m.decibels()), _bits(one.decibels())), f"{wire} step {t}"
            assert np.array_equal(_bits(m.bars()), _bits(one.bars())), f"{wire} step {t}"
        pin = wf.PinnedBuffer((streams, frames, 6, 3), np.uint8)
        with pytest.raises(ValueError):
            m.push_pcm(pin, interleaved=True, wire="s24")
        pinned = binding.Pcm(data=pin.ptr, format=16, channels=6, channel_base=0, frames=frames, memory=binding.PCM_PINNED, slot=0)
        assert wf.lib().wf_hip_multi_push_pcm(m.m, 0, streams, C.byref(pinned)) == ERR_INVALID
        for fmt in (9, 15, 21, 23, 29):
            host = binding.Pcm(data=pin.ptr, format=fmt, channels=6, channel_base=0, frames=frames, memory=binding.PCM_HOST, slot=0)
            assert wf.lib().wf_hip_multi_push_pcm(m.m, 0, streams, C.byref(host)) == ERR_INVALID, fmt
        m.tick()
        one.tick()
        m.sync()
        assert np.array_equal(_bits(m.decibels()), _bits(one.decibels())), "after the refused calls"
        pin.close()


def test_invalid_calls_are_refused_before_anything_is_enqueued():
    streams, frames = 3, 800
    L = wf.lib()
    pkt = random_packet(np.random.default_rng(23), "s24", streams, 6, frames, True)
    good = dict(data=pkt.ctypes.data, format=16, channels=6, channel_base=3, frames=frames, memory=binding.PCM_HOST, slot=0)
    with wf.SpectrumBatch(_cfg(1), streams) as b, wf.SpectrumBatch(_cfg(1), streams) as twin:
        for fmt in (9, 15, 21, 23, 29, 0xFFFFFFFF):
            assert L.wf_hip_push_pcm(b.h, 0, streams, C.byref(binding.Pcm(**{**good, "format": fmt}))) == ERR_INVALID, fmt
        for change in [dict(channels=0), dict(channels=9), dict(channel_base=6), dict(data=None), dict(memory=3)]:
            assert L.wf_hip_push_pcm(b.h, 0, streams, C.byref(binding.Pcm(**{**good, **change}))) == ERR_INVALID, change
        for bad, wire in [(pkt[..., :2], "s24"), (pkt.reshape(streams, frames, 18), "s24"), (pkt, "s16_be"), (pkt, "ulaw"), (pkt.view(np.int8), "s24"),
                          (pkt, "l24")]:
            with pytest.raises(ValueError):
                b.push_pcm(bad, interleaved=True, channel_base=3, wire=wire)
        # the handle has seen none of it
        b.push_pcm(pkt, interleaved=True, channel_base=3, wire="s24")
        twin.push_audio(captured(pkt, "s24", True, 3, 1))
        b.tick()
        twin.tick()
        _assert_same(b, twin, "after the refused calls")


def test_against_the_reference():
    if not wfref.available():
        pytest.skip("oracle/_ref/libwfref.so not built")
    cap = 2
    cfg = wf.Config.defaults(fft_size=2048, capture_channels=cap, stereo=1, slope=1.0)
    streams, hop = 3, 800
    refs = [wfref.RefSource(ref_settings(cfg), channels=cap) for _ in range(streams)]
    rng = np.random.default_rng(17)
    with wf.SpectrumBatch(cfg, streams) as b:
        assert b.capture_channels == refs[0].capture_channels
        for t in range(6):
            pkt = random_packet(rng, "s24", streams, 2, hop, True)
            b.push_pcm(pkt, interleaved=True, wire="s24")
            b.tick()
            got = b.decibels()
            audio = captured(pkt, "s24", True, 0, cap)
            for s, r in enumerate(refs):
                r.feed_and_tick(audio[s, 0], audio[s, 1])
                for c in range(b.output_channels):
                    assert_db_close(got[s, c], r.decibels(c), f"tick {t} stream {s} ch {c}", deep=True)
