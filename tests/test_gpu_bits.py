"""Bit meter on the device (WF_HIP_OUT_BITS) against the numpy restatement (tests/bits_ref.py) of the frames pushed: windows of
128, 1024, 2000, 4096 and 8192 (the cap) frames and a meter batch of 2208, three streams of different kinds each, uneven packets;
a mono capture; exotic bit patterns; bit identity across push paths, repeated reads and slices; fresh, reset and hidden streams;
refusals; nothing else moving; a three-shard group; the 2^32 wrap of the write positions.

Every comparison is for equality, and that is derived, not measured (include/wf_hip.h, "bit statistics"; bits_ref.mismatches):
the definition consists of comparisons, exact float64 operations and integer operations, so every field is equal bit for bit.
test_bits_cpu.py shows that the entries compared here are no trivial ones."""
import ctypes as C

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import bits_ref as ref
from pcm_convert import captured
from tools import synth
from measure_common import Hip, check_abi_refusals, check_shards_match, check_slices_and_repeats, packets, run_wrap_child

pytestmark = pytest.mark.gpu
ERR_INVALID = -1
SEED = ref.GPU_SEED
HOP = 801


def _cfg(fft=4096, sr=48000, channels=2, **kw):
    return wf.Config.defaults(**{**dict(fft_size=fft, sample_rate=sr, capture_channels=channels, stereo=1 if channels == 2 else 0, slope=1.0,
                                        bars=1, floor_db=-70), **kw})


def _check(got, frames, w, what=""):
    assert got.dtype == binding.BITS_DTYPE and got.shape == (frames.shape[0],)
    c = got["ch"]
    print(f"{what}: P {got['window'].tolist()}, word length {c['word_length'].tolist()}, magnitude bits {c['magnitude_bits'].tolist()}, "
          f"over {c['over'].tolist()}, fine {c['fine'].tolist()}, repeats {c['repeats'].tolist()}, longest run {c['max_run'].tolist()} at "
          f"{c['max_run_start'].tolist()} of {c['max_run_value'].tolist()}")
    bad = ref.mismatches(got, frames, w)
    assert not bad, bad[:8]
    n = frames.shape[1]
    assert np.all(c["hist"][:, :n].astype(np.int64).sum(axis=2) == got["window"][:, None])
    assert np.all(c["mag"][:, :n].astype(np.int64).sum(axis=2) == got["window"][:, None])


def _silence(p, streams, channels=2):
    s = np.zeros((), binding.BITS_DTYPE)
    for c in range(channels):
        s["ch"][c]["hist"][128] = s["ch"][c]["mag"][0] = s["ch"][c]["max_run"] = p
        s["ch"][c]["repeats"] = p - 1
    s["window"] = p
    return np.repeat(s, streams)


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=ref.case_id)
def test_bits_equal_the_restatement_of_the_frames(case):
    fft, sr, kw, w, kinds = case
    x = ref.case_audio(case)  # one ring and P / 2 + 3 frames: the window wraps the ring and ends at an odd position
    with wf.SpectrumBatch(_cfg(fft, sr, 2, **kw), x.shape[0]) as b:
        assert b.fft_size == w and b.ring_frames == ref.ring_frames(w)
        assert wf.lib().wf_hip_output_bytes(b.h, binding.OUT_BITS) == 1360  # before the first read
        for lo, hi in packets(np.random.default_rng(w), x.shape[-1], 700):
            b.push_audio(np.ascontiguousarray(x[:, :, lo:hi]))
        got = b.bits()
    assert np.all(got["window"] == ref.window_frames(w))
    _check(got, x, w, f"{ref.case_id(case)} {ref.case_kinds(case)}")


def test_a_mono_capture_leaves_the_second_channel_zero():
    rng = np.random.default_rng(5)
    kinds = ("float", "clipped", "gap", "u8")
    with wf.SpectrumBatch(_cfg(2000, channels=1), len(kinds)) as b:
        assert b.capture_channels == 1 and wf.lib().wf_hip_output_bytes(b.h, binding.OUT_BITS) == 1360
        x = np.stack([ref.signal(k, rng, b.ring_frames + 1003, 2000)[None] for k in kinds])
        for lo, hi in packets(rng, x.shape[-1], 700):
            b.push_audio(np.ascontiguousarray(x[:, :, lo:hi]))
        got = b.bits()
    assert not got["ch"][:, 1].tobytes().strip(b"\0")  # all zero bytes
    assert np.all(got["ch"]["word_length"][:, 0] == (32, 32, 32, 8)) and got["ch"]["over"][1, 0] > 0
    _check(got, x, 2000, "one captured channel")


def test_exotic_bit_patterns():
    """-0.0 / +0.0 alternating, denormals, +-inf, 1.0 and -1.0 through wf_hip_push_pcm as planar float32, whose bits pass unchanged"""
    p = 256
    f = np.float32
    x = np.zeros((3, 2, p), np.float32)
    x[0, 0, 1::2] = -0.0                                     # no two neighbours equal as patterns, every code 0
    x[0, 1] = np.arange(1, p + 1, dtype=np.uint32).view(np.float32)                       # positive denormals
    x[1, 0] = (np.arange(1, p + 1, dtype=np.uint32) * 32749 | 0x80000000).astype(np.uint32).view(np.float32)  # negative denormals and more
    x[1, 1] = np.tile(np.array([np.inf, -np.inf, 1.0, -1.0, np.nextafter(f(1), f(0)), 2.0 ** -31, -2.0 ** -31, 2.0 ** -32], np.float32), p // 8)
    x[2, 0] = np.tile(np.array([1.0, 1.0, 1.0, -1.0, -1.0, -1.0, -1.0, 0.0], np.float32), p // 8)
    x[2, 1, :100] = np.inf
    x[2, 1, 100:] = -1e-42
    assert not np.isnan(x).any()
    with wf.SpectrumBatch(_cfg(p), 3) as b:
        b.push_pcm(x, interleaved=False)
        got = b.bits()
    c = got["ch"]
    assert c["repeats"][0, 0] == 0 and c["max_run"][0, 0] == 1 and c["word_length"][0, 0] == 0 and c["hist"][0, 0, 128] == p
    assert c["fine"][0, 1] == p and c["word_length"][0, 1] == 0 and c["fine"][1, 0] == p and c["ones"][1, 0, 31] == p
    assert c["over"][1, 1] == 3 * p // 8 and c["fine"][1, 1] == p // 8
    assert c["max_run"][2, 0] == 4 and c["max_run_start"][2, 0] == 3 and c["max_run_value"][2, 0] == -1.0 and c["over"][2, 0] == 3 * p // 8
    assert c["max_run"][2, 1] == p - 100 and c["max_run_start"][2, 1] == 100 and c["over"][2, 1] == 100 and c["hist"][2, 1, 127] == p - 100
    assert c["max_run_value"][2, 1].view(np.uint32) == f(-1e-42).view(np.uint32)  # the denormal comes back as it went in
    _check(got, x, p, "exotic patterns")


def test_every_push_path_counts():
    """the same s16 frames through push_audio, wf_hip_push_pcm (s16 interleaved: every value exact in float32) and
    push_audio_device read bit-identically, with word length 16"""
    streams, fft, frames = 3, 1024, 801
    rng = np.random.default_rng(2)
    wave = (8000.0 * np.sin(2.0 * np.pi * np.arange(6 * frames) / 57.3))[None, :, None]
    pkts = [(wave[:, i * frames:(i + 1) * frames] + rng.integers(-5000, 5000, (streams, frames, 2))).astype(np.int16) for i in range(6)]
    hip = Hip()
    reads = {}
    for path in ("float", "pcm", "device"):
        with wf.SpectrumBatch(_cfg(fft), streams) as b:
            for pkt in pkts:
                conv = np.ascontiguousarray(captured(pkt, True, 0, 2))  # [streams, 2, frames] float32
                if path == "float":
                    b.push_audio(conv)
                elif path == "pcm":
                    b.push_pcm(pkt, interleaved=True)
                else:
                    d = hip.upload(conv)
                    b.push_audio_device(d, streams, frames)
                    b.sync()
                    assert hip.free(d) == 0
            reads[path] = b.bits()
    assert reads["pcm"].tobytes() == reads["float"].tobytes() and reads["device"].tobytes() == reads["float"].tobytes()
    hist = np.concatenate([captured(pkt, True, 0, 2) for pkt in pkts], axis=2)
    assert np.all(reads["float"]["ch"]["word_length"] == 16) and np.all(reads["float"]["ch"]["fine"] == 0)
    _check(reads["float"], hist, fft, "s16 packets")


def test_repeated_reads_and_slices():
    """a slice as a handle's first read equals the entry of the full read; reads with nothing in between, and a read after a
    tick, are bit-identical"""
    fft, streams = 2048, 5
    rng = np.random.default_rng(11)
    kinds = ("float", "constant", "two_runs", "clipped", "s16")
    x = np.stack([np.stack([ref.signal(k, rng, 3001, fft), ref.signal("gap", rng, 3001, fft)]) for k in kinds])
    with wf.SpectrumBatch(_cfg(fft), streams, ring_frames=fft) as b:
        assert b.ring_frames == fft
        b.push_audio(np.ascontiguousarray(x[..., :2000]))
        b.push_audio(np.ascontiguousarray(x[..., 2000:]))
        full = check_slices_and_repeats(b, "bits")
    _check(full, x, fft, "the window is the whole ring")


def test_fresh_reset_and_hidden_streams():
    fft, streams = 1024, 4
    with wf.SpectrumBatch(_cfg(fft), streams) as b:
        rng = np.random.default_rng(13)
        x = np.stack([np.stack([ref.signal(k, rng, b.ring_frames + HOP, fft), ref.signal("s24", rng, b.ring_frames + HOP, fft)])
                      for k in ("float", "clipped", "stuck", "run_last")])
        silence = _silence(fft, streams)
        assert ref.mismatches(silence, np.zeros((streams, 2, fft), np.float32), fft) == []
        assert b.bits().tobytes() == silence.tobytes()  # freshly created: zeros, one run of P
        b.set_hidden(np.array([0, 1, 0, 0], np.uint8))
        b.push_audio(x)
        b.tick()
        before = b.bits()
        _check(before, x, fft, "one stream hidden")  # the hidden stream's ring reads like any other
        assert np.all(before["ch"]["magnitude_bits"] == 31)
        b.reset(2, 1)
        after = b.bits()
    assert after[2:3].tobytes() == silence[:1].tobytes()
    keep = [0, 1, 3]
    assert after[keep].tobytes() == before[keep].tobytes()


def test_refusals():
    L = wf.lib()
    with wf.SpectrumBatch(wf.Config.defaults(waveform=1, stereo=1, width=640, meter_ms=100), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_BITS) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.bits()
        assert e.value.code == ERR_INVALID and "waveform batch" in str(e.value) and "bit statistics" in str(e.value), str(e.value)
        out = np.empty(2, binding.BITS_DTYPE)
        assert L.wf_hip_read(b.h, binding.OUT_BITS, 0, 2, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID
        assert b"bit statistics" in L.wf_hip_last_error(b.h)
    with wf.SpectrumBatch(_cfg(1024), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_BITS) == 1360  # before the first read
        check_abi_refusals(b, binding.OUT_BITS, binding.BITS_DTYPE, 2, _silence(1024, 2))


def test_a_small_meter_buffer_is_served():
    """there is no lower limit on the window: a meter buffer of 48 frames, less than a wavefront, of one captured channel"""
    rng = np.random.default_rng(17)
    with wf.SpectrumBatch(_cfg(1024, channels=1, meter=1, bars=0, meter_ms=1), 3) as b:
        assert b.fft_size == 48 and b.capture_channels == 1
        x = np.stack([ref.signal(k, rng, b.ring_frames + 21, 48)[None] for k in ("float", "run_last", "clipped")])
        b.push_audio(x)
        got = b.bits()
    assert np.all(got["window"] == 48)
    _check(got, x, 48, "meter buffer of 48 frames")


def test_nothing_else_moves(monkeypatch):
    """decibels, bars, scope(), gonio() and signal() read before and after a bits() are identical; guard bytes behind every block
    intact (wf_hip_sync checks them)"""
    monkeypatch.setenv("WF_HIP_CANARY", "1")
    streams, hop = 3, 800
    with wf.SpectrumBatch(_cfg(4096), streams) as b:
        for t in range(6):
            b.push_audio(synth.block(SEED, 0, streams, 2, t * hop, hop))
            b.tick()
        names = ("decibels", "bars", "scope", "gonio", "signal")
        before = {n: np.asarray(getattr(b, n)()).tobytes() for n in names}
        got = b.bits()
        b.sync()
        for n in names:
            assert np.asarray(getattr(b, n)()).tobytes() == before[n], n
        assert b.bits().tobytes() == got.tobytes()
        b.sync()
    hist = np.concatenate([synth.block(SEED, 0, streams, 2, t * hop, hop) for t in range(6)], axis=2)
    assert hist.shape[-1] >= 4096
    _check(got, hist, 4096, "between the other readers")


def test_three_shards_match_one_handle():
    cfg = _cfg(2048)
    streams = 7
    kinds = ("float", "s16", "clipped", "u8", "stuck", "silence", "s24")
    with wf.SpectrumBatch(cfg, streams) as one, wf.MultiBatch(cfg, streams, [0, 0, 0]) as m:
        for t in range(5):
            rng = np.random.default_rng(100 + t)
            x = np.stack([np.stack([ref.signal(k, rng, HOP), ref.signal("float", rng, HOP)]) for k in kinds])
            one.push_audio(x)
            m.push_audio(x)
            one.tick()
            m.tick()
        m.sync()
        want = check_shards_match(one, m, "bits", (2, 4))
        assert np.all(want["window"] == 2048) and want["ch"]["word_length"][:, 0].tolist() == [32, 16, 32, 8, 16, 0, 24]


def test_across_the_2_to_the_32_wrap():
    """tests/bits_wrap_child.py: twin handles on the development build, one aged to just below 2^32, walked across the wrap in small
    hops with bits() equal at every hop.  One child process (the release library has no test aids)"""
    run_wrap_child("bits_wrap_child.py", 60)
