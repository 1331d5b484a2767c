"""Constant-Q spectrum on the device (WF_HIP_OUT_CQ) against the float64 restatement (tests/cq_ref.py) of the frames pushed:
windows capped at 128, 4096, 8192 and 16384 frames, four sample rates, an FFT size that is no power of two, a ring wider than
the cap, one captured channel, a meter batch; sines at A4 and A1 against analytic truth; bit identity across push paths, repeated
reads and slices; reset and hidden streams; refusals; nothing else moving; a three-shard group.

The bound against the restatement is derived, not measured (include/wf_hip.h, "determinism"; cq_ref.mismatches): per covered
bin |got - want| <= 2 float32 ulps of want, or |10^(got/20) - a_want| <= 1e-10 pk with pk the largest |x| of the newest Lmax
frames; a bin with a_want >= 1e-3 pk must pass the first arm, and test_cq_cpu.py shows that those are at least 80 % of the
covered bins of every case here.  The geometry fields and whatever is not computed are compared exactly."""
import ctypes as C

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import cq_ref as ref
from pcm_convert import captured
from tools import synth
from measure_common import Hip, check_abi_refusals, check_shards_match, check_slices_and_repeats, packets

pytestmark = pytest.mark.gpu
ERR_INVALID = -1
SEED = ref.GPU_SEED
HOP = 801
A4, A1 = 57, 21


def _cfg(fft=4096, sr=48000, channels=2, **kw):
    return wf.Config.defaults(**{**dict(fft_size=fft, sample_rate=sr, capture_channels=channels, stereo=1 if channels == 2 else 0, slope=1.0,
                                        bars=1, floor_db=-70), **kw})


def _check(got, frames, sr, ring_frames, what=""):
    assert got.dtype == binding.CQ_DTYPE and got.shape == (frames.shape[0],)
    ulps, far, lin, share = ref.worst(got, frames, sr, ring_frames)
    print(f"{what}: Lmax {int(got['max_window'][0])}, covered {int(got['end_covered'][0])}, first resolved {int(got['first_resolved'][0])}, "
          f"strong share {share:.3f}, worst strong bin {ulps:.2f} float32 ulps, {far} bins beyond two ulps, "
          f"worst |10^(got/20) - a| / pk among them {lin:.3e}")
    assert share >= 0.8
    bad = ref.mismatches(got, frames, sr, ring_frames)
    assert not bad, bad[:8]


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=ref.case_id)
def test_cq_equals_the_reference_of_the_frames(case):
    fft, sr, ring, ch, kw, lmax = case
    x = ref.case_audio(case)  # Lmax + 2 * 801 frames: the window wraps the ring and ends at no aligned position
    with wf.SpectrumBatch(_cfg(fft, sr, ch, **kw), x.shape[0], ring_frames=ring) as b:
        assert ref.max_window(b.ring_frames) == lmax
        for lo, hi in packets(np.random.default_rng(fft), x.shape[-1], 699):
            b.push_audio(np.ascontiguousarray(x[:, :, lo:hi]))
        got = b.cq()
        assert wf.lib().wf_hip_output_bytes(b.h, binding.OUT_CQ) == 976
        ring_frames = b.ring_frames
    if ch == 1:
        assert np.all(np.isneginf(got["db"][:, 1]))
    _check(got, x, sr, ring_frames, ref.case_id(case))


def test_sines_at_a4_and_a1():
    """ring_frames 16384 at 48 kHz resolves A1 (55 Hz, L = 14677): both sines read 20 log10 A in their own bin, which is the
    largest; the default ring at FFT 1024 (Lmax 4096) says that A1 is not resolved"""
    sr, frames = 48000, 16384 + HOP
    t = np.arange(frames)
    amps = (0.5, 0.25)
    x = np.stack([np.stack([a * np.sin(2 * np.pi * f * t / sr + 0.3)] * 2) for f, a in zip((440.0, 55.0), amps)]).astype(np.float32)
    with wf.SpectrumBatch(_cfg(4096, sr), 2, ring_frames=16384) as b:
        b.push_audio(x)
        got = b.cq()
    assert np.all(got["first_resolved"] == 20) and np.all(got["max_window"] == 16384) and np.all(got["end_covered"] == 120)
    for s, (bin_, amp) in enumerate(zip((A4, A1), amps)):
        db = got["db"][s]
        print(f"bin {bin_}: {db[0, bin_]:.5f} dB, want {20 * np.log10(amp):.5f}; neighbours {db[0, bin_ - 1]:.3f} {db[0, bin_ + 1]:.3f}")
        assert abs(db[0, bin_] - 20.0 * np.log10(amp)) <= 1e-3 and db[1, bin_] == db[0, bin_]
        assert int(np.argmax(db[0])) == bin_ and int(np.argmax(db[1])) == bin_
        assert bin_ >= got["first_resolved"][s]
    assert not ref.mismatches(got, x, sr, 16384)
    with wf.SpectrumBatch(_cfg(1024, sr), 1) as b:
        b.push_audio(x[1:, :, -4096:])
        short = b.cq()
    assert short["max_window"][0] == 4096 and short["first_resolved"][0] == 44 > A1


def test_every_push_path_counts():
    """the same frames through push_audio, wf_hip_push_pcm (s16 interleaved: every value exact in float32) and
    push_audio_device read bit-identically"""
    streams, fft, frames = 3, 1024, 801
    rng = np.random.default_rng(2)
    pkts = [rng.integers(-32768, 32768, (streams, frames, 2)).astype(np.int16) for _ in range(6)]
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
            reads[path] = b.cq()
            ring_frames = b.ring_frames
    assert reads["pcm"].tobytes() == reads["float"].tobytes() and reads["device"].tobytes() == reads["float"].tobytes()
    hist = np.concatenate([captured(pkt, True, 0, 2) for pkt in pkts], axis=2)
    assert hist.shape[-1] >= ring_frames == 4096
    assert not ref.mismatches(reads["float"], hist, 48000, ring_frames)


def test_repeated_reads_and_slices():
    """a slice as a handle's first read equals the entry of the full read; reads with nothing in between are bit-identical; the
    window is the whole of a ring it has wrapped"""
    fft, sr, streams = 2048, 48000, 5
    x = ref.audio(np.random.default_rng(11), streams, 3001, sr)
    with wf.SpectrumBatch(_cfg(fft, sr), streams, ring_frames=fft) as b:
        assert b.ring_frames == fft
        b.push_audio(np.ascontiguousarray(x[..., :2000]))
        b.push_audio(np.ascontiguousarray(x[..., 2000:]))
        full = check_slices_and_repeats(b, "cq")
    _check(full, x, sr, fft, "wrapped ring")


def test_reset_and_hidden_streams():
    fft, sr, streams = 1024, 48000, 4
    with wf.SpectrumBatch(_cfg(fft, sr), streams) as b:
        ring_frames = b.ring_frames
        x = ref.audio(np.random.default_rng(13), streams, ring_frames + HOP, sr)
        silence = ref.cq(np.zeros((1, 2, ring_frames), np.float32), sr, ring_frames)
        assert np.all(np.isneginf(silence["db"])) and silence["max_window"][0] == 4096 and silence["first_resolved"][0] == 44
        assert b.cq().tobytes() == np.repeat(silence, streams).tobytes()  # freshly created: zeros, the geometry set
        b.set_hidden(np.array([0, 1, 0, 0], np.uint8))
        b.push_audio(x)
        b.tick()
        before = b.cq()
        _check(before, x, sr, ring_frames, "one stream hidden")  # the hidden stream's ring reads like any other
        b.reset(2, 1)
        after = b.cq()
    assert after[2:3].tobytes() == silence.tobytes()
    keep = [0, 1, 3]
    assert after[keep].tobytes() == before[keep].tobytes()


def test_refusals():
    L = wf.lib()
    with wf.SpectrumBatch(wf.Config.defaults(waveform=1, stereo=1, width=640, meter_ms=100), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_CQ) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.cq()
        assert e.value.code == ERR_INVALID and "waveform batch" in str(e.value), str(e.value)
        out = np.empty(2, binding.CQ_DTYPE)
        assert L.wf_hip_read(b.h, binding.OUT_CQ, 0, 2, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID
        assert b"constant-Q" in L.wf_hip_last_error(b.h)
    with wf.SpectrumBatch(_cfg(1024), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_CQ) == 976  # before the first read
        out = check_abi_refusals(b, binding.OUT_CQ, binding.CQ_DTYPE, 2)
        assert np.all(out["max_window"][:2] == 4096)


def test_nothing_else_moves(monkeypatch):
    """twin handles for 12 ticks, one of them read between the ticks: rows, bars, last_silent and every other output stay
    bit-identical; guard bytes behind every block intact (wf_hip_sync checks them); a handle's first read equals its twin's
    thirteenth"""
    monkeypatch.setenv("WF_HIP_CANARY", "1")
    cfg = _cfg(4096, tsmoothing=wf.TSMOOTH["exponential"])
    streams, hop = 8, 800
    with wf.SpectrumBatch(cfg, streams) as a, wf.SpectrumBatch(cfg, streams) as b:
        for t in range(12):
            x = synth.block(SEED, 0, streams, 2, t * hop, hop)
            a.push_audio(x)
            b.push_audio(x)
            a.tick()
            b.tick()
            b.cq()
        b.sync()
        a.sync()
        for name in ("decibels", "bars", "tsmooth", "last_silent", "signal", "bands", "peaks", "pitch", "stereo"):
            assert np.asarray(getattr(a, name)()).tobytes() == np.asarray(getattr(b, name)()).tobytes(), name
        first = a.cq()
        assert first.tobytes() == b.cq().tobytes()
        a.sync()
        b.sync()
        ring_frames = a.ring_frames
    hist = np.concatenate([synth.block(SEED, 0, streams, 2, t * hop, hop) for t in range(12)], axis=2)
    assert hist.shape[-1] >= ring_frames
    assert not ref.mismatches(first, hist, 48000, ring_frames)


def test_three_shards_match_one_handle():
    cfg = _cfg(2048)
    streams = 7
    with wf.SpectrumBatch(cfg, streams) as one, wf.MultiBatch(cfg, streams, [0, 0, 0]) as m:
        for t in range(5):
            x = synth.block(SEED, 0, streams, 2, t * HOP, HOP)
            one.push_audio(x)
            m.push_audio(x)
            one.tick()
            m.tick()
        m.sync()
        want = check_shards_match(one, m, "cq", (2, 4))
        assert np.all(np.isfinite(want["db"]))
