"""Delay finder on the device (WF_HIP_OUT_DELAY) against the float64 restatement (tests/delay_ref.py) of the frames pushed: windows
of 128 (the smallest), 1024, 2048 (shorter than the FFT), 4096 and 4096 of 16384 (the cap) frames, a meter batch and a mono
mixdown display, nine streams of different kinds each -- white noise at an integer and a fractional delay, an inverted channel near
the end of the lag range, a channel 100 dB under its partner, tones in noise, dual mono, independent noise, a silent channel, a NaN
-- in uneven packets; bit identity across push paths, repeated reads and slices; reset and hidden streams; refusals; nothing else
moving on a twin; a three-shard group; the 2^32 wrap of the write positions.

The bound against the restatement is derived, not measured (delay_ref's docstring): both sides work in float64 from the same float32
samples and differ in the order of operations, and tests/test_delay_cpu.py shows on these very seeds and shapes that no decision is
near a tie and that four orderings agree to 1e-9, so one float32 rounding is all that can separate them.  (On an MI355X the
scalar float32 fields came out equal on every case here, the curve within 5.9e-11 and delay_frames within 1.4e-12.)"""
import ctypes as C

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import delay_ref as ref
from pcm_convert import captured
from tools import synth
from measure_common import Hip, check_abi_refusals, check_shards_match, check_slices_and_repeats, packets, run_wrap_child

pytestmark = pytest.mark.gpu
ERR_INVALID = -1
HOP = 801


def _cfg(fft=4096, sr=48000, **kw):
    return wf.Config.defaults(**{**dict(fft_size=fft, sample_rate=sr, capture_channels=2, stereo=1, slope=1.0, bars=1, floor_db=-70), **kw})


def _check(got, frames, w, sr, what=""):
    """every entry of `got` within the bound of the restatement of `frames`, each figure printed first"""
    want = ref.delay(frames, w, sr)
    assert got.dtype == binding.DELAY_DTYPE and got.shape == want.shape
    print(f"{what}: P {got['window'].tolist()}, valid {got['valid'].tolist()}, lag {got['lag'].tolist()}, polarity {got['polarity'].tolist()}, "
          f"delay {got['delay_frames'].tolist()}, peak {got['peak'].tolist()}, ambiguity {got['ambiguity'].tolist()}, "
          f"worst |got - want| {ref.worst(got, want)}")
    p = ref.window_frames(w)
    for s, x in enumerate(frames):  # the conditions the bound rests on (test_delay_cpu.py), for whatever is compared here
        vals = ref.analyse(x[0, -p:], x[1, -p:], sr)[1]
        assert not vals or (vals["margin_argmax"] >= 1e-3 and vals["margin_pi"] >= 1e-6 and abs(abs(vals["f_raw"]) - 0.5) >= 1e-6), (s, vals)
    bad = ref.mismatches(got, want)
    assert not bad, bad[:8]
    assert not got["reserved"].any() and not got["reserved2"].any()
    return want


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=ref.case_id)
def test_delay_equals_the_restatement_of_the_frames(case):
    fft, sr, kw, w = case
    x = ref.case_audio(case)  # one ring and P / 2 + 3 frames: the window wraps the ring and ends at an odd position
    p = ref.window_frames(w)
    with wf.SpectrumBatch(_cfg(fft, sr, **kw), x.shape[0]) as b:
        assert b.fft_size == w and b.ring_frames == ref.ring_frames(w) and b.capture_channels == 2
        assert wf.lib().wf_hip_output_bytes(b.h, binding.OUT_DELAY) == 320  # before the first read
        for lo, hi in packets(np.random.default_rng(w), x.shape[-1], 700):
            b.push_audio(np.ascontiguousarray(x[:, :, lo:hi]))
        got = b.delay()
    assert np.all(got["window"] == p)
    _check(got, x, w, sr, ref.case_id(case))
    assert got["valid"].tolist() == [int(name not in ref.INVALID) for name, _, _ in ref.KINDS]
    assert got[7:].tobytes() == ref.zero_record(p, 2).tobytes()  # a silent channel and a NaN: the zero record
    lr = p // 4
    assert got["lag"][:6].tolist() == [3, -7, lr - 1, 11, 2, 0] and got["polarity"][:6].tolist() == [1, 1, -1, 1, 1, 1]


def test_every_push_path_counts():
    """the same s16 frames through push_audio, wf_hip_push_pcm (s16 interleaved: every value exact in float32) and
    push_audio_device read bit-identically"""
    streams, fft, frames, sr = 3, 1024, 801, 48000
    rng = np.random.default_rng(2)
    base = np.stack([ref.stream(k, rng, 6 * frames, fft) for k in ("white +3", "white -7.3", "inverted L-1")])  # [streams, 2, n]
    wave = np.round(32768.0 * 0.9 * np.clip(base, -1.0, 1.0)).astype(np.int16).transpose(0, 2, 1)  # [streams, n, 2]
    pkts = [np.ascontiguousarray(wave[:, i * frames:(i + 1) * frames]) for i in range(6)]
    hip = Hip()
    reads = {}
    for path in ("float", "pcm", "device"):
        with wf.SpectrumBatch(_cfg(fft, sr), streams) as b:
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
            reads[path] = b.delay()
    assert reads["pcm"].tobytes() == reads["float"].tobytes() and reads["device"].tobytes() == reads["float"].tobytes()
    hist = np.concatenate([captured(pkt, True, 0, 2) for pkt in pkts], axis=2)
    want = _check(reads["float"], hist, fft, sr, "s16 packets")
    assert np.all(want["valid"] == 1) and want["lag"].tolist() == [3, -7, 255] and want["polarity"].tolist() == [1, 1, -1]


def test_repeated_reads_and_slices():
    """a slice as a handle's first read equals the entry of the full read; reads with nothing in between, and a read after a
    tick, are bit-identical.  The window is the whole ring"""
    fft, streams, sr = 2048, 5, 48000
    rng = np.random.default_rng(11)
    kinds = ("white +3", "tones +2.25", "-100 dB +11", "silent ch0", "independent")
    x = np.stack([ref.stream(k, rng, 3001, fft) for k in kinds])
    with wf.SpectrumBatch(_cfg(fft, sr), streams, ring_frames=fft) as b:
        assert b.ring_frames == fft
        b.push_audio(np.ascontiguousarray(x[..., :2000]))
        b.push_audio(np.ascontiguousarray(x[..., 2000:]))
        full = check_slices_and_repeats(b, "delay")
    assert full["valid"].tolist() == [1, 1, 1, 0, 1] and full["lag"][:3].tolist() == [3, 2, 11]
    want = ref.delay(x, fft, sr)
    keep = [0, 1, 2, 3]  # (independent noise is drawn here without the CPU test's check of its margins: bit identity only)
    assert ref.mismatches(full[keep], want[keep]) == []


def test_fresh_reset_and_hidden_streams():
    fft, streams, sr = 1024, 4, 48000
    with wf.SpectrumBatch(_cfg(fft, sr), streams) as b:
        rng = np.random.default_rng(13)
        x = np.stack([ref.stream(k, rng, b.ring_frames + HOP, fft) for k in ("white +3", "white -7.3", "dual mono", "inverted L-1")])
        zero = ref.zero_record(fft, streams)
        assert ref.mismatches(zero, ref.delay(np.zeros((streams, 2, fft), np.float32), fft, sr)) == []
        assert b.delay().tobytes() == zero.tobytes()  # freshly created, both channels silent: valid = 0 and every field 0
        b.set_hidden(np.array([0, 1, 0, 0], np.uint8))
        b.push_audio(x)
        b.tick()
        before = b.delay()
        _check(before, x, fft, sr, "one stream hidden")  # the hidden stream's ring reads like any other
        assert np.all(before["valid"] == 1) and before["lag"].tolist() == [3, -7, 0, 255]
        b.reset(2, 1)
        after = b.delay()
    assert after[2:3].tobytes() == zero[:1].tobytes()
    keep = [0, 1, 3]
    assert after[keep].tobytes() == before[keep].tobytes()


def test_refusals():
    L = wf.lib()
    with wf.SpectrumBatch(wf.Config.defaults(waveform=1, stereo=1, width=640, meter_ms=100), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_DELAY) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.delay()
        assert e.value.code == ERR_INVALID and "waveform batch" in str(e.value) and "delay" in str(e.value), str(e.value)
        out = np.empty(2, binding.DELAY_DTYPE)
        assert L.wf_hip_read(b.h, binding.OUT_DELAY, 0, 2, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID
        assert b"delay" in L.wf_hip_last_error(b.h)
    with wf.SpectrumBatch(_cfg(1024, capture_channels=1, stereo=0), 2) as b:  # one captured channel: nothing to compare
        assert b.capture_channels == 1 and L.wf_hip_output_bytes(b.h, binding.OUT_DELAY) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.delay()
        assert e.value.code == ERR_INVALID and "two captured channels" in str(e.value) and "delay" in str(e.value), str(e.value)
        assert b.thd().shape == (2,)  # the other readers of such a batch are unharmed
    with wf.SpectrumBatch(_cfg(1024), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_DELAY) == 320  # before the first read
        check_abi_refusals(b, binding.OUT_DELAY, binding.DELAY_DTYPE, 2, ref.zero_record(1024, 2))


def test_nothing_else_moves_on_a_twin(monkeypatch):
    """twin handles over 20 ticks, one of them read every tick: rows, bars and t-smooth -- and every other output -- stay
    bit-identical between the two, guard bytes behind every block intact (wf_hip_sync checks them)"""
    monkeypatch.setenv("WF_HIP_CANARY", "1")
    streams, hop, fft, sr = 3, 800, 4096, 48000
    names = ("decibels", "bars", "signal", "pitch", "stereo", "scope", "gonio", "bits", "thd")
    cfg = _cfg(fft, sr, tsmoothing=binding.TSMOOTH["exponential"])
    with wf.SpectrumBatch(cfg, streams) as read, wf.SpectrumBatch(cfg, streams) as quiet:
        for t in range(20):
            a = synth.block(ref.GPU_SEED, 0, streams, 2, t * hop, hop)
            for b in (read, quiet):
                b.push_audio(a)
                b.tick()
            got = read.delay()
            assert np.asarray(read.decibels()).tobytes() == np.asarray(quiet.decibels()).tobytes(), t
            assert np.asarray(read.bars()).tobytes() == np.asarray(quiet.bars()).tobytes(), t
            assert read.tsmooth().tobytes() == quiet.tsmooth().tobytes(), t
        read.sync()
        quiet.sync()
        for n in names:
            assert np.asarray(getattr(read, n)()).tobytes() == np.asarray(getattr(quiet, n)()).tobytes(), n
        assert read.delay().tobytes() == got.tobytes() == quiet.delay().tobytes()  # the twin's first read
        read.sync()
        quiet.sync()
    assert np.all(got["window"] == fft) and np.all(got["valid"] == 1)


def test_three_shards_match_one_handle():
    fft, sr = 2048, 48000
    cfg = _cfg(fft, sr)
    streams = 7
    kinds = ("white +3", "white -7.3", "inverted L-1", "silent ch0", "-100 dB +11", "dual mono", "tones +2.25")
    rng = np.random.default_rng(100)
    x = np.stack([ref.stream(k, rng, 5 * HOP, fft) for k in kinds])
    with wf.SpectrumBatch(cfg, streams) as one, wf.MultiBatch(cfg, streams, [0, 0, 0]) as m:
        for t in range(5):
            a = np.ascontiguousarray(x[..., t * HOP:(t + 1) * HOP])
            one.push_audio(a)
            m.push_audio(a)
            one.tick()
            m.tick()
        m.sync()
        want = check_shards_match(one, m, "delay", (2, 4))
    assert np.all(want["window"] == fft) and want["valid"].tolist() == [1, 1, 1, 0, 1, 1, 1]
    assert want["lag"].tolist() == [3, -7, 511, 0, 11, 0, 2] and want["polarity"].tolist() == [1, 1, -1, 0, 1, 1, 1]
    _check(want, x, fft, sr, "one handle of the seven streams")


def test_across_the_2_to_the_32_wrap():
    """tests/delay_wrap_child.py: twin handles on the development build, one aged to just below 2^32, walked across the wrap in
    small hops with delay() equal on both and within the bound of the restatement at every hop.  One child process (the release
    library has no test aids)"""
    run_wrap_child("delay_wrap_child.py", 60)
