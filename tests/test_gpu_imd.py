"""Two-tone intermodulation analyser on the device (WF_HIP_OUT_IMD) against the float64 restatement (tests/imd_ref.py) of the frames
pushed: windows of 512 (the smallest), 2048 (shorter than the FFT), 8192 and 8192 of 16384 (the cap) frames, a meter batch, one
captured channel and a mono mixdown of two, six streams of different kinds each -- a twin tone and a low tone under a high one
through a polynomial, two pure sines, one sine, an octave, a silent channel next to a live one on either side -- in uneven packets;
bit identity across push paths, repeated reads and slices; fresh, reset and hidden streams; refusals; nothing else moving on a twin,
the distortion analyser included, whose tables it shares; a three-shard group; the 2^32 wrap of the write positions.

The bound against the restatement is derived, not measured (imd_ref's docstring): both sides work in float64 from the same float32
samples and differ in the order of operations, and tests/test_imd_cpu.py shows on these very seeds and shapes that no argmax, no
product's or harmonic's bin and not the 30 dB decision is near a tie and that two orderings agree to 1e-7 dB, so one float32
rounding is all that can separate them."""
import ctypes as C

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import imd_ref as ref
from pcm_convert import captured
from tools import synth
from measure_common import Hip, check_abi_refusals, check_shards_match, check_slices_and_repeats, packets, run_wrap_child

pytestmark = pytest.mark.gpu
ERR_INVALID = -1
HOP = 801
ENTRY = 368


def _cfg(fft=4096, sr=48000, **kw):
    return wf.Config.defaults(**{**dict(fft_size=fft, sample_rate=sr, capture_channels=2, stereo=1, slope=1.0, bars=1, floor_db=-70), **kw})


def _check(got, frames, w, sr, what=""):
    """every entry of `got` within the bound of the restatement of `frames`, each figure printed first"""
    want = ref.imd(frames, w, sr)
    assert got.dtype == binding.IMD_DTYPE and got.shape == want.shape
    g, f = got["ch"], want["ch"]
    with np.errstate(invalid="ignore"):
        worst = {n: float(np.nanmax(np.where(np.isfinite(f[n]), np.abs(g[n].astype(np.float64) - f[n].astype(np.float64)), 0.0)))
                 for n in ref.DB_FIELDS}
        hz = max(float(np.max(np.abs(g[n] - f[n]) / np.maximum(f[n], 1e-300))) for n in ref.HZ_FIELDS)
    print(f"{what}: P {got['window'].tolist()}, tones {g['tones'].tolist()}, bins {g['lo_bin'].tolist()} + {g['hi_bin'].tolist()}, products "
          f"{[[hex(v) for v in row] for row in g['products'].tolist()]}, imd {g['imd_db'].tolist()}, td+n {g['tdn_db'].tolist()}, worst "
          f"|got - want| {worst}, lo_hz / hi_hz worst relative {hz:.3g}")
    bad = ref.mismatches(got, want)
    assert not bad, bad[:8]
    assert not got["reserved"].any() and not g["reserved"].any()
    assert np.array_equal(g["valid"], (g["tones"] == 2).astype(np.uint32))
    return want


def _zero(p, streams):
    s = np.zeros((), binding.IMD_DTYPE)
    s["window"] = p
    return np.repeat(s, streams)


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=ref.case_id)
def test_imd_equals_the_restatement_of_the_frames(case):
    fft, sr, kw, w, channels = case
    x = ref.case_audio(case)  # one ring and P / 2 + 3 frames: the window wraps the ring and ends at an odd position
    with wf.SpectrumBatch(_cfg(fft, sr, **kw), x.shape[0]) as b:
        assert b.fft_size == w and b.ring_frames == ref.ring_frames(w) and b.capture_channels == channels
        assert wf.lib().wf_hip_output_bytes(b.h, binding.OUT_IMD) == ENTRY  # before the first read
        for lo, hi in packets(np.random.default_rng(w), x.shape[-1], 700):
            b.push_audio(np.ascontiguousarray(x[:, :, lo:hi]))
        got = b.imd()
    p = ref.window_frames(w)
    assert np.all(got["window"] == p)
    _check(got, x, w, sr, ref.case_id(case))
    # silence reads no tone, one sine one; the twin's tones lie 10 bins apart at P = 512, within the 2H of one tone
    tones = {"silence": 0, "single": 1, "twin": 2 if p > 512 else 1}
    want = np.array([[tones.get(k, 2) for k in pair[:channels]] for pair in ref.STREAM_KINDS])
    assert np.array_equal(got["ch"]["tones"][:, :channels], want)
    if channels == 1:
        assert not got["ch"][:, 1].tobytes().strip(b"\0")  # all zero bytes


def test_every_push_path_counts():
    """the same s16 frames through push_audio, wf_hip_push_pcm (s16 interleaved: every value exact in float32) and
    push_audio_device read bit-identically"""
    streams, fft, frames, sr = 3, 1024, 801, 48000
    rng = np.random.default_rng(2)
    n = np.arange(6 * frames, dtype=np.float64)
    pairs = ((21.37, 133.21), (33.87, 301.13), (57.21, 240.59))  # bins of 1024
    wave = np.stack([32768.0 * ref.polynomial(ref.two_tones(n, lo / fft, hi / fft, 0.4, 0.3), 1e-2, 1e-2) for lo, hi in pairs])[:, :, None]
    pkts = [np.round(wave[:, i * frames:(i + 1) * frames] + rng.integers(-3, 4, (streams, frames, 2))).astype(np.int16) for i in range(6)]
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
            reads[path] = b.imd()
    assert reads["pcm"].tobytes() == reads["float"].tobytes() and reads["device"].tobytes() == reads["float"].tobytes()
    hist = np.concatenate([captured(pkt, True, 0, 2) for pkt in pkts], axis=2)
    want = _check(reads["float"], hist, fft, sr, "s16 packets")
    assert np.all(want["ch"]["valid"] == 1) and want["ch"]["lo_bin"][:, 0].tolist() == [21, 34, 57]
    assert want["ch"]["hi_bin"][:, 0].tolist() == [133, 301, 241] and np.all(want["ch"]["products"] & 1)


def test_repeated_reads_and_slices():
    """a slice as a handle's first read equals the entry of the full read; reads with nothing in between, and a read after a
    tick, are bit-identical.  The window is the whole ring"""
    fft, streams, sr = 2048, 5, 48000
    rng = np.random.default_rng(11)
    kinds = ("twin", "wide", "single", "silence", "octave")
    x = np.stack([np.stack([ref.signal(k, rng, 3001, fft), ref.signal("wide", rng, 3001, fft)]) for k in kinds])
    with wf.SpectrumBatch(_cfg(fft, sr), streams, ring_frames=fft) as b:
        assert b.ring_frames == fft
        b.push_audio(np.ascontiguousarray(x[..., :2000]))
        b.push_audio(np.ascontiguousarray(x[..., 2000:]))
        full = check_slices_and_repeats(b, "imd")
    _check(full, x, fft, sr, "the window is the whole ring")
    assert full["ch"]["tones"][:, 0].tolist() == [2, 2, 1, 0, 2]


def test_fresh_reset_and_hidden_streams():
    fft, streams, sr = 1024, 4, 48000
    with wf.SpectrumBatch(_cfg(fft, sr), streams) as b:
        rng = np.random.default_rng(13)
        x = np.stack([np.stack([ref.signal(k, rng, b.ring_frames + HOP, fft), ref.signal("twin", rng, b.ring_frames + HOP, fft)])
                      for k in ("twin", "wide", "octave", "clean")])
        zero = _zero(fft, streams)
        assert ref.mismatches(zero, ref.imd(np.zeros((streams, 2, fft), np.float32), fft, sr)) == []
        assert b.imd().tobytes() == zero.tobytes()  # freshly created: zeros, tones = 0, valid = 0 and every field 0
        b.set_hidden(np.array([0, 1, 0, 0], np.uint8))
        b.push_audio(x)
        b.tick()
        before = b.imd()
        _check(before, x, fft, sr, "one stream hidden")  # the hidden stream's ring reads like any other
        assert np.all(before["ch"]["valid"] == 1)
        b.reset(2, 1)
        after = b.imd()
    assert after[2:3].tobytes() == zero[:1].tobytes()
    keep = [0, 1, 3]
    assert after[keep].tobytes() == before[keep].tobytes()


def test_refusals():
    L = wf.lib()
    with wf.SpectrumBatch(wf.Config.defaults(waveform=1, stereo=1, width=640, meter_ms=100), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_IMD) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.imd()
        assert e.value.code == ERR_INVALID and "waveform batch" in str(e.value) and "intermodulation" in str(e.value), str(e.value)
        out = np.empty(2, binding.IMD_DTYPE)
        assert L.wf_hip_read(b.h, binding.OUT_IMD, 0, 2, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID
        assert b"intermodulation" in L.wf_hip_last_error(b.h)
    with wf.SpectrumBatch(_cfg(256), 2) as b:  # 17 bins below a tone and room for the regions above it: at least 512 frames
        assert L.wf_hip_output_bytes(b.h, binding.OUT_IMD) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.imd()
        assert e.value.code == ERR_INVALID and "512" in str(e.value) and "intermodulation" in str(e.value), str(e.value)
        assert b.bits().shape == (2,)  # the other readers of such a batch are unharmed
    with wf.SpectrumBatch(_cfg(1024), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_IMD) == ENTRY  # before the first read
        check_abi_refusals(b, binding.OUT_IMD, binding.IMD_DTYPE, 2, _zero(1024, 2))


def test_nothing_else_moves_on_a_twin(monkeypatch):
    """twin handles over 20 ticks, one of them read every tick: every other output stays bit-identical between the two, the
    distortion analyser -- whose tables the read one has built -- included, guard bytes behind every block intact (wf_hip_sync
    checks them)"""
    monkeypatch.setenv("WF_HIP_CANARY", "1")
    streams, hop, fft, sr = 3, 800, 4096, 48000
    names = ("decibels", "bars", "signal", "pitch", "stereo", "scope", "gonio", "bits", "thd")
    with wf.SpectrumBatch(_cfg(fft, sr), streams) as read, wf.SpectrumBatch(_cfg(fft, sr), streams) as quiet:
        for t in range(20):
            a = synth.block(ref.GPU_SEED, 0, streams, 2, t * hop, hop)
            for b in (read, quiet):
                b.push_audio(a)
                b.tick()
            got = read.imd()
            assert np.asarray(read.decibels()).tobytes() == np.asarray(quiet.decibels()).tobytes(), t
            assert np.asarray(read.bars()).tobytes() == np.asarray(quiet.bars()).tobytes(), t
        read.sync()
        quiet.sync()
        for n in names:  # (thd: on `read` behind the intermodulation analyser's tables, on `quiet` as its own first read)
            assert np.asarray(getattr(read, n)()).tobytes() == np.asarray(getattr(quiet, n)()).tobytes(), n
        assert read.imd().tobytes() == got.tobytes() == quiet.imd().tobytes()  # the twin's first read, behind its thd()
        read.sync()
        quiet.sync()
    hist = np.concatenate([synth.block(ref.GPU_SEED, 0, streams, 2, t * hop, hop) for t in range(20)], axis=2)
    assert np.all(got["window"] == fft) and got["ch"]["valid"].shape == (streams, 2)
    want = ref.imd(hist, fft, sr)
    assert want["ch"]["tones"].tolist() == got["ch"]["tones"].tolist() and want["ch"]["valid"].tolist() == got["ch"]["valid"].tolist()


def test_three_shards_match_one_handle():
    fft, sr = 2048, 48000
    cfg = _cfg(fft, sr)
    streams = 7
    kinds = ("twin", "wide", "octave", "silence", "twin", "single", "clean")
    rng = np.random.default_rng(100)
    x = np.stack([np.stack([ref.signal(k, rng, 5 * HOP, fft), ref.signal("wide", rng, 5 * HOP, fft)]) for k in kinds])
    with wf.SpectrumBatch(cfg, streams) as one, wf.MultiBatch(cfg, streams, [0, 0, 0]) as m:
        for t in range(5):
            a = np.ascontiguousarray(x[..., t * HOP:(t + 1) * HOP])
            one.push_audio(a)
            m.push_audio(a)
            one.tick()
            m.tick()
        m.sync()
        want = check_shards_match(one, m, "imd", (2, 4))
    assert np.all(want["window"] == fft) and want["ch"]["tones"][:, 0].tolist() == [2, 2, 2, 0, 2, 1, 2]
    _check(want, x, fft, sr, "one handle of the seven streams")


def test_across_the_2_to_the_32_wrap():
    """tests/imd_wrap_child.py: twin handles on the development build, one aged to just below 2^32, walked across the wrap in small
    hops with imd() equal on both and within the bound of the restatement at every hop.  One child process (the release library
    has no test aids)"""
    run_wrap_child("imd_wrap_child.py", 60)
