"""Vectorscope on the device (WF_HIP_OUT_GONIO) against the float64 restatement (tests/gonio_ref.py) of the frames pushed: windows
of 128, 1024, 2000, 4096 and 8192 (the cap) frames and a meter batch of 2208, three streams of different kinds each, uneven
packets; the clamp of the range; bit identity across push paths, repeated reads and slices; fresh, reset and hidden streams;
refusals; nothing else moving; a three-shard group; the 2^32 wrap of the write positions.

Every comparison is for equality, and that is derived, not measured (include/wf_hip.h, "vectorscope"; gonio_ref.mismatches): the
definition consists of comparisons, integer counts, exact float64 operations and single correctly rounded operations, so every
field is equal bit for bit.  test_gonio_cpu.py shows that the pictures compared here are spread ones, with the three signs of zoom
among them."""
import ctypes as C

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import gonio_ref as ref
from pcm_convert import captured
from tools import synth
from measure_common import Hip, check_abi_refusals, check_shards_match, check_slices_and_repeats, packets, run_wrap_child

pytestmark = pytest.mark.gpu
ERR_INVALID = -1
SEED = ref.GPU_SEED
HOP = 801
G = ref.GRID


def _cfg(fft=4096, sr=48000, channels=2, **kw):
    return wf.Config.defaults(**{**dict(fft_size=fft, sample_rate=sr, capture_channels=channels, stereo=1 if channels == 2 else 0, slope=1.0,
                                        bars=1, floor_db=-70), **kw})


def _check(got, frames, w, what=""):
    assert got.dtype == binding.GONIO_DTYPE and got.shape == (frames.shape[0],)
    print(f"{what}: P {got['window'].tolist()}, zoom {got['zoom'].tolist()}, peak {got['peak'].tolist()}, occupied {got['occupied'].tolist()}, "
          f"largest cell {got['cell'].max(axis=(1, 2)).tolist()}, in phase {got['in_phase'].tolist()}, out of phase {got['out_phase'].tolist()}")
    bad = ref.mismatches(got, frames, w)
    assert not bad, bad[:8]
    assert np.all(got["cell"].astype(np.int64).sum(axis=(1, 2)) == got["window"])


def _silence(p, streams):
    s = np.zeros((), binding.GONIO_DTYPE)
    s["cell"][G // 2, G // 2] = p
    s["window"], s["occupied"] = p, 1
    return np.repeat(s, streams)


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=ref.case_id)
def test_gonio_equals_the_restatement_of_the_frames(case):
    fft, sr, kw, w, kinds = case
    x = ref.case_audio(case)  # one ring and P / 2 + 3 frames: the window wraps the ring and ends at an odd position
    with wf.SpectrumBatch(_cfg(fft, sr, 2, **kw), x.shape[0]) as b:
        assert b.fft_size == w and b.ring_frames == ref.ring_frames(w)
        assert wf.lib().wf_hip_output_bytes(b.h, binding.OUT_GONIO) == 8224  # before the first read
        for lo, hi in packets(np.random.default_rng(w), x.shape[-1], 700):
            b.push_audio(np.ascontiguousarray(x[:, :, lo:hi]))
        got = b.gonio()
    assert np.all(got["window"] == ref.window_frames(w))
    for k, g in zip(kinds, got):
        if k in ref.PICTURE_KINDS:
            assert g["occupied"] >= 64
    _check(got, x, w, f"{ref.case_id(case)} {kinds}")


def test_the_clamp_of_the_range():
    """audio below 2^-24: the range stays at zoom 24 and the picture shrinks towards the centre"""
    case = ref.GPU_CASES[1]
    x = (ref.case_audio(case).astype(np.float64) * ref.CLAMP_SCALE).astype(np.float32)
    with wf.SpectrumBatch(_cfg(1024), 3) as b:
        b.push_audio(x)
        got = b.gonio()
    assert np.all(got["zoom"] == 24) and np.all(got["peak"] > 0) and np.all(got["peak"] < 2.0 ** -24)
    _check(got, x, 1024, "scaled by 2^-30")


def test_every_push_path_counts():
    """the same frames through push_audio, wf_hip_push_pcm (s16 interleaved: every value exact in float32) and
    push_audio_device read bit-identically"""
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
            reads[path] = b.gonio()
    assert reads["pcm"].tobytes() == reads["float"].tobytes() and reads["device"].tobytes() == reads["float"].tobytes()
    hist = np.concatenate([captured(pkt, True, 0, 2) for pkt in pkts], axis=2)
    assert np.all(reads["float"]["occupied"] >= 64) and np.all(reads["float"]["zoom"] == 1)
    _check(reads["float"], hist, fft, "s16 packets")


def test_repeated_reads_and_slices():
    """a slice as a handle's first read equals the entry of the full read; reads with nothing in between, and a read after a
    tick, are bit-identical"""
    fft, streams = 2048, 5
    rng = np.random.default_rng(11)
    x = np.stack([ref.signal(k, rng, 3001) for k in ("noise", "mono", "lissajous", "loud", "left")])
    with wf.SpectrumBatch(_cfg(fft), streams, ring_frames=fft) as b:
        assert b.ring_frames == fft
        b.push_audio(np.ascontiguousarray(x[..., :2000]))
        b.push_audio(np.ascontiguousarray(x[..., 2000:]))
        full = check_slices_and_repeats(b, "gonio")
    _check(full, x, fft, "the window is the whole ring")


def test_fresh_reset_and_hidden_streams():
    fft, streams = 1024, 4
    # (a mono mixdown still captures two channels: cfg.stereo does not matter)
    with wf.SpectrumBatch(_cfg(fft, stereo=0), streams) as b:
        assert b.capture_channels == 2
        rng = np.random.default_rng(13)
        x = np.stack([ref.signal(k, rng, b.ring_frames + HOP) for k in ("noise", "correlated", "lissajous", "antiphase")])
        silence = _silence(fft, streams)
        assert ref.mismatches(silence, np.zeros((streams, 2, fft), np.float32), fft) == []
        assert b.gonio().tobytes() == silence.tobytes()  # freshly created: zeros, one cell of P, zoom 0
        b.set_hidden(np.array([0, 1, 0, 0], np.uint8))
        b.push_audio(x)
        b.tick()
        before = b.gonio()
        _check(before, x, fft, "one stream hidden")  # the hidden stream's ring reads like any other
        assert np.all(before["occupied"] > 8)
        b.reset(2, 1)
        after = b.gonio()
    assert after[2:3].tobytes() == silence[:1].tobytes()
    keep = [0, 1, 3]
    assert after[keep].tobytes() == before[keep].tobytes()


def test_refusals():
    L = wf.lib()
    with wf.SpectrumBatch(wf.Config.defaults(waveform=1, stereo=1, width=640, meter_ms=100), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_GONIO) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.gonio()
        assert e.value.code == ERR_INVALID and "waveform batch" in str(e.value) and "vectorscope" in str(e.value), str(e.value)
        out = np.empty(2, binding.GONIO_DTYPE)
        assert L.wf_hip_read(b.h, binding.OUT_GONIO, 0, 2, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID
        assert b"vectorscope" in L.wf_hip_last_error(b.h)
    with wf.SpectrumBatch(_cfg(1024, channels=1), 2) as b:  # one captured channel
        assert b.capture_channels == 1 and L.wf_hip_output_bytes(b.h, binding.OUT_GONIO) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.gonio()
        assert e.value.code == ERR_INVALID and "vectorscope" in str(e.value) and "one captured channel" in str(e.value), str(e.value)
        assert b.signal().shape == (2,)  # nothing was enqueued that would trouble the next call
    with wf.SpectrumBatch(_cfg(1024), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_GONIO) == 8224  # before the first read
        check_abi_refusals(b, binding.OUT_GONIO, binding.GONIO_DTYPE, 2, _silence(1024, 2))


def test_a_small_meter_buffer_is_served():
    """there is no lower limit on the window: a meter buffer of 48 frames, less than a wavefront"""
    rng = np.random.default_rng(17)
    with wf.SpectrumBatch(_cfg(1024, meter=1, bars=0, meter_ms=1), 3) as b:
        assert b.fft_size == 48
        x = np.stack([ref.signal(k, rng, b.ring_frames + 21) for k in ("noise", "left", "loud")])
        b.push_audio(x)
        got = b.gonio()
    assert np.all(got["window"] == 48)
    _check(got, x, 48, "meter buffer of 48 frames")


def test_nothing_else_moves(monkeypatch):
    """decibels, bars, scope() and signal() read before and after a gonio() are identical; guard bytes behind every block intact
    (wf_hip_sync checks them)"""
    monkeypatch.setenv("WF_HIP_CANARY", "1")
    streams, hop = 3, 800
    with wf.SpectrumBatch(_cfg(4096), streams) as b:
        for t in range(6):
            b.push_audio(synth.block(SEED, 0, streams, 2, t * hop, hop))
            b.tick()
        names = ("decibels", "bars", "scope", "signal")
        before = {n: np.asarray(getattr(b, n)()).tobytes() for n in names}
        got = b.gonio()
        b.sync()
        for n in names:
            assert np.asarray(getattr(b, n)()).tobytes() == before[n], n
        assert b.gonio().tobytes() == got.tobytes()
        b.sync()
    hist = np.concatenate([synth.block(SEED, 0, streams, 2, t * hop, hop) for t in range(6)], axis=2)
    assert hist.shape[-1] >= 4096
    _check(got, hist, 4096, "between the other readers")


def test_three_shards_match_one_handle():
    cfg = _cfg(2048)
    streams = 7
    kinds = ("noise", "mono", "lissajous", "quiet", "left", "loud", "correlated")
    with wf.SpectrumBatch(cfg, streams) as one, wf.MultiBatch(cfg, streams, [0, 0, 0]) as m:
        for t in range(5):
            rng = np.random.default_rng(100 + t)
            x = np.stack([ref.signal(k, rng, HOP) for k in kinds])
            one.push_audio(x)
            m.push_audio(x)
            one.tick()
            m.tick()
        m.sync()
        want = check_shards_match(one, m, "gonio", (2, 4))
        assert np.all(want["window"] == 2048) and np.all(want["occupied"] > 8) and len(set(want["zoom"].tolist())) >= 3


def test_across_the_2_to_the_32_wrap():
    """tests/gonio_wrap_child.py: twin handles on the development build, one aged to just below 2^32, walked across the wrap in small
    hops with gonio() equal at every hop.  One child process (the release library has no test aids)"""
    run_wrap_child("gonio_wrap_child.py", 60)
