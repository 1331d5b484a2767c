"""Oscilloscope on the device (WF_HIP_OUT_SCOPE) against the float64 restatement (tests/scope_ref.py) of the frames pushed: windows
of 128, 1024, 2000, 4096 and 8192 (the cap) frames, a meter batch, one captured channel, uneven packets; a trace that stands
still; bit identity across push paths, repeated reads and slices; fresh, reset and hidden streams; refusals; nothing else moving;
a three-shard group.

The bound against the restatement is derived, not measured (include/wf_hip.h, "oscilloscope"; scope_ref.mismatches): the
definition consists of comparisons, exact float64 operations and single correctly rounded operations, so every integer field is
equal, lo and hi are equal as values, and frac is equal -- or within one float32 ulp, should the device's float64 division not be
correctly rounded; the comparison prints which of the two held.  test_scope_cpu.py shows that every stream of every case here
triggers and has a period, so none of this passes on free-running streams."""
import ctypes as C

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import scope_ref as ref
from pcm_convert import captured
from tools import synth
from measure_common import Hip, check_abi_refusals, check_shards_match, check_slices_and_repeats, packets

pytestmark = pytest.mark.gpu
ERR_INVALID = -1
SEED = ref.GPU_SEED
HOP = 801


def _cfg(fft=4096, sr=48000, channels=2, **kw):
    return wf.Config.defaults(**{**dict(fft_size=fft, sample_rate=sr, capture_channels=channels, stereo=1 if channels == 2 else 0, slope=1.0,
                                        bars=1, floor_db=-70), **kw})


def _check(got, frames, w, what=""):
    assert got.dtype == binding.SCOPE_DTYPE and got.shape == (frames.shape[0],)
    print(f"{what}: P {int(got['window'][0])}, V {int(got['view'][0])}, K {int(got['columns'][0])}, starts {got['start'].tolist()}, "
          f"triggered {got['triggered'].tolist()}, periods {got['period'].tolist()}, frac {got['frac'].tolist()}: "
          f"frac {ref.frac_outcome(got, frames, w)} (to the restatement's float32)")
    bad = ref.mismatches(got, frames, w)
    assert not bad, bad[:8]


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=ref.case_id)
def test_scope_equals_the_restatement_of_the_frames(case):
    fft, sr, ch, kw, w = case
    x = ref.case_audio(case)  # one ring and P / 2 + 3 frames: the window wraps the ring and ends at an odd position
    with wf.SpectrumBatch(_cfg(fft, sr, ch, **kw), x.shape[0]) as b:
        assert b.fft_size == w and b.ring_frames == ref.ring_frames(w)
        assert wf.lib().wf_hip_output_bytes(b.h, binding.OUT_SCOPE) == 4128  # before the first read
        for lo, hi in packets(np.random.default_rng(w), x.shape[-1], 699):
            b.push_audio(np.ascontiguousarray(x[:, :, lo:hi]))
        got = b.scope()
    p, v, k = ref.geometry(w)
    assert np.all(got["window"] == p) and np.all(got["view"] == v) and np.all(got["columns"] == k)
    assert np.all(got["triggered"] == 1) and np.all(got["period"] > 0)
    if ch == 1:
        assert not got["lo"][:, 1].any() and not got["hi"][:, 1].any()
    assert not got["lo"][:, :, k:].any() and not got["hi"][:, :, k:].any()
    _check(got, x, w, ref.case_id(case))


def test_the_trace_stands_still():
    """a wave of integer period 100 read from a table, pushed in 12 hops of 801 frames (no multiple of 100) after the window has
    filled: every read triggers with period 100 and draws the first read's picture bit for bit, from another place in the ring"""
    t, fft, hops = 100, 1024, 12
    x = ref.table_periodic(t, fft + 37 + hops * HOP)
    x = np.ascontiguousarray(np.broadcast_to(x, (2, 2, x.size)))
    with wf.SpectrumBatch(_cfg(fft), 2) as b:
        at = fft + 37
        b.push_audio(np.ascontiguousarray(x[..., :at]))
        reads = []
        for _ in range(hops):
            b.push_audio(np.ascontiguousarray(x[..., at:at + HOP]))
            at += HOP
            reads.append(b.scope())
            assert not ref.mismatches(reads[-1], x[..., :at], fft)
    for r in reads:
        assert np.all(r["triggered"] == 1) and np.all(r["period"] == t)
        assert r["lo"].tobytes() == reads[0]["lo"].tobytes() and r["hi"].tobytes() == reads[0]["hi"].tobytes()
        assert np.array_equal(r["frac"], reads[0]["frac"])
    starts = [int(r["start"][0]) for r in reads]
    print(f"starts {starts}")
    assert len(set(starts)) >= 2  # the view really moved in the ring


def test_every_push_path_counts():
    """the same frames through push_audio, wf_hip_push_pcm (s16 interleaved: every value exact in float32) and
    push_audio_device read bit-identically"""
    streams, fft, frames = 3, 1024, 801
    rng = np.random.default_rng(2)
    wave = (8000.0 * np.sin(2.0 * np.pi * np.arange(6 * frames) / 57.3))[None, :, None]
    pkts = [(wave[:, i * frames:(i + 1) * frames] + rng.integers(-500, 500, (streams, frames, 2))).astype(np.int16) for i in range(6)]
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
            reads[path] = b.scope()
    assert reads["pcm"].tobytes() == reads["float"].tobytes() and reads["device"].tobytes() == reads["float"].tobytes()
    hist = np.concatenate([captured(pkt, True, 0, 2) for pkt in pkts], axis=2)
    assert np.all(reads["float"]["triggered"] == 1)
    _check(reads["float"], hist, fft, "s16 packets")


def test_repeated_reads_and_slices():
    """a slice as a handle's first read equals the entry of the full read; reads with nothing in between, and a read after a
    tick, are bit-identical"""
    fft, streams = 2048, 5
    x = ref.audio(np.random.default_rng(11), streams, 3001, fft)
    with wf.SpectrumBatch(_cfg(fft), streams, ring_frames=fft) as b:
        assert b.ring_frames == fft
        b.push_audio(np.ascontiguousarray(x[..., :2000]))
        b.push_audio(np.ascontiguousarray(x[..., 2000:]))
        full = check_slices_and_repeats(b, "scope")
    _check(full, x, fft, "the window is the whole ring")


def test_fresh_reset_and_hidden_streams():
    fft, streams = 1024, 4
    with wf.SpectrumBatch(_cfg(fft), streams) as b:
        x = ref.audio(np.random.default_rng(13), streams, b.ring_frames + HOP, fft)
        silence = ref.scope(np.zeros((1, 2, fft), np.float32), fft)
        assert (silence["start"][0], silence["triggered"][0], silence["period"][0], silence["frac"][0]) == (512, 0, 0, 0.0)
        assert (silence["window"][0], silence["view"][0], silence["columns"][0]) == (1024, 512, 256) and not silence["lo"].any()
        assert b.scope().tobytes() == np.repeat(silence, streams).tobytes()  # freshly created: zeros, a free run, the geometry set
        b.set_hidden(np.array([0, 1, 0, 0], np.uint8))
        b.push_audio(x)
        b.tick()
        before = b.scope()
        _check(before, x, fft, "one stream hidden")  # the hidden stream's ring reads like any other
        assert np.all(before["triggered"] == 1)
        b.reset(2, 1)
        after = b.scope()
    assert after[2:3].tobytes() == silence.tobytes()
    keep = [0, 1, 3]
    assert after[keep].tobytes() == before[keep].tobytes()


def test_refusals():
    L = wf.lib()
    with wf.SpectrumBatch(wf.Config.defaults(waveform=1, stereo=1, width=640, meter_ms=100), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_SCOPE) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.scope()
        assert e.value.code == ERR_INVALID and "waveform batch" in str(e.value) and "oscilloscope" in str(e.value), str(e.value)
        out = np.empty(2, binding.SCOPE_DTYPE)
        assert L.wf_hip_read(b.h, binding.OUT_SCOPE, 0, 2, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID
        assert b"oscilloscope" in L.wf_hip_last_error(b.h)
    with wf.SpectrumBatch(_cfg(1024, meter=1, bars=0, meter_ms=1), 2) as b:  # a meter buffer of 48 frames
        assert b.fft_size == 48 and L.wf_hip_output_bytes(b.h, binding.OUT_SCOPE) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.scope()
        assert e.value.code == ERR_INVALID and "oscilloscope" in str(e.value) and "64 frames" in str(e.value), str(e.value)
    with wf.SpectrumBatch(_cfg(1024), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_SCOPE) == 4128  # before the first read
        out = check_abi_refusals(b, binding.OUT_SCOPE, binding.SCOPE_DTYPE, 2)
        assert np.all(out["window"][:2] == 1024) and np.all(out["start"][:2] == 512)


def test_nothing_else_moves(monkeypatch):
    """twin handles for 12 ticks, one of them read between the ticks: rows, bars, tsmooth, last_silent and every other measurement
    output stay bit-identical; guard bytes behind every block intact (wf_hip_sync checks them); a handle's first read equals its
    twin's thirteenth"""
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
            b.scope()
        b.sync()
        a.sync()
        for name in ("decibels", "bars", "tsmooth", "last_silent", "signal", "bands", "peaks", "pitch", "stereo", "cq"):
            assert np.asarray(getattr(a, name)()).tobytes() == np.asarray(getattr(b, name)()).tobytes(), name
        first = a.scope()
        assert first.tobytes() == b.scope().tobytes()
        a.sync()
        b.sync()
    hist = np.concatenate([synth.block(SEED, 0, streams, 2, t * hop, hop) for t in range(12)], axis=2)
    assert hist.shape[-1] >= 4096
    assert not ref.mismatches(first, hist, 4096)


def test_three_shards_match_one_handle():
    cfg = _cfg(2048)
    streams = 7
    with wf.SpectrumBatch(cfg, streams) as one, wf.MultiBatch(cfg, streams, [0, 0, 0]) as m:
        for t in range(5):
            x = ref.audio(np.random.default_rng(100 + t), streams, HOP, 2048)
            one.push_audio(x)
            m.push_audio(x)
            one.tick()
            m.tick()
        m.sync()
        want = check_shards_match(one, m, "scope", (2, 4))
        assert np.all(want["window"] == 2048) and want["hi"][:, :, :256].any()
