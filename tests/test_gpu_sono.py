"""Sonogram on the device (WF_HIP_OUT_SONO) against the float64 restatement (tests/sono_ref.py) of the frames pushed: rings of 2048
to 32768 frames (4, 12, 28, 60 and 64 columns), one and two captured channels, a meter batch, three streams each -- noise, a burst
and tones behind silence with a dead right channel, a fast chirp -- in packets of unequal odd sizes; columns that stand still
between reads; bit identity across push paths, repeated reads and slices; fresh, reset, hidden and paused streams; refusals;
nothing else moving; a three-shard group; the 2^32 wrap of the write positions.

The bound (sono_ref.mismatches; include/wf_hip.h, "sonogram"): header words and every -inf of the restatement exactly; a cell whose
band power is at least 1e-9 of its column's largest within two float32 ulps of the restatement's float32 -- a float64 transform of
1024 points leaves |X| with an absolute error of about 1e-15 of the column's rms, at that ratio below 1e-10 dB against a float32
ulp of 4e-6 dB at -60 dB, and the second ulp is for a value on a rounding boundary --; the remaining cells with their linear power
within 1e-10 of the column's largest.  The noise streams pass by the first arm alone (test_sono_cpu.py shows they can)."""
import ctypes as C

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import sono_ref as ref
from pcm_convert import captured
from tools import synth
from measure_common import Hip, check_abi_refusals, check_shards_match, check_slices_and_repeats, run_wrap_child

pytestmark = pytest.mark.gpu
ERR_INVALID = -1
P, H = ref.P, ref.H
ENTRY = 32800


def _cfg(fft=4096, sr=48000, channels=2, **kw):
    return wf.Config.defaults(**{**dict(fft_size=fft, sample_rate=sr, capture_channels=channels, stereo=1 if channels == 2 else 0, slope=1.0,
                                        bars=1, floor_db=-70), **kw})


def _hist(wpos0, *pushed):
    """the frames behind a fresh handle's counter: wpos0 zeros of create, then what was pushed"""
    first = pushed[0]
    return np.concatenate([np.zeros(first.shape[:2] + (wpos0,), np.float32), *pushed], axis=2)


def _check(got, hist, sr, ring_cap, what="", noise=(0,)):
    """against the restatement of `hist` (its end is the counter); the streams `noise` must pass by the first arm alone (the
    cases' noise stream, for which test_sono_cpu.py shows that they can)"""
    assert got.dtype == binding.SONO_DTYPE and got.shape == (hist.shape[0],)
    bad, arm2 = ref.mismatches(got, hist, hist.shape[-1], sr, ring_cap)
    print(f"{what}: T {got['columns'].tolist()}, newest {got['newest'].tolist()}, cells by the second arm per stream {None if arm2 is None else arm2.tolist()}, "
          f"loudest cell {np.max(got['db'], axis=(1, 2, 3)).tolist()}")
    assert not bad, bad[:8]
    for s in noise:
        assert arm2[s] == 0, (what, s, arm2.tolist())


def _fresh(streams, ring_cap, wpos, sr=48000):
    s = np.zeros((), binding.SONO_DTYPE)
    s["db"] = -np.inf
    s["columns"], s["newest"], s["window"], s["hop"] = ref.columns(ring_cap), wpos // H, P, H
    s["first_covered"], s["end_covered"] = ref.covered(sr)
    return np.repeat(s, streams)


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=ref.case_id)
def test_sono_equals_the_restatement_of_the_frames(case, monkeypatch):
    fft, sr, ch, kw, ring_frames, ring_cap, t = case
    if ring_cap == 16384:  # guard bytes behind every block, checked by wf_hip_sync
        monkeypatch.setenv("WF_HIP_CANARY", "1")
    x = ref.case_audio(case)
    wpos0 = ref.case_wpos0(case)
    with wf.SpectrumBatch(_cfg(fft, sr, ch, **kw), x.shape[0], ring_frames=ring_frames) as b:
        assert b.ring_frames == ring_cap and b.capture_channels == ch and ref.columns(ring_cap) == t
        assert wf.lib().wf_hip_output_bytes(b.h, binding.OUT_SONO) == ENTRY  # before the first read
        assert b.sono().tobytes() == _fresh(3, ring_cap, wpos0, sr).tobytes()  # freshly created: zeros
        for lo, hi in ref.packets(np.random.default_rng(ring_cap), x.shape[-1]):
            b.push_audio(np.ascontiguousarray(x[:, :, lo:hi]))
        got = b.sono()
        b.sync()
        again = b.sono()
        b.sync()
    assert got.tobytes() == again.tobytes()
    hist = _hist(wpos0, x)
    assert hist.shape[-1] % H != 0 and np.all(got["columns"] == t) and np.all(got["newest"] == hist.shape[-1] // H)
    assert np.all(np.isneginf(got["db"][:, :, t:]))
    if ch == 1:
        assert np.all(np.isneginf(got["db"][:, 1]))
    else:
        assert np.all(np.isneginf(got["db"][1, 1])) and np.all(np.isfinite(got["db"][0, :, :t]))
    _check(got, hist, sr, ring_cap, ref.case_id(case))


def test_columns_stand_still():
    """read, push 300 frames, read again: newest advances by the hops completed and every column in both reads is the same bytes
    at its new age"""
    case = ref.GPU_CASES[4]
    fft, sr, ch, kw, ring_frames, ring_cap, t = case
    x = ref.case_audio(case)
    more = ref.signal("noise", np.random.default_rng(5), 300)[None].repeat(3, axis=0)
    with wf.SpectrumBatch(_cfg(fft, sr, ch), 3, ring_frames=ring_frames) as b:
        b.push_audio(x)
        one = b.sono()
        b.push_audio(more)
        two = b.sono()
    wpos = fft + x.shape[-1]
    d = (wpos + 300) // H - wpos // H
    assert d in (1, 2) and np.all(two["newest"] - one["newest"] == d) and np.all(one["newest"] == wpos // H)
    for a in range(t - d):
        assert two["db"][:, :, a + d].tobytes() == one["db"][:, :, a].tobytes(), a
    assert not np.array_equal(two["db"][:, :, 0], one["db"][:, :, 0])
    _check(two, _hist(fft, x, more), sr, ring_cap, "300 frames later")


def test_every_push_path_counts():
    """the same frames through push_audio, the pinned asynchronous push, two ragged pushes per packet, wf_hip_push_pcm (s16
    interleaved: every value exact in float32) and push_audio_device read bit-identically; push_synth and muted packets advance
    the counter and read as the restatement of what they leave in the rings"""
    streams, fft, frames, ring_cap = 3, 1024, 801, 4096
    rng = np.random.default_rng(2)
    wave = (8000.0 * np.sin(2.0 * np.pi * np.arange(6 * frames) / 57.3))[None, :, None]
    pkts = [(wave[:, i * frames:(i + 1) * frames] + rng.integers(-5000, 5000, (streams, frames, 2))).astype(np.int16) for i in range(6)]
    convs = [np.ascontiguousarray(captured(pkt, True, 0, 2)) for pkt in pkts]  # [streams, 2, frames] float32
    split = np.array([0, int(0.4 * frames), frames], np.uint32)  # a packet in two ragged pushes: the streams differ in how it is cut
    hip = Hip()
    reads = {}
    for path in ("float", "pinned", "ragged", "pcm", "device", "synth", "muted"):
        with wf.SpectrumBatch(_cfg(fft), streams) as b:
            assert b.ring_frames == ring_cap
            for i, (pkt, conv) in enumerate(zip(pkts, convs)):
                if path == "float":
                    b.push_audio(conv)
                elif path == "pinned":
                    pin = wf.PinnedBuffer((streams, 2, frames))
                    pin.array[...] = conv
                    b.push_audio_async(pin, streams, frames, i & 1)
                    b.sync()
                    pin.close()
                elif path == "ragged":
                    for cnt, off in ((split, np.zeros(streams, np.uint32)), (np.uint32(frames) - split, split)):
                        mx = int(cnt.max())
                        pin = wf.PinnedBuffer((streams, 2, mx))
                        pin.array[...] = 0
                        for s in range(streams):
                            pin.array[s, :, :cnt[s]] = conv[s, :, off[s]:off[s] + cnt[s]]
                        b.push_audio_ragged_async(pin, cnt, mx, 0)
                        b.sync()
                        pin.close()
                elif path == "pcm":
                    b.push_pcm(pkt, interleaved=True)
                elif path == "device":
                    d = hip.upload(conv)
                    b.push_audio_device(d, streams, frames)
                    b.sync()
                    assert hip.free(d) == 0
                elif path == "synth":
                    b.push_synth(synth.DEFAULT_SEED, i * frames, frames)
                elif i % 2:
                    b.push_audio_muted(conv)
                else:
                    b.push_audio(conv)
            reads[path] = b.sono()
    for path in ("pinned", "ragged", "pcm", "device"):
        assert reads[path].tobytes() == reads["float"].tobytes(), path
    for path in reads:
        assert np.all(reads[path]["newest"] == (fft + 6 * frames) // H), path  # every path counts
    _check(reads["float"], _hist(fft, *convs), 48000, ring_cap, "s16 packets", noise=())
    _check(reads["synth"], _hist(fft, synth.block(synth.DEFAULT_SEED, 0, streams, 2, 0, 6 * frames)), 48000, ring_cap, "push_synth", noise=())
    muted = [c if i % 2 == 0 else np.zeros_like(c) for i, c in enumerate(convs)]
    _check(reads["muted"], _hist(fft, *muted), 48000, ring_cap, "every other packet muted", noise=())
    assert reads["muted"].tobytes() != reads["float"].tobytes()


def test_repeated_reads_and_slices():
    """a slice as a handle's first read equals the entry of the full read; reads with nothing in between, and a read after a
    tick, are bit-identical"""
    streams, fft = 5, 2048
    rng = np.random.default_rng(11)
    x = np.stack([ref.signal(k, rng, 5001) for k in ("noise", "chirp", "burst", "noise", "chirp")])
    with wf.SpectrumBatch(_cfg(fft), streams) as b:
        assert b.ring_frames == 4096
        b.push_audio(np.ascontiguousarray(x[..., :2000]))
        b.push_audio(np.ascontiguousarray(x[..., 2000:]))
        full = check_slices_and_repeats(b, "sono")
    _check(full, _hist(fft, x), 48000, 4096, "five streams", noise=())


def test_fresh_reset_hidden_and_paused_streams():
    fft, streams, ring_cap = 1024, 4, 4096
    with wf.SpectrumBatch(_cfg(fft, stereo=0), streams) as b:  # (a mono mixdown still captures two channels)
        assert b.capture_channels == 2 and b.ring_frames == ring_cap
        rng = np.random.default_rng(13)
        x = np.stack([ref.signal(k, rng, ring_cap + 801) for k in ("noise", "chirp", "noise", "chirp")])
        assert b.sono().tobytes() == _fresh(streams, ring_cap, fft).tobytes()
        b.set_hidden(np.array([0, 1, 0, 3], np.uint8))  # hidden, paused
        b.push_audio(x)
        b.tick()
        before = b.sono()
        _check(before, _hist(fft, x), 48000, ring_cap, "one stream hidden, one paused", noise=())
        b.reset(2, 1)
        after = b.sono()
    assert after[2:3].tobytes() == _fresh(1, ring_cap, fft).tobytes()  # as a fresh one: the counter starts over
    keep = [0, 1, 3]
    assert after[keep].tobytes() == before[keep].tobytes()


def test_refusals():
    L = wf.lib()
    with wf.SpectrumBatch(wf.Config.defaults(waveform=1, stereo=1, width=640, meter_ms=100), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_SONO) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.sono()
        assert e.value.code == ERR_INVALID and "waveform batch" in str(e.value) and "sonogram" in str(e.value), str(e.value)
        out = np.empty(2, binding.SONO_DTYPE)
        assert L.wf_hip_read(b.h, binding.OUT_SONO, 0, 2, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID
        assert b"sonogram" in L.wf_hip_last_error(b.h)
    with wf.SpectrumBatch(_cfg(128), 2, ring_frames=1024) as b:  # a ring of 1024 frames: T would be 0
        assert b.ring_frames == 1024 and L.wf_hip_output_bytes(b.h, binding.OUT_SONO) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.sono()
        assert e.value.code == ERR_INVALID and "sonogram" in str(e.value) and "2048" in str(e.value), str(e.value)
        assert b.signal().shape == (2,)  # nothing was enqueued that would trouble the next call
    with wf.SpectrumBatch(_cfg(1024), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_SONO) == ENTRY  # before the first read
        check_abi_refusals(b, binding.OUT_SONO, binding.SONO_DTYPE, 2, _fresh(2, 4096, 1024))


def test_nothing_else_moves(monkeypatch):
    """rows, bars and the other measurement outputs read before and after a sono() are identical; guard bytes behind every block
    intact (wf_hip_sync checks them)"""
    monkeypatch.setenv("WF_HIP_CANARY", "1")
    streams, hop = 3, 800
    with wf.SpectrumBatch(_cfg(4096), streams) as b:
        for t in range(12):
            b.push_audio(synth.block(synth.DEFAULT_SEED, 0, streams, 2, t * hop, hop))
            b.tick()
        names = ("decibels", "bars", "signal", "pitch", "bands", "peaks", "stereo", "cq", "scope", "gonio")
        before = {n: np.asarray(getattr(b, n)()).tobytes() for n in names}
        got = b.sono()
        b.sync()
        for n in names:
            assert np.asarray(getattr(b, n)()).tobytes() == before[n], n
        assert b.sono().tobytes() == got.tobytes()
        b.sync()
    hist = _hist(4096, *[synth.block(synth.DEFAULT_SEED, 0, streams, 2, t * hop, hop) for t in range(12)])
    _check(got, hist, 48000, 8192, "between the other readers", noise=())


def test_three_shards_match_one_handle():
    cfg = _cfg(2048)
    streams = 7
    kinds = ("noise", "chirp", "burst", "noise", "chirp", "burst", "noise")
    with wf.SpectrumBatch(cfg, streams) as one, wf.MultiBatch(cfg, streams, [0, 0, 0]) as m:
        for t in range(6):
            rng = np.random.default_rng(100 + t)
            x = np.stack([ref.signal(k, rng, 801) for k in kinds])
            one.push_audio(x)
            m.push_audio(x)
            one.tick()
            m.tick()
        m.sync()
        want = check_shards_match(one, m, "sono", (2, 4))
        assert np.all(want["columns"] == 12) and np.all(np.isfinite(want["db"][0, :, :12]))


def test_across_the_2_to_the_32_wrap():
    """tests/sono_wrap_child.py: twin handles on the development build, one aged to just below 2^32, walked across the wrap in small
    hops with the cells of sono() equal at every hop.  One child process (the release library has no test aids)"""
    run_wrap_child("sono_wrap_child.py", 120)
