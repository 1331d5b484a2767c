"""Onset detector on the device (WF_HIP_OUT_ONSET) against the float64 restatement (tests/onset_ref.py) of the frames pushed: rings of
8192 to 65536 frames (27, 59, 123 and 128 columns; at 128 the last round of the kernel has one wave with a column), one and two
captured channels, a meter batch, 44100 Hz, three streams each -- noise, a burst and tones behind silence, a fast chirp -- in
packets of unequal odd sizes; columns and decided flags that stand still between reads; bit identity across push paths, repeated
reads and slices; fresh, reset, hidden and paused streams; refusals; nothing else moving; a three-shard group; the 2^32 wrap of the
write positions.

The bound (onset_ref.mismatches; include/wf_hip.h, "onsets"): header words, zeros and the ages >= T exactly; every strength within
one float32 ulp of the restatement's, or 1e-9 -- a float64 transform of 1024 points and log1p leave about 1e-12 per band and 1e-10
per sum, so two correctly rounded float32 values can differ by one step and no more --; flags, onsets and last_* bit for bit
pick() of the device's own strengths, and equal to the restatement's, which test_onset_cpu.py makes legitimate: on these cases no
decision of the restatement lies within four ulps of flipping."""
import ctypes as C

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import onset_ref as ref
from pcm_convert import captured
from tools import synth
from measure_common import Hip, check_abi_refusals, check_shards_match, check_slices_and_repeats, run_wrap_child

pytestmark = pytest.mark.gpu
ERR_INVALID = -1
P, H = ref.P, ref.H
ENTRY = 2240


def _cfg(fft=4096, sr=48000, channels=2, **kw):
    return wf.Config.defaults(**{**dict(fft_size=fft, sample_rate=sr, capture_channels=channels, stereo=1 if channels == 2 else 0, slope=1.0,
                                        bars=1, floor_db=-70), **kw})


def _hist(wpos0, *pushed):
    """the frames behind a fresh handle's counter: wpos0 zeros of create, then what was pushed"""
    first = pushed[0]
    return np.concatenate([np.zeros(first.shape[:2] + (wpos0,), np.float32), *pushed], axis=2)


def _check(got, hist, sr, ring_cap, what=""):
    """against the restatement of `hist` (its end is the counter)"""
    assert got.dtype == binding.ONSET_DTYPE and got.shape == (hist.shape[0],)
    bad, worst = ref.mismatches(got, hist, hist.shape[-1], sr, ring_cap)
    print(f"{what}: T {got['columns'].tolist()}, newest {got['newest'].tolist()}, onsets {got['onsets'].tolist()}, last_age {got['last_age'].tolist()}, "
          f"largest strength {got['strength'].max(axis=1).tolist()}, largest difference {worst} ulps")
    assert not bad, bad[:8]


def _fresh(streams, ring_cap, wpos):
    return ref.onset(np.zeros((streams, 1, 1), np.float32), wpos, 48000, ring_cap)


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=ref.case_id)
def test_onset_equals_the_restatement_of_the_frames(case, monkeypatch):
    fft, sr, ch, kw, ring_frames, ring_cap, t = case
    if ring_cap == 16384:  # guard bytes behind every block, checked by wf_hip_sync
        monkeypatch.setenv("WF_HIP_CANARY", "1")
    x = ref.case_audio(case)
    wpos0 = ref.case_wpos0(case)
    with wf.SpectrumBatch(_cfg(fft, sr, ch, **kw), x.shape[0], ring_frames=ring_frames) as b:
        assert b.ring_frames == ring_cap and b.capture_channels == ch and ref.columns(ring_cap) == t
        assert wf.lib().wf_hip_output_bytes(b.h, binding.OUT_ONSET) == ENTRY  # before the first read
        assert b.onset().tobytes() == _fresh(3, ring_cap, wpos0).tobytes()  # freshly created: zeros
        for lo, hi in ref.packets(np.random.default_rng(ring_cap), x.shape[-1]):
            b.push_audio(np.ascontiguousarray(x[:, :, lo:hi]))
        got = b.onset()
        b.sync()
        again = b.onset()
        b.sync()
    assert got.tobytes() == again.tobytes()
    hist = _hist(wpos0, x)
    assert hist.shape[-1] % H != 0 and np.all(got["columns"] == t) and np.all(got["newest"] == hist.shape[-1] // H)
    assert not np.any(got["strength"][:, t:]) and not np.any(got["group"][:, :, t:]) and not np.any(got["flags"][:, t:])
    assert np.all(got["flags"][:, 3:t - 16] & 0x80) and not np.any(got["flags"][:, :3] & 0x80) and not np.any(got["flags"][:, t - 16:] & 0x80)
    assert got["onsets"][0] == 0 and got["onsets"][1] >= 1 and np.any(got["flags"][2] & 0x0F)
    _check(got, hist, sr, ring_cap, ref.case_id(case))


def test_columns_and_decided_flags_stand_still():
    """read, push 300 frames, read again: newest advances by the hops completed, every column in both reads is the same bytes at
    its new age, and so are the flags of every column decided in both"""
    case = ref.GPU_CASES[3]
    fft, sr, ch, kw, ring_frames, ring_cap, t = case
    x = ref.case_audio(case)
    more = ref.signal("noise", np.random.default_rng(5), 300)[None].repeat(3, axis=0)
    with wf.SpectrumBatch(_cfg(fft, sr, ch), 3, ring_frames=ring_frames) as b:
        b.push_audio(x)
        one = b.onset()
        b.push_audio(more)
        two = b.onset()
    wpos = fft + x.shape[-1]
    d = (wpos + 300) // H - wpos // H
    assert d in (1, 2) and np.all(two["newest"] - one["newest"] == d) and np.all(one["newest"] == wpos // H)
    assert two["strength"][:, d:t].tobytes() == one["strength"][:, :t - d].tobytes()
    assert two["group"][:, :, d:t].tobytes() == one["group"][:, :, :t - d].tobytes()
    both = np.arange(3, t - 16 - d)
    assert np.array_equal(two["flags"][:, both + d], one["flags"][:, both]) and np.any(one["flags"][:, both] & 0x0F)
    assert not np.array_equal(two["strength"][:, 0], one["strength"][:, 0])
    # (the appended noise is no committed case: its strengths are held, its flags to pick() of the device's own strengths)
    own = ref.entries(ref.device_strengths(two), wpos + 300)
    assert two["flags"].tobytes() == own["flags"].tobytes() and np.array_equal(two["onsets"], own["onsets"])
    want = ref.strengths(_hist(fft, x, more), wpos + 300, sr, ring_cap)
    err = np.abs(ref.device_strengths(two).astype(np.float64) - want.astype(np.float64))
    assert np.all((err <= np.spacing(np.abs(want)).astype(np.float64)) | (err <= ref.ABS_TOL))


def _strengths_hold(got, hist, sr, ring_cap, what):
    """audio that is no committed case: the header exactly, the strengths within the bound, the flags and the summary bit for bit
    pick() of the device's own strengths"""
    wpos = hist.shape[-1]
    t = ref.columns(ring_cap)
    own = ref.entries(ref.device_strengths(got), wpos)
    for name in ref.FIELDS[2:]:
        assert got[name].tobytes() == own[name].tobytes(), (what, name)
    want = ref.strengths(hist, wpos, sr, ring_cap)
    dev = ref.device_strengths(got)
    err = np.abs(dev.astype(np.float64) - want.astype(np.float64))
    assert np.all((err <= np.spacing(np.abs(want)).astype(np.float64)) | (err <= ref.ABS_TOL)), (what, float(err.max()))
    assert not np.any(got["strength"][:, t:]) and not np.any(got["group"][:, :, t:])


def test_every_push_path_counts():
    """the same frames through push_audio, the pinned asynchronous push, two ragged pushes per packet, wf_hip_push_pcm (s16
    interleaved: every value exact in float32) and push_audio_device read bit-identically; push_synth and muted packets advance
    the counter and read as the restatement of what they leave in the rings"""
    streams, fft, frames, ring_cap = 3, 1024, 801, 8192
    n_pkts = 11  # 8811 frames: the ring is written once over
    rng = np.random.default_rng(2)
    wave = (8000.0 * np.sin(2.0 * np.pi * np.arange(n_pkts * frames) / 57.3))[None, :, None]
    pkts = [(wave[:, i * frames:(i + 1) * frames] + rng.integers(-5000, 5000, (streams, frames, 2))).astype(np.int16) for i in range(n_pkts)]
    convs = [np.ascontiguousarray(captured(pkt, True, 0, 2)) for pkt in pkts]  # [streams, 2, frames] float32
    split = np.array([0, int(0.4 * frames), frames], np.uint32)  # a packet in two ragged pushes: the streams differ in how it is cut
    hip = Hip()
    reads = {}
    for path in ("float", "pinned", "ragged", "pcm", "device", "synth", "muted"):
        with wf.SpectrumBatch(_cfg(fft), streams, ring_frames=ring_cap) as b:
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
            reads[path] = b.onset()
    for path in ("pinned", "ragged", "pcm", "device"):
        assert reads[path].tobytes() == reads["float"].tobytes(), path
    for path in reads:
        assert np.all(reads[path]["newest"] == (fft + n_pkts * frames) // H), path  # every path counts
    _strengths_hold(reads["float"], _hist(fft, *convs), 48000, ring_cap, "s16 packets")
    _strengths_hold(reads["synth"], _hist(fft, synth.block(synth.DEFAULT_SEED, 0, streams, 2, 0, n_pkts * frames)), 48000, ring_cap, "push_synth")
    muted = [c if i % 2 == 0 else np.zeros_like(c) for i, c in enumerate(convs)]
    _strengths_hold(reads["muted"], _hist(fft, *muted), 48000, ring_cap, "every other packet muted")
    assert reads["muted"].tobytes() != reads["float"].tobytes()
    assert np.any(reads["muted"]["flags"] & 0x0F)  # a packet behind a muted one is an event


def test_repeated_reads_and_slices():
    """a slice as a handle's first read equals the entry of the full read; reads with nothing in between, and a read after a
    tick, are bit-identical"""
    streams, fft, ring_cap = 5, 2048, 8192
    rng = np.random.default_rng(11)
    x = np.stack([ref.signal(k, rng, 9001) for k in ("noise", "chirp", "burst", "noise", "chirp")])
    with wf.SpectrumBatch(_cfg(fft), streams, ring_frames=ring_cap) as b:
        assert b.ring_frames == ring_cap
        b.push_audio(np.ascontiguousarray(x[..., :4000]))
        b.push_audio(np.ascontiguousarray(x[..., 4000:]))
        full = check_slices_and_repeats(b, "onset")
    _strengths_hold(full, _hist(fft, x), 48000, ring_cap, "five streams")


def test_fresh_reset_hidden_and_paused_streams():
    fft, streams, ring_cap = 1024, 4, 8192
    with wf.SpectrumBatch(_cfg(fft, stereo=0), streams, ring_frames=ring_cap) as b:  # (a mono mixdown still captures two channels)
        assert b.capture_channels == 2 and b.ring_frames == ring_cap
        rng = np.random.default_rng(13)
        x = np.stack([ref.signal(k, rng, ring_cap + 801) for k in ("noise", "chirp", "noise", "chirp")])
        assert b.onset().tobytes() == _fresh(streams, ring_cap, fft).tobytes()
        b.set_hidden(np.array([0, 1, 0, 3], np.uint8))  # hidden, paused
        b.push_audio(x)
        b.tick()
        before = b.onset()
        _strengths_hold(before, _hist(fft, x), 48000, ring_cap, "one stream hidden, one paused")
        assert np.all(before["strength"][:, :27].max(axis=1) > 1.0)  # the hidden and the paused stream are read like any other
        b.reset(2, 1)
        after = b.onset()
    assert after[2:3].tobytes() == _fresh(1, ring_cap, fft).tobytes()  # as a fresh one: the counter starts over
    keep = [0, 1, 3]
    assert after[keep].tobytes() == before[keep].tobytes()


def test_refusals():
    L = wf.lib()
    with wf.SpectrumBatch(wf.Config.defaults(waveform=1, stereo=1, width=640, meter_ms=100), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_ONSET) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.onset()
        assert e.value.code == ERR_INVALID and "waveform batch" in str(e.value) and "onset" in str(e.value), str(e.value)
        out = np.empty(2, binding.ONSET_DTYPE)
        assert L.wf_hip_read(b.h, binding.OUT_ONSET, 0, 2, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID
        assert b"onset" in L.wf_hip_last_error(b.h)
    with wf.SpectrumBatch(_cfg(1024), 2, ring_frames=4096) as b:  # a ring of 4096 frames: no column would be decided
        assert b.ring_frames == 4096 and L.wf_hip_output_bytes(b.h, binding.OUT_ONSET) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.onset()
        assert e.value.code == ERR_INVALID and "onset" in str(e.value) and "8192" in str(e.value) and "ring_frames" in str(e.value), str(e.value)
        assert b.signal().shape == (2,)  # nothing was enqueued that would trouble the next call
    with wf.SpectrumBatch(_cfg(4096), 2) as b:
        assert b.ring_frames == 8192 and L.wf_hip_output_bytes(b.h, binding.OUT_ONSET) == ENTRY  # before the first read
        check_abi_refusals(b, binding.OUT_ONSET, binding.ONSET_DTYPE, 2, _fresh(2, 8192, 4096))


def test_nothing_else_moves(monkeypatch):
    """rows, bars and the other measurement outputs read before and after an onset() are identical; guard bytes behind every
    block intact (wf_hip_sync checks them)"""
    monkeypatch.setenv("WF_HIP_CANARY", "1")
    streams, hop = 3, 800
    with wf.SpectrumBatch(_cfg(4096), streams) as b:
        for t in range(12):
            b.push_audio(synth.block(synth.DEFAULT_SEED, 0, streams, 2, t * hop, hop))
            b.tick()
        names = ("decibels", "bars", "signal", "pitch", "bands", "peaks", "stereo", "cq", "scope", "gonio", "sono", "bits", "thd", "delay")
        before = {n: np.asarray(getattr(b, n)()).tobytes() for n in names}
        got = b.onset()
        b.sync()
        for n in names:
            assert np.asarray(getattr(b, n)()).tobytes() == before[n], n
        assert b.onset().tobytes() == got.tobytes()
        b.sync()
    hist = _hist(4096, *[synth.block(synth.DEFAULT_SEED, 0, streams, 2, t * hop, hop) for t in range(12)])
    _strengths_hold(got, hist, 48000, 8192, "between the other readers")


def test_three_shards_match_one_handle():
    cfg = _cfg(4096)
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
        want = check_shards_match(one, m, "onset", (2, 4))
        assert np.all(want["columns"] == 27) and np.all(want["strength"][[0, 1, 3, 4, 6], :18] > 0)


def test_across_the_2_to_the_32_wrap():
    """tests/onset_wrap_child.py: twin handles on the development build, one aged to just below 2^32, walked across the wrap in
    small hops with the strengths and flags of onset() equal at every hop.  One child process (the release library has no test aids)"""
    run_wrap_child("onset_wrap_child.py", 120)
