"""Tempo and beat phase on the device (WF_HIP_OUT_TEMPO) against the float64 restatement (tests/tempo_ref.py) of the frames pushed:
rings of 131072 frames (T = 507: eight chunks of the columns kernel, the last of 59 columns with a last round that is not full),
2^18 (with the guard bytes on) and 2^20 (T capped at 2048: 32 full chunks), one and two captured channels, 44100 and 8000 Hz, a
meter batch; kicks at 120 BPM, bursts at 150 BPM and noise, in packets of unequal odd sizes; the onset detector's strengths bit for
bit; a slice as the first read; streams at different write positions; bit identity across push paths; silence, a reset stream and a
NaN in the ring; refusals; a two-shard group; the 2^32 wrap of the write positions.

The bound (tempo_ref.mismatches; include/wf_hip.h, "tempo"): every strength within one float32 ulp of the restatement's, or 1e-9,
and 0 from age T on; every other float32 field within one float32 rounding (or 1e-9) of the rule in numpy float64 on the device's
own strengths, every integer equal to it; and on the committed cases the integers equal to the restatement's from its own
strengths, which test_tempo_cpu.py makes legitimate: their decisions stand at least four times farther from flipping than a change
of every strength by one ulp can move them."""
import ctypes as C

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import tempo_ref as ref
from pcm_convert import captured
from tools import synth
from measure_common import check_abi_refusals, check_shards_match, run_wrap_child

pytestmark = pytest.mark.gpu
ERR_INVALID = -1
P, H = ref.P, ref.H
ENTRY = 10592
RING = 131072


def _cfg(fft=1024, sr=48000, channels=2, **kw):
    return wf.Config.defaults(**{**dict(fft_size=fft, sample_rate=sr, capture_channels=channels, stereo=1 if channels == 2 else 0, slope=1.0,
                                        bars=1, floor_db=-70), **kw})


def _hist(wpos0, *pushed):
    """the frames behind a fresh handle's counter: wpos0 zeros of create, then what was pushed"""
    first = pushed[0]
    return np.concatenate([np.zeros(first.shape[:2] + (wpos0,), np.float32), *pushed], axis=2)


def _packets(rng, total):
    """(lo, hi) of packets of unequal odd lengths of 1 .. 16001 frames that add up to `total`"""
    cuts, at = [], 0
    while at < total:
        n = min(2 * int(rng.integers(0, 8001)) + 1, total - at)
        cuts.append((at, at + n))
        at += n
    return cuts


def _check(got, hist, wpos, sr, ring, what="", integers=True):
    assert got.dtype == binding.TEMPO_DTYPE and got.shape == (hist.shape[0],)
    bad, worst = ref.mismatches(got, hist, wpos, sr, ring, integers)
    print(f"{what}: T {got['columns'].tolist()}, valid {got['valid'].tolist()}, bpm {got['bpm'].tolist()}, lag {got['lag'].tolist()}, second "
          f"{got['lag2'].tolist()}, beat_age {got['beat_age'].tolist()}, confidence {got['confidence'].tolist()}, largest difference of a "
          f"strength {worst} ulps")
    assert not bad, bad[:8]


def _fresh(streams, sr, ring, wpos):
    return ref.tempo(np.zeros((streams, 1, 1), np.float32), wpos, sr, ring)


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=ref.case_id)
def test_tempo_equals_the_restatement_of_the_frames(case, monkeypatch):
    fft, sr, ch, kw, ring, t, kinds = case
    if ring == 1 << 18:  # guard bytes behind every block, checked by wf_hip_sync
        monkeypatch.setenv("WF_HIP_CANARY", "1")
    x = ref.case_audio(case)
    wpos0 = ref.case_wpos0(case)
    with wf.SpectrumBatch(_cfg(fft, sr, ch, **kw), x.shape[0], ring_frames=ring) as b:
        assert b.ring_frames == ring and b.capture_channels == ch and ref.columns(ring) == t
        assert wf.lib().wf_hip_output_bytes(b.h, binding.OUT_TEMPO) == ENTRY  # before the first read
        fresh = b.tempo()
        assert fresh.tobytes() == _fresh(len(kinds), sr, ring, wpos0).tobytes() and not fresh["valid"].any()  # freshly created: zeros
        for lo, hi in _packets(np.random.default_rng(ring), x.shape[-1]):
            b.push_audio(np.ascontiguousarray(x[:, :, lo:hi]))
        got = b.tempo()
        onset = b.onset()
        b.sync()
        again = b.tempo()
        b.sync()
    assert got.tobytes() == again.tobytes()
    wpos = wpos0 + x.shape[-1]
    assert wpos % H != 0 and np.all(got["columns"] == t) and np.all(got["newest"] == wpos // H)
    assert not np.any(got["strength"][:, t:]) and np.all(got["strength"][:, :t] >= 0)
    assert got["strength"][:, :128].tobytes() == onset["strength"].tobytes()  # the same code on the same columns
    assert got["valid"].tolist() == [0 if (k == "noise" and sr == 8000) else 1 for k in kinds]
    _check(got, _hist(wpos0, x), wpos, sr, ring, ref.case_id(case))


def test_a_slice_first_and_streams_at_different_positions():
    """the first read of a handle is a slice (first = 1, count = 1): the blocks are allocated whole; then 200 frames more for every
    stream and 131 on top for one, so that its counter stands a hop further and elsewhere in the hop than the others'"""
    case = ref.GPU_CASES[0]
    fft, sr, ch, kw, ring, t, kinds = case
    x = ref.case_audio(case)
    rng = np.random.default_rng(3)
    extra = np.stack([ref.noise(rng, -20.0, 200)[None].repeat(ch, axis=0) for _ in range(3)])
    more = ref.noise(rng, -20.0, 131)[None, None].repeat(ch, axis=1)
    with wf.SpectrumBatch(_cfg(fft, sr, ch), 3, ring_frames=ring) as b:
        b.push_audio(x)
        part = b.tempo(1, 1)
        full = b.tempo()
        assert part.shape == (1,) and part.tobytes() == full[1:2].tobytes()
        assert b.tempo(2, 1).tobytes() == full[2:].tobytes()
        b.push_audio(extra)
        b.push_audio(more, first=1)
        moved = b.tempo()
        b.tick()
        assert b.tempo().tobytes() == moved.tobytes()  # a tick does not move the rings
    wpos = fft + x.shape[-1]
    _check(full, _hist(fft, x), wpos, sr, ring, "the whole batch behind a slice")
    assert (wpos + 200) // H == wpos // H and (wpos + 331) // H == wpos // H + 1
    assert moved["newest"].tolist() == [wpos // H, wpos // H + 1, wpos // H]
    assert moved["strength"][[0, 2], :t].tobytes() == full["strength"][[0, 2], :t].tobytes()  # no hop completed: the same columns
    assert moved["strength"][1, 1:t].tobytes() == full["strength"][1, :t - 1].tobytes()  # one completed: the others a column older
    # (the appended noise is no committed case: its integers are held to the rule on the device's own strengths)
    _check(moved[[0, 2]], _hist(fft, x[[0, 2]], extra[[0, 2]]), wpos + 200, sr, ring, "200 frames more", integers=False)
    _check(moved[1:2], _hist(fft, x[1:2], extra[1:2], more), wpos + 331, sr, ring, "331 frames more", integers=False)


def test_every_push_path_leaves_the_same_bits():
    """the same frames through push_audio, the pinned asynchronous push and wf_hip_push_pcm (s16 interleaved: every value exact in
    float32) read bit-identically; push_synth reads as the restatement of what it leaves in the rings"""
    streams, fft, ring, sr = 2, 1024, RING, 48000
    rng = np.random.default_rng(2)
    frames = ring + 515
    x = np.stack([ref.kicks(rng, 120.0, frames)[0], ref.bursts(rng, 150.0, frames)[0]])
    pcm = np.round(np.stack([x, 0.5 * x], axis=2) * 32767.0).astype(np.int16)  # [streams, frames, 2]
    conv = np.ascontiguousarray(captured(pcm, True, 0, 2))  # [streams, 2, frames] float32
    cuts = _packets(np.random.default_rng(7), frames)
    reads = {}
    for path in ("float", "pinned", "pcm", "synth"):
        with wf.SpectrumBatch(_cfg(fft), streams, ring_frames=ring) as b:
            if path == "synth":
                b.push_synth(synth.DEFAULT_SEED, 0, frames)
            for i, (lo, hi) in enumerate(cuts if path != "synth" else ()):
                if path == "float":
                    b.push_audio(np.ascontiguousarray(conv[:, :, lo:hi]))
                elif path == "pinned":
                    pin = wf.PinnedBuffer((streams, 2, hi - lo))
                    pin.array[...] = conv[:, :, lo:hi]
                    b.push_audio_async(pin, streams, hi - lo, i & 1)
                    b.sync()
                    pin.close()
                else:
                    b.push_pcm(np.ascontiguousarray(pcm[:, lo:hi]), interleaved=True)
            reads[path] = b.tempo()
    for path in ("pinned", "pcm"):
        assert reads[path].tobytes() == reads["float"].tobytes(), path
    assert np.all(reads["float"]["valid"] == 1) and reads["float"]["lag"].tolist() == [94, 75]
    _check(reads["float"], _hist(fft, conv), fft + frames, sr, ring, "s16 packets", integers=False)
    _check(reads["synth"], _hist(fft, synth.block(synth.DEFAULT_SEED, 0, streams, 2, 0, frames)), fft + frames, sr, ring, "push_synth",
           integers=False)
    assert np.all(reads["synth"]["newest"] == (fft + frames) // H)


def test_silence_a_reset_stream_and_a_nan_in_the_ring():
    fft, sr, ring = 1024, 48000, RING
    rng = np.random.default_rng(4)
    frames = ring + 515
    k = ref.kicks(rng, 120.0, frames)[0]
    x = np.stack([np.stack([k, k]), np.zeros((2, frames), np.float32), np.stack([k, k]), np.stack([k, k])])
    x[3, 1, frames - 40000] = np.nan
    with wf.SpectrumBatch(_cfg(fft), 4, ring_frames=ring) as b:
        b.push_audio(x)
        before = b.tempo()
        b.reset(2, 1)
        after = b.tempo()
    zero = _fresh(1, sr, ring, fft + frames)
    assert before[1:2].tobytes() == zero.tobytes() and not before["valid"][1]  # silence: r[0] = 0
    assert before["valid"].tolist() == [1, 0, 1, 1] and before[2:3].tobytes() == before[0:1].tobytes()
    assert after[2:3].tobytes() == _fresh(1, sr, ring, fft).tobytes()  # as a fresh one: the counter starts over
    assert after[[0, 1, 3]].tobytes() == before[[0, 1, 3]].tobytes()
    # the NaN: the four columns that hold it have no level, their strengths and their successors' read 0 (max(NaN, 0) on the
    # device), and the entry is the rule on those finite strengths
    nan = before[3]
    for f in ref.FIELDS:
        assert np.all(np.isfinite(nan[f])), f
    assert nan["valid"] == 1 and abs(nan["bpm"] - 120.0) < 0.6
    own = ref.entries(before["strength"][3:4, :507], fft + frames, sr)
    for f in ref.UINT_FIELDS + ("reserved",):
        assert nan[f].tobytes() == own[0][f].tobytes(), f
    for f in ("acf",) + ref.FLOAT_FIELDS:
        d = np.abs(nan[f].astype(np.float64) - own[0][f].astype(np.float64))
        assert np.all((d <= np.spacing(np.abs(own[0][f])).astype(np.float64)) | (d <= ref.ABS_TOL)), f
    differ = np.flatnonzero(before["strength"][3] != before["strength"][0])
    assert 1 <= len(differ) <= 6 and np.all(before["strength"][3][differ[:-1]] == 0)
    _check(before[:1], _hist(fft, x[:1]), fft + frames, sr, ring, "kicks beside silence", integers=False)


def test_refusals():
    L = wf.lib()
    with wf.SpectrumBatch(wf.Config.defaults(waveform=1, stereo=1, width=640, meter_ms=100), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_TEMPO) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.tempo()
        assert e.value.code == ERR_INVALID and "waveform batch" in str(e.value) and "tempo" in str(e.value), str(e.value)
    with wf.SpectrumBatch(_cfg(1024), 2, ring_frames=65536) as b:
        assert b.ring_frames == 65536 and L.wf_hip_output_bytes(b.h, binding.OUT_TEMPO) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.tempo()
        assert e.value.code == ERR_INVALID and "tempo" in str(e.value) and "131072" in str(e.value) and "ring_frames" in str(e.value), str(e.value)
        out = np.empty(2, binding.TEMPO_DTYPE)
        assert L.wf_hip_read(b.h, binding.OUT_TEMPO, 0, 2, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID
        assert b"tempo" in L.wf_hip_last_error(b.h)
        assert b.onset().shape == (2,)  # nothing was enqueued that would trouble the next call
    with wf.SpectrumBatch(_cfg(1024, sr=384000), 1, ring_frames=RING) as b:  # 240 BPM is a lag of 375 columns, beyond the 287 there are
        assert b.ring_frames == RING and L.wf_hip_output_bytes(b.h, binding.OUT_TEMPO) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.tempo()
        assert e.value.code == ERR_INVALID and "tempo" in str(e.value) and "sample rate" in str(e.value), str(e.value)
    with wf.SpectrumBatch(_cfg(1024), 2, ring_frames=RING) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_TEMPO) == ENTRY
        check_abi_refusals(b, binding.OUT_TEMPO, binding.TEMPO_DTYPE, 2, _fresh(2, 48000, RING, 1024))


def test_two_shards_match_one_handle():
    cfg = _cfg(1024)
    rng = np.random.default_rng(9)
    frames = RING + 515
    x = np.stack([np.stack([k, k]) for k in (ref.kicks(rng, 120.0, frames)[0], ref.bursts(rng, 150.0, frames)[0], ref.noise(rng, -20.0, frames))])
    with wf.SpectrumBatch(cfg, 3, ring_frames=RING) as one, wf.MultiBatch(cfg, 3, [0, 0], ring_frames=RING) as m:
        one.push_audio(x)
        m.push_audio(x)
        m.sync()
        want = check_shards_match(one, m, "tempo", (1, 2))
    assert want["valid"].tolist() == [1, 1, 1] and want["lag"][:2].tolist() == [94, 75]


def test_across_the_2_to_the_32_wrap():
    """tests/tempo_wrap_child.py: twin handles on the development build, one aged to just below 2^32, read before the wrap, with the
    span read across it and behind it.  One child process (the release library has no test aids)"""
    run_wrap_child("tempo_wrap_child.py", 120)
