"""Impulse response on the device (WF_HIP_OUT_IMPULSE) against the float64 restatement (tests/impulse_ref.py) of the frames pushed,
on the shapes of tests/xfer_ref.py's GPU_CASES -- segments of 256 (the fewest bins per thread, and the most indices from P up), 512
(under an FFT that is no power of two), 1024 (the default ring of the headline shape), 2048 with 13 and with 32 segments, a meter
batch and a mono mixdown display -- nine streams each: three taps (+1 at 37 frames, -0.5 and +0.25 behind it), a negative lag at the
end of the range with one echo, an inverted copy at -6 dB, the three taps under noise of equal power, independent noise, dual mono,
two echoes 20 frames apart with a third inside the guard of the first, a measured channel that is +0.0 under every segment (the
no-response record), and a silent reference or a NaN by turns (the zero record) -- in uneven packets, one ring and H + 3 frames long,
so that the span wraps the ring and the counter ends off the anchor.  Then bit identity across push paths, repeated reads, slices
and pushes within a hop; reset and hidden streams; refusals; nothing else moving on a twin; a three-shard group; seven streams at
staggered write positions; the 2^32 wrap of the counters.

The bound is impulse_ref's, derived and not measured; tests/test_impulse_cpu.py shows on these very seeds and shapes that four
orderings agree within 1e-13 of the peak and that no decision is near a tie, and every comparison here asserts the margins first.
Independent noise has no lag to find: the restatement takes the device's for that stream.  The fields the record shares with
wf_hip_xfer are compared bit for bit with an xfer() read at the same moment.  (On an MI355X every float32 field came out equal to
the restatement's on every case here, the staggered batch and the 2^32 wrap included; the float64 values behind `frames` and
delay_ms at lag 0 differed by 6e-16 frames at the most, which the bound's FRAC_FLOOR is for.)

The margins asked are impulse_ref.margins_hold's: 1e-3 in every figure, but 1e-5 in the prominence of a stream that lists maxima
of its noise floor -- the stream under equal noise, and in the staggered batch a stream whose ring the audio has not filled yet."""
import ctypes as C

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import measure_stagger as ms
import impulse_ref as ref
import xfer_ref
from pcm_convert import captured
from tools import synth
from measure_common import Hip, check_abi_refusals, check_shards_match, packets, run_wrap_child

pytestmark = pytest.mark.gpu
OUT_IMPULSE = binding.OUT_IMPULSE  # (the output these tests are about: a library without it fails every one of them)
ERR_INVALID = -1
ENTRY = 16576
INDEPENDENT = ref.KINDS.index("independent")
NOISY = ref.KINDS.index("three taps, noise")


def _cfg(fft=4096, sr=48000, **kw):
    return wf.Config.defaults(**{**dict(fft_size=fft, sample_rate=sr, capture_channels=2, stereo=1, slope=1.0, bars=1, floor_db=-70), **kw})


def _padding_is_zero(got):
    """reserved words, the arrival slots not used and the indices from P up"""
    assert not got["reserved"].any() and not got["arrivals"]["reserved"].any()
    for s in range(len(got)):
        p, n = int(got["window"][s]), int(got["count"][s])
        assert not got["ir"][s, p:].any() and not got["etc_db"][s, p:].any(), s
        assert n <= ref.ARRIVALS and not np.frombuffer(got["arrivals"][s, n:].tobytes(), np.uint8).any(), s


def _check(got, xf, frames, w, ring, sr, wpos, what="", free=(), noisy=(), kinds=None):
    """every entry of `got` within the bound of the restatement of `frames`, each figure printed first, and its shared fields the
    bits of `xf`, an xfer() read at the same moment.  free: the streams whose lag is noise -- the restatement takes the device's
    there; everywhere else its own search must agree.  noisy: the streams that list maxima of their noise floor (ref.margins_hold); where `kinds` are given,
    those that list more arrivals than their kind has taps -- a ring that the audio has not filled yet"""
    lags = [int(got["lag"][s]) if s in free else None for s in range(len(frames))]
    want = ref.impulse(frames, w, ring, sr, lag=lags, wpos=wpos)
    assert got.dtype == binding.IMPULSE_DTYPE == ref.IMPULSE_DTYPE and got.shape == want.shape
    margin = ref.margins(frames, w, ring, sr, lag=lags, wpos=wpos)
    if kinds is not None:
        noisy = [s for s, name in enumerate(kinds) if want["count"][s] > ref.TAPS_OF[name]]
    print(f"{what}: P {got['window'].tolist()}, K {got['segments'].tolist()}, valid {got['valid'].tolist()}, lag {got['lag'].tolist()}, "
          f"count {got['count'].tolist()}, peak_index {got['peak_index'].tolist()}, peak_db {got['peak_db'].tolist()}, "
          f"least margins {np.nanmin(margin, axis=0).tolist()}, worst |got - want| {ref.worst(got, want)}")
    for s in range(len(frames)):  # the condition the bound rests on (test_impulse_cpu.py), for whatever is compared here
        if want["valid"][s] and s not in free:
            assert ref.margins_hold(margin[s], s in noisy), (s, margin[s])
    bad = ref.mismatches(got, want)
    assert not bad, bad[:8]
    _padding_is_zero(got)
    for name in ref.SHARED_FIELDS:
        assert got[name].tobytes() == xf[name].tobytes(), name
    return want


@pytest.mark.parametrize("index", range(len(xfer_ref.GPU_CASES)), ids=[xfer_ref.case_id(c) for c in xfer_ref.GPU_CASES])
def test_impulse_equals_the_restatement_of_the_frames(index):
    case = xfer_ref.GPU_CASES[index]
    fft, sr, kw, w, ring = case
    kinds = ref.case_kinds(index)
    x = ref.case_audio(case, index)
    cap = xfer_ref.ring_frames(w, ring)
    p, k = xfer_ref.geometry(w, cap)
    l = p // 4
    with wf.SpectrumBatch(_cfg(fft, sr, **kw), x.shape[0], ring_frames=ring or 0) as b:
        assert b.fft_size == w and b.ring_frames == cap and b.capture_channels == 2
        assert wf.lib().wf_hip_output_bytes(b.h, OUT_IMPULSE) == ENTRY  # before the first read
        for lo, hi in packets(np.random.default_rng(w), x.shape[-1], 700):
            b.push_audio(np.ascontiguousarray(x[:, :, lo:hi]))
        got = b.impulse()
        xf = b.xfer()
    wpos = xfer_ref.case_wpos0(case) + x.shape[-1]
    assert wpos % (p // 2) != 0 and x.shape[-1] > cap  # off the anchor, and the span wraps the ring
    assert np.all(got["window"] == p) and np.all(got["hop"] == p // 2) and np.all(got["segments"] == k)
    _check(got, xf, x, w, cap, sr, wpos, xfer_ref.case_id(case), free=(INDEPENDENT,), noisy=(NOISY,))
    assert got["valid"].tolist() == [int(name not in ref.INVALID) for name in kinds]
    assert got[8:].tobytes() == ref.zero_record(w, cap, 1).tobytes()  # a silent reference or a NaN: the zero record
    assert [int(got["lag"][s]) for s in range(8) if s != INDEPENDENT] == [ref.true_lag(name, p) for name in kinds[:8] if name != "independent"]
    assert np.all(got["newest"][:8] == wpos // (p // 2))
    taps = got[kinds.index("three taps")]
    assert taps["count"] == 3 and taps["peak_index"] == l and taps["arrivals"]["polarity"][:3].tolist() == [1, -1, 1]
    assert np.all(np.abs(taps["arrivals"]["frames"][:3] - (ref.TAP_DELAY + np.array(ref.tap_offsets(p)))) < 0.05)
    echo = got[kinds.index("delay -(L-1), echo")]
    assert echo["count"] == 2 and abs(echo["arrivals"]["frames"][1] - (ref.ECHO_OFFSET - (l - 1))) < 0.05
    inv = got[kinds.index("inverted -6 dB")]
    assert inv["count"] == 1 and inv["arrivals"]["polarity"][0] == -1 and abs(inv["peak_db"] + 6.02) < 0.01 and inv["peak_index"] == l
    dual = got[kinds.index("dual mono")]
    assert dual["count"] == 1 and dual["arrivals"]["polarity"][0] == 1 and dual["lag_peak"] == 1.0 and abs(dual["peak_db"]) < 1e-3
    guard = got[kinds.index("guarded echoes")]  # the tap 6 frames behind the first is inside its guard: not listed
    assert guard["count"] == 2 and np.all(np.abs(guard["arrivals"]["frames"][:2] - (ref.GUARD_DELAY + np.array([0, 20]))) < 0.05)
    none = got[kinds.index("tone, measured zero")]  # the no-response record
    assert none["valid"] == 1 and none["count"] == 0 and not none["ir"].any() and not np.signbit(none["ir"]).any()
    assert np.all(np.isneginf(none["etc_db"][:p])) and not none["arrivals"].tobytes().strip(b"\0")
    assert none["peak_index"] == 0 and not any(none[n] for n in ("peak_db", "delay_ms", "energy_db", "direct_db", "lag", "lag_peak"))


def test_every_push_path_counts():
    """the same s16 frames through push_audio, wf_hip_push_pcm (s16 interleaved: every value exact in float32) and
    push_audio_device read bit-identically"""
    streams, fft, frames, sr = 3, 1024, 801, 48000
    rng = np.random.default_rng(2)
    packets = 12  # 9612 frames: more than the ring of 4096
    base = np.stack([ref.stream(k, rng, packets * frames, 512) for k in ("three taps", "delay -(L-1), echo", "guarded echoes")])
    wave = np.round(32768.0 * 0.5 * np.clip(base, -2.0, 2.0)).astype(np.int16).transpose(0, 2, 1)  # [streams, n, 2]
    pkts = [np.ascontiguousarray(wave[:, i * frames:(i + 1) * frames]) for i in range(packets)]
    hip = Hip()
    reads = {}
    for path in ("float", "pcm", "device"):
        with wf.SpectrumBatch(_cfg(fft, sr), streams) as b:
            assert b.ring_frames == 4096
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
            reads[path] = b.impulse()
            xf = b.xfer()
    for path in ("pcm", "device"):
        assert reads[path].tobytes() == reads["float"].tobytes(), path
    hist = np.concatenate([captured(pkt, True, 0, 2) for pkt in pkts], axis=2)
    want = _check(reads["float"], xf, hist, fft, 4096, sr, fft + packets * frames, "s16 packets")
    assert np.all(want["valid"] == 1) and want["lag"].tolist() == [37, -127, 12] and np.all(want["window"] == 512)


def test_repeated_reads_slices_and_pushes_within_a_hop():
    """a slice as a handle's first read, into a buffer full of ones, equals the entry of the full read, padding included; reads with
    nothing in between, a read after a tick, and a read after a push of fewer frames than are left to the next anchor are
    bit-identical; the push that crosses the anchor moves `newest` by one"""
    fft, sr, ring = 1024, 48000, 8192
    kinds = ("three taps", "guarded echoes", "independent", "silent reference", "delay -(L-1), echo")
    streams = len(kinds)
    p, k = xfer_ref.geometry(fft, ring)
    h = p // 2
    total = ring + h + 3
    rng = np.random.default_rng(11)
    x = np.stack([ref.stream(name, rng, total + h, p) for name in kinds])
    L = wf.lib()
    with wf.SpectrumBatch(_cfg(fft, sr), streams, ring_frames=ring) as b:
        assert b.ring_frames == ring and (fft + total) % h == 3
        b.push_audio(np.ascontiguousarray(x[..., :5000]))
        b.push_audio(np.ascontiguousarray(x[..., 5000:total]))
        part = np.frombuffer(b"\xff" * ENTRY, binding.IMPULSE_DTYPE).copy()  # the first read is a slice: the block is allocated whole
        assert L.wf_hip_read(b.h, OUT_IMPULSE, 1, 1, part.ctypes.data_as(C.c_void_p)) == 0
        _padding_is_zero(part)
        full = b.impulse()
        xf = b.xfer()
        assert part.tobytes() == full[1:2].tobytes()
        assert b.impulse(3, 2).tobytes() == full[3:].tobytes()
        for _ in range(3):
            assert b.impulse().tobytes() == full.tobytes()
        b.tick()
        assert b.impulse().tobytes() == full.tobytes()  # a tick does not move the rings
        b.push_audio(np.ascontiguousarray(x[..., total:total + h - 4]))  # one frame short of the next anchor
        assert b.impulse().tobytes() == full.tobytes()
        b.push_audio(np.ascontiguousarray(x[..., total + h - 4:total + h - 3]))  # the anchor
        moved = b.impulse()
        xf_moved = b.xfer()
    assert np.all(moved["newest"][[0, 1, 2, 4]] == full["newest"][[0, 1, 2, 4]] + 1) and moved.tobytes() != full.tobytes()
    assert full["valid"].tolist() == [1, 1, 1, 0, 1] and full["lag"][[0, 1, 4]].tolist() == [37, 12, -255]
    _check(full, xf, x[..., :total], fft, ring, sr, fft + total, "before the anchor", free=(2,))
    _check(moved, xf_moved, x[..., :total + h - 3], fft, ring, sr, fft + total + h - 3, "behind the anchor", free=(2,))


def test_fresh_reset_and_hidden_streams():
    fft, streams, sr = 1024, 4, 48000
    with wf.SpectrumBatch(_cfg(fft, sr), streams) as b, wf.SpectrumBatch(_cfg(fft, sr), streams) as twin:
        ring = b.ring_frames
        p, k = xfer_ref.geometry(fft, ring)
        rng = np.random.default_rng(13)
        n = ring + 801
        x = np.stack([ref.stream(name, rng, n, p) for name in ("three taps", "delay -(L-1), echo", "dual mono", "inverted -6 dB")])
        zero = ref.zero_record(fft, ring, streams)
        assert ref.mismatches(zero, ref.impulse(np.zeros((streams, 2, fft), np.float32), fft, ring, sr)) == []
        assert b.impulse().tobytes() == zero.tobytes()  # freshly created, both channels silent: valid = 0
        b.set_hidden(np.array([0, 1, 0, 0], np.uint8))
        b.push_audio(x)
        b.tick()
        before = b.impulse()
        _check(before, b.xfer(), x, fft, ring, sr, fft + n, "one stream hidden")  # the hidden stream's ring reads like any other
        assert np.all(before["valid"] == 1) and before["lag"].tolist() == [37, -(p // 4 - 1), 0, 0]
        b.reset(2, 1)
        after = b.impulse()
        # a fresh twin fed what the reset stream has seen since: nothing
        twin.push_audio(x)
        twin.reset(2, 1)
        assert twin.impulse().tobytes() == after.tobytes()
    assert after[2:3].tobytes() == zero[:1].tobytes()
    keep = [0, 1, 3]
    assert after[keep].tobytes() == before[keep].tobytes()


def test_refusals():
    L = wf.lib()
    with wf.SpectrumBatch(wf.Config.defaults(waveform=1, stereo=1, width=640, meter_ms=100), 2) as b:
        assert L.wf_hip_output_bytes(b.h, OUT_IMPULSE) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.impulse()
        assert e.value.code == ERR_INVALID and "waveform batch" in str(e.value) and "impulse response" in str(e.value), str(e.value)
        out = np.empty(2, binding.IMPULSE_DTYPE)
        assert L.wf_hip_read(b.h, OUT_IMPULSE, 0, 2, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID
        assert b"impulse response" in L.wf_hip_last_error(b.h)
    with wf.SpectrumBatch(_cfg(1024, capture_channels=1, stereo=0), 2) as b:  # one captured channel: nothing to compare
        assert b.capture_channels == 1 and L.wf_hip_output_bytes(b.h, OUT_IMPULSE) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.impulse()
        assert e.value.code == ERR_INVALID and "two captured channels" in str(e.value) and "impulse response" in str(e.value), str(e.value)
        assert b.thd().shape == (2,)  # the other readers of such a batch are unharmed
    with wf.SpectrumBatch(_cfg(240), 2) as b:  # W < 256
        assert b.fft_size == 240 and L.wf_hip_output_bytes(b.h, OUT_IMPULSE) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.impulse()
        assert e.value.code == ERR_INVALID and "at least 256 frames" in str(e.value) and "impulse response" in str(e.value), str(e.value)
        assert b.delay().shape == (2,)
    with wf.SpectrumBatch(_cfg(256), 2, ring_frames=256) as b:  # a ring that leaves P under the transform's smallest
        assert b.ring_frames == 256 and L.wf_hip_output_bytes(b.h, OUT_IMPULSE) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.impulse()
        assert e.value.code == ERR_INVALID and "ring of at least 512 frames" in str(e.value), str(e.value)
    with wf.SpectrumBatch(_cfg(1024), 2) as b:
        assert L.wf_hip_output_bytes(b.h, OUT_IMPULSE) == ENTRY  # before the first read
        check_abi_refusals(b, OUT_IMPULSE, binding.IMPULSE_DTYPE, 2, ref.zero_record(1024, b.ring_frames, 2))


def test_nothing_else_moves_on_a_twin(monkeypatch):
    """twin handles over 12 ticks, one of them read every tick: rows, bars, t-smooth and the transfer function stay bit-identical
    between the two, guard bytes behind every block intact (wf_hip_sync checks them)"""
    monkeypatch.setenv("WF_HIP_CANARY", "1")
    streams, hop, fft, sr = 3, 800, 4096, 48000
    cfg = _cfg(fft, sr, tsmoothing=binding.TSMOOTH["exponential"])
    with wf.SpectrumBatch(cfg, streams) as read, wf.SpectrumBatch(cfg, streams) as quiet:
        for t in range(12):
            a = synth.block(xfer_ref.GPU_SEED, 0, streams, 2, t * hop, hop)
            for b in (read, quiet):
                b.push_audio(a)
                b.tick()
            before = read.xfer()
            got = read.impulse()
            assert read.xfer().tobytes() == before.tobytes() == quiet.xfer().tobytes(), t
            assert np.asarray(read.decibels()).tobytes() == np.asarray(quiet.decibels()).tobytes(), t
            assert np.asarray(read.bars()).tobytes() == np.asarray(quiet.bars()).tobytes(), t
            assert read.tsmooth().tobytes() == quiet.tsmooth().tobytes(), t
        read.sync()
        quiet.sync()
        assert read.impulse().tobytes() == got.tobytes() == quiet.impulse().tobytes()  # the twin's first read
        read.sync()
        quiet.sync()
    assert np.all(got["window"] == 1024) and np.all(got["segments"] == 13) and np.all(got["valid"] == 1)


def test_three_shards_match_one_handle():
    fft, sr, hop = 2048, 48000, 801
    cfg = _cfg(fft, sr)
    kinds = ("three taps", "delay -(L-1), echo", "inverted -6 dB", "silent reference", "guarded echoes", "dual mono", "tone, measured zero")
    streams = len(kinds)
    rng = np.random.default_rng(100)
    hops = 11  # 8811 frames into the default ring of 4096
    p = xfer_ref.geometry(fft, 4096)[0]
    x = np.stack([ref.stream(k, rng, hops * hop, p, (fft + hops * hop) % (p // 2)) for k in kinds])
    with wf.SpectrumBatch(cfg, streams) as one, wf.MultiBatch(cfg, streams, [0, 0, 0]) as m:
        assert one.ring_frames == 4096
        for t in range(hops):
            a = np.ascontiguousarray(x[..., t * hop:(t + 1) * hop])
            one.push_audio(a)
            m.push_audio(a)
            one.tick()
            m.tick()
        m.sync()
        want = check_shards_match(one, m, "impulse", (2, 4))
        xf = one.xfer()
    assert np.all(want["window"] == 512) and want["valid"].tolist() == [1, 1, 1, 0, 1, 1, 1]
    assert want["lag"].tolist() == [37, -127, 0, 0, 12, 0, 0] and want["count"].tolist() == [3, 2, 1, 0, 2, 1, 0]
    _check(want, xf, x, fft, 4096, sr, fft + hops * hop, "one handle of the seven streams")


@pytest.mark.parametrize("case", [c for c in ms.CASES if c.channels == 2], ids=lambda c: c.name)
def test_staggered_write_positions(case):
    """measure_stagger's plan -- seven streams whose counters all differ, a packet longer than the ring, a reset, three push paths --
    with this output's kinds in it: every stream against the restatement of its own ring and counter at every read"""
    script = ref.stagger_script(case)
    rings = ms.Rings.of(case)
    seen = []
    with wf.SpectrumBatch(wf.Config.defaults(**case.kw), ms.STREAMS, ring_frames=case.ring_frames) as b:
        assert b.ring_frames == case.ring_cap and b.fft_size == case.W

        def on_read(i, tag):
            got = b.impulse()
            _check(got, b.xfer(), rings.histories(), case.W, case.ring_cap, case.sr, rings.counter.astype(np.int64), f"{case.name} {tag}",
                   kinds=ref.STAGGER_KINDS)
            seen.append(tag)

        ms.replay(script, rings, (b,), on_read, lambda shape: wf.PinnedBuffer(shape))
    assert "the reset of stream 5" in seen and "the packet longer than the ring" in seen and seen[-1] == "the end"
    assert rings.counter.tolist() == ms.final_counters(case).tolist() and len(set(rings.counter.tolist())) == ms.STREAMS


def test_across_the_2_to_the_32_wrap():
    """tests/impulse_wrap_child.py: twin handles on the development build, one aged to just below 2^32, walked across the wrap in
    small hops with impulse() equal on both and within the bound of the restatement at every hop.  One child process (the release
    library has no test aids)"""
    run_wrap_child("impulse_wrap_child.py", 90)
