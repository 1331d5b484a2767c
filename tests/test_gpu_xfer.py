"""Transfer function on the device (WF_HIP_OUT_XFER) against the float64 restatement (tests/xfer_ref.py) of the frames pushed:
segments of 256 (the fewest bins per thread), 512 (under an FFT that is no power of two), 1024 (the default ring of the headline
shape), 2048 (the cap) and 2048 with 32 segments (the segment cap), a meter batch and a mono mixdown display, nine streams each -- a
FIR and a delay of 37 frames, a negative delay at the end of the lag range, an inverted channel at -6 dB, added noise of equal power,
independent noise, dual mono, a measured channel that is +0.0 wherever its segments read under a reference of a tone in noise, a
silent reference, a NaN -- in uneven packets, one ring and H + 3 frames long, so that the span wraps the ring and the counter ends
off the anchor; bit identity across push paths, repeated reads, slices and pushes within a hop; reset and hidden streams; refusals;
nothing else moving on a twin; a three-shard group; seven streams at staggered write positions; the 2^32 wrap of the counters.

The bound against the restatement is derived, not measured (xfer_ref's docstring): both sides work in float64 from the same float32
samples and differ in the order of operations, and tests/test_xfer_cpu.py shows on these very seeds and shapes that the argmax of
the lag search is not near a tie and that four orderings agree to 1e-9, so one float32 rounding is all that can separate them.
Independent noise has no lag to find: the restatement takes the device's for that stream.  (On an MI355X every float32 field came
out equal to the restatement's on every case here, the staggered batch and the 2^32 wrap included, but for phases of an inverted
channel that read +pi where the restatement reads -pi: 1.7e-7 apart on the circle.)

The measured channel of stream 7 is +0.0 in every frame a segment of channel 0 covers and carries one sample in the L frames of
slack behind them: the definition calls a channel silent when its whole span is +-0, slack included, so this is how Syy == 0 on
live bins and valid == 1 come together."""
import ctypes as C

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import measure_stagger as ms
import xfer_ref as ref
from pcm_convert import captured
from tools import synth
from measure_common import Hip, check_abi_refusals, check_shards_match, check_slices_and_repeats, packets, run_wrap_child

pytestmark = pytest.mark.gpu
OUT_XFER = binding.OUT_XFER  # (the output these tests are about: a library without it fails every one of them)
ERR_INVALID = -1
ENTRY = 12336
INDEPENDENT = ref.KINDS.index("independent")


def _cfg(fft=4096, sr=48000, **kw):
    return wf.Config.defaults(**{**dict(fft_size=fft, sample_rate=sr, capture_channels=2, stereo=1, slope=1.0, bars=1, floor_db=-70), **kw})


def _check(got, frames, w, ring, sr, wpos, what="", free=()):
    """every entry of `got` within the bound of the restatement of `frames`, each figure printed first.  free: the streams whose
    lag is noise -- the restatement takes the device's there; everywhere else its own search must agree"""
    lags = [int(got["lag"][s]) if s in free else None for s in range(len(frames))]
    want = ref.xfer(frames, w, ring, sr, lag=lags, wpos=wpos)
    assert got.dtype == binding.XFER_DTYPE and got.shape == want.shape
    print(f"{what}: P {got['window'].tolist()}, K {got['segments'].tolist()}, valid {got['valid'].tolist()}, lag {got['lag'].tolist()}, "
          f"lag_peak {got['lag_peak'].tolist()}, mean coherence {got['mean_coherence'].tolist()}, "
          f"worst |got - want| {ref.worst(got, want)}")
    margin = ref.margins(frames, w, ring, sr, wpos)
    for s in range(len(frames)):  # the condition the bound rests on (test_xfer_cpu.py), for whatever is compared here
        g0 = want["valid"][s] and want["lag_peak"][s] != 0
        assert s in free or not g0 or margin[s] >= 1e-3, (s, margin[s])
    bad = ref.mismatches(got, want)
    assert not bad, bad[:8]
    assert not got["reserved"].any()
    m = int(got["window"][0]) // 2
    for name in ("gain_db", "phase", "coherence"):
        assert not got[name][:, 0].any() and not got[name][:, m:].any(), name  # index 0 and the indices from M up
    return want


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=ref.case_id)
def test_xfer_equals_the_restatement_of_the_frames(case):
    fft, sr, kw, w, ring = case
    x = ref.case_audio(case)
    cap = ref.ring_frames(w, ring)
    p, k = ref.geometry(w, cap)
    with wf.SpectrumBatch(_cfg(fft, sr, **kw), x.shape[0], ring_frames=ring or 0) as b:
        assert b.fft_size == w and b.ring_frames == cap and b.capture_channels == 2
        assert wf.lib().wf_hip_output_bytes(b.h, binding.OUT_XFER) == ENTRY  # before the first read
        for lo, hi in packets(np.random.default_rng(w), x.shape[-1], 700):
            b.push_audio(np.ascontiguousarray(x[:, :, lo:hi]))
        got = b.xfer()
    wpos = ref.case_wpos0(case) + x.shape[-1]
    assert wpos % (p // 2) != 0 and x.shape[-1] > cap  # off the anchor, and the span wraps the ring
    assert np.all(got["window"] == p) and np.all(got["hop"] == p // 2) and np.all(got["segments"] == k)
    _check(got, x, w, cap, sr, wpos, ref.case_id(case), free=(INDEPENDENT,))
    assert got["valid"].tolist() == [int(name not in ref.INVALID) for name in ref.KINDS]
    assert got[7:].tobytes() == ref.zero_record(w, cap, 2).tobytes()  # a silent reference and a NaN: the zero record
    assert got["lag"][:4].tolist() == [37, -(p // 4 - 1), 0, 0] and got["lag"][5:7].tolist() == [0, 0]
    assert np.all(got["newest"][:7] == wpos // (p // 2))
    live = slice(1, p // 2)
    dual = got[ref.KINDS.index("dual mono")]  # gain 0.0 dB, phase 0, coherence 1, lag 0: exactly
    assert dual["lag"] == 0 and dual["mean_coherence"] == 1.0 and dual["lag_peak"] == 1.0 and np.all(dual["coherence"][live] == 1.0)
    assert not dual["gain_db"].any() and not dual["phase"].any()
    zero = got[ref.KINDS.index("tone, measured zero")]  # live bins with Syy == 0
    assert zero["valid"] == 1 and np.all(np.isneginf(zero["gain_db"][live])) and not zero["phase"].any() and not zero["coherence"].any()
    assert zero["lag"] == 0 and zero["lag_peak"] == 0.0 and zero["mean_coherence"] == 0.0
    inv = got[ref.KINDS.index("inverted -6 dB")]
    assert np.all(np.abs(inv["gain_db"][live] - np.float32(-6.0206)) < 1e-4) and np.all(np.abs(np.abs(inv["phase"][live]) - np.float32(np.pi)) < 1e-6)


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=ref.case_id)
def test_dual_mono_reads_exactly(case):
    """dual mono reads gain 0.0 dB, phase 0, coherence 1 and lag 0 exactly, as the restatement does, whose two transforms of the same
    samples are the same bits.  On the device both channels come out of ONE complex transform, and separated from Z[k] and
    conj Z[P - k] -- two values that reach the same number by different butterflies -- the spectra of equal inputs differ in their
    last bits: |gain_db| up to 2.9e-15 dB and |phase| up to 1.3e-16 rad were read that way.  So a segment whose channels are the same
    bits takes both spectra from Z[k] alone (include/wf_hip.h, "transfer function", spectra), and the sums are compiled unfused"""
    fft, sr, kw, w, ring = case
    cap = ref.ring_frames(w, ring)
    p, k = ref.geometry(w, cap)
    x = ref.case_audio(case)[ref.KINDS.index("dual mono")][None]
    with wf.SpectrumBatch(_cfg(fft, sr, **kw), 1, ring_frames=ring or 0) as b:
        b.push_audio(x)
        dual = b.xfer()[0]
    live = slice(1, p // 2)
    print(f"{ref.case_id(case)}: worst |gain_db| {float(np.max(np.abs(dual['gain_db'][live]))):.3g} dB, worst |phase| "
          f"{float(np.max(np.abs(dual['phase'][live]))):.3g} rad, least coherence {float(np.min(dual['coherence'][live]))!r}, lag {int(dual['lag'])}")
    assert dual["valid"] == 1 and dual["lag"] == 0 and dual["lag_peak"] == 1.0 and dual["mean_coherence"] == 1.0
    assert np.all(dual["coherence"][live] == 1.0)
    assert np.all(dual["gain_db"][live] == 0.0) and np.all(dual["phase"][live] == 0.0)


def test_every_push_path_counts():
    """the same s16 frames through push_audio, its async form, wf_hip_push_pcm (s16 interleaved: every value exact in float32) and
    push_audio_device read bit-identically"""
    streams, fft, frames, sr = 3, 1024, 801, 48000
    rng = np.random.default_rng(2)
    packets = 12  # 9612 frames: more than the ring of 4096
    base = np.stack([ref.stream(k, rng, packets * frames, 512) for k in ("fir +37", "delay -(L-1)", "added noise")])  # [streams, 2, n]
    wave = np.round(32768.0 * 0.9 * np.clip(base, -1.0, 1.0)).astype(np.int16).transpose(0, 2, 1)  # [streams, n, 2]
    pkts = [np.ascontiguousarray(wave[:, i * frames:(i + 1) * frames]) for i in range(packets)]
    hip = Hip()
    reads = {}
    for path in ("float", "async", "pcm", "device"):
        with wf.SpectrumBatch(_cfg(fft, sr), streams) as b:
            assert b.ring_frames == 4096
            for i, pkt in enumerate(pkts):
                conv = np.ascontiguousarray(captured(pkt, True, 0, 2))  # [streams, 2, frames] float32
                if path == "float":
                    b.push_audio(conv)
                elif path == "async":
                    pin = wf.PinnedBuffer(conv.shape)
                    try:
                        b.ingest_done(0)
                        pin.array[...] = conv
                        b.push_audio_ragged_async(pin, np.full(streams, frames, np.uint32), frames, 0)
                        b.sync()
                    finally:
                        pin.close()
                elif path == "pcm":
                    b.push_pcm(pkt, interleaved=True)
                else:
                    d = hip.upload(conv)
                    b.push_audio_device(d, streams, frames)
                    b.sync()
                    assert hip.free(d) == 0
            reads[path] = b.xfer()
    for path in ("async", "pcm", "device"):
        assert reads[path].tobytes() == reads["float"].tobytes(), path
    hist = np.concatenate([captured(pkt, True, 0, 2) for pkt in pkts], axis=2)
    want = _check(reads["float"], hist, fft, 4096, sr, fft + packets * frames, "s16 packets")
    assert np.all(want["valid"] == 1) and want["lag"].tolist() == [37, -127, 0] and np.all(want["window"] == 512)


def test_repeated_reads_slices_and_pushes_within_a_hop():
    """a slice as a handle's first read equals the entry of the full read; reads with nothing in between, a read after a tick, and
    a read after a push of fewer frames than are left to the next anchor are bit-identical; the push that crosses the anchor moves
    `newest` by one"""
    fft, sr, ring = 1024, 48000, 8192
    kinds = ("fir +37", "added noise", "independent", "silent reference", "delay -(L-1)")
    streams = len(kinds)
    p, k = ref.geometry(fft, ring)
    h = p // 2
    total = ring + h + 3
    rng = np.random.default_rng(11)
    x = np.stack([ref.stream(name, rng, total + h, p) for name in kinds])
    with wf.SpectrumBatch(_cfg(fft, sr), streams, ring_frames=ring) as b:
        assert b.ring_frames == ring and (fft + total) % h == 3
        b.push_audio(np.ascontiguousarray(x[..., :5000]))
        b.push_audio(np.ascontiguousarray(x[..., 5000:total]))
        full = check_slices_and_repeats(b, "xfer")
        b.push_audio(np.ascontiguousarray(x[..., total:total + h - 4]))  # one frame short of the next anchor
        assert b.xfer().tobytes() == full.tobytes()
        b.push_audio(np.ascontiguousarray(x[..., total + h - 4:total + h - 3]))  # the anchor
        moved = b.xfer()
    assert np.all(moved["newest"][[0, 1, 2, 4]] == full["newest"][[0, 1, 2, 4]] + 1) and moved.tobytes() != full.tobytes()
    assert full["valid"].tolist() == [1, 1, 1, 0, 1] and full["lag"][[0, 1, 4]].tolist() == [37, 0, -255]
    _check(full, x[..., :total], fft, ring, sr, fft + total, "before the anchor", free=(2,))
    _check(moved, x[..., :total + h - 3], fft, ring, sr, fft + total + h - 3, "behind the anchor", free=(2,))


def test_fresh_reset_and_hidden_streams():
    fft, streams, sr = 1024, 4, 48000
    with wf.SpectrumBatch(_cfg(fft, sr), streams) as b:
        ring = b.ring_frames
        p, k = ref.geometry(fft, ring)
        rng = np.random.default_rng(13)
        n = ring + 801
        x = np.stack([ref.stream(name, rng, n, p) for name in ("fir +37", "delay -(L-1)", "dual mono", "inverted -6 dB")])
        zero = ref.zero_record(fft, ring, streams)
        assert ref.mismatches(zero, ref.xfer(np.zeros((streams, 2, fft), np.float32), fft, ring, sr)) == []
        assert b.xfer().tobytes() == zero.tobytes()  # freshly created, both channels silent: valid = 0
        b.set_hidden(np.array([0, 1, 0, 0], np.uint8))
        b.push_audio(x)
        b.tick()
        before = b.xfer()
        _check(before, x, fft, ring, sr, fft + n, "one stream hidden")  # the hidden stream's ring reads like any other
        assert np.all(before["valid"] == 1) and before["lag"].tolist() == [37, -(p // 4 - 1), 0, 0]
        b.reset(2, 1)
        after = b.xfer()
    assert after[2:3].tobytes() == zero[:1].tobytes()
    keep = [0, 1, 3]
    assert after[keep].tobytes() == before[keep].tobytes()


def test_refusals():
    L = wf.lib()
    with wf.SpectrumBatch(wf.Config.defaults(waveform=1, stereo=1, width=640, meter_ms=100), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_XFER) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.xfer()
        assert e.value.code == ERR_INVALID and "waveform batch" in str(e.value) and "transfer function" in str(e.value), str(e.value)
        out = np.empty(2, binding.XFER_DTYPE)
        assert L.wf_hip_read(b.h, binding.OUT_XFER, 0, 2, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID
        assert b"transfer function" in L.wf_hip_last_error(b.h)
    with wf.SpectrumBatch(_cfg(1024, capture_channels=1, stereo=0), 2) as b:  # one captured channel: nothing to compare
        assert b.capture_channels == 1 and L.wf_hip_output_bytes(b.h, binding.OUT_XFER) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.xfer()
        assert e.value.code == ERR_INVALID and "two captured channels" in str(e.value) and "transfer function" in str(e.value), str(e.value)
        assert b.thd().shape == (2,)  # the other readers of such a batch are unharmed
    with wf.SpectrumBatch(_cfg(240), 2) as b:  # W < 256
        assert b.fft_size == 240 and L.wf_hip_output_bytes(b.h, binding.OUT_XFER) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.xfer()
        assert e.value.code == ERR_INVALID and "at least 256 frames" in str(e.value) and "transfer function" in str(e.value), str(e.value)
        assert b.delay().shape == (2,)
    with wf.SpectrumBatch(_cfg(256), 2, ring_frames=256) as b:  # a ring that leaves P under the transform's smallest
        assert b.ring_frames == 256 and L.wf_hip_output_bytes(b.h, binding.OUT_XFER) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.xfer()
        assert e.value.code == ERR_INVALID and "ring of at least 512 frames" in str(e.value), str(e.value)
    with wf.SpectrumBatch(_cfg(1024), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_XFER) == ENTRY  # before the first read
        check_abi_refusals(b, binding.OUT_XFER, binding.XFER_DTYPE, 2, ref.zero_record(1024, b.ring_frames, 2))


def test_nothing_else_moves_on_a_twin(monkeypatch):
    """twin handles over 20 ticks, one of them read every tick: rows, bars and t-smooth -- and every other output -- stay
    bit-identical between the two, guard bytes behind every block intact (wf_hip_sync checks them)"""
    monkeypatch.setenv("WF_HIP_CANARY", "1")
    streams, hop, fft, sr = 3, 800, 4096, 48000
    names = ("decibels", "bars", "signal", "pitch", "stereo", "scope", "gonio", "bits", "thd", "delay", "onset", "sono", "cq")
    cfg = _cfg(fft, sr, tsmoothing=binding.TSMOOTH["exponential"])
    with wf.SpectrumBatch(cfg, streams) as read, wf.SpectrumBatch(cfg, streams) as quiet:
        for t in range(20):
            a = synth.block(ref.GPU_SEED, 0, streams, 2, t * hop, hop)
            for b in (read, quiet):
                b.push_audio(a)
                b.tick()
            got = read.xfer()
            assert np.asarray(read.decibels()).tobytes() == np.asarray(quiet.decibels()).tobytes(), t
            assert np.asarray(read.bars()).tobytes() == np.asarray(quiet.bars()).tobytes(), t
            assert read.tsmooth().tobytes() == quiet.tsmooth().tobytes(), t
        read.sync()
        quiet.sync()
        for n in names:
            assert np.asarray(getattr(read, n)()).tobytes() == np.asarray(getattr(quiet, n)()).tobytes(), n
        assert read.xfer().tobytes() == got.tobytes() == quiet.xfer().tobytes()  # the twin's first read
        read.sync()
        quiet.sync()
    assert np.all(got["window"] == 1024) and np.all(got["segments"] == 13) and np.all(got["valid"] == 1)


def test_three_shards_match_one_handle():
    fft, sr, hop = 2048, 48000, 801
    cfg = _cfg(fft, sr)
    kinds = ("fir +37", "delay -(L-1)", "inverted -6 dB", "silent reference", "added noise", "dual mono", "tone, measured zero")
    streams = len(kinds)
    rng = np.random.default_rng(100)
    hops = 11  # 8811 frames into the default ring of 4096
    p = ref.geometry(fft, 4096)[0]
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
        want = check_shards_match(one, m, "xfer", (2, 4))
    assert np.all(want["window"] == 512) and want["valid"].tolist() == [1, 1, 1, 0, 1, 1, 1]
    assert want["lag"].tolist() == [37, -127, 0, 0, 0, 0, 0]
    _check(want, x, fft, 4096, sr, fft + hops * hop, "one handle of the seven streams")


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
            got = b.xfer()
            hist, wpos = rings.histories(), rings.counter.astype(np.int64)
            want = ref.xfer(hist, case.W, case.ring_cap, case.sr, wpos=wpos)
            margin = [ref.analyse(hist[s], case.W, case.ring_cap, case.sr, wpos=wpos[s])[1].get("margin", 1.0) for s in range(ms.STREAMS)]
            print(f"{case.name} {tag}: counters {wpos.tolist()}, valid {got['valid'].tolist()}, lag {got['lag'].tolist()}, "
                  f"least margin {min(margin):.3g}, worst {ref.worst(got, want)}")
            assert min(m for m, v in zip(margin, want["valid"]) if v) >= 1e-3, (tag, margin)
            bad = ref.mismatches(got, want)
            assert not bad, (tag, bad[:6])
            seen.append(tag)

        ms.replay(script, rings, (b,), on_read, lambda shape: wf.PinnedBuffer(shape))
    assert "the reset of stream 5" in seen and "the packet longer than the ring" in seen and seen[-1] == "the end"
    assert rings.counter.tolist() == ms.final_counters(case).tolist() and len(set(rings.counter.tolist())) == ms.STREAMS


def test_across_the_2_to_the_32_wrap():
    """tests/xfer_wrap_child.py: twin handles on the development build, one aged to just below 2^32, walked across the wrap in
    small hops with xfer() equal on both and within the bound of the restatement at every hop.  One child process (the release
    library has no test aids)"""
    run_wrap_child("xfer_wrap_child.py", 60)
