"""Stereo image on the device (WF_HIP_OUT_STEREO) against the float64 restatement (tests/stereo_ref.py) of the frames pushed,
over windows from 128 to 4096 frames, three sample rates, an FFT size that is no power of two, a window shorter than the FFT, a
meter batch and a mono mixdown of two captured channels; a delayed sine and an inverted channel against analytic truth; bit
identity across push paths and repeated reads; slices; reset and hidden streams; refusals; nothing else moving; a three-shard
group.

The bound against the restatement is derived, not measured (include/wf_hip.h, "determinism"): both sides work in float64 from
the same float32 samples and differ in the order of the transform's operations, below 1e-12 in every field before the one
rounding to float32.  So |got - want| <= max(1 float32 ulp of want, 1e-9) for correlation, coherence and balance_db, and for
phase_deg wherever the restatement's coherence is >= 0.01; `covered` and `window` are equal (stereo_ref.mismatches).  The bands
under 0.01, where the phase is not compared, must be at most 1 % of those that overlap the bins."""

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import stereo_ref as ref
from pcm_convert import captured
from tools import synth
from measure_common import Hip, check_abi_refusals, check_shards_match, check_slices_and_repeats, packets

pytestmark = pytest.mark.gpu
ERR_INVALID = -1
SEED = 20261017
HOP = 800


def _cfg(fft=4096, sr=48000, **kw):
    return wf.Config.defaults(**{**dict(fft_size=fft, sample_rate=sr, capture_channels=2, stereo=1, slope=1.0, bars=1, floor_db=-70), **kw})


def _check(got, want, sr, what=""):
    assert got.dtype == binding.STEREO_DTYPE and got.shape == want.shape
    live = ref.overlapping(sr, int(want["window"].flat[0]))
    share = ref.low_coherence_share(want, sr)
    worst = {n: float(np.nanmax(np.abs(got[n][:, live].astype(np.float64) - want[n][:, live].astype(np.float64)))) for n in ref.FIELDS}
    print(f"{what}: P {int(want['window'].flat[0])}, {int(live.sum())} bands overlap, covered {int(want['covered'].flat[0]):#010x}, "
          f"share of bands with coherence < 0.01: {share:.4f}, worst |got - want| {worst}")
    assert share <= 0.01
    bad = ref.mismatches(got, want)
    assert not bad, bad[:8]


CASES = [  # (fft, sample rate, overrides)
    (128, 48000, {}), (2064, 44100, {}), (4096, 48000, {}), (16384, 96000, {}), (1024, 48000, dict(meter=1, bars=0)),
    (1024, 48000, dict(stereo=0)),
]


@pytest.mark.parametrize("fft,sr,kw", CASES, ids=[f"n{f}_sr{s}" + "".join(f"_{k}{v}" for k, v in kw.items() if k != "bars") for f, s, kw in CASES])
def test_stereo_equals_the_reference_of_the_frames(fft, sr, kw):
    streams = 3
    rng = np.random.default_rng(SEED + fft)
    with wf.SpectrumBatch(_cfg(fft, sr, **kw), streams) as b:
        p = ref.window_frames(b.fft_size)
        x = ref.audio(rng, streams, p + 2 * HOP, sr)
        for lo, hi in packets(np.random.default_rng(fft), x.shape[-1], 699):
            b.push_audio(np.ascontiguousarray(x[:, :, lo:hi]))
        got = b.stereo()
        assert wf.lib().wf_hip_output_bytes(b.h, binding.OUT_STEREO) == 504
    want = ref.stereo(x[..., -p:], sr)
    assert np.all(got["window"] == p)
    _check(got, want, sr, f"fft {fft} sr {sr} {kw}")


def test_a_delayed_sine_and_an_inverted_channel():
    """P = 4096, 48 kHz.  Stream 0: a 1 kHz sine, r six frames late: 360 * 1000 * 6 / 48000 = 45 degrees in band 17 (1 kHz).
    Stream 1: noise with r = -l."""
    sr, p, f, d = 48000, 4096, 1000.0, 6
    t = np.arange(p + HOP)
    l0 = 0.5 * np.sin(2 * np.pi * f * t / sr)
    r0 = 0.5 * np.sin(2 * np.pi * f * (t - d) / sr)
    n = 0.25 * np.random.default_rng(5).standard_normal(p + HOP)
    x = np.stack([np.stack([l0, r0]), np.stack([n, -n])]).astype(np.float32)
    with wf.SpectrumBatch(_cfg(p, sr), 2) as b:
        b.push_audio(x)
        got = b.stereo()
    g = got[0]
    print("band 17:", g["phase_deg"][17], g["coherence"][17], g["balance_db"][17], g["correlation"][17])
    assert abs(g["phase_deg"][17] - 45.0) <= 0.5 and g["coherence"][17] > 0.999 and abs(g["balance_db"][17]) <= 0.01
    cov = [bb for bb in range(31) if got["covered"][1] >> bb & 1]
    assert len(cov) == 31
    assert np.all(got["correlation"][1, cov] == -1.0) and np.all(got["phase_deg"][1, cov] == 180.0)
    assert np.all(got["coherence"][1, cov] == 1.0) and np.all(np.abs(got["balance_db"][1, cov]) < 1e-6)
    # (not compared with the restatement band by band: far from 1 kHz a pure sine leaves the window's leakage at the level of
    # the transform's own rounding, and the ratio of two such sums is not a number either side can state to an ulp)
    want = ref.stereo(x[..., -p:], sr)
    assert not ref.mismatches(got[1:], want[1:]) and abs(float(want["phase_deg"][0, 17]) - float(g["phase_deg"][17])) < 1e-4


def test_every_push_path_counts():
    """the same frames through push_audio, wf_hip_push_pcm (s16 interleaved: every value exact in float32) and
    push_audio_device read bit-identically"""
    streams, fft, frames = 3, 1024, 801
    rng = np.random.default_rng(2)
    pkts = [rng.integers(-32768, 32768, (streams, frames, 2)).astype(np.int16) for _ in range(3)]
    hip = Hip()
    reads = {}
    for path in ("float", "pcm", "device"):
        with wf.SpectrumBatch(_cfg(fft), streams) as b:
            for pkt in pkts:
                conv = np.ascontiguousarray(captured(pkt, True, 0, 2))  # [streams, 2, frames] float32
                assert np.array_equal(conv, pkt.transpose(0, 2, 1).astype(np.float32) / np.float32(32768.0))
                if path == "float":
                    b.push_audio(conv)
                elif path == "pcm":
                    b.push_pcm(pkt, interleaved=True)
                else:
                    d = hip.upload(conv)
                    b.push_audio_device(d, streams, frames)
                    b.sync()
                    assert hip.free(d) == 0
            reads[path] = b.stereo()
    assert reads["pcm"].tobytes() == reads["float"].tobytes() and reads["device"].tobytes() == reads["float"].tobytes()
    hist = np.concatenate([captured(pkt, True, 0, 2) for pkt in pkts], axis=2)
    assert not ref.mismatches(reads["float"], ref.stereo(hist[..., -fft:], 48000))


def test_repeated_reads_and_slices():
    """a slice as a handle's first read equals the entry of the full read; reads with nothing in between are bit-identical; the
    window wraps round a ring of its own length"""
    fft, sr, streams = 2048, 48000, 5
    x = ref.audio(np.random.default_rng(11), streams, 3001, sr)
    with wf.SpectrumBatch(_cfg(fft, sr), streams, ring_frames=fft) as b:
        assert b.ring_frames == fft
        b.push_audio(np.ascontiguousarray(x[..., :2000]))
        b.push_audio(np.ascontiguousarray(x[..., 2000:]))
        full = check_slices_and_repeats(b, "stereo")
    _check(full, ref.stereo(x[..., -fft:], sr), sr, "wrapped ring")


def test_reset_and_hidden_streams():
    fft, sr, streams = 1024, 48000, 4
    x = ref.audio(np.random.default_rng(13), streams, fft + HOP, sr)
    silence = ref.stereo(np.zeros((1, 2, fft), np.float32), sr)
    with wf.SpectrumBatch(_cfg(fft, sr), streams) as b:
        assert b.stereo().tobytes() == np.repeat(silence, streams).tobytes()  # freshly created: zeros
        b.set_hidden(np.array([0, 1, 0, 0], np.uint8))
        b.push_audio(x)
        b.tick()
        before = b.stereo()
        _check(before, ref.stereo(x[..., -fft:], sr), sr, "one stream hidden")  # the hidden stream's ring reads like any other
        b.reset(2, 1)
        after = b.stereo()
    assert after[2:3].tobytes() == silence.tobytes()
    for name in ref.FIELDS:
        assert np.all(after[name][2] == 0.0), name
    assert after["window"][2] == fft and after["covered"][2] == before["covered"][0]
    keep = [0, 1, 3]
    assert after[keep].tobytes() == before[keep].tobytes()


def test_refusals():
    L = wf.lib()
    for cfg, text in ((_cfg(1024, capture_channels=1, stereo=0), "one captured channel"),
                      (wf.Config.defaults(waveform=1, stereo=1, width=640, meter_ms=100), "waveform batch"),
                      (_cfg(1024, capture_channels=1, stereo=0, meter=1, bars=0), "one captured channel")):
        with wf.SpectrumBatch(cfg, 2) as b:
            assert L.wf_hip_output_bytes(b.h, binding.OUT_STEREO) == 0
            with pytest.raises(wf.WfHipError) as e:
                b.stereo()
            assert e.value.code == ERR_INVALID and text in str(e.value), str(e.value)
    with wf.SpectrumBatch(_cfg(1024), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_STEREO) == 504  # before the first read
        out = check_abi_refusals(b, binding.OUT_STEREO, binding.STEREO_DTYPE, 2)
        assert np.all(out["window"][:2] == 1024)


def test_nothing_else_moves(monkeypatch):
    """twin handles for 20 ticks, one of them read every tick: every other output stays bit-identical; guard bytes intact"""
    monkeypatch.setenv("WF_HIP_CANARY", "1")
    cfg = _cfg(4096, tsmoothing=wf.TSMOOTH["exponential"])
    streams = 16
    with wf.SpectrumBatch(cfg, streams) as a, wf.SpectrumBatch(cfg, streams) as b:
        for t in range(20):
            x = synth.block(SEED, 0, streams, 2, t * HOP, HOP)
            a.push_audio(x)
            b.push_audio(x)
            a.tick()
            b.tick()
            b.stereo()
        b.sync()
        a.sync()
        for name in ("decibels", "bars", "tsmooth", "last_silent", "signal", "bands", "peaks", "pitch"):
            assert np.asarray(getattr(a, name)()).tobytes() == np.asarray(getattr(b, name)()).tobytes(), name
        first = a.stereo()
        assert first.tobytes() == b.stereo().tobytes()  # a handle's first read equals another's twenty-first
        b.sync()
    hist = np.concatenate([synth.block(SEED, 0, streams, 2, t * HOP, HOP) for t in range(20)], axis=2)
    assert not ref.mismatches(first, ref.stereo(hist[..., -4096:], 48000))


def test_three_shards_match_one_handle():
    cfg = _cfg(2048)
    streams, hop = 7, 801
    with wf.SpectrumBatch(cfg, streams) as one, wf.MultiBatch(cfg, streams, [0, 0, 0]) as m:
        for t in range(5):
            x = synth.block(SEED, 0, streams, 2, t * hop, hop)
            one.push_audio(x)
            m.push_audio(x)
            one.tick()
            m.tick()
        m.sync()
        want = check_shards_match(one, m, "stereo", (2, 4))
