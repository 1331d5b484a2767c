"""The loudness producer on the device (wf_hip_enable_loudness, WF_HIP_OUT_LOUDNESS): EBU Tech 3341 / 3342-style cases against
analytic truth, true peak of sines off the sample grid, a fuzz against the float64 reference (tests/loudness_ref.py),
packet-split invariance, bit identity across every push path and batch kind, nothing else moving, lifecycle and errors, and a
10-minute stationary run."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import waveform_amd as wf
import loudness_ref as ref
from tools import synth

pytestmark = pytest.mark.gpu
ERR_INVALID = -1
FIELDS = ("momentary", "short_term", "integrated", "range", "true_peak")


def _cfg(cap=2, fs=48000, **kw):
    return wf.Config.defaults(**{**dict(fft_size=1024, sample_rate=fs, capture_channels=cap, stereo=1 if cap == 2 else 0, bars=1, slope=1.0), **kw})


def _db(a):
    return 10.0 ** (a / 20.0)


def _tone(fs, f, seconds, dbfs, phase=0.0):
    t = np.arange(int(round(fs * seconds))) / fs
    return _db(dbfs) * np.sin(2 * np.pi * f * t + phase)


def _feed(b, x, sizes, first=0):
    """x: float32 [streams, channels, frames] in packets of the given sizes (cycled until x is used up)"""
    n, pos, i = x.shape[2], 0, 0
    while pos < n:
        k = min(int(sizes[i % len(sizes)]), n - pos)
        b.push_audio(np.ascontiguousarray(x[:, :, pos:pos + k]), first=first)
        pos += k
        i += 1


def _close(got, want, tol, floor=None):
    """within tol, or both -inf; with `floor`: both at or below it (a filter tail decaying into float32 underflow reads -inf
    where the float64 reference still sees -2000 LUFS)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    both_inf = np.isneginf(got) & np.isneginf(want)
    both_low = (got <= floor) & (want <= floor) if floor is not None else False
    return np.all(both_inf | both_low | (np.abs(got - want) <= tol))


def _bits_equal(a, b):
    return a.tobytes() == b.tobytes()


def test_tech3341_levels_and_gating():
    fs = 48000
    silence = lambda s: np.zeros(int(fs * s))
    seq = np.concatenate([_tone(fs, 997, 10, -36), _tone(fs, 997, 60, -23), _tone(fs, 997, 10, -36)])
    mono = [np.concatenate([silence(80), _tone(fs, 997, 20, -23)]),
            np.concatenate([silence(80), _tone(fs, 997, 20, -33)]),
            np.concatenate([silence(20), seq]),
            np.concatenate([_tone(fs, 997, 10, -72), seq, _tone(fs, 997, 10, -72)]),
            np.concatenate([silence(60), _tone(fs, 997, 20, -20), _tone(fs, 997, 20, -30)])]
    x = np.stack([np.stack([m, m]) for m in mono]).astype(np.float32)
    with wf.SpectrumBatch(_cfg(), len(mono), ring_frames=1 << 16) as b:
        b.enable_loudness()
        _feed(b, x, [fs])
        r = b.loudness()
    for s, level in ((0, -23.0), (1, -33.0)):
        for k in ("momentary", "short_term", "integrated"):
            assert abs(r[k][s] - level) <= 0.1, (s, k, r[k][s])
    assert abs(r["integrated"][2] + 23.0) <= 0.1, r["integrated"][2]
    assert abs(r["integrated"][3] + 23.0) <= 0.1, r["integrated"][3]
    assert abs(r["range"][4] - 10.0) <= 1.0, r["range"][4]
    assert np.all(r["frames"] == x.shape[2])


@pytest.mark.parametrize("fs", [48000, 44100])
def test_true_peak_of_sines(fs):
    cases = [(f, a, p) for f in (fs / 4, fs / 6, fs / 8, 997.0) for a in (-6.0, 0.0) for p in (0.0, 45.0, 60.0)]
    # a 20 ms raised-cosine fade-in: an abrupt onset rings through any band-limited interpolator (a real overshoot, not the
    # meter's error)
    fade = np.ones(int(fs * 0.5))
    k = int(fs * 0.02)
    fade[:k] = 0.5 - 0.5 * np.cos(np.pi * np.arange(k) / k)
    x = np.stack([np.stack([_tone(fs, f, 0.5, a, np.deg2rad(p)) * fade] * 2) for f, a, p in cases]).astype(np.float32)
    with wf.SpectrumBatch(_cfg(fs=fs), len(cases)) as b:
        b.enable_loudness()
        _feed(b, x, [1000])
        tp = b.loudness()["true_peak"]
    sample_peak = 20 * np.log10(np.abs(x).max(axis=(1, 2)))
    for i, (f, a, p) in enumerate(cases):
        assert a - 0.4 <= tp[i] <= a + 0.2, (f, a, p, tp[i])
        assert tp[i] >= sample_peak[i]
        if f == fs / 4 and p == 45.0:
            assert 2.6 <= tp[i] - sample_peak[i] <= 3.2, (a, tp[i], sample_peak[i])


def _fuzz_audio(rng, streams, cap, fs, seconds):
    n = int(fs * seconds)
    x = np.zeros((streams, cap, n))
    for s in range(streams):
        if s % 2:
            src = synth.block(synth.DEFAULT_SEED + s, s, 1, cap, 0, n)[0].astype(np.float64)
        else:  # shaped noise: a random one-pole low-pass or high-pass of Gaussian noise
            w = rng.standard_normal((cap, n)) * 0.3
            a = rng.uniform(0.0, 0.95)
            for c in range(cap):
                w[c] = np.cumsum(w[c]) * (1 - a) if rng.random() < 0.5 else w[c] - a * np.roll(w[c], 1)
            src = np.clip(w / max(np.abs(w).max(), 1e-9), -1, 1)
        # piecewise levels from -60 to 0 dBFS with silent stretches, segments of at least half a second
        gain = np.zeros(n)
        pos = 0
        while pos < n:
            k = int(rng.uniform(0.5, 2.0) * fs)
            gain[pos:pos + k] = 0.0 if rng.random() < 0.2 else _db(rng.uniform(-60.0, 0.0))
            pos += k
        x[s] = src * gain
    return x.astype(np.float32)


@pytest.mark.parametrize("cap,fs,ragged", [(1, 48000, False), (2, 48000, True), (1, 44100, True), (2, 44100, False)])
def test_fuzz_against_the_reference(cap, fs, ragged):
    streams, seconds = 16, 6.0
    rng = np.random.default_rng(cap * 7 + fs)
    x = _fuzz_audio(rng, streams, cap, fs, seconds)
    n = x.shape[2]
    with wf.SpectrumBatch(_cfg(cap, fs), streams, ring_frames=1 << 14) as b:
        b.enable_loudness()
        if not ragged:
            sizes = rng.integers(1, int(fs * 0.13), 64)
            sizes[::5] = 1
            _feed(b, x, sizes)
        else:
            max_frames = int(fs * 0.13)
            pin = [wf.PinnedBuffer((streams, cap, max_frames)), wf.PinnedBuffer((streams, cap, max_frames))]
            pos = np.zeros(streams, np.int64)
            t = 0
            while np.any(pos < n):
                slot = t & 1
                b.ingest_done(slot)
                frames = np.minimum(rng.integers(0, max_frames + 1, streams), n - pos).astype(np.uint32)
                frames[rng.integers(0, streams)] = min(1, n - pos.min())  # single frames too
                frames = np.minimum(frames, n - pos).astype(np.uint32)
                for s in range(streams):
                    pin[slot].array[s, :, :frames[s]] = x[s, :, pos[s]:pos[s] + frames[s]]
                b.push_audio_ragged_async(pin[slot], frames, max_frames, slot)
                pos += frames
                t += 1
            b.sync()
            for p in pin:
                p.close()
        got = b.loudness()
    want = ref.measure(x, fs)
    assert np.all(got["frames"] == n)
    assert np.all(got["reserved"] == 0)
    for k, tol in (("momentary", 0.01), ("short_term", 0.01), ("integrated", 0.05), ("range", 0.2), ("true_peak", 0.05)):
        bad = [(s, float(got[k][s]), float(want[k][s])) for s in range(streams) if not _close(got[k][s], want[k][s], tol, floor=-150.0)]
        assert not bad, (k, bad)


def test_packet_split_invariance():
    fs, seconds = 48000, 6.0
    rng = np.random.default_rng(5)
    x = _fuzz_audio(rng, 1, 2, fs, seconds)
    n = x.shape[2]
    with wf.SpectrumBatch(_cfg(), 3, ring_frames=1 << 19) as b:
        b.enable_loudness()
        b.push_audio(x, first=0)                         # one packet
        _feed(b, x, [800], first=1)                      # 800-frame hops
        _feed(b, x, rng.integers(1, 9000, 200), first=2)  # random splits
        r = b.loudness()
    assert np.all(r["frames"] == n)
    for k in FIELDS:
        assert _close(r[k][1:], r[k][0], 1e-3), (k, r[k])


def _hops(rng, streams, cap, hops=60, frames=800):
    return [rng.uniform(-0.5, 0.5, (streams, cap, frames)).astype(np.float32) for _ in range(hops)]


def test_paths_match_push_audio():
    streams, cap, frames = 5, 2, 800
    rng = np.random.default_rng(3)
    pkts = _hops(rng, streams, cap)

    def twin_of(feed, cfg=None):
        cfg = cfg or _cfg()
        with wf.SpectrumBatch(cfg, streams) as b, wf.SpectrumBatch(_cfg(), streams) as twin:
            b.enable_loudness()
            twin.enable_loudness()
            want_pkts = feed(b)
            for p in want_pkts:
                twin.push_audio(p)
            got, want = b.loudness(), twin.loudness()
        assert _bits_equal(got, want), (got, want)
        return got

    # _async through both slots
    def feed_async(b):
        pin = [wf.PinnedBuffer((streams, cap, frames)), wf.PinnedBuffer((streams, cap, frames))]
        for t, p in enumerate(pkts):
            b.ingest_done(t & 1)
            pin[t & 1].array[...] = p
            b.push_audio_async(pin[t & 1], streams, frames, t & 1)
        b.sync()
        return pkts
    assert np.all(twin_of(feed_async)["frames"] == len(pkts) * frames)

    # _muted: zeros in the rings, so zeros measured
    def feed_muted(b):
        for p in pkts:
            b.push_audio_muted(p)
        return [np.zeros_like(p) for p in pkts]
    r = twin_of(feed_muted)
    assert np.all(np.isneginf(r["momentary"])) and np.all(np.isneginf(r["true_peak"]))

    # push_synth against tools/synth.py
    def feed_synth(b):
        out = []
        for t in range(len(pkts)):
            b.push_synth(synth.DEFAULT_SEED, t * frames, frames)
            out.append(synth.block(synth.DEFAULT_SEED, 0, streams, cap, t * frames, frames))
        return out
    twin_of(feed_synth)

    # push_pcm: s16 interleaved, u8 planar from host memory
    for dtype, inter in ((np.int16, True), (np.uint8, False)):
        def feed_pcm(b, dtype=dtype, inter=inter):
            from pcm_convert import captured, random_packet
            out = []
            for t in range(len(pkts)):
                pkt = random_packet(rng, dtype, streams, cap, frames, inter)
                b.push_pcm(pkt, interleaved=inter)
                out.append(captured(pkt, inter, 0, cap))
            return out
        twin_of(feed_pcm)

    # meter and waveform batches measure what a spectrum batch does
    def feed_audio(b):
        for p in pkts:
            b.push_audio(p)
        return pkts
    for kind in (dict(meter=1, bars=0), dict(waveform=1, bars=0)):
        twin_of(feed_audio, _cfg(**kind))


def test_ragged_async_matches_per_stream_pushes():
    streams, cap, max_frames = 6, 2, 1200
    rng = np.random.default_rng(9)
    with wf.SpectrumBatch(_cfg(), streams) as b, wf.SpectrumBatch(_cfg(), streams) as twin:
        b.enable_loudness()
        twin.enable_loudness()
        pin = [wf.PinnedBuffer((streams, cap, max_frames)), wf.PinnedBuffer((streams, cap, max_frames))]
        for t in range(50):
            slot = t & 1
            b.ingest_done(slot)
            frames = rng.integers(0, max_frames + 1, streams).astype(np.uint32)
            data = rng.uniform(-1, 1, (streams, cap, max_frames)).astype(np.float32)
            pin[slot].array[...] = data
            b.push_audio_ragged_async(pin[slot], frames, max_frames, slot)
            for s in range(streams):
                if frames[s]:
                    twin.push_audio(data[s:s + 1, :, :frames[s]], first=s)
        b.sync()
        got, want = b.loudness(), twin.loudness()
        for p in pin:
            p.close()
    assert _bits_equal(got, want)


def test_device_memory_paths():
    """_device and push_pcm f32 planar from device memory, in a child process (torch brings its own HIP runtime and has to
    be imported before libwaveform_hip.so is loaded)"""
    pytest.importorskip("torch")
    child = Path(__file__).resolve().parent / "loudness_device_child.py"
    r = subprocess.run([sys.executable, str(child)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "loudness device ok" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


def test_three_shards_match_one_handle():
    streams, cap = 7, 2
    rng = np.random.default_rng(4)
    pkts = _hops(rng, streams, cap, hops=40)
    devices = [i % wf.device_count() for i in range(3)]
    with wf.SpectrumBatch(_cfg(), streams) as one, wf.MultiBatch(_cfg(), streams, devices) as m:
        one.enable_loudness()
        m.enable_loudness()
        for p in pkts:
            one.push_audio(p)
            m.push_audio(p)
        m.reset_loudness(2, 3)
        one.reset_loudness(2, 3)
        for p in pkts[:10]:
            one.push_audio(p)
            m.push_audio(p)
        m.sync()
        assert _bits_equal(m.loudness(), one.loudness())


def test_nothing_else_moves():
    streams, cap = 4, 2
    rng = np.random.default_rng(8)
    pkts = _hops(rng, streams, cap, hops=30)
    for kind in (dict(normalize_volume=1), dict(meter=1, bars=0), dict(waveform=1, bars=0)):
        cfg = _cfg(**kind)
        with wf.SpectrumBatch(cfg, streams) as b, wf.SpectrumBatch(cfg, streams) as twin:
            if kind.get("normalize_volume"):
                b.enable_input_rms()
                twin.enable_input_rms()
            b.enable_loudness()
            for p in pkts:
                b.push_audio(p)
                twin.push_audio(p)
                b.tick()
                twin.tick()
            outs = ["decibels"] if not kind.get("meter") else ["meter"]
            if kind.get("normalize_volume"):
                outs += ["bars", "tsmooth", "input_rms"]
            for name in outs:
                assert _bits_equal(getattr(b, name)(), getattr(twin, name)()), (kind, name)


def test_lifecycle_and_errors():
    streams, cap = 4, 2
    rng = np.random.default_rng(6)
    pkts = _hops(rng, streams, cap, hops=20)
    with wf.SpectrumBatch(_cfg(), streams) as b:
        with pytest.raises(wf.WfHipError) as e:
            b.loudness()  # before enable
        assert e.value.code == ERR_INVALID
        assert b.L.wf_hip_output_bytes(b.h, wf.binding.OUT_LOUDNESS) == 0
        b.enable_loudness()
        assert b.L.wf_hip_output_bytes(b.h, wf.binding.OUT_LOUDNESS) == 32
        for p in pkts:
            b.push_audio(p)
        before = b.loudness()
        b.reset()  # the reference's update(): loudness is left alone
        assert _bits_equal(b.loudness(), before)
        b.reset_loudness(1, 2)
        r = b.loudness()
        assert _bits_equal(r[[0, 3]], before[[0, 3]])
        assert np.all(r["frames"][1:3] == 0) and np.all(np.isneginf(r["true_peak"][1:3])) and np.all(r["range"][1:3] == 0)
        # silence reads -inf and a range of 0
        b.reset_loudness()
        for _ in range(40):
            b.push_silence(1200)
        r = b.loudness()
        for k in ("momentary", "short_term", "integrated", "true_peak"):
            assert np.all(np.isneginf(r[k])), k
        assert np.all(r["range"] == 0) and np.all(r["frames"] == 48000)
        # a push longer than the ring is refused while the producer is on, and nothing is enqueued
        big = np.zeros((streams, cap, b.ring_frames + 1), np.float32)
        with pytest.raises(wf.WfHipError) as e:
            b.push_audio(big)
        assert e.value.code == ERR_INVALID
        with pytest.raises(wf.WfHipError) as e:
            b.push_synth(1, 0, b.ring_frames + 1)
        assert e.value.code == ERR_INVALID
        assert np.all(b.loudness()["frames"] == 48000)
    with wf.SpectrumBatch(_cfg(fs=44105), 2) as b:
        with pytest.raises(wf.WfHipError) as e:
            b.enable_loudness()
        assert e.value.code == ERR_INVALID


def test_ten_minute_stationary_run():
    fs, streams, cap = 48000, 3, 2
    one_s = np.stack([np.stack([_tone(fs, 997, 1.0, -23.0)] * 2)] * streams).astype(np.float32)
    with wf.SpectrumBatch(_cfg(), streams, ring_frames=1 << 16) as b:
        b.enable_loudness()
        for _ in range(20):
            b.push_audio(one_s)
        at20 = b.loudness()
        for _ in range(580):
            b.push_audio(one_s)
        at600 = b.loudness()
    assert np.all(at600["frames"] == 600 * fs)
    assert np.all(np.abs(at600["integrated"] - at20["integrated"]) <= 0.01), (at20["integrated"], at600["integrated"])
    assert np.all(np.abs(at600["integrated"] + 23.0) <= 0.1)
