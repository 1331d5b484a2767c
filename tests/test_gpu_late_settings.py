"""Settings that arrive after ticks have run.  The handle keeps the constant part of every kernel's arguments from create on
(wf_hip::tick) and patches the rest in per tick; what an entry point changes later -- per-stream delays, per-stream volume
compensation, the bars-only flag, the bars mirrors -- must reach the very next tick.  Twin handles get the same synthetic audio
and six ticks; one twin has the setting's storage in place from the start, the other meets it first before tick 3; rows, bars
and m_last_silent are compared bit for bit after every tick.

Shapes: N = 1024 with 3 stereo streams (two spectra per workgroup, the last workgroup's spare subgroup clamped) and N = 8192 with
2 stereo streams (split: one channel per workgroup, rotating flag and verdict words), 8 bars each."""
import numpy as np
import pytest

import waveform_amd as wf
from tools import synth
from test_gpu_reset import _Hip, same

pytestmark = pytest.mark.gpu
SEED = synth.DEFAULT_SEED
HOP, TICKS, LATE = 800, 6, 3
SHAPES = [(1024, 3), (8192, 2)]


def _cfg(n, **over):
    kw = dict(fft_size=n, stereo=1, slope=1.0, bars=1, interp_mode=1, bar_width=4, bar_gap=2, width=48)  # 48 / (4 + 2) = 8 bars
    kw.update(over)
    return wf.Config.defaults(**kw)


def _lead(n):
    """frames pushed ahead of tick 0: a whole window and the largest delay of any case, so that no tick runs short of samples"""
    return n + 2048


def _run(cfg, streams, before=None, tick_kw=None):
    """six ticks of one handle; before(batch, t) runs ahead of tick t, tick_kw(t) gives the tick's parameters.  Returns the
    outputs after every tick and leaves nothing behind."""
    n = int(cfg.fft_size)
    outs = []
    with wf.SpectrumBatch(cfg, streams, ring_frames=_lead(n) + HOP * (TICKS + 1)) as b:
        assert b.num_bars == 8, b.num_bars
        assert ("split" in b.kernel_name()) == (n == 8192), b.kernel_name()
        b.push_audio(synth.block(SEED, 0, streams, b.capture_channels, 0, _lead(n)))
        for t in range(TICKS):
            b.push_audio(synth.block(SEED, 0, streams, b.capture_channels, _lead(n) + t * HOP, HOP))
            if before:
                before(b, t)
            b.tick(**(tick_kw(t) if tick_kw else {}))
            outs.append(dict(decibels=b.decibels(), bars=b.bars(), last_silent=b.last_silent()))
    return outs


def _assert_same(a, b, ticks=range(TICKS), keys=("decibels", "bars", "last_silent"), what=""):
    for t in ticks:
        for k in keys:
            assert same(a[t][k], b[t][k]), f"{what}: {k} differs after tick {t}"


@pytest.mark.parametrize("n,streams", SHAPES)
def test_stream_delays_set_late(n, streams):
    """A has its delay words (all zero) from before tick 0, B meets wf_hip_set_stream_delay first before tick 3: the same rows
    throughout -- and the delays do arrive (the rows of tick 3 differ from an undelayed twin's)"""
    cfg = _cfg(n)
    real = np.array([0, 400, 1204], np.uint32)[:streams]

    def a_sets(b, t):
        if t == 0:
            b.set_stream_delay(np.zeros(streams, np.uint32))
        if t == LATE:
            b.set_stream_delay(real)

    def b_sets(b, t):
        if t == LATE:
            b.set_stream_delay(real)

    a, b_, plain = _run(cfg, streams, a_sets), _run(cfg, streams, b_sets), _run(cfg, streams)
    _assert_same(a, b_, what=f"N={n}: delays set late")
    _assert_same(a, plain, ticks=range(LATE), what=f"N={n}: zero delays")
    assert not same(a[LATE]["decibels"][1:], plain[LATE]["decibels"][1:]), "the delays set before tick 3 did not reach tick 3"
    assert same(a[LATE]["decibels"][0], plain[LATE]["decibels"][0])  # (stream 0: delay 0)


@pytest.mark.parametrize("n,streams", SHAPES)
def test_odd_stream_delay_leaves_the_vector_fetch(n, streams):
    """an odd delay first set before tick 3, on both twins: from that tick on the windows start off the 16-byte grid.  Without
    temporal smoothing a tick's rows depend on its window alone, so from tick 3 on they equal those of a handle that had the odd
    delays -- and so the scalar fetch -- from the start"""
    cfg = _cfg(n, tsmoothing=0)
    odd = np.array([3, 401, 7], np.uint32)[:streams]

    def a_sets(b, t):
        if t == 0:
            b.set_stream_delay(np.zeros(streams, np.uint32))
        if t == LATE:
            b.set_stream_delay(odd)

    def b_sets(b, t):
        if t == LATE:
            b.set_stream_delay(odd)

    def from_the_start(b, t):
        if t == 0:
            b.set_stream_delay(odd)

    a, b_, ref = _run(cfg, streams, a_sets), _run(cfg, streams, b_sets), _run(cfg, streams, from_the_start)
    _assert_same(a, b_, what=f"N={n}: odd delays set late")
    _assert_same(a, ref, ticks=range(LATE, TICKS), keys=("decibels", "bars"), what=f"N={n}: odd delays against the scalar fetch from the start")
    assert not same(a[LATE - 1]["decibels"], ref[LATE - 1]["decibels"])  # (before: other windows)


@pytest.mark.parametrize("n,streams", SHAPES)
def test_input_rms_set_late(n, streams):
    """normalize_volume: A sets per-stream values equal to the tick's common input_rms before tick 0 (its ticks read the per-stream
    words all along), B only ever the distinct values before tick 3 (its first ticks use the common value): one formula, the same rows"""
    cfg = _cfg(n, normalize_volume=1)
    common = 0.1
    distinct = np.array([0.05, 0.2, 0.4], np.float32)[:streams]

    def a_sets(b, t):
        if t == 0:
            b.set_input_rms(np.full(streams, common, np.float32))
        if t == LATE:
            b.set_input_rms(distinct)

    def b_sets(b, t):
        if t == LATE:
            b.set_input_rms(distinct)

    kw = lambda t: dict(input_rms=common)  # noqa: E731
    a, b_, plain = _run(cfg, streams, a_sets, kw), _run(cfg, streams, b_sets, kw), _run(cfg, streams, None, kw)
    _assert_same(a, b_, what=f"N={n}: input_rms set late")
    assert not same(a[LATE]["decibels"], plain[LATE]["decibels"]), "the values set before tick 3 did not reach tick 3"


@pytest.mark.parametrize("n,streams", SHAPES)
def test_bars_only_flag_passed_late(n, streams):
    """WF_HIP_TICK_NO_DECIBELS first at tick 3 (the stale row and the verdict words are allocated by that tick): the bars equal those
    of a twin that keeps storing its rows"""
    cfg = _cfg(n)
    a = _run(cfg, streams, None, lambda t: dict(flags=wf.TICK_NO_DECIBELS if t >= LATE else 0))
    b_ = _run(cfg, streams)
    _assert_same(a, b_, ticks=range(LATE), what=f"N={n}: before the flag")
    _assert_same(a, b_, ticks=range(LATE, TICKS), keys=("bars", "last_silent"), what=f"N={n}: bars-only ticks")


def test_bars_mirrors_set_late():
    """wf_hip_set_bars_mirrors first called after tick 2 (N = 1024: the split geometry refuses mirrors): the set handed over after
    tick 3 equals bars(), and after the hand-over and tick 4 the other set does"""
    n, streams = SHAPES[0]
    cfg = _cfg(n)
    hip = _Hip()
    with wf.SpectrumBatch(cfg, streams, ring_frames=_lead(n) + HOP * (TICKS + 1)) as b:
        shape = (streams, b.display_channels, b.num_bars)
        sets = [hip.alloc(int(np.prod(shape)) * 4) for _ in range(2)]
        consumer = hip.stream()
        try:
            seen = []
            b.push_audio(synth.block(SEED, 0, streams, b.capture_channels, 0, _lead(n)))
            for t in range(TICKS):
                b.push_audio(synth.block(SEED, 0, streams, b.capture_channels, _lead(n) + t * HOP, HOP))
                b.tick()
                if t == LATE - 1:
                    b.set_bars_mirrors([sets[0]], [sets[1]])
                if t in (LATE, LATE + 1):
                    ptr = b.bars_mirror_ready(consumer)
                    assert ptr in sets and ptr not in seen
                    seen.append(ptr)
                    assert hip.stream_sync(consumer) == 0
                    assert same(hip.download(ptr, shape), b.bars()), f"mirror set handed over after tick {t}"
        finally:
            b.sync()
            hip.stream_destroy(consumer)
            for p in sets:
                hip.free(p)


# The tick kernel's launch keys with mirrors, family by family (waveform_amd/csrc/wf_tick_geom.hip: Pow2Family's table is indexed by
# aligned / mirrors / display kind).  name: what kernel_name() must say, so that a case cannot drift to another family.
MIRROR_CASES = {
    "512_bars": (512, dict(), "tables via LDS"),                                    # two spectra per workgroup, prefix-sum bars
    "512_curve": (512, dict(bars=0, curve=1, interp_mode=2), "tables via LDS"),     # ... the general display code
    "256_bars": (256, dict(), "zero-padded"),                                       # one instantiation with mirrors, scalar fetch
    "1024_monomix_curve": (1024, dict(stereo=0, bars=0, curve=1, interp_mode=2), "curve row shared by both spectra"),
    "8192_split_bars": (8192, dict(), ",split"),                                    # serves the mirrors in its only instantiation
    "8192_one_channel_bars": (8192, dict(capture_channels=1), "SPW=1>"),
}


def _run_mirrored(cfg, name, mirrors, odd):
    """four ticks of a two-stream handle, with the mirror sets in place from before tick 0 or without; odd: 3 frames pushed first, so
    that every window starts off the 16-byte grid.  Returns the outputs after every tick, the set handed over among them."""
    n, streams, ticks = int(cfg.fft_size), 2, 4
    hip, outs, last = _Hip(), [], None
    with wf.SpectrumBatch(cfg, streams, ring_frames=_lead(n) + HOP * (ticks + 1) + 4) as b:
        assert name in b.kernel_name() and b.num_bars > 0, (b.kernel_name(), b.num_bars)
        shape = (streams, b.display_channels, b.num_bars)
        sets = [hip.alloc(int(np.prod(shape)) * 4) for _ in range(2)] if mirrors else []
        consumer = hip.stream()
        try:
            if mirrors:
                b.set_bars_mirrors([sets[0]], [sets[1]])
            if odd:
                b.push_audio(synth.block(SEED, 0, streams, b.capture_channels, 0, odd))
            b.push_audio(synth.block(SEED, 0, streams, b.capture_channels, odd, _lead(n)))
            for t in range(ticks):
                b.push_audio(synth.block(SEED, 0, streams, b.capture_channels, odd + _lead(n) + t * HOP, HOP))
                b.tick()
                o = dict(decibels=b.decibels(), bars=b.bars(), last_silent=b.last_silent())
                if mirrors:
                    ptr = b.bars_mirror_ready(consumer)
                    assert ptr in sets and ptr != last, f"tick {t}: the set handed over"
                    last = ptr
                    assert hip.stream_sync(consumer) == 0
                    o["handed_over"] = hip.download(ptr, shape)
                outs.append(o)
        finally:
            b.sync()
            hip.stream_destroy(consumer)
            for p in sets:
                hip.free(p)
    return outs


@pytest.mark.parametrize("odd", [0, 3], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("case", MIRROR_CASES)
def test_bars_mirrors_on_every_family(case, odd):
    """twins, one with mirror sets and one without: rows, bars and m_last_silent equal bit for bit after every tick (the
    instantiation that also stores into the mirrors computes what the plain one does), and every set handed over equals bars()"""
    n, over, name = MIRROR_CASES[case]
    cfg = _cfg(n, **over)
    with_m, plain = _run_mirrored(cfg, name, True, odd), _run_mirrored(cfg, name, False, odd)
    _assert_same(with_m, plain, ticks=range(4), what=f"{case}: mirrors against none")
    for t, o in enumerate(with_m):
        assert same(o["handed_over"], o["bars"]), f"{case}: mirror set handed over after tick {t}"
    assert not same(with_m[0]["bars"], with_m[3]["bars"])  # (the ticks did something)
