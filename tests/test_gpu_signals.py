"""The spectrum tick on lone samples, sample pairs, tones and non-finite audio (tests/signals.py), one fft size per kernel family
of wf_tick_plan.hpp, through the C ABI on wf.SpectrumBatch.  Every other parity module feeds noise or digital silence, under which
every thread of a silence scan holds a non-zero sample and every bin sits near the frame's peak.

  a. lone-sample sweep   a window that is zero but for ONE sample, at every position class: the stream is not silent (a thread,
                         row, wavefront or workgroup whose share dropped out of the OR would say it is) and its row is the flat
                         row of the closed form (a sample fetched from the wrong place lands on another window weight)
  b. zero classes        -0.0f is zero; a denormal, a NaN and an infinity are not
  c. two-sample rows     |a + b e^{-2 pi i k (q - p) / N}| 2 / N, no window: every bin sharp, the transform's indexing pinned
  d. tones               rows no farther from the double DFT than 8 x the reference's own float FFT is
                         (signals.assert_no_worse_than_reference; the measured ratios: profiles/tick_signals_accuracy.txt)
  e. isolation           a NaN or an infinity in one stream changes no bit of any other stream of the batch

Nothing here goes through the linear arm of assert_db_close, so the counts test_zz_display_arm_stays_rare bounds are unchanged.
"""
import numpy as np
import pytest

import scenarios
import signals
import test_gpu_fuzz as fuzz
from helpers import LIN_EPS, assert_db_close
from oracle import restate, wfref
from test_tick_plan_cpu import plans  # noqa: F401  (the library's own planner compiled into a program: a module-scoped fixture)
from tools import synth

pytestmark = pytest.mark.gpu

# one size per production family: the smallest legal size of each, both DEC values of the zero-padded sizes, and for the
# power-of-two kernel the smallest, 1024, the headline size, the first split geometry and the largest
FAMILY = {128: "ZERO_PADDED", 256: "ZERO_PADDED", 144: "MIXED_RADIX", 720: "FIXED_PLAN", 1616: "BLUESTEIN", 16416: "MR_TWO_ROWS",
          18032: "MR_ROWS", 16400: "BLUESTEIN_ROWS", 65536: "WHOLE_65536", 512: "POW2", 1024: "POW2", 4096: "POW2", 8192: "POW2",
          32768: "POW2"}
SIZES = sorted(FAMILY)
HANN, BLACKMAN_HARRIS = 1, 4
K = 8  # one binary order of magnitude over the reference's own error against the double DFT; not measured, not to be widened
# Families whose worst frame exceeds K (profiles/tick_signals_accuracy.txt) are held to LIN_EPS of the frame's peak instead, the
# existing linear arm, uncounted ("Tones").  The cause is the same in all three and is not the transform's
# twiddles: DC and a sine on a bin are signals on which the reference's FFTW lands on the double DFT to the bit at the peak bins,
# so E_ref collapses to 1e-8 of the peak -- under one float32 ulp of the peak magnitude -- while the device's window, transform,
# scale, smoothing and hardware log2 leave the one or two peak bins 2 to 3 ulps of their float32 dB value away (4e-8 to 6e-8 of
# a 0.18 peak).  Every other bin of those frames is inside K.  A library built with WF_TW1_POW2=0 (every pass-1 twiddle row loaded
# from its table) misses the same cases by the same figures; one built with WF_FAST_DB=0 (log10f) misses eleven, in other families too.
# (Both build switches are retired since; commit 0c206e5 is the last that has them.)
LIN_EPS_FAMILIES = {"ZERO_PADDED": 23.58, "POW2": 22.74, "MR_TWO_ROWS": 17.42}  # family -> its worst measured ratio (needed k: 11.8, 11.4, 11.6)


def _check_family(plans, n):  # noqa: F811
    """a plan change must not silently move a size to another kernel"""
    for lay in ("one", "stereo", "monomix"):
        assert plans["T"][(n, lay)]["family"] == FAMILY[n], (n, lay, plans["T"][(n, lay)]["family"])


def test_sizes_are_the_smallest_of_their_families(plans):  # noqa: F811
    fam = {}
    for (n, lay), rec in plans["T"].items():
        fam.setdefault(rec["family"], []).append(n)
    smallest = {f: min(v) for f, v in fam.items()}
    assert smallest == {"ZERO_PADDED": 128, "MIXED_RADIX": 144, "FIXED_PLAN": 720, "BLUESTEIN": 1616, "MR_TWO_ROWS": 16416,
                        "MR_ROWS": 18032, "BLUESTEIN_ROWS": 16400, "WHOLE_65536": 65536, "POW2": 512}
    assert sorted(fam["ZERO_PADDED"]) == [128] * 3 + [256] * 3
    for n in SIZES:
        _check_family(plans, n)


def _mono_cfg(n, window, **kw):
    return scenarios.make_config(dict(fft_size=n, capture_channels=1, stereo=0, tsmoothing=0, slope=0.0, window=window, **kw))


def _window(cfg):
    o = restate.OracleSource(cfg)
    try:
        return o.window()
    finally:
        o.close()


def sweep_positions(n):
    """every position for N <= 1024; above that the edges of every unit a kernel could divide a window into, and 128 drawn"""
    if n <= 1024:
        return list(range(n))
    pos = set(range(9)) | {63, 64, 65, 255, 256, 257} | {n // 4 - 1, n // 4, n // 4 + 1, n // 2 - 1, n // 2, n // 2 + 1} | set(range(n - 4, n))
    for m in range(1, 64):
        pos |= {m * (n // 64), m * (n // 64) - 1}
    pos |= set(map(int, np.random.default_rng(3000 + n).integers(0, n, 128)))
    return sorted(pos)


class _Pusher:
    """a batch plus the number of frames pushed so far (the ring's write position)"""

    def __init__(self, cfg, streams):
        import waveform_amd as wf
        self.b = wf.SpectrumBatch(cfg, streams)
        self.pos = 0

    def zeros(self, frames):
        if frames:
            self.b.push_silence(frames)
            self.pos += frames

    def window(self, audio):
        self.b.push_audio(audio)
        self.pos += audio.shape[2]

    def straddle(self, n):
        """zeros until the next window of n frames lies across the ring's wrap, starting at an odd position"""
        ring = self.b.ring_frames
        self.zeros((ring - n // 2 + 1 - self.pos) % ring)
        assert self.pos % ring + n > ring and self.pos % 4 == 1, (self.pos, ring, n)


# ---- a. the lone-sample sweep -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_lone_sample_sweep(n, plans):  # noqa: F811
    _check_family(plans, n)
    cfg = _mono_cfg(n, HANN)
    w, wsum = _window(cfg)
    pos = sweep_positions(n)
    audio = np.zeros((len(pos), 1, n), np.float32)
    audio[np.arange(len(pos)), 0, pos] = 0.5
    live = np.array([w[p] != 0.0 for p in pos])
    assert (~live).sum() >= 1 and pos[0] == 0 and w[0] == 0.0  # the stream whose only sample the window zeroes: DB_MIN, not silent
    level = np.array([signals.lone_sample_row(0.5, p, w, wsum, 1, db_min=restate.db_min())[0] for p in pos])
    want = np.repeat(level[:, None], n // 2, axis=1)
    pb = _Pusher(cfg, len(pos))
    try:
        for variant in ("aligned", 1, 2, 3, "wrap"):
            if variant == "wrap":
                pb.straddle(n)
            elif variant != "aligned":
                pb.zeros(variant)  # the window start is no multiple of 4 frames: the fetch that is not ALIGNED
                assert pb.pos % 4 != 0
            pb.window(audio)
            pb.b.tick()
            what = f"{FAMILY[n]} N={n} lone sample, {variant}"
            silent = pb.b.last_silent()
            assert not silent.any(), f"{what}: silent with one sample at window positions {[pos[i] for i in np.flatnonzero(silent)][:20]}"
            got = pb.b.decibels()[:, 0]
            assert_db_close(got[live], want[live], what, lin_eps=None)
            assert_db_close(got[~live], want[~live], what + " (w[p] = 0)", lin_eps=None, deep=True)
    finally:
        pb.b.close()


LAYOUTS = {"stereo": dict(capture_channels=2, stereo=1), "monomix": dict(capture_channels=2, stereo=0), "dup": dict(capture_channels=1, stereo=1)}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", [512, 144, 16400, 65536])  # (the last two: the partner-channel reads of the kernels beyond a CU's LDS)
def test_lone_sample_two_channel_layouts(n, layout, plans):  # noqa: F811
    """the sample in channel 0 only and in channel 1 only: plan_stream and the partner-channel reads.  Expected: the restatement
    playing that stream alone"""
    import waveform_amd as wf
    _check_family(plans, n)
    lay = LAYOUTS[layout]
    cfg = scenarios.make_config(dict(fft_size=n, tsmoothing=0, slope=0.0, window=HANN, **lay))
    cap = lay["capture_channels"]
    pos = sorted({0, 1, 2, 3, 63, 64, 65, n // 2 - 1, n // 2, n - 2, n - 1, *map(int, np.random.default_rng(n).integers(0, n, 16))})
    cases = [(p, c) for p in pos for c in range(cap)]
    audio = np.zeros((len(cases), cap, n), np.float32)
    for s, (p, c) in enumerate(cases):
        audio[s, c, p] = 0.5
    for pre in (0, 3):
        want_db, want_silent = [], []
        for s in range(len(cases)):
            o = restate.OracleSource(cfg)
            if pre:
                o.push_audio(np.zeros((cap, pre), np.float32))
            o.push_audio(audio[s])
            o.tick()
            want_db.append(o.decibels())
            want_silent.append(o.last_silent)
            o.close()
        with wf.SpectrumBatch(cfg, len(cases)) as b:
            if pre:
                b.push_silence(pre)
            b.push_audio(audio)
            b.tick()
            got, silent = b.decibels(), b.last_silent()
        assert not any(want_silent) and not silent.any(), f"N={n} {layout} pre {pre}: silent {[cases[i] for i in np.flatnonzero(silent)]}"
        assert_db_close(got[:, : b.display_channels], np.stack(want_db), f"{FAMILY[n]} N={n} {layout}, {pre} frames first", lin_eps=None, deep=True)


# ---- b. zero classes ----------------------------------------------------------------------------------------------------------
CLASSES = [("-0.0", -0.0, True), ("denormal 1e-40", 1e-40, False), ("NaN", float("nan"), False), ("+Inf", float("inf"), False),
           ("-Inf", float("-inf"), False)]


@pytest.mark.parametrize("n", SIZES)
def test_zero_classes(n, plans):  # noqa: F811
    """x == 0.0f is the reference's test (src/source_generic.cpp:63-72): -0.0f is zero, NaNs and infinities are not, and neither is
    a denormal.  Nothing is asserted about the rows of the NaN and Inf streams"""
    import waveform_amd as wf
    _check_family(plans, n)
    cfg = _mono_cfg(n, HANN)
    pos = [1, n - 1] + list(map(int, np.random.default_rng(5000 + n).integers(0, n, 6)))
    cases = [("+0.0", None, 0.0, True)] + [(name, p, v, s) for p in pos for name, v, s in CLASSES]
    audio = np.zeros((len(cases), 1, n), np.float32)
    for i, (_, p, v, _) in enumerate(cases):
        if p is not None:
            audio[i, 0, p] = v
    assert np.float32(1e-40) != 0.0 and np.signbit(audio[1, 0, pos[0]])
    o = restate.OracleSource(cfg)
    o.push_audio(audio[0])
    o.tick()
    zero_row, zero_silent = o.decibels(), o.last_silent
    o.close()
    with wf.SpectrumBatch(cfg, len(cases)) as b:
        b.push_audio(audio)
        b.tick()
        got, silent = b.decibels()[:, :1], b.last_silent()
    assert zero_silent and bool(silent[0]), "a window of +0.0f reads silent at the first tick"
    assert np.array_equal(got[0], zero_row)
    for i, (name, p, _, want) in enumerate(cases):
        assert bool(silent[i]) == want, f"{FAMILY[n]} N={n}: a lone {name} at window position {p} reads silent = {bool(silent[i])}"
        if want:
            assert np.array_equal(got[i].view(np.uint32), got[0].view(np.uint32)), f"N={n}: the row of {name} at {p} is not the all-zero stream's"


# ---- c. two-sample rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_two_sample_rows(n, plans):  # noqa: F811
    """0.5 and 0.125 at 16 drawn position pairs, and swapped: the magnitude stays within 0.375 .. 0.625 of 2 / N, so no bin is a null
    and the dB arm alone judges every bin"""
    import waveform_amd as wf
    _check_family(plans, n)
    cfg = _mono_cfg(n, 0)
    r = np.random.default_rng(7000 + n)
    pairs = [tuple(map(int, r.choice(n, 2, replace=False))) for _ in range(16)]
    cases = [c for p, q in pairs for c in ((p, q), (q, p))]
    audio = np.zeros((len(cases), 1, n), np.float32)
    for s, (p, q) in enumerate(cases):
        audio[s, 0, p], audio[s, 0, q] = 0.5, 0.125
    want = np.stack([signals.two_sample_row(0.5, p, 0.125, q, n) for p, q in cases])
    with wf.SpectrumBatch(cfg, len(cases)) as b:
        b.push_audio(audio)
        b.tick()
        got, silent = b.decibels()[:, 0], b.last_silent()
    assert not silent.any()
    assert_db_close(got, want, f"{FAMILY[n]} N={n} two samples", lin_eps=None)


# ---- d. tones -----------------------------------------------------------------------------------------------------------------
def tone_specs(n):
    return {
        "sine on a bin": signals.sine(n, max(n // 32 + 5, 9), 0.5),
        "sine between bins": signals.sine(n, n / 41.0 + 0.5 - (n / 41.0) % 1.0, 10.0 ** (-6.0 / 20.0), 0.3),
        "DC 0.25": signals.dc(0.25),
        "square": signals.square(n, n / 100.0, 0.5),  # a period of 100 frames at every size
        "two_tone": signals.two_tone(n),
    }


TICKS = 3  # (the restatement's O(n p) DFT takes under 10 ms per stereo tick at every size here: no case needs fewer ticks)


def _tone_case(n, window, name, spec, smoothing, bars, ticks):
    """one batch of 2 stereo streams (the second hears the signal 1000 frames later, its right channel 77 more), hop 800; returns
    the worst ratio of signals.assert_no_worse_than_reference over ticks, streams and channels, the smallest k that would have passed
    them all (signals.needed_k) and the worst E_ref / peak"""
    import waveform_amd as wf
    cfg_dict = dict(fft_size=n, stereo=1, window=window, **({"tsmoothing": 0} if smoothing == "none" else {"tsmoothing": 1, "gravity": 0.8}))
    if bars:
        cfg_dict.update(bars=1, interp_mode=1, log_scale=1)
    cfg = scenarios.make_config(cfg_dict)
    feeds = [scenarios._Feeder(2) for _ in range(2)]
    chans = [(dict(spec, offset=1000 * s), dict(spec, offset=1000 * s + 77)) for s in range(2)]
    oras = [scenarios.OracleBackend(cfg) for _ in range(2)]
    refs = [scenarios.RefBackend(cfg) for _ in range(2)]
    worst = k_worst = e_worst = 0.0
    what = f"{FAMILY[n]} N={n} {name}, window {window}, smoothing {smoothing}{', bars' if bars else ''}"
    with wf.SpectrumBatch(cfg, 2) as b:
        if bars:
            assert b.num_bars == 26
        for t in range(ticks):
            audio = np.stack([f.block("signal", n if t == 0 else 800, ch) for f, ch in zip(feeds, chans)])
            b.push_audio(audio)
            b.tick()
            got, silent = b.decibels(), b.last_silent()
            gbars = b.bars() if bars else None
            for s in range(2):
                for be in (oras[s], refs[s]):
                    be.push(audio[s], muted=False)
                    be.tick(1.0 / 60.0)
                truth, ref = oras[s].observe(), refs[s].observe()
                assert bool(silent[s]) == truth["silent"] == ref["silent"], f"{what} tick {t} stream {s}: m_last_silent"
                fallback = FAMILY[n] in LIN_EPS_FAMILIES
                ratio = signals.assert_no_worse_than_reference(got[s, :2], ref["db"], truth["db"], None if fallback else K, f"{what} tick {t} stream {s}")
                if fallback:
                    signals.assert_within_peak(got[s, :2], truth["db"], LIN_EPS, f"{what} tick {t} stream {s}")
                worst = max(worst, ratio)
                k_worst = max(k_worst, signals.needed_k(got[s, :2], ref["db"], truth["db"]))
                peak = signals._linear(truth["db"], 0.0).max(axis=-1, keepdims=True)
                e_worst = max(e_worst, float((signals.reference_error(ref["db"], truth["db"]) / peak).max()))
                if bars:
                    g = dict(db=got[s, :2], bars=gbars[s], silent=bool(silent[s]))
                    fuzz._compare_display(g, truth, f"{what} stream {s} vs the restatement", t, cfg=cfg)
                    fuzz._compare_display(g, ref, f"{what} stream {s} vs libwfref", t, cfg=cfg)
    return worst, k_worst, e_worst


@pytest.mark.parametrize("window", [HANN, BLACKMAN_HARRIS])
@pytest.mark.parametrize("n", SIZES)
def test_tones_no_worse_than_reference(n, window, plans):  # noqa: F811
    if not wfref.available():
        pytest.skip("oracle/_ref/libwfref.so not built")
    _check_family(plans, n)
    for name, spec in tone_specs(n).items():
        for smoothing in ("none", "ema"):
            ratio, k, e_ref = _tone_case(n, window, name, spec, smoothing, False, TICKS)
            print(f"RATIO {FAMILY[n]:<14} N={n:<5} window={window} {name:<17} {smoothing:<4} max|got-truth|/E_ref = {ratio:5.2f}   needed k = {k:5.2f}   E_ref/peak = {e_ref:.1e}")
    if window == HANN:  # one bars configuration per size: 26 Lanczos bars on the log axis, by the display criterion of the fuzz
        ratio, k, e_ref = _tone_case(n, window, "sine between bins", tone_specs(n)["sine between bins"], "ema", True, TICKS)
        print(f"RATIO {FAMILY[n]:<14} N={n:<5} window={window} {'sine between bins':<17} ema+bars max|got-truth|/E_ref = {ratio:5.2f}   needed k = {k:5.2f}   E_ref/peak = {e_ref:.1e}")


# ---- e. isolation -------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run_noise_batch(cfg, n, ticks, poison):
    """8 stereo streams of noise: a fill of n + 400 frames, then 800 per tick.  poison: {(packet, stream, channel, offset): value}.
    Returns per tick (rows, bars, silent)"""
    import waveform_amd as wf
    out, at = [], 0
    with wf.SpectrumBatch(cfg, 8) as b:
        for t in range(ticks):
            frames = n + 400 if t == 0 else 800
            audio = synth.block(scenarios.SEED, 0, 8, 2, at, frames)
            at += frames
            for (packet, s, c, off), v in poison.items():
                if packet == t:
                    audio[s, c, off] = v
            b.push_audio(audio)
            b.tick()
            out.append((b.decibels(), b.bars(), b.last_silent()))
    return out


@pytest.mark.parametrize("n", [4096, 1616])
def test_non_finite_audio_stays_in_its_stream(n, plans):  # noqa: F811
    _check_family(plans, n)
    others = [s for s in range(8) if s not in (2, 5)]
    # EMA with fast peaks, bars on: the NaN of stream 2 and the +Inf of stream 5 (one packet) stay in their smoothing state; every
    # other stream is byte-identical to the clean batch, tick by tick
    cfg = scenarios.make_config(dict(fft_size=n, stereo=1, tsmoothing=1, fast_peaks=1, bars=1, interp_mode=1))
    clean = _run_noise_batch(cfg, n, 6, {})
    dirty = _run_noise_batch(cfg, n, 6, {(2, 2, 0, 100): np.nan, (2, 5, 1, 200): np.inf})
    for t, (c, d) in enumerate(zip(clean, dirty)):
        for name, x, y in zip(("rows", "bars", "m_last_silent"), c, d):
            assert np.array_equal(_bits(x[others]) if x.dtype == np.float32 else x[others], _bits(y[others]) if y.dtype == np.float32 else y[others]), \
                f"N={n} tick {t}: {name} of a clean stream changed"
    assert not np.array_equal(_bits(clean[2][0][2]), _bits(dirty[2][0][2])), "the NaN never reached stream 2"
    # no smoothing: the sample sits at frame 500 of the fill, inside the first window (frames 400 ...) and outside every later one
    cfg = scenarios.make_config(dict(fft_size=n, stereo=1, tsmoothing=0, bars=1, interp_mode=1))
    clean = _run_noise_batch(cfg, n, 4, {})
    dirty = _run_noise_batch(cfg, n, 4, {(0, 2, 0, 500): np.nan, (0, 5, 1, 500): np.inf})
    for t, (c, d) in enumerate(zip(clean, dirty)):
        which = others if t == 0 else list(range(8))
        for name, x, y in zip(("rows", "bars", "m_last_silent"), c, d):
            assert np.array_equal(_bits(x[which]) if x.dtype == np.float32 else x[which], _bits(y[which]) if y.dtype == np.float32 else y[which]), \
                f"N={n} tick {t}, no smoothing: {name} differ from the clean batch"
    assert not np.array_equal(_bits(clean[0][0][2]), _bits(dirty[0][0][2])), "the NaN never reached stream 2"
