"""tests/signals.py without a device: the generators, the closed forms against the restatement, the restatement against the
reference on every signal class, the proof that the accuracy criterion of the tone tests has teeth, and the silence semantics
(what counts as a zero sample) on the restatement and the reference.  tests/test_gpu_signals.py holds the device to the same.

E_ref: the largest |reference - restatement| of a frame in linear magnitude, relative to the frame's peak -- the error of the
reference's float FFTW against the DFT in double, the yardstick of signals.assert_no_worse_than_reference.  Measured by
test_restatement_matches_reference_on_signals (stereo, EMA, 3 ticks of 800 frames, worst frame; printed by the test):

  N      window           sine on a bin  sine between  DC 0.25   square    two_tone
  1024   Hann             1.1e-07        2.2e-07       2.2e-07   2.2e-07   2.2e-07
  1024   Blackman-Harris  4.3e-08        3.3e-07       1.8e-08   2.2e-07   2.2e-07
  4096   Hann             2.2e-07        4.4e-08       2.2e-07   1.6e-07   3.3e-07
  4096   Blackman-Harris  2.2e-07        3.3e-07       2.2e-07   9.1e-08   2.2e-07
  2096   Hann             2.2e-07        3.3e-07       2.8e-08   1.6e-07   2.7e-07
  2096   Blackman-Harris  1.5e-07        2.2e-07       1.5e-07   2.7e-07   2.2e-07

The recurring 2.2e-07 is one float32 ulp of a dB value between -16 and -32 (1.9e-6 dB): at the peak the rows' own number format
is most of E_ref, which is why the criterion grants every bin its own half ulp on top.  All of them sit under LIN_EPS = 1e-6 (the
linear arm of assert_db_close) by a factor of 3 to 50: that arm would pass a transform that much less accurate than the
reference, which is why the tone tests do not use it.
"""
import numpy as np
import pytest

import scenarios
import signals
import test_gpu_fuzz as fuzz
from helpers import LIN_EPS, assert_db_close
from oracle import restate, wfref

HANN, BLACKMAN_HARRIS = 1, 4
CHUNKS = (37, 441, 800, 1024, 3, 1600, 1, 1094)


def _specs(n):
    return {
        "sine_on_bin": signals.sine(n, 37 if n >= 256 else 9, 0.5),
        "sine_between": signals.sine(n, (100.5 if n >= 512 else 20.5), 10.0 ** (-6.0 / 20.0), 0.3),
        "dc": signals.dc(0.25),
        "square": signals.square(n, 10.25 if n >= 256 else 5.25, 0.5),
        "two_tone": signals.two_tone(n),
    }


# ---- generators ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sine_on_bin", "sine_between", "dc", "square", "two_tone", "impulses"])
def test_packets_of_any_size_join_up(name):
    n = 800
    spec = signals.impulses([(0, 0.5), (36, -1.0), (37, 0.25), (4999, 1e-40)]) if name == "impulses" else _specs(n)[name]
    whole = signals.render(spec, 0, sum(CHUNKS))
    assert whole.dtype == np.float32 and whole.shape == (sum(CHUNKS),)
    at, parts = 0, []
    for c in CHUNKS:
        parts.append(signals.render(spec, at, c))
        at += c
    assert np.array_equal(np.concatenate(parts).view(np.uint32), whole.view(np.uint32))
    # the same through the feeder of the scenario scripts, on two channels with a spec each
    f = scenarios._Feeder(2)
    blocks = [f.block("signal", c, (spec, None)) for c in CHUNKS]
    joined = np.concatenate(blocks, axis=1)
    assert np.array_equal(joined[0].view(np.uint32), whole.view(np.uint32)) and not joined[1].any()
    shifted = dict(spec, offset=123)
    assert np.array_equal(signals.render(shifted, 0, 500).view(np.uint32), whole[123:623].view(np.uint32))


def test_generators_exact_values_at_the_edges():
    n = 1024
    s = signals.render(signals.sine(n, 256, 0.5), 0, 2 * n + 1)  # a quarter of the sample rate: 0, amp, 0, -amp
    assert s[0] == 0.0 and s[1] == np.float32(0.5) and s[3] == np.float32(-0.5) and s[n] == 0.0 and s[2 * n] == 0.0
    assert np.array_equal(s[:n], s[n:2 * n])  # a whole number of bins: periodic in n to the bit
    far = signals.render(signals.sine(n, 256, 0.5), (1 << 40) + 1, 1)  # reduced modulo n before the sine: exact however far
    assert far[0] == np.float32(0.5)
    d = signals.render(signals.dc(0.25), 7, 5)
    assert (d == np.float32(0.25)).all()
    q = signals.render(signals.square(n, 1, 0.5), 0, 2 * n)
    assert q[0] == 0.5 and q[n // 2 - 1] == 0.5 and q[n // 2] == -0.5 and q[n - 1] == -0.5 and q[n] == 0.5
    assert set(np.unique(q)) == {np.float32(-0.5), np.float32(0.5)}
    t = signals.render(signals.two_tone(n), 0, n).astype(np.float64)
    assert t[0] == 0.0 and 0.49 < np.abs(t).max() <= 0.5001
    i = signals.render(signals.impulses([(5, 0.5), (9, float("nan")), (10, -0.0), (11, 1e-40), (12, float("-inf"))]), 4, 10)
    assert i[1] == 0.5 and np.isnan(i[5]) and np.signbit(i[6]) and i[6] == 0.0 and 0.0 < i[7] < 1.2e-38 and i[8] == -np.inf
    assert np.count_nonzero(i.view(np.uint32)) == 5
    assert not signals.render(signals.impulses([(3, 1.0), (14, 1.0)]), 4, 10).any()  # both outside [4, 14)
    assert not signals.render(None, 0, 16).any()


def test_existing_step_kinds_are_untouched():
    """the feeder's noise is still the counter hash, and a signal step advances the same position counter"""
    from tools import synth
    f = scenarios._Feeder(2, stream=3)
    a = f.block("noise", 441)
    f.block("signal", 100, signals.dc(0.5))
    b = f.block("noise_amp", 37, 0.25)
    assert np.array_equal(a, synth.block(scenarios.SEED, 3, 1, 2, 0, 441)[0])
    assert np.array_equal(b, synth.block(scenarios.SEED, 3, 1, 2, 541, 37)[0] * np.float32(0.25))


# ---- the closed forms against the restatement ---------------------------------------------------------------------------------
def _mono(n, window, slope, **kw):
    return scenarios.make_config(dict(fft_size=n, capture_channels=1, stereo=0, tsmoothing=0, window=window, slope=slope, **kw))


def _tick_window(cfg, samples):
    """one window of `samples` [n] through a fresh restated source: (row, last_silent, window, window sum, slope table)"""
    o = restate.OracleSource(cfg)
    try:
        o.push_audio(np.asarray(samples, np.float32)[None])
        o.tick()
        w, wsum = o.window()
        return o.decibels(0), o.last_silent, w, wsum, (o.slope() if cfg.slope > 0 else None)
    finally:
        o.close()


@pytest.mark.parametrize("slope", [0.0, 1.0])
@pytest.mark.parametrize("window", [HANN, 0])
@pytest.mark.parametrize("n", [128, 512, 800, 2096])  # 2096 = 16 * 131: a prime factor above 127
def test_lone_sample_rows_are_flat(n, window, slope):
    cfg = _mono(n, window, slope)
    r = np.random.default_rng(n + 7 * window)
    for p in sorted({0, 1, 2, n // 2 - 1, n // 2, n - 2, n - 1, *map(int, r.integers(0, n, 6))}):
        for a in (0.5, -0.25):
            x = np.zeros(n, np.float32)
            x[p] = a
            row, silent, w, wsum, sl = _tick_window(cfg, x)
            assert not silent, f"N={n} window {window} p={p}: a window with one sample is not silent"
            want = signals.lone_sample_row(a, p, w, wsum, n // 2, slope=sl, db_min=restate.db_min())
            if window == HANN and p == 0:  # w[0] = 0: the window zeroes the only sample -- the row reads DB_MIN, the stream is live
                assert w[0] == 0.0 and (row == np.float32(restate.db_min())).all()
            assert_db_close(row, want, f"N={n} window {window} slope {slope} p={p} a={a}", lin_eps=None)
            if slope == 0.0:
                assert np.ptp(row.astype(np.float64)) <= 2e-4, f"N={n} p={p}: the row of one sample is flat"


@pytest.mark.parametrize("slope", [0.0, 1.0])
@pytest.mark.parametrize("n", [128, 512, 800, 2096])
def test_two_sample_rows(n, slope):
    cfg = _mono(n, 0, slope)
    r = np.random.default_rng(100 + n)
    pairs = [(0, 1), (0, n - 1), (n // 2, n // 2 + 1)] + [tuple(map(int, r.choice(n, 2, replace=False))) for _ in range(5)]
    for p, q in pairs:
        for a, b in ((0.5, 0.125), (0.125, 0.5), (0.5, -0.125)):
            x = np.zeros(n, np.float32)
            x[p], x[q] = a, b
            row, silent, w, wsum, sl = _tick_window(cfg, x)
            assert not silent and w is None and wsum == n
            assert_db_close(row, signals.two_sample_row(a, p, b, q, n, slope=sl), f"N={n} slope {slope} ({a} at {p}, {b} at {q})", lin_eps=None)


# ---- the restatement against the reference on every signal class ---------------------------------------------------------------
needs_ref = pytest.mark.skipif(not wfref.available(), reason="oracle/_ref/libwfref.so not built")


def _script(n, spec, ticks=3, hop=800):
    steps = [("signal", n, spec), ("tick",)]
    for _ in range(ticks - 1):
        steps += [("signal", hop, spec), ("tick",)]
    return steps


@needs_ref
@pytest.mark.parametrize("window", [HANN, BLACKMAN_HARRIS])
@pytest.mark.parametrize("n", [1024, 4096, 2096])
def test_restatement_matches_reference_on_signals(n, window):
    """tones: the silent flag, E_ref (under LIN_EPS, the project's existing arm -- and far under it, see the table above), bars by
    the existing display criterion; lone and paired samples: rows by the dB arm alone"""
    cfg_dict = dict(fft_size=n, stereo=1, window=window, bars=1, interp_mode=1)
    cfg = scenarios.make_config(cfg_dict)
    for name, spec in _specs(n).items():
        sc = dict(cfg=cfg_dict, steps=_script(n, (spec, dict(spec, offset=1000))), record="all")
        got = scenarios.play(scenarios.OracleBackend(cfg), sc)
        want = scenarios.play(scenarios.RefBackend(cfg), sc)
        worst = 0.0
        for t, (g, w) in enumerate(zip(got, want)):
            what = f"N={n} window {window} {name}"
            assert g["silent"] == w["silent"] is False, f"{what} tick {t}: m_last_silent"
            peak = signals._linear(g["db"], 0.0).max(axis=-1, keepdims=True)
            e = signals.reference_error(w["db"], g["db"]) / peak
            worst = max(worst, float(e.max()))
            assert (e <= LIN_EPS).all(), f"{what} tick {t}: the reference is {e.max():.2e} of the peak from the double DFT"
            assert signals.assert_no_worse_than_reference(w["db"], w["db"], g["db"], 1, what) <= 1.0  # (the reference against itself)
            fuzz._compare_display(g, w, what + ": restatement vs libwfref", t, cfg=cfg)
        print(f"E_ref / peak  N={n} window={window} {name}: {worst:.1e}")
    mono = dict(fft_size=n, capture_channels=1, stereo=0, tsmoothing=0, window=window)
    for points in ([(n // 3, 0.5)], [(0, 0.5)], [(5, 0.5), (n - 7, 0.125)]):
        sc = dict(cfg=mono, steps=[("signal", n, signals.impulses(points)), ("tick",)], record="all")
        c = scenarios.make_config(mono)
        g, w = scenarios.play(scenarios.OracleBackend(c), sc)[0], scenarios.play(scenarios.RefBackend(c), sc)[0]
        assert g["silent"] == w["silent"] is False
        assert_db_close(g["db"], w["db"], f"N={n} window {window} samples {points}", lin_eps=None)


# ---- the criterion has teeth --------------------------------------------------------------------------------------------------
@needs_ref
def test_criterion_fails_what_the_linear_arm_passes():
    """a Hann-windowed sine at N = 4096 with an error of 1e-6 of the peak spread over the bins: inside the linear arm of
    assert_db_close, far outside 8 x the reference's own distance from the double DFT"""
    import helpers
    n = 4096
    cfg_dict = dict(fft_size=n, capture_channels=1, stereo=0, tsmoothing=0, window=HANN)
    cfg = scenarios.make_config(cfg_dict)
    sc = dict(cfg=cfg_dict, steps=_script(n, signals.sine(n, 100.5, 0.5, 0.3), ticks=1), record="all")
    truth = scenarios.play(scenarios.OracleBackend(cfg), sc)[0]["db"][0]
    ref = scenarios.play(scenarios.RefBackend(cfg), sc)[0]["db"][0]
    lin = 10.0 ** (truth.astype(np.float64) / 20.0)
    r = np.random.default_rng(20)
    bent = np.abs(lin + 0.99e-6 * lin.max() * r.choice([-1.0, 1.0], lin.shape))  # every bin, seeded signs
    bent_db = (20.0 * np.log10(np.maximum(bent, 1e-300))).astype(np.float32)
    before = dict(helpers.ARM_STATS)
    assert signals.assert_no_worse_than_reference(ref, ref, truth, 1, "the reference's own row") <= 1.0
    with pytest.raises(AssertionError, match="farther from the double DFT"):
        signals.assert_no_worse_than_reference(bent_db, ref, truth, 8, "1e-6 of the peak")
    assert helpers.ARM_STATS == before, "the criterion counts nothing in ARM_STATS"
    assert_db_close(bent_db, truth, "1e-6 of the peak passes the existing criterion")  # (by its linear arm: counted, CPU process only)
    assert helpers.ARM_STATS["linear_arm"] > before["linear_arm"]


# ---- what counts as silence ---------------------------------------------------------------------------------------------------
SPECIAL = {"denormal": 1e-40, "nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}


@pytest.mark.parametrize("n", [512, 800])
def test_silence_semantics(n):
    """the reference tests x == 0.0f sample by sample (src/source_generic.cpp:63-72): a denormal, a NaN and an infinity are
    not zero, -0.0f is"""
    cfg_dict = dict(fft_size=n, capture_channels=1, stereo=0, tsmoothing=0)
    cfg = scenarios.make_config(cfg_dict)
    backends = [scenarios.OracleBackend] + ([scenarios.RefBackend] if wfref.available() else [])

    def one_tick(be, points):
        return scenarios.play(be(cfg), dict(cfg=cfg_dict, steps=[("signal", n, signals.impulses(points)), ("tick",)], record="all"))[0]

    for be in backends:
        zeros = one_tick(be, [])
        assert zeros["silent"], f"{be.__name__}: a window of +0.0f reads silent at the first tick"
        for p in (0, 1, n // 2, n - 1):
            neg = one_tick(be, [(p, -0.0)])
            assert neg["silent"] and np.array_equal(neg["db"], zeros["db"]), f"{be.__name__}: -0.0f at {p} is zero"
            for name, v in SPECIAL.items():
                assert not one_tick(be, [(p, v)])["silent"], f"{be.__name__}: a lone {name} at {p} is not silence"
