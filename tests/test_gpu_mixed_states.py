"""Batches whose streams are in DIFFERENT states, stream by stream against the reference.

Every other comparison with the restatement or the reference plays one script in every stream of its batch; the tests that do
mix states (reset, bars-only, wrap) compare the library with a twin handle of itself.  Here one batch holds a live stream, one
that latches silent and comes back, one fed on one channel only, one hidden and later timed out, one with muted packets, one
that is not ticked in some frames, a late starter 20 ms ahead of the video (its first ticks underflow), and a twin of the
latching one at another position -- each with its own noise and packet size, the roles' positions rotating with the seed
(scenarios.draw_mixed).  scenarios.play_batch() drives them in lock step through the per-stream forms of the C ABI; every
stream's records are then held against its script played ALONE on the restatement (the reference library where the
restatement's DFT cannot go), with test_gpu_fuzz._compare: no tolerance of this module's own.

What it is for: the per-stream words of spectrum_tick_kernel (write position, flags, gain, delay), the workgroup's facts of
two streams sharing a workgroup, the clamped spare subgroup, the split geometries' verdict words, the bars-only verdict words,
the underflow / paused / hidden gates inside the mixed-radix transform -- an index that reads the neighbour's word is invisible
to a batch of identical streams.
"""
import time

import numpy as np
import pytest

import helpers
import scenarios
import test_gpu_fuzz as fuzz
from helpers import assert_db_close, assert_levels_close

LAYOUTS = {"mono": dict(capture_channels=1, stereo=0), "mixdown": dict(capture_channels=2, stereo=0),
           "stereo": dict(capture_channels=2, stereo=1), "dup": dict(capture_channels=1, stereo=1)}
DISPLAYS = {
    "none": dict(),
    "bars": dict(bars=1, interp_mode=1),                                     # Lanczos bars: the prefix-sum kernels where they exist
    "curve": dict(curve=1, interp_mode=2, filter_mode=1, filter_radius=1.5),  # Catmull-Rom curve, Gaussian filter
    "mirror": dict(bars=1, interp_mode=1, mirror_freq_axis=1),
    "nodb": dict(bars=1, interp_mode=1),                                      # + WF_HIP_TICK_NO_DECIBELS on every tick
}
# size -> (the part of kernel_name() the size is there for, the (layout, display) pairs).  Every size with one captured channel
# and with two; every split size with stereo and with the mono mixdown (which itself runs split at 32768 only: at 8192 and 16384
# its two spectra share a workgroup).
SHAPES = {
    128: ("zero-padded", [("mono", "none"), ("stereo", "bars"), ("dup", "curve")]),
    512: ("N=512,", [("mono", "bars"), ("mixdown", "nodb")]),
    1024: ("N=1024,", [("mono", "nodb"), ("stereo", "none"), ("mixdown", "curve")]),
    2048: ("N=2048,", [("dup", "mirror"), ("stereo", "nodb")]),
    4096: ("N=4096,T=128", [("mono", "curve"), ("stereo", "bars"), ("mixdown", "mirror")]),
    8192: ("N=8192,", [("mono", "bars"), ("stereo", "nodb"), ("mixdown", "curve")]),
    16384: ("N=16384,", [("dup", "none"), ("stereo", "curve"), ("mixdown", "bars")]),
    32768: ("N=32768,", [("mono", "bars"), ("stereo", "none"), ("mixdown", "mirror")]),
    65536: ("big_whole_kernel", [("mono", "curve"), ("stereo", "bars")]),
    800: ("mixed radix 5x10x8", [("mono", "bars"), ("mixdown", "none"), ("stereo", "nodb")]),
    1760: ("mixed radix 10x8x11", [("dup", "none"), ("stereo", "curve")]),
    1088: ("mixed radix 17x", [("mono", "none"), ("stereo", "mirror")]),
    2096: ("Bluestein", [("mono", "bars"), ("stereo", "none")]),
    8000: ("mixed radix", [("mono", "none"), ("stereo", "bars"), ("mixdown", "none")]),
    48000: ("big_mr_rows_kernel", [("mono", "none"), ("stereo", "bars")]),
    16400: ("big_br_", [("dup", "none"), ("mixdown", "curve")]),
}
SPLIT_SIZES = (8192, 16384, 32768)  # a stereo pair runs with its channels in different workgroups; at 32768 the mono mixdown too
# packets and reserves in multiples of 4 frames: the ALIGNED instantiations (vector window fetch) in a mixed batch
ALIGNED = [(1024, "mono", "none"), (4096, "stereo", "bars"), (8192, "stereo", "none")]


def _cases():
    out = []
    for n, (_, pairs) in SHAPES.items():
        for layout, display in pairs:
            out.append((n, layout, display, len(out), False))
    for n, layout, display in ALIGNED:
        out.append((n, layout, display, len(out), True))
    return out


CASES = _cases()


def case_config(n, layout, display, extra=None):
    """every size keeps the exponential smoothing (the per-stream state m_tsmooth_buf: a channel that is skipped keeps it, one
    that is processed on silence decays it, so a wrong verdict shows in the rows) with a gravity at which the display decays
    below floor - 10 within a few ticks: 0.2 below 16384 (the time-varying kind, at 2048 and 800, 0.02: enough even in frames of
    1/144 s), 0.05 from 16384 on, where a window takes longest to empty"""
    d = dict(fft_size=n, slope=1.0, **LAYOUTS[layout], **DISPLAYS[display])
    d.update(dict(tsmoothing=1, gravity=0.05) if n >= 16384 else (dict(tsmoothing=2, gravity=0.02, fast_peaks=int(n == 2048)) if n in (2048, 800) else dict(tsmoothing=1, gravity=0.2)))
    d.update(extra or {})
    return d


def streams_for(n, cap):
    return (4 if n > 16384 else 7 if cap == 1 else 5)


def solo_backend(cfg, rms=None):
    """the checker for one stream: the restatement, or the reference itself where the restatement's DFT cannot go"""
    if fuzz._largest_prime_factor(int(cfg.fft_size)) <= fuzz.RESTATEMENT_MAX_PRIME or cfg.meter or cfg.waveform:
        return scenarios.OracleBackend(cfg, input_rms=rms)
    from oracle import wfref
    assert wfref.available(), "oracle/_ref/libwfref.so is needed to check this length (largest prime factor too large for the restatement)"
    assert rms is None
    return scenarios.RefBackend(cfg)


def assert_mixed(cfg, scripts, want, what):
    """on the checker's own records: the batch really was mixed at some tick, whatever later edits do to the scripts"""
    pairs = cfg.capture_channels == 1 and len(scripts) == 7
    hits = scenarios.mixed_ticks(cfg, scripts, want, pairs)
    assert hits, f"{what}: at no tick is one stream latched silent next to a live one while another is hidden" + \
        (" and another processes one channel only" if cfg.capture_channels == 2 else "")
    return hits


def assert_twins_equal(scripts, got, what):
    n = 0
    for i, sc in enumerate(scripts):
        j = sc["twin_of"]
        if j is None:
            continue
        n += 1
        for t, (a, b) in enumerate(zip(got[i], got[j])):
            assert a["silent"] == b["silent"] and np.array_equal(a["db"], b["db"], equal_nan=True), f"{what} tick {t}: streams {i} and {j} are twins and differ"
            assert (a["bars"] is None) == (b["bars"] is None) and (a["bars"] is None or np.array_equal(a["bars"], b["bars"], equal_nan=True)), \
                f"{what} tick {t}: the displays of the twin streams {i} and {j} differ"
    assert n == 1, "every batch carries one pair of twins"


# the module's own totals: differences of the shared counters around its cases
TOTALS = {"values": 0, "linear_arm": 0, "linear_arm_visible": 0, "deep": 0, "display_checks": 0, "display_arm": 0, "seconds": 0.0, "cases": 0}


class _Counted:
    def __enter__(self):
        self.t0 = time.perf_counter()
        self.a = dict(helpers.ARM_STATS)
        self.d = (fuzz.ARM["display_checks"], fuzz.ARM["display_arm"])
        return self

    def __exit__(self, *exc):
        for k in ("values", "linear_arm", "linear_arm_visible", "deep"):
            TOTALS[k] += helpers.ARM_STATS[k] - self.a[k]
        TOTALS["display_checks"] += fuzz.ARM["display_checks"] - self.d[0]
        TOTALS["display_arm"] += fuzz.ARM["display_arm"] - self.d[1]
        TOTALS["seconds"] += time.perf_counter() - self.t0
        TOTALS["cases"] += 1


def _compare_display_only(got, want, cfg, what):
    """bars-only ticks: the rows are stale by contract, so m_last_silent and the display alone -- the display with the pixel
    tolerance of test_gpu_fuzz._compare, without its second arm (there are no rows of the device's to render from)"""
    px = fuzz._px_tol(cfg)
    for t, (g, w) in enumerate(zip(got, want)):
        assert g["silent"] == w["silent"], f"{what} tick {t}: m_last_silent {g['silent']} != {w['silent']}"
        assert g["bars"] is not None and w["bars"] is not None
        err = np.abs(g["bars"].astype(np.float64) - w["bars"])
        assert np.all(err <= 1e-5 * np.abs(w["bars"]) + px), f"{what} tick {t} bars: max err {err.max():.3e} px (tolerance {px:.1e})"


def fixed_rms(scripts):
    """m_input_rms per stream for wf_hip_set_input_rms, by the stream's noise (twins share it); 0.0: "no audio seen yet", the
    full max_gain"""
    return [(0.5, 0.0316, 0.0, 1e-4, 0.1, 0.02, 0.25)[sc["noise_id"] - 1] for sc in scripts]


class Case:
    """what run_case plays: the configuration, the scripts of its streams, the tick flags and the fixed m_input_rms values"""

    def __init__(self, n, layout, display, seed, aligned=False, extra=None, rms=None, kernel=None):
        self.n = n
        self.cfg = scenarios.make_config(case_config(n, layout, display, extra))
        self.S = streams_for(n, int(self.cfg.capture_channels))
        self.scripts = scenarios.draw_mixed(seed, self.cfg, self.S, aligned=aligned, base_sync_ms=5 if aligned else None)
        self.what = f"mixed batch {n} {layout} {display} seed {seed}{' aligned' if aligned else ''}"
        self.flags = scenarios.WF_HIP_TICK_NO_DECIBELS if display == "nodb" else 0
        self.fixed = fixed_rms(self.scripts) if rms == "set" else None
        self.kernel = kernel if kernel is not None else SHAPES[n][0]


def play_hip(case):
    """the batch on the device: (records per stream, kernel_name(), launches_per_tick())"""
    cfg, n, what = case.cfg, case.n, case.what
    hip = scenarios.HipBatch(cfg, case.S, rms=case.fixed, flags=case.flags)
    try:
        name = hip.kernel_name()
        assert case.kernel in name, (what, name)
        if n in SPLIT_SIZES:
            assert ("split" in name) == (cfg.capture_channels == 2 and (bool(cfg.stereo) or n == 32768)), (what, name)
        if n == 128:
            assert "SPW=2" in name, (what, name)
        launches = hip.batch.launches_per_tick()
        got = scenarios.play_batch(hip, case.scripts)
    finally:
        hip.close()
    return got, name, launches


def compare_with_solo(case, got):
    """every stream's records against its own script played alone on the checker"""
    cfg, scripts, what, fixed = case.cfg, case.scripts, case.what, case.fixed
    want = []
    for i, sc in enumerate(scripts):
        want.append(scenarios.play(solo_backend(cfg, None if fixed is None else fixed[i]), sc))
    assert_mixed(cfg, scripts, want, what)
    undo = fuzz._undo_db(cfg)
    for i, sc in enumerate(scripts):
        w = f"{what} stream {i} ({sc['role']}, sync {sc['sync_ms']} ms)"
        if case.flags:
            _compare_display_only(got[i], want[i], cfg, w)
        else:
            fuzz._compare(got[i], want[i], undo, w, cfg_stepped=int(cfg.vertices) == 3, cfg=cfg)  # (stepped bars: as run_spectrum_case)
    assert_twins_equal(scripts, got, what)


def run_case(n, layout, display, seed, aligned=False, extra=None, rms=None, kernel=None):
    case = Case(n, layout, display, seed, aligned, extra, rms, kernel)
    with _Counted():
        got, _, _ = play_hip(case)
        compare_with_solo(case, got)


@pytest.mark.gpu
@pytest.mark.parametrize("n,layout,display,seed,aligned", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}-s{c[3]}{'-aligned' if c[4] else ''}" for c in CASES])
def test_every_stream_of_a_mixed_batch_matches_its_own_reference(n, layout, display, seed, aligned):
    run_case(n, layout, display, seed, aligned)


# volume normalisation: the gain is a per-stream word (vol_comp_stream) or comes from the device producer's per-stream state
NORMALIZE = dict(normalize_volume=1, volume_target=-12.0, max_gain=24.0)


@pytest.mark.gpu
@pytest.mark.parametrize("n,layout,rms", [(2048, "stereo", "set"), (800, "mono", "set"), (2048, "mono", "device"), (800, "stereo", "device")])
def test_mixed_batch_with_volume_normalisation(n, layout, rms):
    """once with per-stream wf_hip_set_input_rms values, once with the device producer against the restated one"""
    run_case(n, layout, "bars", 100 + n + len(layout), extra=NORMALIZE, rms=rms, kernel="mixed radix" if n == 800 else "N=2048,")


@pytest.mark.gpu
def test_mixed_meter_batch():
    """live, latching, hidden / timed out, muted and paused streams of one level-meter batch, judged like run_meter_case"""
    cfg_dict = dict(meter=1, meter_ms=50, tsmoothing=0, capture_channels=2)
    cfg = scenarios.make_config(cfg_dict)
    S = 6
    scripts = scenarios.draw_mixed(3, cfg, S)
    hip = scenarios.HipBatch(cfg, S)
    try:
        assert "meter_tick_kernel" in hip.kernel_name()
        got = scenarios.play_batch(hip, scripts)
    finally:
        hip.close()
    want = [scenarios.play(scenarios.OracleBackend(cfg), sc) for sc in scripts]
    truth = [scenarios.play(scenarios.OracleBackend(cfg, exact=True), sc) for sc in scripts]
    assert_mixed(cfg, scripts, want, "mixed meter batch")
    for i, sc in enumerate(scripts):
        for t, (g, w, x) in enumerate(zip(got[i], want[i], truth[i])):
            what = f"mixed meter batch stream {i} ({sc['role']}) tick {t}"
            assert g["silent"] == w["silent"] or g["silent"] == x["silent"], f"{what}: m_last_silent {g['silent']} != {w['silent']}"
            assert_levels_close(g["db"], w["db"], x["db"], what + " levels")
            tol = 1e-5 * np.abs(w["bars"]) + 2e-3
            gb, wb, xb = (np.asarray(v["bars"], np.float64) for v in (g, w, x))
            assert ((np.abs(gb - wb) <= tol) | (np.abs(gb - xb) <= np.abs(wb - xb) + tol)).all(), f"{what} bars: got {gb}, reference {wb}, exact sum {xb}"
    assert_twins_equal(scripts, got, "mixed meter batch")


@pytest.mark.gpu
def test_mixed_waveform_batch():
    """per-stream audio timestamps, reserves, paused and hidden streams of one waveform batch, judged like the waveform fuzz"""
    cfg_dict = dict(waveform=1, stereo=1, capture_channels=2, width=333, meter_ms=50)
    cfg = scenarios.make_config(cfg_dict)
    S = 6
    scripts = scenarios.draw_mixed(2, cfg, S)
    hip = scenarios.HipBatch(cfg, S)
    try:
        assert "waveform_tick_kernel" in hip.kernel_name()
        got = scenarios.play_batch(hip, scripts)
    finally:
        hip.close()
    want = [scenarios.play(scenarios.OracleBackend(cfg), sc) for sc in scripts]
    states = [scenarios.script_states(sc["steps"]) for sc in scripts]
    assert any(any(s[t]["hidden"] for s in states) and any(s[t]["paused"] for s in states) for t in range(scenarios.MIXED_TICKS)), \
        "no tick with a hidden and a paused stream"
    assert len({sc["sync_ms"] for sc in scripts}) > 1, "the streams share one reserve"
    for i, sc in enumerate(scripts):
        for t, (g, w) in enumerate(zip(got[i], want[i])):
            what = f"mixed waveform batch stream {i} ({sc['role']}, sync {sc['sync_ms']} ms) tick {t}"
            assert g["silent"] == w["silent"], f"{what}: m_last_silent {g['silent']} != {w['silent']}"
            assert_db_close(g["db"], w["db"], what + " rows", lin_eps=None)
            assert g["wts"] == w["wts"], f"{what}: m_waveform_ts {g['wts']} != {w['wts']}"
    assert_twins_equal(scripts, got, "mixed waveform batch")


@pytest.mark.gpu
def test_zz_mixed_arms_stay_rare():
    """runs last in this module.  The linear and deep arms of assert_db_close are a cap, not a measurement: over this module's
    own comparisons they may decide at most 1e-5 of the values (the bound README.md states for the suite; with too few values
    for that to allow even one, none), of them at most 1e-6 above -75 dB; the display's second arm at most 5 of 1000 checks (the
    bound of test_gpu_fuzz.py)."""
    t = TOTALS
    print(f"mixed-state module: {t['cases']} cases in {t['seconds']:.1f} s; {t['values']} dB values, linear arm {t['linear_arm']} "
          f"(visible {t['linear_arm_visible']}), deep arm {t['deep']}; display checks {t['display_checks']}, second arm {t['display_arm']}")
    assert t["linear_arm"] + t["deep"] <= int(1e-5 * t["values"]), t
    assert t["linear_arm_visible"] <= int(1e-6 * t["values"]), t
    if t["display_checks"] >= 200:
        assert t["display_arm"] <= max(1, 5 * t["display_checks"] // 1000), t
