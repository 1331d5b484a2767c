"""The driver and the scripts of tests/test_gpu_mixed_states.py without a device.

play_batch() is run on a "batch" made of S restated sources (scenarios.OracleBatch) and must give, bit for bit, what every
script gives played alone: that pins the lock step, the rule for a frame a source is not ticked in, and the split of the A/V-sync
reserve into the tick's common part and the per-stream remainders.  Every script is then played alone on the reference library
itself, which shows that the roles mean on the reference what the GPU module assumes (a paused tick is an un-ticked source, a
capture timeout ends with the next packet), that every drawn case is mixed in the module's sense, and that the restatement
alone stays inside the bound the GPU module puts on the linear and deep arms.
"""
import numpy as np
import pytest

import helpers
import scenarios
import test_gpu_fuzz as fuzz
import test_gpu_mixed_states as mixed
from oracle import wfref

CPU_MAX = 4096
CPU_CASES = [c for c in mixed.CASES if c[0] <= CPU_MAX]
TOTALS = {"values": 0, "linear_arm": 0, "linear_arm_visible": 0, "deep": 0}


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def assert_same_records(got, want, what):
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        assert g["silent"] == w["silent"] and _same(g["db"], w["db"]) and _same(g["bars"], w["bars"]), f"{what} tick {t}"
        assert g.get("wts") == w.get("wts") and _same(g.get("rms"), w.get("rms")), f"{what} tick {t}"


def _batch_against_solo(cfg, scripts, what, rms=None):
    got = scenarios.play_batch(scenarios.OracleBatch(cfg, len(scripts), rms=rms), scripts)
    want = [scenarios.play(scenarios.OracleBackend(cfg, input_rms=None if rms is None else rms[i]), sc) for i, sc in enumerate(scripts)]
    for i, sc in enumerate(scripts):
        assert_same_records(got[i], want[i], f"{what} stream {i} ({sc['role']})")
    mixed.assert_twins_equal(scripts, got, what)
    return want


@pytest.mark.parametrize("n,layout,display,seed,aligned", CPU_CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}-s{c[3]}{'-aligned' if c[4] else ''}" for c in CPU_CASES])
def test_batch_driver_and_roles_on_the_reference(n, layout, display, seed, aligned):
    cfg_dict = mixed.case_config(n, layout, display)
    cfg = scenarios.make_config(cfg_dict)
    S = mixed.streams_for(n, int(cfg.capture_channels))
    scripts = scenarios.draw_mixed(seed, cfg, S, aligned=aligned, base_sync_ms=5 if aligned else None)
    what = f"mixed batch {n} {layout} {display} seed {seed}"
    if aligned:
        assert all(st[1] % 4 == 0 for sc in scripts for st in sc["steps"] if st[0] not in ("tick", "hide", "show", "timeout"))
        assert all(sc["sync_ms"] * 48 % 4 == 0 and sc["sync_ms"] > 0 for sc in scripts)
    restated = _batch_against_solo(cfg, scripts, what)
    mixed.assert_mixed(cfg, scripts, restated, what)
    if not wfref.available():
        pytest.skip("oracle/_ref/libwfref.so not built")
    before = dict(helpers.ARM_STATS)
    undo = fuzz._undo_db(cfg)
    ref = []
    for i, sc in enumerate(scripts):
        ref.append(scenarios.play(scenarios.RefBackend(cfg), sc))
        fuzz._compare(restated[i], ref[i], undo, f"{what} stream {i} ({sc['role']}): restatement vs libwfref", cfg=cfg)
    mixed.assert_mixed(cfg, scripts, ref, what + " (libwfref)")
    for k in TOTALS:
        TOTALS[k] += helpers.ARM_STATS[k] - before[k]


@pytest.mark.parametrize("seed", range(7))
def test_every_rotation_of_the_roles_is_mixed(seed):
    """seven streams of one captured channel: every role at every position of a workgroup pair and in the half-filled last
    workgroup, and at each rotation a latched stream sits next to a live one"""
    cfg = scenarios.make_config(mixed.case_config(512, "mono", "none"))
    scripts = scenarios.draw_mixed(seed, cfg, 7)
    assert sorted(sc["role"] for sc in scripts) == sorted("+".join(r) for r in scenarios.MIXED_ROLES[(1, 7)])
    assert scripts[seed % 7]["role"] == "latches" and scripts[(seed + 3) % 7]["twin_of"] == seed % 7
    mixed.assert_mixed(cfg, scripts, _batch_against_solo(cfg, scripts, f"rotation {seed}"), f"rotation {seed}")


@pytest.mark.parametrize("rms", ["set", "device"])
def test_batch_driver_with_volume_normalisation(rms):
    cfg = scenarios.make_config(mixed.case_config(800, "stereo", "bars", mixed.NORMALIZE))
    scripts = scenarios.draw_mixed(11, cfg, 5)
    _batch_against_solo(cfg, scripts, f"normalised batch ({rms})", rms=mixed.fixed_rms(scripts) if rms == "set" else None)


@pytest.mark.parametrize("kind", ["meter", "waveform"])
def test_batch_driver_on_meter_and_waveform(kind):
    cfg = scenarios.make_config(dict(meter=1, meter_ms=50, tsmoothing=0, capture_channels=2) if kind == "meter" else
                                dict(waveform=1, stereo=1, capture_channels=2, width=333, meter_ms=50))
    scripts = scenarios.draw_mixed(3 if kind == "meter" else 2, cfg, 6)
    want = _batch_against_solo(cfg, scripts, f"mixed {kind} batch")
    if kind == "meter":
        mixed.assert_mixed(cfg, scripts, want, "mixed meter batch")


def test_split_reserves():
    assert scenarios.split_reserves([240, 960, 240, 0]) == (0, [240, 960, 240, 0])
    assert scenarios.split_reserves([240, 960, 241]) == (240, [0, 720, 1])


def test_zz_restatement_arms_stay_rare():
    """runs last in this module: the restatement against the reference on the mixed scripts, under the GPU module's bound"""
    t = TOTALS
    print(f"mixed-state scripts, restatement vs libwfref: {t['values']} dB values, linear arm {t['linear_arm']} "
          f"(visible {t['linear_arm_visible']}), deep arm {t['deep']}")
    assert t["linear_arm"] + t["deep"] <= int(1e-5 * t["values"]), t
    assert t["linear_arm_visible"] <= int(1e-6 * t["values"]), t
