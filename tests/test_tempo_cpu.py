"""Tempo and beat phase (WF_HIP_OUT_TEMPO) without a device: the structured dtype against the C layout, the appended output number,
the library's own builder of the lags and the preference against the restatement
(tests/tempo_ref.py), what the restatement reads on pulse trains, noise, a sine and silence, the margins of the signals of the
device comparison, and a gfx950 compile of the kernels with no scratch and no spills.

What the restatement reads here, re-measured (include/wf_hip.h, "tempo", quotes these): the recovered pulse trains within 0.13 %
(119.84 for 120), confidence at least 0.80 (60 BPM kicks at T = 1019), last_beat_frame within 432 frames of a true beat (120 BPM at
T = 2043); noise at -20 dBFS valid with a confidence of 0.076 to 0.089; 174 BPM reads 87 from T = 1019 on with bpm2 at 173, 200 BPM
bursts read 100 with bpm2 at 201, 60 BPM at T = 507 reads 120."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import tempo_ref as ref
from kernel_usage import kernel_usage

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "waveform_amd" / "csrc"
SR = 48000
RINGS = {507: 131072, 1019: 1 << 18, 2043: 1 << 19}


def test_tempo_dtype_matches_the_c_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wf_hip.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %d %d %d %d %d %d %d %d %g", sizeof(wf_hip_tempo), (int)WF_HIP_OUT_TEMPO, (int)WF_HIP_OUT_IMD, (int)WF_HIP_TEMPO_WINDOW,\n'
                   "         (int)WF_HIP_TEMPO_HOP, (int)WF_HIP_TEMPO_COLUMNS, (int)WF_HIP_TEMPO_LAGS, (int)WF_HIP_TEMPO_MAX_LAG,\n"
                   "         (int)WF_HIP_TEMPO_MIN_RING, (double)WF_HIP_TEMPO_MARGIN);\n"
                   + "".join(f'  printf(" %zu", offsetof(wf_hip_tempo, {n}));\n' for n in ref.FIELDS) +
                   '  printf(" %d", (int)WF_HIP_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [float(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    dt = binding.TEMPO_DTYPE
    assert got == [dt.itemsize, binding.OUT_TEMPO, binding.OUT_IMD, binding.TEMPO_WINDOW, binding.TEMPO_HOP, binding.TEMPO_COLUMNS,
                   binding.TEMPO_LAGS, binding.TEMPO_MAX_LAG, binding.TEMPO_MIN_RING, binding.TEMPO_MARGIN] \
        + [dt.fields[n][1] for n in ref.FIELDS] + [13]
    assert dt.itemsize == 10592 and dt.itemsize % 8 == 0 and dt == ref.TEMPO_DTYPE and dt.names == ref.FIELDS
    # the header's numbers: 2048 strengths, 576 lags, nine floats, thirteen words, two reserved
    assert [dt.fields[n][1] for n in ref.FIELDS] == [0, 8192] + [10496 + 4 * i for i in range(9 + 13)] + [10584]
    assert ref.FIELDS == ("strength", "acf", "bpm", "period", "confidence", "salience", "bpm2", "salience2", "ambiguity", "strength_max",
                          "strength_mean", "valid", "columns", "newest", "lag_lo", "lag_hi", "lag", "lag2", "beat_age", "period_frames",
                          "last_beat_frame", "next_beat_frame", "window", "hop", "reserved")
    assert dt.fields["strength"][0].shape == (2048,) and dt.fields["acf"][0].shape == (576,) and dt.fields["reserved"][0].shape == (2,)
    assert all(dt.fields[n][0] == np.float32 for n in ref.FLOAT_FIELDS) and all(dt.fields[n][0] == np.uint32 for n in ref.UINT_FIELDS)
    assert (ref.WINDOW, ref.HOP, ref.COLUMNS, ref.LAGS, ref.MAX_LAG, ref.MIN_RING, ref.MARGIN) == \
        (binding.TEMPO_WINDOW, binding.TEMPO_HOP, binding.TEMPO_COLUMNS, binding.TEMPO_LAGS, binding.TEMPO_MAX_LAG, binding.TEMPO_MIN_RING,
         binding.TEMPO_MARGIN) == (1024, 256, 2048, 576, 287, 131072, 2.0)
    assert 2 * ref.MAX_LAG + 2 == ref.LAGS


# ---- the host's builder ---------------------------------------------------------------------------------------------------------

PROGRAM = r"""
#include <cstdio>
#include <initializer_list>
#include "wf_measure_tables.hpp"
using namespace wf::host;
int main() {
  for(unsigned sr : {8000u, 22050u, 44100u, 48000u, 96000u, 192000u, 384000u})
    for(unsigned ring : {65536u, 131072u, 262144u, 524288u, 1048576u, 4194304u}) {
      const TempoTables t = tempo_tables(sr, ring);
      const TempoPlan p = tempo_plan(sr, ring);
      if(p.columns != t.plan.columns || p.lag_lo != t.plan.lag_lo || p.lag_hi != t.plan.lag_hi || t.prior.size() != WF_HIP_TEMPO_MAX_LAG + 1) return 2;
      std::printf("%u %u %u %u %u %d", sr, ring, p.columns, p.lag_lo, p.lag_hi, (int)p.served());
      for(double w : t.prior) std::printf(" %.17g", w);
      std::printf("\n");
    }
  return 0;
}
"""


def test_the_lags_and_the_preference_of_the_library(tmp_path):
    """wf::host::tempo_tables, compiled into a program of its own under the address and undefined-behaviour sanitizers, against
    the restatement: T, lag_lo, lag_hi and whether the output is served exactly; w[L] to rtol 1e-12 (two libm calls)"""
    src = tmp_path / "tempo_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "tempo_tables"
    subprocess.run(["g++", "-std=c++20", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(CSRC),
                    "-I", str(ROOT / "include"), str(src), str(CSRC / "wf_measure_tables.cpp"), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == 42
    seen = set()
    for line in lines:
        f = line.split()
        sr, ring, t, lo, hi, served = (int(v) for v in f[:6])
        w = np.array(f[6:], np.float64)
        if ring < ref.MIN_RING:
            assert (t, served) == (0, 0)
            continue
        assert t == ref.columns(ring) and (lo, hi) == ref.lag_range(sr, t) and bool(served) == ref.served(sr, ring), line[:60]
        np.testing.assert_allclose(w, ref.prior(sr), rtol=1e-12, atol=0)
        assert w[0] == 0.0 and np.all(w[1:] > 0) and np.all(w <= 1.0)
        seen.add((sr, ring, t, lo, hi, served))
    assert (48000, 131072, 507, 47, 126, 1) in seen and (48000, 1 << 18, 1019, 47, 254, 1) in seen
    assert (48000, 1 << 19, 2043, 47, 281, 1) in seen and (48000, 1 << 20, 2048, 47, 281, 1) in seen
    assert (8000, 131072, 507, 8, 46, 1) in seen and (384000, 1 << 20, 2048, 375, 287, 0) in seen
    assert ref.prior(SR)[94] > 0.999 and abs(ref.prior(SR)[47] - np.exp(-0.5)) < 0.01  # 119.7 BPM; 239.4 BPM, an octave up


# ---- what the restatement reads -------------------------------------------------------------------------------------------------

def _read(x, t, sr=SR):
    """the entry and the decisions' values of a mono signal whose last frame is the counter's, from T = t columns"""
    o = ref.strengths(x[None, None], len(x), sr, RINGS[t])
    assert o.shape == (1, t)
    entry, vals = ref.analyse(o[0], len(x), sr)
    return entry, vals, o[0]


def _frames(t):
    return (t + 1) * ref.H + ref.P + 77


RECOVERED = [(507, bpm) for bpm in (90, 120, 128, 150)] + [(t, bpm) for t in (1019, 2043) for bpm in (60, 72.5, 90, 120, 128, 150)]


@pytest.mark.parametrize("kind", (ref.kicks, ref.bursts), ids=("kicks", "bursts"))
@pytest.mark.parametrize("t,bpm", RECOVERED)
def test_pulse_trains_read_their_tempo_and_phase(t, bpm, kind):
    x, at, period = kind(np.random.default_rng(int(bpm * 10) + t), bpm, _frames(t))
    e, v, o = _read(x, t)
    err = ref.beat_error(int(e["last_beat_frame"]), at, period)
    print(f"T {t}, {bpm} BPM {kind.__name__}: bpm {float(e['bpm']):.2f}, confidence {float(e['confidence']):.3f}, lag {int(e['lag'])}, second "
          f"{float(e['bpm2']):.1f} (ambiguity {float(e['ambiguity']):.2f}), last beat {err:.0f} frames off, margins {ref.margins(o, len(x), SR)}")
    assert e["valid"] == 1 and e["columns"] == t
    assert abs(e["bpm"] / bpm - 1.0) < 0.005
    assert e["confidence"] > 0.7
    assert err <= 768
    assert e["period_frames"] == int(e["period"] * 256) and e["period"] * 16 == int(e["period"] * 16)
    assert int(e["next_beat_frame"]) == int(e["last_beat_frame"]) + int(e["period_frames"])
    assert abs(60.0 * SR / (256.0 * e["period"]) / e["bpm"] - 1.0) < 1.0 / (32 * e["lag"]) + 1e-6  # a sixteenth of a column
    assert np.all(e["acf"][2 * int(e["lag_hi"]) + 2:] == 0) and e["acf"][0] == 1.0


def _within_a_column(bpm, lag):
    return lag and abs(60.0 * SR / (256.0 * bpm) - lag) <= 1.0


@pytest.mark.parametrize("t,bpm,kind,reads", [(1019, 174, ref.kicks, 87), (2043, 174, ref.bursts, 87), (507, 200, ref.bursts, 100),
                                              (2043, 200, ref.bursts, 100), (507, 60, ref.kicks, 120), (507, 60, ref.bursts, 120),
                                              (507, 174, ref.kicks, 174), (2043, 200, ref.kicks, 200)])
def test_what_is_not_recovered_is_still_named(t, bpm, kind, reads):
    """the octave the rule settles on is stated, not recovered: the truth is bpm or bpm2's lag within one column, or its octave"""
    x, at, period = kind(np.random.default_rng(int(bpm * 10) + t), bpm, _frames(t))
    e, v, o = _read(x, t)
    print(f"T {t}, {bpm} BPM {kind.__name__}: reads {float(e['bpm']):.2f}, second {float(e['bpm2']):.2f}, ambiguity {float(e['ambiguity']):.2f}")
    assert e["valid"] == 1 and abs(e["bpm"] / reads - 1.0) < 0.01
    lags = (int(e["lag"]), int(e["lag2"]))
    assert any(_within_a_column(b, lag) for lag in lags for b in (bpm, bpm / 2.0, bpm * 2.0))
    if reads != bpm and t > 507:  # (at T = 507 a lag of 60 BPM is outside the range)
        assert any(_within_a_column(bpm, lag) for lag in lags) and e["ambiguity"] > 0.5


@pytest.mark.parametrize("t", (507, 1019, 2043))
def test_noise_a_sine_and_silence(t):
    frames = _frames(t)
    e, _, o = _read(ref.noise(np.random.default_rng(5 + t), -20.0, frames), t)
    print(f"T {t}: noise at -20 dBFS: confidence {float(e['confidence']):.3f}, largest strength {float(e['strength_max']):.2f}")
    assert e["valid"] == 1 and e["confidence"] < 0.2 and e["strength_max"] >= 2.0 and e["strength_max"] == o.max()
    for name, x in (("noise at -60 dBFS", ref.noise(np.random.default_rng(6 + t), -60.0, frames)), ("a steady sine", ref.steady_sine(frames)),
                    ("silence", np.zeros(frames, np.float32))):
        e, vals, o = _read(x, t)
        assert e["valid"] == 0 and vals is None and o.max() < 0.1, name
        for f in ref.DERIVED:
            assert not np.any(e[f]), (name, f)
        lo, hi = ref.lag_range(SR, t)
        assert (e["columns"], e["newest"], e["lag_lo"], e["lag_hi"], e["window"], e["hop"]) == (t, frames // 256, lo, hi, 1024, 256)
        assert np.array_equal(e["strength"][:t], o) and not np.any(e["strength"][t:])


def test_a_strength_that_is_not_finite_and_a_curve_below_the_margin():
    x, _, _ = ref.kicks(np.random.default_rng(1), 120.0, _frames(507))
    e, _, o = _read(x, 507)
    assert e["valid"] == 1
    for bad in (np.nan, np.inf):
        p = o.copy()
        p[300] = bad
        q, vals = ref.analyse(p, len(x), SR)
        assert q["valid"] == 0 and vals is None and not any(np.any(q[f]) for f in ref.DERIVED)
    low, _ = ref.analyse(o * np.float32(1.9 / o.max()), len(x), SR)
    assert low["valid"] == 0
    high, _ = ref.analyse(o * np.float32(2.1 / o.max()), len(x), SR)
    assert high["valid"] == 1 and high["lag"] == e["lag"]


def test_the_counter_wraps():
    x, _, _ = ref.kicks(np.random.default_rng(2), 120.0, _frames(507))
    _, _, o = _read(x, 507)
    a, _ = ref.analyse(o, 5000 * 256 + 3, SR)
    for wpos in ((1 << 32) + 40 * 256 + 3, (1 << 32) - 256 + 3, (1 << 32) + 3):
        b, _ = ref.analyse(o, wpos, SR)
        shift = (wpos - (5000 * 256 + 3)) % (1 << 32)
        assert int(b["last_beat_frame"]) == (int(a["last_beat_frame"]) + shift) % (1 << 32)
        assert int(b["next_beat_frame"]) == (int(a["next_beat_frame"]) + shift) % (1 << 32) and b["newest"] == (wpos % (1 << 32)) // 256
        assert b["lag"] == a["lag"] and b["beat_age"] == a["beat_age"]


def test_mismatches_applies_the_bound():
    case = ref.GPU_CASES[0]
    fft, sr, ch, kw, ring, t, kinds = case
    x = ref.case_audio(case)
    wpos = fft + x.shape[-1]
    want = ref.tempo(x, wpos, sr, ring)
    assert ref.mismatches(want, x, wpos, sr, ring) == ([], 0.0)
    got = want.copy()
    got["strength"][0, 5] = np.nextafter(got["strength"][0, 5], np.float32(1e9))  # one ulp: inside (and no integer moves: the margins)
    bad, worst = ref.mismatches(got, x, wpos, sr, ring)
    assert bad == [] and worst == 1.0
    got["strength"][0, 5] += 4 * np.spacing(got["strength"][0, 5])
    assert {m[0] for m in ref.mismatches(got, x, wpos, sr, ring)[0]} == {"strength"}
    got = want.copy()
    got["strength"][1, t] = 1e-3  # an age >= T is 0
    assert {m[0] for m in ref.mismatches(got, x, wpos, sr, ring)[0]} == {"strength"}
    for name in ("acf",) + ref.FLOAT_FIELDS:
        got = want.copy()
        f = got[name]
        where = (0, 3) if name == "acf" else (0,)
        f[where] = np.nextafter(f[where], np.float32(1e9))
        assert ref.mismatches(got, x, wpos, sr, ring)[0] == [], name
        f[where] += 3 * np.spacing(np.abs(f[where])) + np.float32(3e-9)
        assert [m[0].split()[0] for m in ref.mismatches(got, x, wpos, sr, ring)[0]] == [name], name
    for name in ref.UINT_FIELDS + ("reserved",):
        got = want.copy()
        got[name][2] += 1
        assert {m[0].split()[0] for m in ref.mismatches(got, x, wpos, sr, ring)[0]} == {name}
    got = want.copy()
    got["bpm"][1] = np.nan
    assert [m[0].split()[0] for m in ref.mismatches(got, x, wpos, sr, ring)[0]] == ["bpm"]
    assert ref.mismatches(want[:1], x, wpos, sr, ring)[0][0][0] == "shape"


# ---- the conditions of the device comparison ------------------------------------------------------------------------------------

def test_the_gpu_cases_have_margins():
    """on the very seeds and shapes of tests/test_gpu_tempo.py: the salience of the best lag over its nearest competitor, phi's
    maximum over its runner-up and 16 (lag + p) from a half-integer each stand at least four times farther from flipping than a
    change of every strength by one float32 ulp can move them (tempo_ref.margins: a first-order bound, doubled), and the largest
    strength stands thousands of ulps from the margin 2.0.  With these the integers of the device equal the restatement's"""
    kinds = set()
    for case in ref.GPU_CASES:
        fft, sr, ch, kw, ring, t, streams = case
        x = ref.case_audio(case)
        assert x.shape == (len(streams), ch, ring + ref.P // 2 + 3) and ref.columns(ring) == t and ref.served(sr, ring)
        wpos = ref.case_wpos0(case) + x.shape[-1]
        assert wpos % ref.H != 0
        o = ref.strengths(x, wpos, sr, ring)
        for s, kind in enumerate(streams):
            e, vals = ref.analyse(o[s], wpos, sr)
            m = ref.margins(o[s], wpos, sr)
            print(f"{ref.case_id(case)} {kind}: valid {int(e['valid'])}, bpm {float(e['bpm']):.2f}, lag {int(e['lag'])}, second {int(e['lag2'])}, "
                  f"beat_age {int(e['beat_age'])}, confidence {float(e['confidence']):.3f}, largest strength {float(o[s].max()):.2f}, margins {m}")
            if kind == "noise" and sr == 8000:  # the spectrum ends at 4 kHz, 48 of the 64 bands: no strength reaches the margin
                assert e["valid"] == 0 and (ref.MARGIN - float(o[s].max())) / float(np.spacing(o[s].max())) >= 1000.0
                continue
            assert e["valid"] == 1 and min(m["salience"], m["phase"], m["half"]) >= 4.0 and m["valid"] >= 1000.0, (case, kind, m)
            kinds.add(kind)
            if kind == "kicks120" and sr != 8000:
                assert abs(e["bpm"] - 120.0) < 0.6 and e["confidence"] > 0.9
            elif kind == "bursts150" and sr != 8000:
                assert abs(e["bpm"] - 150.0) < 0.75 and e["confidence"] > 0.9
            elif kind == "noise":
                assert e["confidence"] < 0.2
    assert kinds == {"kicks120", "bursts150", "noise"}
    assert [ref.lag_range(c[1], c[5]) for c in ref.GPU_CASES] == [(47, 126), (44, 126), (47, 254), (47, 281), (47, 126), (8, 46)]


def test_tempo_kernels_have_no_scratch():
    cols = kernel_usage("wf_hip_measure", "tempo_columns_kernel")
    rule = kernel_usage("wf_hip_measure", "tempo_read_kernel")
    assert len(cols) == 2 and len(rule) == 1, (cols, rule)  # one and two captured channels; the rule
    for name, r in {**cols, **rule}.items():
        print(name, r)
        assert r.get("ScratchSize [bytes/lane]") == 0 and r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
    for r in cols.values():
        assert r.get("LDS Size [bytes/block]") == 0 and r.get("VGPRs") <= 256, r  # the transforms' LDS is dynamic; two workgroups to a CU
    for r in rule.values():
        assert r.get("LDS Size [bytes/block]") <= 32768, r
