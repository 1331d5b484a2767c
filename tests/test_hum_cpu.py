"""The mains hum detector (WF_HIP_OUT_HUM) without a device: the structured dtype against the C layout, the appended output number,
the library's own plan and tables against the restatement (tests/hum_ref.py), the polyphase
form of the spectrum against numpy's windowed FFT, what the restatement reads on the issue's cases, the clearance of every window
of the device comparison, and a gfx950 compile of the kernel with no scratch and no spills.

What the restatement read here when the bounds below were written (each bound is twice the worst seen; 30 seeds per plan, lines at
-40 / -46 / -43 / -52 dBFS on harmonics 1, 2, 3, 5 of 50 or 60 +- 0.2 Hz under white noise at -40 dBFS): the right family and
exactly those four lines in every seed; mains_hz within 0.0265 Hz at 48000 / 16384, 0.0104 at 48000 / 32768, 0.0097 at
44100 / 32768, 0.0159 at 96000 / 32768, 0.0111 at 32000 / 16384 and 0.0222 at 16000 / 8192; levels within 1.33, 0.72, 1.18, 0.66,
1.19 and 1.42 dB.  White noise alone (200 seeds per plan) and pink noise at -30 dBFS (50 per plan) found nothing.  Noise-free
six-line combs at 49.83, 50.0, 50.17, 59.8 and 60.21 Hz: mains_hz within 1.6e-5 Hz, levels within 7.8e-4 dB and hum_db within
4.7e-5 dB at every plan.  Bass notes of four harmonics at 48.999, 51.913, 58.270 and 61.735 Hz read family 0; with six harmonics
the 6th of 58.27 Hz (349.6 Hz) reads as a lone 7th of 50 Hz, which is the rule and not an accident."""
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import hum_ref as ref
from kernel_usage import kernel_usage

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "waveform_amd" / "csrc"
# the issue's table: (sample rate, ring) -> (D, N, M), and the bounds on mains_hz and the levels of the hum under noise
PLANS = {(48000, 16384): (32, 16384, 512), (48000, 32768): (32, 32768, 1024), (48000, 1 << 17): (32, 32768, 1024),
         (44100, 32768): (32, 32768, 1024), (96000, 32768): (64, 32768, 512), (32000, 16384): (16, 16384, 1024),
         (16000, 8192): (8, 8192, 1024)}
BOUNDS = {(48000, 16384): (0.053, 2.66), (48000, 32768): (0.021, 1.45), (44100, 32768): (0.0194, 2.37), (96000, 32768): (0.0318, 1.33),
          (32000, 16384): (0.0222, 2.39), (16000, 8192): (0.0445, 2.85)}
SIX = {1: -30.0, 2: -40.0, 3: -36.0, 4: -50.0, 5: -44.0, 6: -56.0}
CHANNEL_FIELDS = ("mains_hz", "hum_db", "total_db", "ratio_db", "odd_db", "even_db", "noise_db", "valid", "family", "lines", "mask", "hz",
                  "level_db", "snr_db", "reserved")


def test_hum_dtype_matches_the_c_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wf_hip.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %d %d %d %g %g %d %d %d", sizeof(wf_hip_hum), sizeof(wf_hip_hum_channel), (int)WF_HIP_OUT_HUM,\n'
                   "         (int)WF_HIP_OUT_TEMPO, (int)WF_HIP_HUM_HARMONICS, (double)WF_HIP_HUM_MARGIN_DB, (double)WF_HIP_HUM_TOL_HZ,\n"
                   "         (int)WF_HIP_HUM_FLOOR_SPAN, (int)WF_HIP_HUM_FLOOR_GUARD, (int)WF_HIP_HUM_MAX_WINDOW);\n"
                   + "".join(f'  printf(" %zu", offsetof(wf_hip_hum_channel, {n}));\n' for n in CHANNEL_FIELDS)
                   + "".join(f'  printf(" %zu", offsetof(wf_hip_hum, {n}));\n' for n in ref.FIELDS) +
                   '  printf(" %d", (int)WF_HIP_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [float(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    dt, ch = binding.HUM_DTYPE, binding.HUM_CHANNEL_DTYPE
    assert got == [dt.itemsize, ch.itemsize, binding.OUT_HUM, binding.OUT_TEMPO, binding.HUM_HARMONICS, binding.HUM_MARGIN_DB, binding.HUM_TOL_HZ,
                   binding.HUM_FLOOR_SPAN, binding.HUM_FLOOR_GUARD, binding.HUM_MAX_WINDOW] \
        + [ch.fields[n][1] for n in CHANNEL_FIELDS] + [dt.fields[n][1] for n in ref.FIELDS] + [13]
    assert (dt.itemsize, ch.itemsize) == (304, 144) and dt.itemsize % 16 == 0
    assert dt == ref.HUM_DTYPE and ch == ref.CHANNEL_DTYPE and ch.names == CHANNEL_FIELDS == ref.CHANNEL_FIELDS and dt.names == ref.FIELDS
    assert (ref.HARMONICS, ref.MARGIN_DB, ref.TOL_HZ, ref.FLOOR_SPAN, ref.FLOOR_GUARD, ref.MAX_WINDOW) == \
        (binding.HUM_HARMONICS, binding.HUM_MARGIN_DB, binding.HUM_TOL_HZ, binding.HUM_FLOOR_SPAN, binding.HUM_FLOOR_GUARD,
         binding.HUM_MAX_WINDOW) == (8, 15.0, 0.5, 20, 3, 32768)


# ---- the host's builder ---------------------------------------------------------------------------------------------------------

PROGRAM = r"""
#include <cstdio>
#include <initializer_list>
#include "wf_measure_tables.hpp"
using namespace wf::host;
int main() {
  for(unsigned sr : {1000u, 2000u, 2560u, 8000u, 16000u, 22050u, 32000u, 40960u, 44100u, 48000u, 88200u, 96000u, 98304u, 98305u, 192000u})
    for(unsigned ring : {2048u, 4096u, 8192u, 16384u, 32768u, 131072u}) {
      const HumPlan p = hum_plan(sr, ring);
      const HumTables t = hum_tables(sr, ring);
      if(t.plan.N != p.N || t.plan.K != p.K || t.plan.served() != p.served()) return 2;
      std::printf("%u %u %d %d %u %u %u %u %u %u %u %.17g", sr, ring, (int)p.served(), (int)p.too_fast(), p.D, p.N, p.M, p.log2m, p.K, p.noise_lo,
                  p.noise_hi, p.hz);
      for(unsigned i = 0; i < 16; ++i) std::printf(" %u %u", p.lo[i], p.hi[i]);
      std::printf(" %zu %zu %zu", t.tw.size(), t.comb.size(), t.ranges.size());
      // a checksum of the tables against the restatement: the twiddle of m = 3, and W_N^(r k) at (r, k) = (D - 1, -1) and (D - 1, K)
      if(p.served()) {
        const size_t bins = p.K + 2, last = (size_t)(p.D - 1) * bins;
        std::printf(" %.17g %.17g %.17g %.17g %.17g %.17g", t.tw[6], t.tw[7], t.comb[2 * last], t.comb[2 * last + 1], t.comb[2 * (last + bins - 1)],
                    t.comb[2 * (last + bins - 1) + 1]);
        for(unsigned i = 0; i < 16; ++i) if(t.ranges[i] != p.lo[i] || t.ranges[16 + i] != p.hi[i]) return 3;
      }
      std::printf("\n");
    }
  return 0;
}
"""


def test_the_plan_and_the_tables_of_the_library(tmp_path):
    """wf::host::hum_plan and hum_tables, compiled into a program of their own under the address and undefined-behaviour sanitizers,
    against the restatement: every integer exactly, hz exactly, the tables' sizes, and three of their entries to 1e-15"""
    src = tmp_path / "hum_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "hum_tables"
    subprocess.run(["g++", "-std=c++20", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(CSRC),
                    "-I", str(ROOT / "include"), str(src), str(CSRC / "wf_measure_tables.cpp"), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == 15 * 6
    seen = {}
    for line in lines:
        f = line.split()
        sr, ring, served, too_fast, D, N, M, log2m, K, nlo, nhi = (int(v) for v in f[:11])
        pl = ref.plan(sr, ring)
        assert bool(served) == pl.served, line[:40]
        assert bool(too_fast) == (sr < 2560 or sr > 3 * 32768), line[:40]
        seen[(sr, ring)] = (D, N, M) if served else None
        if not served:
            assert [int(v) for v in f[44:47]] == [0, 0, 0]
            continue
        assert (D, N, M, K, nlo, nhi) == (pl.D, pl.N, pl.M, pl.K, pl.noise_lo, pl.noise_hi) and 1 << log2m == M and float(f[11]) == pl.hz
        assert M in (512, 1024) and D >= 2 and 1280 <= sr / D < 2560 and pl.hz <= 3.0 and K + 1 < M // 2, line[:40]
        rng = [int(v) for v in f[12:44]]
        for i in range(16):
            fam, h = ref.FAMILIES[i // 8], 1 + i % 8
            lo, hi = pl.search(fam, h)
            assert (rng[2 * i], rng[2 * i + 1]) == (lo, hi), (line[:40], fam, h)
            # the issue's formulas in floating point, where they are not within rounding of a whole number
            a, b = h * (fam - 0.5) / pl.hz - 0.5, h * (fam + 0.5) / pl.hz + 0.5
            if abs(a - round(a)) > 1e-9:
                assert lo == max(math.ceil(a), 6)
            if abs(b - round(b)) > 1e-9:
                assert hi == math.floor(b)
            assert hi + ref.FLOOR_SPAN < K and lo >= 6
        assert [int(v) for v in f[44:47]] == [M, 2 * D * (K + 2), 32]
        want = [math.cos(2 * math.pi * 3 / M), -math.sin(2 * math.pi * 3 / M)]
        for k in (-1, K):
            ang = 2 * math.pi * (((D - 1) * k) % N) / N
            want += [math.cos(ang), -math.sin(ang)]
        np.testing.assert_allclose([float(v) for v in f[47:53]], want, rtol=0, atol=1e-15)
    for key, dnm in PLANS.items():
        if key in seen:
            assert seen[key] == dnm, key
    assert seen[(48000, 8192)] is None and seen[(192000, 32768)] is None and seen[(192000, 131072)] is None  # the issue's refusals
    assert seen[(1000, 4096)] is None and seen[(2000, 4096)] is None and seen[(98305, 32768)] is None and seen[(98304, 32768)] == (64, 32768, 512)


def test_the_restatement_of_the_plan_reads_the_issues_table():
    for (sr, ring), (D, N, M) in PLANS.items():
        pl = ref.plan(sr, ring)
        assert (pl.D, pl.N, pl.M, pl.served) == (D, N, M, True) and pl.K == math.ceil(8 * 60.5 / pl.hz) + 22
    assert round(ref.plan(48000, 16384).hz, 2) == 2.93 and round(ref.plan(48000, 32768).hz, 2) == 1.46
    assert not ref.plan(48000, 8192).served and round(ref.plan(48000, 8192).hz, 1) == 5.9 and not ref.plan(192000, 32768).served
    # no equal-tempered note at A = 440 Hz lies within 0.5 Hz of 50 or 60 Hz
    notes = 440.0 * 2.0 ** (np.arange(-60, 40) / 12.0)
    assert np.min(np.abs(notes[:, None] - np.array([50.0, 60.0]))) > ref.TOL_HZ


@pytest.mark.parametrize("sr,ring", [(16000, 8192), (48000, 16384), (48000, 32768), (96000, 32768)], ids=["D8", "D32", "D32-M1024", "D64"])
def test_the_polyphase_form_is_the_windowed_transform(sr, ring):
    """bins 0 .. K - 1 from D / 2 paired M-point transforms, the combination twiddles and the Hann window across frequency, against
    numpy's FFT of the N frames through the window: 1e-12 of the largest bin"""
    pl = ref.plan(sr, ring)
    assert pl.D == {"16000": 8, "48000": 32, "96000": 64}[str(sr)]
    x = ref.comb(np.random.default_rng(sr + ring), 50.1, ref.LEVELS, pl.N, sr, -40.0)
    a, b = ref.spectrum(x, pl), ref.polyphase(x, pl)
    assert a.shape == b.shape == (pl.K,)
    assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(a))
    # a sine of amplitude A at a bin centre reads |H| = A
    n = np.arange(pl.N)
    s = (0.25 * np.sin(2 * np.pi * 40 * n / pl.N + 0.3)).astype(np.float32)
    assert abs(abs(ref.spectrum(s, pl)[40]) - 0.25) < 1e-7


# ---- what the restatement reads -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sr,ring", list(BOUNDS), ids=[f"{s}-{r}" for s, r in BOUNDS])
def test_hum_under_noise_is_found_and_noise_alone_finds_nothing(sr, ring):
    pl = ref.plan(sr, ring)
    bound_hz, bound_db = BOUNDS[(sr, ring)]
    worst_hz = worst_db = 0.0
    for seed in range(30):
        rng = np.random.default_rng(seed)
        fam = (50, 60)[seed & 1]
        f0 = fam + rng.uniform(-0.2, 0.2)
        e = ref.channel(ref.comb(rng, f0, ref.LEVELS, pl.N, sr, -40.0), sr, ring)
        assert (e["valid"], e["family"], e["mask"], e["lines"]) == (1, fam, 0b10111, 4), (seed, e["family"], bin(e["mask"]))
        worst_hz = max(worst_hz, abs(e["mains_hz"] - f0))
        worst_db = max(worst_db, max(abs(e["level_db"][h - 1] - level) for h, level in ref.LEVELS.items()))
        assert abs(e["ratio_db"] - (e["hum_db"] - e["total_db"])) < 1e-12 and np.all(e["snr_db"][[0, 1, 2, 4]] >= ref.MARGIN_DB)
        assert not np.any(e["hz"][[3, 5, 6, 7]]) and not np.any(e["level_db"][[3, 5, 6, 7]]) and not np.any(e["snr_db"][[3, 5, 6, 7]])
    print(f"{sr} / {ring}: mains_hz within {worst_hz:.4f} Hz, levels within {worst_db:.2f} dB")
    assert worst_hz <= bound_hz and worst_db <= bound_db
    for seed in range(200):
        e = ref.channel(ref.noise(np.random.default_rng(1000 + seed), -40.0, pl.N), sr, ring)
        assert e["valid"] == 1 and e["family"] == 0 and e["lines"] == 0 and e["mask"] == 0, seed
        assert not any(np.any(e[n]) for n in ("mains_hz", "hum_db", "ratio_db", "odd_db", "even_db", "hz", "level_db", "snr_db"))
        # white noise of rms s has 6 s^2 / N in every bin of |H|^2: the floor reads it within a dB or two
        assert abs(e["noise_db"] - 10.0 * math.log10(6.0 * 1e-4 / pl.N)) < 2.0 and abs(e["total_db"] + 40.0) < 0.5
    for seed in range(50):
        e = ref.channel(ref.pink(np.random.default_rng(2000 + seed), -30.0, pl.N), sr, ring)
        assert e["family"] == 0, seed


@pytest.mark.parametrize("sr,ring", list(BOUNDS), ids=[f"{s}-{r}" for s, r in BOUNDS])
def test_noise_free_combs_and_the_edge_cases(sr, ring):
    pl = ref.plan(sr, ring)
    hum_db = 10.0 * math.log10(sum(10.0 ** (level / 10.0) / 2.0 for level in SIX.values()))
    for f0 in (49.83, 50.0, 50.17, 59.8, 60.21):
        e = ref.channel(ref.comb(np.random.default_rng(int(f0 * 100)), f0, SIX, pl.N, sr), sr, ring)
        assert (e["family"], e["mask"], e["lines"]) == (round(f0 / 10) * 10, 0b111111, 6), f0
        assert abs(e["mains_hz"] - f0) <= 3.2e-5 and abs(e["hum_db"] - hum_db) <= 9.4e-5, (f0, e["mains_hz"], e["hum_db"])
        assert max(abs(e["level_db"][h - 1] - level) for h, level in SIX.items()) <= 1.6e-3, f0
        assert np.allclose(e["hz"][:6], f0, rtol=0, atol=1e-3)
    # bass notes beside the mains: G1, G#1, A#1 and B1 with four harmonics are no hum ...
    for f in (48.999, 51.913, 58.270, 61.735):
        x = ref.comb(np.random.default_rng(int(f * 10)), f, {h: -20.0 - 6.0 * h for h in range(1, 5)}, pl.N, sr, -60.0)
        assert ref.channel(x, sr, ring)["family"] == 0, f
    # ... but the 6th harmonic of A#1, 349.6 Hz, is 0.06 Hz from the 7th of 50 Hz: a lone line, by the rule
    x = ref.comb(np.random.default_rng(582), 58.270, {h: -20.0 - 6.0 * h for h in range(1, 7)}, pl.N, sr, -60.0)
    e = ref.channel(x, sr, ring)
    assert (e["family"], e["mask"]) == (50, 1 << 6)
    # a comb without its fundamental
    e = ref.channel(ref.comb(np.random.default_rng(5), 50.05, ref.NO_FUNDAMENTAL, pl.N, sr, -60.0), sr, ring)
    assert (e["family"], e["mask"], e["lines"]) == (50, 0b101110, 4) and abs(e["mains_hz"] - 50.05) < 0.005
    assert e["hz"][0] == 0 and e["odd_db"] != 0 and e["even_db"] != 0
    # a lone 300 Hz line is the 6th of 50 Hz and the 5th of 60 Hz alike: 50, by the tie rule
    e = ref.channel(ref.comb(np.random.default_rng(6), 300.0, {1: -40.0}, pl.N, sr, -60.0), sr, ring)
    assert (e["family"], e["mask"], e["lines"]) == (50, 1 << 5, 1) and abs(e["mains_hz"] - 50.0) < 0.005
    assert e["odd_db"] == 0.0 and abs(e["even_db"] + 43.01) < 0.1 and abs(e["level_db"][5] + 40.0) < 0.1
    # 50 Hz with a weaker 60 Hz comb reads 50
    rng = np.random.default_rng(7)
    x = ref.comb(rng, 50.0, ref.LEVELS, pl.N, sr, -60.0) + ref.comb(rng, 60.0, {h: level - 10.0 for h, level in ref.LEVELS.items()}, pl.N, sr)
    e = ref.channel(x, sr, ring)
    assert e["family"] == 50 and e["mask"] & 0b10111 == 0b10111 and abs(e["mains_hz"] - 50.0) < 0.01
    # silence, a NaN and an infinity
    for bad in (np.zeros(pl.N, np.float32), np.where(np.arange(pl.N) == 7, np.nan, x).astype(np.float32),
                np.where(np.arange(pl.N) == pl.N - 1, np.inf, x).astype(np.float32)):
        e = ref.channel(bad, sr, ring)
        assert not any(np.any(v) for v in e.values())
    assert ref.fresh(2, sr, ring)["window"].tolist() == [pl.N, pl.N] and not ref.fresh(2, sr, ring)["ch"]["valid"].any()


def test_what_it_cannot_do():
    """white noise at -30 dBFS over a -50 dBFS hum at N = 16384: the lines stand 4 dB over the floor's density, and most are missed"""
    sr, ring = 48000, 16384
    pl = ref.plan(sr, ring)
    full = sum(ref.channel(ref.comb(np.random.default_rng(s), 50.0, {h: level - 10.0 for h, level in ref.LEVELS.items()}, pl.N, sr, -30.0),
                           sr, ring)["mask"] == 0b10111 for s in range(20))
    assert full == 0


# ---- the conditions of the device comparison ------------------------------------------------------------------------------------

def test_the_gpu_windows_have_clearance():
    """every window tests/test_gpu_hum.py and tests/hum_wrap_child.py read: each candidate line, accepted or rejected, stands at
    least 3 dB from the 15 dB margin, so no rounding of the device moves an integer field"""
    worst = math.inf
    names = set()
    for name, sr, ring, x in ref.gpu_windows():
        assert ref.plan(sr, ring).served and x.shape[-1] >= ref.plan(sr, ring).N
        for s in range(x.shape[0]):
            for c in range(x.shape[1]):
                cl = ref.clearance(x[s, c], sr, ring)
                assert cl >= 3.0, (name, s, c, cl)
                worst = min(worst, cl)
        names.add(name.split()[0])
    print(f"the nearest candidate stands {worst:.2f} dB from the margin")
    assert {"stagger", "s16", "synth", "wrap"} <= names and len(names) == 4 + 2 * len(ref.GPU_PLANS)


def test_mismatches_applies_the_bound():
    sr, ring = ref.SR, ref.RING
    x = ref.case_audio(sr, ring, 2)
    want = ref.hum(x, sr, ring)
    assert ref.mismatches(want, x, sr, ring) == []
    exact = ref.channel(x[0, 0], sr, ring)
    for name in ref.CHANNEL_FLOATS + ref.CHANNEL_ARRAYS:
        got = want.copy()
        f = got["ch"][name]
        where = (0, 0, 0) if f.ndim == 3 else (0, 0)
        w = float(np.atleast_1d(exact[name])[0])
        # the float32 on the other side of the float64 value: within one rounding of it
        f[where] = np.nextafter(f[where], np.float32(np.inf if float(f[where]) <= w else -np.inf))
        assert ref.mismatches(got, x, sr, ring) == [], name
        f[where] += 3 * np.spacing(np.abs(f[where])) + np.float32(3e-9)
        assert [m[0] for m in ref.mismatches(got, x, sr, ring)] == [name], name
    for name in ref.CHANNEL_UINTS + ("reserved",):
        got = want.copy()
        got["ch"][name][2, 1] += 1
        assert [m[:3] for m in ref.mismatches(got, x, sr, ring)] == [(name, 2, 1)]
    for name in ("window", "decimation", "reserved", "resolution_hz"):
        got = want.copy()
        got[name][1] += 1
        assert [m[0] for m in ref.mismatches(got, x, sr, ring)] == [name]
    got = want.copy()
    got["ch"]["mains_hz"][1, 0] = np.nan
    assert [m[0] for m in ref.mismatches(got, x, sr, ring)] == ["mains_hz"]
    assert ref.mismatches(want[:1], x, sr, ring)[0][0] == "shape"
    mono = ref.hum(x[:, :1], sr, ring)
    assert ref.mismatches(mono, x[:, :1], sr, ring) == [] and not mono["ch"][:, 1].tobytes().strip(b"\0")


def test_hum_kernel_has_no_scratch():
    use = kernel_usage("wf_hip_measure", "hum_read_kernel")
    assert len(use) == 1, use  # one kernel for one and two captured channels: the grid's second dimension is the channel
    for name, r in use.items():
        print(name, r)
        assert r.get("ScratchSize [bytes/lane]") == 0 and r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
        assert r.get("VGPRs") <= 256 and r.get("LDS Size [bytes/block]") <= 2048, r  # the hand-overs; the rest is dynamic
