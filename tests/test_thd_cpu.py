"""Distortion analyser (WF_HIP_OUT_THD) without a device: the structured dtype against the C layout, the appended output number,
the host tables (wf::host::thd_tables, compiled into a program of their own) against the restatement (tests/thd_ref.py), analytic
truth on the restatement, the conditions of the device comparison on its own seeds and shapes, and a gfx950 compile of the read
kernels with no scratch, no spills and next to no static LDS."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import thd_ref as ref
from kernel_usage import kernel_usage

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "waveform_amd" / "csrc"


def test_thd_dtype_matches_the_c_layout(tmp_path):
    top = ("ch", "window", "reserved")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wf_hip.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %d %d %d %d %d", sizeof(wf_hip_thd), sizeof(wf_hip_thd_channel), (int)WF_HIP_OUT_THD, (int)WF_HIP_OUT_BITS,\n'
                   "         (int)WF_HIP_THD_MAX_WINDOW, (int)WF_HIP_THD_LOBE, (int)WF_HIP_THD_HARMONICS);\n"
                   + "".join(f'  printf(" %zu", offsetof(wf_hip_thd_channel, {n}));\n' for n in ref.FIELDS)
                   + "".join(f'  printf(" %zu", offsetof(wf_hip_thd, {n}));\n' for n in top) +
                   '  printf(" %zu %d", offsetof(wf_hip_thd, ch[1]), (int)WF_HIP_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    dt, ch = binding.THD_DTYPE, binding.THD_CHANNEL_DTYPE
    assert got == [dt.itemsize, ch.itemsize, binding.OUT_THD, binding.OUT_BITS, binding.THD_MAX_WINDOW, binding.THD_LOBE,
                   binding.THD_HARMONICS] + [ch.fields[n][1] for n in ref.FIELDS] + [dt.fields[n][1] for n in top] + [ch.itemsize, 13]
    assert dt.itemsize == 208 and ch.itemsize == 96 and dt.itemsize % 16 == 0
    assert dt == ref.THD_DTYPE and dt.names == top and ch == ref.THD_CHANNEL_DTYPE and ch.names == ref.FIELDS
    assert ref.FIELDS == ("fundamental_hz", "fundamental_db", "thd_db", "thdn_db", "snr_db", "noise_db", "sfdr_db", "spur_hz", "enob",
                          "harmonic_db", "fundamental_bin", "spur_bin", "harmonics", "valid", "reserved")
    assert [ch.fields[n][1] for n in ref.FIELDS] == [0, 8, 12, 16, 20, 24, 28, 32, 36, 40, 76, 80, 84, 88, 92]
    assert [dt.fields[n][1] for n in top] == [0, 192, 196]
    assert ch.fields["fundamental_hz"][0] == np.float64 and ch.fields["harmonic_db"][0].shape == (9,)
    assert ch.fields["harmonic_db"][0].base == np.float32 and dt.fields["reserved"][0].shape == (3,)
    assert (ref.MAX_WINDOW, ref.LOBE, ref.HARMONICS) == (binding.THD_MAX_WINDOW, binding.THD_LOBE, binding.THD_HARMONICS) == (8192, 8, 9)


# ---- the host tables ----------------------------------------------------------------------------------------------------------------

TABLE_SIZES = (512, 2064, 4096, 8192, 16384, 65536)  # fft sizes: P = 512, 2048, 4096, 8192, 8192, 8192

PROGRAM = r"""
#include <cstdio>
#include <initializer_list>
#include "wf_measure_tables.hpp"
using namespace wf::host;
int main() {
  for(unsigned n : {512u, 2064u, 4096u, 8192u, 16384u, 65536u}) {
    const ThdTables t = thd_tables(48000, n);
    if(t.P != thd_window(n) || t.tab.size() != 2 * (size_t)t.P || (1u << t.log2p) != t.P) return 2;
    const ThdTables u = thd_tables(44100, n);  // the sample rate changes nothing
    if(u.tab != t.tab || u.S != t.S) return 3;
    std::printf("T %u %u %u %.17g", n, t.P, t.log2p, t.S);
    for(double x : t.tab) std::printf(" %.17g", x);
    std::printf("\n");
  }
  return 0;
}
"""


def _build_and_run(directory, name, extra=()):
    src = directory / "thd_tables_main.cpp"
    src.write_text(PROGRAM)
    exe = directory / name
    subprocess.run(["g++", "-std=c++20", "-O2", *extra, "-I", str(CSRC), "-I", str(ROOT / "include"), str(src),
                    str(CSRC / "wf_measure_tables.cpp"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    text = _build_and_run(tmp_path_factory.mktemp("thd_tables"), "tables")
    out = {"text": text}
    for line in text.splitlines():
        f = line.split()
        assert f[0] == "T"
        out[int(f[1])] = (int(f[2]), int(f[3]), float(f[4]), np.array(f[5:], np.float64))
    assert sorted(k for k in out if k != "text") == sorted(TABLE_SIZES)
    return out


@pytest.mark.parametrize("n", TABLE_SIZES)
def test_thd_tables(tables, n):
    """P equal; the taper and S to 1e-15 relative, entry by entry (both sides sum the same long double terms); the twiddles to
    test_measure_tables_cpu.py's 1e-12"""
    p, log2p, s, tab = tables[n]
    assert p == ref.window_frames(n) and 1 << log2p == p and tab.size == 2 * p
    w = ref.taper(p)
    worst = float(np.max(np.abs(tab[:p] - w) / w))
    print(f"fft {n}: P {p}, S {s!r} against {ref.lobe_power(p)!r}, taper worst relative difference {worst:.3g}, w[0] {w[0]:.6g}")
    np.testing.assert_allclose(tab[:p], w, rtol=1e-15, atol=0)
    np.testing.assert_allclose(s, ref.lobe_power(p), rtol=1e-15, atol=0)
    assert np.all(w > 0) and abs(w[0] - 5.91e-8) < 1e-9 and abs(w[p // 2] - 1.0) < 1e-12  # the coefficients add up to 1
    x = 2.0 * np.pi * np.arange(p // 2, dtype=np.float64) / float(p)
    tw = tab[p:].reshape(p // 2, 2)
    np.testing.assert_allclose(tw[:, 0], np.cos(x), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(tw[:, 1], -np.sin(x), rtol=1e-12, atol=1e-15)
    assert tw[0, 0] == 1.0 and tw[0, 1] == 0.0


def test_the_tables_program_is_clean_under_the_sanitizers(tables, tmp_path):
    """the same program with -fsanitize=address,undefined, run directly: exit 0 and the same output"""
    text = _build_and_run(tmp_path, "tables_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert text == tables["text"]


def test_the_taper_is_a_minus_180_db_window():
    """side lobes below -175 dB of the main lobe beyond +-7 bins, seen on a transform sixteen times longer"""
    p = 512
    spec = np.abs(np.fft.rfft(ref.taper(p), 16 * p))
    db = 20.0 * np.log10(spec / spec[0] + 1e-300)
    print("highest side lobe beyond 7 bins:", db[7 * 16:].max(), "dB; at 8 bins and beyond:", db[8 * 16:].max())
    assert db[7 * 16:].max() < -175.0 and db[6 * 16] > -175.0


# ---- analytic truth on the restatement ----------------------------------------------------------------------------------------------

def test_a_tone_with_harmonics_and_noise():
    """P = 8192, 48 kHz: a 1 kHz sine of amplitude 0.5, H2 at -60 dBc, H3 at -70 dBc, white noise at -90 dBFS, seed 1"""
    p, sr = 8192, 48000
    x = ref.tone(np.arange(p, dtype=np.float64), 1000.0 / sr, np.random.default_rng(1)).astype(np.float32)
    r = ref.thd_one(x[None], p, sr)["ch"][0]
    print({n: r[n].tolist() for n in ref.FIELDS})
    assert r["valid"] == 1 and r["fundamental_bin"] == 171 and r["harmonics"] == 0x1ff
    assert abs(r["fundamental_db"] - 20.0 * np.log10(0.5)) <= 0.01
    assert abs(r["fundamental_hz"] - 1000.0) <= 0.01
    assert abs(r["harmonic_db"][0] + 60.0) <= 0.1
    assert abs(r["harmonic_db"][1] + 70.0) <= 0.2
    assert abs(r["noise_db"] + 90.0) <= 0.5
    # what follows from these: the spur is H2's peak bin, THD is the two harmonics, and the noise of a band of M bins is 3 dB
    # below its variance over the whole circle
    assert r["spur_bin"] == 341 and abs(r["spur_hz"] - 341 * sr / p) < 1e-2
    assert abs(r["thd_db"] - 10.0 * np.log10(1e-6 + 1e-7)) <= 0.1
    want_snr = 20.0 * np.log10(0.5) - 3.0103 + 90.0
    assert abs(r["snr_db"] - want_snr) <= 0.5 and abs(r["enob"] - (-float(r["thdn_db"]) - 1.76) / 6.02) < 1e-5
    assert abs(r["thdn_db"] - 10.0 * np.log10(1e-6 + 1e-7 + 10.0 ** (-want_snr / 10.0))) <= 0.2


def test_a_square_wave():
    """odd harmonics at 20 log10(1 / h) within 0.1 dB, even harmonics below -60 dBc.  Sampled at a period of 192 frames exactly:
    what aliases back then falls onto the odd harmonics, whose level is 1 / sin(pi h / 192) rather than 1 / (pi h / 192), 0.03 dB
    more at h = 9"""
    p, sr = 8192, 48000
    n = np.arange(p)
    x = np.where((n % 192) < 96, 0.4, -0.4).astype(np.float32)  # 250 Hz
    r = ref.thd_one(x[None], p, sr)["ch"][0]
    print({k: r[k].tolist() for k in ref.FIELDS})
    assert r["valid"] == 1 and abs(r["fundamental_hz"] - 250.0) <= 0.01 and r["harmonics"] == 0x1ff
    assert abs(r["fundamental_db"] - 20.0 * np.log10(0.4 * 4.0 / np.pi)) <= 0.01
    for h in range(2, 11):
        if h & 1:
            assert abs(r["harmonic_db"][h - 2] - 20.0 * np.log10(1.0 / h)) <= 0.1, h
        else:
            assert r["harmonic_db"][h - 2] < -60.0, h
    assert r["spur_bin"] == 128 and r["spur_hz"] == 750.0 and abs(r["sfdr_db"] - 20.0 * np.log10(3.0)) <= 0.5  # (one bin each)


def test_a_high_fundamental_sets_only_the_in_band_bits():
    p, sr = 4096, 48000
    rng = np.random.default_rng(2)
    n = np.arange(p, dtype=np.float64)
    for f, bits in ((11000.0, 0b1), (9700.0, 0b1), (7000.0, 0b11), (5000.0, 0b111), (12500.0, 0)):
        x = ref.tone(n, f / sr, rng, 0.5, -40.0, -50.0, -80.0).astype(np.float32)
        r = ref.thd_one(x[None], p, sr)["ch"][0]
        assert r["valid"] == 1 and r["harmonics"] == bits and abs(r["fundamental_hz"] - f) < 0.05, (f, r)
        for h in range(2, 11):
            in_band = int(np.floor(h * f * p / sr + 0.5)) + ref.LOBE <= p // 2 - 1
            assert bool(bits >> (h - 2) & 1) == in_band and np.isneginf(r["harmonic_db"][h - 2]) == (not in_band), (f, h)
        if bits & 1:
            assert abs(r["harmonic_db"][0] + 40.0) <= 0.1
        else:
            assert np.isneginf(r["thd_db"]) and np.isfinite(r["thdn_db"])
        assert not any(np.isnan(np.atleast_1d(r[k])).any() for k in ref.FLOAT_FIELDS)


def test_silence_and_a_nan_read_invalid():
    p, sr = 1024, 48000
    zero = np.zeros((), ref.THD_DTYPE)
    zero["window"] = p
    assert ref.thd_one(np.zeros((2, p), np.float32), p, sr).tobytes() == zero.tobytes()
    rng = np.random.default_rng(3)
    x = np.stack([ref.signal("tone", rng, p, p), ref.signal("sine", rng, p, p)])
    live = ref.thd_one(x, p, sr)
    assert live["ch"]["valid"].tolist() == [1, 1]
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[1, 517] = bad
        assert ref.thd_one(y, p, sr).tobytes() == zero.tobytes(), bad  # either channel's: the device shares one transform
        assert ref.thd_one(y[1:], p, sr).tobytes() == zero.tobytes(), bad
    y = x.copy()
    y[1] = 0.0  # a silent channel next to a live one: exact silence
    r = ref.thd_one(y, p, sr)
    assert r["ch"][0].tobytes() == live["ch"][0].tobytes() and r["ch"][1].tobytes() == zero["ch"][1].tobytes()
    assert ref.window_frames(511) == 256 and ref.window_frames(2064) == 2048 and ref.window_frames(65536) == 8192


def test_only_the_newest_frames_count():
    sr, w = 44100, 2064
    rng = np.random.default_rng(4)
    x = np.stack([ref.signal("tone", rng, 3000, 2048), ref.signal("square", rng, 3000, 2048)])
    older = x.copy()
    older[:, :3000 - 2048] = 7.0
    a = ref.thd(x[None], w, sr)
    assert a.tobytes() == ref.thd(older[None], w, sr).tobytes() == ref.thd(x[None, :, 3000 - 2048:], w, sr).tobytes()
    assert a["window"][0] == 2048 and a["ch"]["valid"].tolist() == [[1, 1]]


def test_mismatches_applies_the_bound():
    rng = np.random.default_rng(5)
    x = np.stack([np.stack([ref.signal(a, rng, 1024, 1024), ref.signal(b, rng, 1024, 1024)]) for a, b in (("tone", "high"), ("sine", "silence"))])
    want = ref.thd(x, 1024, 48000)
    assert ref.mismatches(want, want) == [] and np.isneginf(want["ch"]["harmonic_db"][0, 1, 1])
    for name in ref.FLOAT_FIELDS:
        where = (0, 0, 0) if name == "harmonic_db" else (0, 0)
        got = want.copy()
        f = got["ch"][name]
        f[where] = np.nextafter(f[where], np.float32(1e9))  # one ulp: inside
        assert ref.mismatches(got, want) == [], name
        f[where] = f[where] + max(3.0 * float(np.spacing(np.abs(f[where]))), 3e-6)  # three: outside
        assert [m[0] for m in ref.mismatches(got, want)] == ["ch." + name]
    for name in ref.UINT_FIELDS:
        got = want.copy()
        got["ch"][name][1, 0] += 1
        assert [m[0] for m in ref.mismatches(got, want)] == ["ch." + name]
    for name in ("window", "reserved"):
        got = want.copy()
        got[name][1] += 1
        assert {m[0] for m in ref.mismatches(got, want)} == {name}
    got = want.copy()
    got["ch"]["fundamental_hz"][0, 0] *= 1.0 + 1e-10
    assert ref.mismatches(got, want) == []
    got["ch"]["fundamental_hz"][0, 0] *= 1.0 + 1e-8
    assert [m[0] for m in ref.mismatches(got, want)] == ["ch.fundamental_hz"]
    got = want.copy()
    got["ch"]["harmonic_db"][0, 1, 1] = -400.0  # an infinity is matched by an infinity alone
    assert [m[0] for m in ref.mismatches(got, want)] == ["ch.harmonic_db"]
    got = want.copy()
    got["ch"]["thd_db"][0, 0] = np.nan
    assert [m[0] for m in ref.mismatches(got, want)] == ["ch.thd_db"]
    assert ref.mismatches(want[:1], want)[0][0] == "shape"


def test_the_radix2_transform_is_a_transform():
    rng = np.random.default_rng(6)
    for n in (8, 512, 8192):
        z = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        assert np.max(np.abs(ref.fft_radix2(z) - np.fft.fft(z))) < 1e-10 * np.sqrt(n)


# ---- the conditions of the device comparison ----------------------------------------------------------------------------------------

def test_the_gpu_cases_meet_the_conditions_of_the_bound():
    """on the very seeds and shapes of tests/test_gpu_thd.py: for every valid channel the runner-up of each argmax (k0 and k_s)
    lies at least 1e-6 relative below the winner, every h f0 is at least 1e-6 from a half-integer, and numpy.fft and the radix-2
    transform agree on every dB field to 1e-7 dB; the window the device reads wraps the ring.  With these, one float32 rounding is
    all that can separate the device from the restatement, for every entry of every case"""
    seen, windows = set(), []
    for case in ref.GPU_CASES:
        fft, sr, kw, w, channels = case
        if kw.get("meter"):
            assert w == int(sr * (kw["meter_ms"] / 1000.0)) & -16 == 2208
        else:
            assert w == fft
        p = ref.window_frames(w)
        windows.append(p)
        x = ref.case_audio(case)
        ring = ref.ring_frames(w)
        assert x.shape == (len(ref.STREAM_KINDS), channels, ring + p // 2 + 3) and 3 <= x.shape[0] <= 7 and x.shape[-1] % 4 != 0
        assert (x.shape[-1] - p) % ring + p > ring  # the window wraps the ring
        a, b = ref.thd(x, w, sr), ref.thd(x, w, sr, ref.fft_radix2)
        assert ref.mismatches(b, a) == []
        for s, pair in enumerate(ref.STREAM_KINDS):
            for c, kind in enumerate(pair[:channels]):
                r, vals = ref.analyse(x[s, c, -p:], sr)
                _, other = ref.analyse(x[s, c, -p:], sr, ref.fft_radix2)
                assert r.tobytes() == a["ch"][s, c].tobytes()
                seen.add(kind)
                if kind == "silence":
                    assert r["valid"] == 0 and not r.tobytes().strip(b"\0") and not vals
                    continue
                assert r["valid"] == 1
                worst = 0.0
                for name in ref.DB_FIELDS:
                    u, v = np.atleast_1d(vals[name]), np.atleast_1d(other[name])
                    assert np.array_equal(np.isinf(u), np.isinf(v)) and not np.isnan(u).any(), (case, kind, name)
                    fin = np.isfinite(u)
                    if fin.any():
                        worst = max(worst, float(np.max(np.abs(u[fin] - v[fin]))))
                print(f"{ref.case_id(case)} stream {s} ch {c} {kind}: P {p}, k0 {int(r['fundamental_bin'])} (f0 {vals['f0_bins']:.4f} bins, "
                      f"{float(r['fundamental_hz']):.3f} Hz), {float(r['fundamental_db']):.3f} dB, thd {float(r['thd_db']):.2f}, thd+n "
                      f"{float(r['thdn_db']):.2f}, noise {float(r['noise_db']):.2f}, spur bin {int(r['spur_bin'])}, sfdr "
                      f"{float(r['sfdr_db']):.2f}, harmonics {int(r['harmonics']):#05x}; margins k0 {vals['margin_k0']:.3g}, k_s "
                      f"{vals['margin_ks']:.3g}, half-integer {vals['margin_half']:.3g}; two orderings {worst:.3g} dB")
                assert vals["margin_k0"] >= 1e-6 and vals["margin_ks"] >= 1e-6, (case, kind)
                assert vals["margin_half"] >= 1e-6, (case, kind)
                assert worst <= 1e-7, (case, kind, worst)
                assert other["harmonic_bins"] == vals["harmonic_bins"]
                if kind == "tone":
                    # (the noise estimate averages M - 100 bins or so, 2.6 of them -- the taper's noise bandwidth -- to one
                    # independent draw of an exponential distribution, 4.34 dB each: four standard deviations)
                    assert r["harmonics"] == 0x1ff and abs(r["harmonic_db"][0] + 60.0) < 0.5
                    assert abs(r["noise_db"] + 90.0) < 4.0 * 4.34 / np.sqrt((p // 2 - 100) / 2.6)
                elif kind == "square":
                    assert r["harmonics"] == 0x1ff and abs(r["harmonic_db"][1] - 20.0 * np.log10(1.0 / 3.0)) < 0.5
                elif kind == "sine":
                    assert r["thdn_db"] < -130.0  # the float32 quantisation floor
                elif kind == "high":
                    assert r["harmonics"] == 0b1 and r["fundamental_hz"] > sr / 5 and abs(r["harmonic_db"][0] + 40.0) < 0.5
    assert seen == set(ref.KINDS)
    assert windows == [512, 2048, 8192, 8192, 2048, 4096, 1024]
    assert [ref.case_id(c) for c in ref.GPU_CASES] == ["w512_sr48000", "w2064_sr44100", "w8192_sr96000", "w16384_sr48000",
                                                       "w2208_sr48000_meter1", "w4096_sr48000_capture_channels1_stereo0",
                                                       "w1024_sr48000_stereo0"]


def test_thd_kernels_have_no_scratch():
    res = kernel_usage("wf_hip_measure", "thd_read_kernel")
    assert len(res) == 2, res  # one and two captured channels
    for name, r in res.items():
        print(name, r)
        assert r.get("ScratchSize [bytes/lane]") == 0 and r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
        assert r.get("LDS Size [bytes/block]") <= 1024, (name, r)  # the cross-wave hand-over; the transform's LDS is dynamic
