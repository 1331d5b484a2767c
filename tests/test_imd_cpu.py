"""Two-tone intermodulation analyser (WF_HIP_OUT_IMD) without a device: the structured dtype against the C layout, the appended
output number, closed forms of a polynomial non-linearity on the restatement
(tests/imd_ref.py), its behaviour on one tone, silence, an octave and products beyond the band, the conditions of the device
comparison on its own seeds and shapes, and a gfx950 compile of the read kernels with no scratch, no spills and next to no static
LDS."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from waveform_amd import binding
import imd_ref as ref
from kernel_usage import kernel_usage

ROOT = Path(__file__).resolve().parents[1]


def test_imd_dtype_matches_the_c_layout(tmp_path):
    top = ("ch", "window", "reserved")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wf_hip.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %d %d %d %g", sizeof(wf_hip_imd), sizeof(wf_hip_imd_channel), (int)WF_HIP_OUT_IMD, (int)WF_HIP_OUT_CLICK,\n'
                   "         (int)WF_HIP_IMD_PRODUCTS, (double)WF_HIP_IMD_MIN_RATIO);\n"
                   + "".join(f'  printf(" %zu", offsetof(wf_hip_imd_channel, {n}));\n' for n in ref.FIELDS)
                   + "".join(f'  printf(" %zu", offsetof(wf_hip_imd, {n}));\n' for n in top) +
                   '  printf(" %zu %d", offsetof(wf_hip_imd, ch[1]), (int)WF_HIP_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [float(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    dt, ch = binding.IMD_DTYPE, binding.IMD_CHANNEL_DTYPE
    assert got == [dt.itemsize, ch.itemsize, binding.OUT_IMD, binding.OUT_CLICK, binding.IMD_PRODUCTS, binding.IMD_MIN_RATIO] \
        + [ch.fields[n][1] for n in ref.FIELDS] + [dt.fields[n][1] for n in top] + [ch.itemsize, 13]
    assert dt.itemsize == 368 and ch.itemsize == 176 and dt.itemsize % 16 == 0
    assert dt == ref.IMD_DTYPE and dt.names == top and ch == ref.IMD_CHANNEL_DTYPE and ch.names == ref.FIELDS
    assert ref.FIELDS == ("lo_hz", "hi_hz", "lo_db", "hi_db", "ratio_db", "imd_db", "order_db", "dfd2_db", "dfd3_db", "mod_db", "tdn_db",
                          "noise_db", "product_db", "lo_bin", "hi_bin", "products", "tones", "valid", "reserved")
    assert [ch.fields[n][1] for n in ref.FIELDS] == [0, 8, 16, 20, 24, 28, 32, 48, 52, 56, 60, 64, 68, 148, 152, 156, 160, 164, 168]
    assert [dt.fields[n][1] for n in top] == [0, 352, 356]
    assert ch.fields["lo_hz"][0] == np.float64 and ch.fields["hi_hz"][0] == np.float64
    assert ch.fields["product_db"][0].shape == (20,) and ch.fields["order_db"][0].shape == (4,) and ch.fields["reserved"][0].shape == (2,)
    assert ch.fields["product_db"][0].base == np.float32 and dt.fields["reserved"][0].shape == (3,)
    assert (ref.PRODUCTS, ref.MIN_RATIO, ref.LOBE) == (binding.IMD_PRODUCTS, binding.IMD_MIN_RATIO, binding.THD_LOBE) == (20, 1e-3, 8)


def test_the_products_are_enumerated_as_the_definition_says():
    terms = ref.PRODUCT_TERMS
    assert terms[:6] == ((2, 1, 1, -1), (2, 1, 1, 1), (3, 1, 2, -1), (3, 1, 2, 1), (3, 2, 1, -1), (3, 2, 1, 1))
    assert terms[18:] == ((5, 4, 1, -1), (5, 4, 1, 1)) and [t[0] for t in terms] == [2] * 2 + [3] * 4 + [4] * 6 + [5] * 8
    assert all(m + n == o for o, m, n, _ in terms) and ref.MOD_PRODUCTS == (0, 1, 2, 3, 6, 7, 12, 13)


# ---- closed forms on the restatement ------------------------------------------------------------------------------------------------

A2, A3, SR = 2e-3, 1e-3, 48000
# (f_lo, f_hi in Hz at 48 kHz, A_lo, A_hi, the windows it fits: both tones at least 17 bins up).  No product that is measured
# shares a bin with another product, a harmonic or what aliases back: 19 + 20 kHz measures 1, 18 and 21 kHz (the sums 39 and 58 kHz
# lie beyond the band), 250 Hz + 8 kHz the sidebands of 8 kHz, 1.1 + 7 kHz 5.9, 8.1, 4.8, 9.2, 12.9 and 15.1 kHz with the harmonics at
# 2.2, 3.3 and 14 kHz at least 400 Hz from every region that is summed -- 34 bins at P = 4096, but fewer than the 16 two regions need
# at P = 1024, where 1 + 7 kHz, whose |f_hi - 4 f_lo| lies on 3 f_lo, read 0.02 dB off
PAIRS = [(19000.0, 20000.0, 0.4, 0.4, (1024, 4096, 8192)), (250.0, 8000.0, 0.6, 0.15, (4096, 8192)), (1100.0, 7000.0, 0.5, 0.3, (4096, 8192))]


@pytest.mark.parametrize("p", (1024, 4096, 8192))
def test_a_polynomial_reads_its_closed_forms(p):
    """y = x + a2 x^2 + a3 x^3 of two sines, without noise: q0 and q1 have the amplitude a2 A_lo A_hi, q2 and q3
    0.75 a3 A_lo^2 A_hi, q4 and q5 0.75 a3 A_lo A_hi^2, and a tone A + a3 (0.75 A^3 + 1.5 A A'^2), each within 0.01 dB (the
    tolerance tests/test_thd_cpu.py gives its fundamental); the figures of the standards follow by their formulas"""
    n = np.arange(p, dtype=np.float64)
    tol, seen = 0.01, 0
    for f_lo, f_hi, a_lo, a_hi, windows in PAIRS:
        if p not in windows:
            continue
        seen += 1
        x = ref.polynomial(ref.two_tones(n, f_lo / SR, f_hi / SR, a_lo, a_hi), A2, A3).astype(np.float32)
        r = ref.imd_one(x[None], p, SR)["ch"][0]
        assert r["valid"] == 1 and r["tones"] == 2, (p, f_lo)
        assert abs(r["lo_hz"] - f_lo) <= 0.02 and abs(r["hi_hz"] - f_hi) <= 0.02, (r["lo_hz"], r["hi_hz"])
        t_lo = a_lo + A3 * (0.75 * a_lo ** 3 + 1.5 * a_lo * a_hi ** 2)
        t_hi = a_hi + A3 * (0.75 * a_hi ** 3 + 1.5 * a_hi * a_lo ** 2)
        total = 10.0 * np.log10(t_lo * t_lo + t_hi * t_hi)
        amp = [A2 * a_lo * a_hi] * 2 + [0.75 * A3 * a_lo * a_lo * a_hi] * 2 + [0.75 * A3 * a_lo * a_hi * a_hi] * 2
        worst = max(abs(r["lo_db"] - 20.0 * np.log10(t_lo)), abs(r["hi_db"] - 20.0 * np.log10(t_hi)))
        assert abs(r["ratio_db"] - 20.0 * np.log10(t_hi / t_lo)) <= tol
        clear = [bool(int(r["products"]) >> q & 1) for q in range(ref.PRODUCTS)]
        assert clear[0] and clear[2] and clear[4], (p, f_lo, hex(int(r["products"])))
        for q in range(6):
            if clear[q]:
                worst = max(worst, abs(r["product_db"][q] - (20.0 * np.log10(amp[q]) - total)))
            else:
                assert np.isneginf(r["product_db"][q])
        power = [a * a if c else 0.0 for a, c in zip(amp, clear)]
        want = {"dfd2_db": 20.0 * np.log10(amp[0] / (t_lo + t_hi)),
                "dfd3_db": 20.0 * np.log10((amp[2] + amp[4]) / (t_lo + t_hi)),
                "mod_db": 10.0 * np.log10(sum(power[:4]) / (t_hi * t_hi)),  # (the polynomial has no product of the orders 4 and 5)
                "imd_db": 10.0 * np.log10(sum(power)) - total}
        for name, v in want.items():
            worst = max(worst, abs(r[name] - v))
        assert abs(r["order_db"][0] - (10.0 * np.log10(sum(power[:2])) - total)) <= tol
        assert abs(r["order_db"][1] - (10.0 * np.log10(sum(power[2:])) - total)) <= tol
        print(f"P {p}, {f_lo:g} + {f_hi:g} Hz: products {int(r['products']):#07x}, lo {float(r['lo_db']):.4f} hi {float(r['hi_db']):.4f} dB, "
              f"q0..5 {[round(float(v), 3) for v in r['product_db'][:6]]}, imd {float(r['imd_db']):.3f}, dfd2 {float(r['dfd2_db']):.3f}, "
              f"dfd3 {float(r['dfd3_db']):.3f}, mod {float(r['mod_db']):.3f}; worst against the closed forms {worst:.2g} dB")
        assert worst <= tol, (p, f_lo, worst)
        assert not any(np.isnan(np.atleast_1d(r[k])).any() for k in ref.DB_FIELDS + ref.HZ_FIELDS)
        if f_hi == 20000.0:  # the sums lie beyond the band and are not folded back
            assert not clear[1] and not clear[3] and not clear[5] and np.isneginf(r["product_db"][[1, 3, 5]]).all()
    assert seen >= 1


# ---- behaviour ----------------------------------------------------------------------------------------------------------------------

def _zero(p, tones=0):
    z = np.zeros((), ref.IMD_DTYPE)
    z["window"] = p
    z["ch"]["tones"][0] = tones
    return z


@pytest.mark.parametrize("p", (512, 2048, 8192))
def test_one_tone_silence_and_a_nan(p):
    sr = 48000
    rng = np.random.default_rng(3)
    one = ref.imd_one(ref.signal("single", rng, p, p)[None], p, sr)
    assert one.tobytes() == _zero(p, 1).tobytes()  # tones = 1, valid = 0, every other field 0
    assert ref.imd_one(np.zeros((2, p), np.float32), p, sr).tobytes() == _zero(p).tobytes()
    x = np.stack([ref.signal("wide", rng, p, p), ref.signal("clean", rng, p, p)])
    live = ref.imd_one(x, p, sr)
    assert live["ch"]["valid"].tolist() == [1, 1] and live["ch"]["tones"].tolist() == [2, 2]
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[1, p // 2 + 5] = bad
        assert ref.imd_one(y, p, sr).tobytes() == _zero(p).tobytes(), bad  # either channel's: the device shares one transform
        assert ref.imd_one(y[1:], p, sr).tobytes() == _zero(p).tobytes(), bad
    y = x.copy()
    y[1] = 0.0  # a silent channel next to a live one: exact silence
    r = ref.imd_one(y, p, sr)
    assert r["ch"][0].tobytes() == live["ch"][0].tobytes() and not r["ch"][1].tobytes().strip(b"\0")


def test_a_second_tone_30_db_down_is_not_a_tone():
    p, sr = 4096, 48000
    n = np.arange(p, dtype=np.float64)
    for db, tones in ((-29.0, 2), (-31.0, 1)):
        x = ref.two_tones(n, 0.11, 0.23, 0.5, 0.5 * 10.0 ** (db / 20.0)).astype(np.float32)
        r = ref.imd_one(x[None], p, sr)["ch"][0]
        assert r["tones"] == tones and r["valid"] == (tones == 2), (db, r["tones"])
        if tones == 2:
            assert abs(r["ratio_db"] - db) < 0.01 and r["lo_bin"] == round(0.11 * p) and r["hi_bin"] == round(0.23 * p)
        else:
            assert not r.tobytes().replace(b"\1\0\0\0", b"", 1).strip(b"\0")


@pytest.mark.parametrize("p", (1024, 2048, 8192))
def test_an_octave_and_products_beyond_the_band(p):
    sr = 48000
    rng = np.random.default_rng(4)
    r, vals = ref.analyse(ref.signal("octave", rng, p, p), sr)
    assert r["valid"] == 1 and abs(r["hi_hz"] / r["lo_hz"] - 2.0) < 1e-6
    assert not int(r["products"]) & 1 and np.isneginf(r["product_db"][0]) and np.isneginf(r["dfd2_db"])  # q0 lies on the lower tone
    assert vals["product_bins"][0] == r["lo_bin"] and not int(r["products"]) & 4  # and q2 = |f_hi - 2 f_lo| at 0
    assert np.isfinite(r["imd_db"]) and np.isfinite(r["mod_db"])
    r, vals = ref.analyse(ref.signal("twin", rng, p, p), sr)
    assert r["valid"] == 1 and r["lo_bin"] == round(0.79 * p / 2) and r["hi_bin"] == round(0.83 * p / 2)
    for q, kq in enumerate(vals["product_bins"]):
        beyond = kq + ref.LOBE > p // 2 - 1
        if beyond:  # not folded back: -inf and the bit cleared
            assert not int(r["products"]) >> q & 1 and np.isneginf(r["product_db"][q]), q
    assert vals["product_bins"][1] > p // 2 and vals["product_bins"][0] == round(0.02 * p)
    assert int(r["products"]) & 1 and round(0.02 * p) >= 17  # (q0 needs 17 bins)
    assert not any(np.isnan(np.atleast_1d(r[k])).any() for k in ref.DB_FIELDS)


@pytest.mark.parametrize("p", (512, 2048, 8192))
def test_two_pure_sines_have_no_intermodulation(p):
    r = ref.imd_one(ref.signal("clean", np.random.default_rng(5), p, p)[None], p, 48000)["ch"][0]
    print(p, float(r["imd_db"]), float(r["tdn_db"]), float(r["noise_db"]))
    assert r["valid"] == 1 and r["imd_db"] < -120.0 and r["tdn_db"] < -120.0 and r["mod_db"] < -120.0
    assert abs(r["lo_db"] - 20.0 * np.log10(ref.CLEAN_AMPLITUDES[0])) < 0.01 and abs(r["hi_db"] - 20.0 * np.log10(ref.CLEAN_AMPLITUDES[1])) < 0.01


def test_two_tones_within_two_lobes_are_one():
    """at P = 512 the twin's tones lie 10 bins apart, inside the 2H the second search keeps clear of the first"""
    r = ref.imd_one(ref.signal("twin", np.random.default_rng(9), 512, 512)[None], 512, 48000)["ch"][0]
    assert r["tones"] == 1 and r["valid"] == 0


def test_the_noise_floor_reads_the_variance():
    """white noise of variance s^2 under two pure sines reads 10 log10 s^2 (four standard deviations of the estimate, as
    tests/test_thd_cpu.py derives them).  Under the twin kind it does not: what its polynomial sends beyond the band aliases back,
    is in no region and counts as noise, -76 dB of it"""
    p = 8192
    rng = np.random.default_rng(6)
    x = ref.two_tones(np.arange(p, dtype=np.float64), 0.11, 0.23, 0.4, 0.4) + 10.0 ** (-90.0 / 20.0) * rng.standard_normal(p)
    r = ref.imd_one(x.astype(np.float32)[None], p, 48000)["ch"][0]
    print(float(r["noise_db"]), float(r["tdn_db"]))
    assert r["valid"] == 1 and abs(r["noise_db"] + 90.0) < 4.0 * 4.34 / np.sqrt((p // 2 - 250) / 2.6)
    twin = ref.imd_one(ref.signal("twin", rng, p, p)[None], p, 48000)["ch"][0]
    assert -80.0 < twin["noise_db"] < -72.0


def test_only_the_newest_frames_count():
    sr, w = 44100, 2064
    rng = np.random.default_rng(7)
    x = np.stack([ref.signal("twin", rng, 3000, 2048), ref.signal("wide", rng, 3000, 2048)])
    older = x.copy()
    older[:, :3000 - 2048] = 7.0
    a = ref.imd(x[None], w, sr)
    assert a.tobytes() == ref.imd(older[None], w, sr).tobytes() == ref.imd(x[None, :, 3000 - 2048:], w, sr).tobytes()
    assert a["window"][0] == 2048 and a["ch"]["valid"].tolist() == [[1, 1]]


def test_mismatches_applies_the_bound():
    rng = np.random.default_rng(8)
    x = np.stack([np.stack([ref.signal(a, rng, 1024, 1024), ref.signal(b, rng, 1024, 1024)]) for a, b in (("twin", "wide"), ("clean", "silence"))])
    want = ref.imd(x, 1024, 48000)
    assert ref.mismatches(want, want) == [] and np.isneginf(want["ch"]["product_db"][0, 0, 1])
    for name in ref.DB_FIELDS:
        where = (0, 0, 0) if name in ("order_db", "product_db") else (0, 0)
        got = want.copy()
        f = got["ch"][name]
        assert np.isfinite(f[where]), name
        f[where] = np.nextafter(f[where], np.float32(1e9))  # one ulp: inside
        assert ref.mismatches(got, want) == [], name
        f[where] = f[where] + max(3.0 * float(np.spacing(np.abs(f[where]))), 3e-6)  # three: outside
        assert [m[0] for m in ref.mismatches(got, want)] == ["ch." + name]
    for name in ref.UINT_FIELDS:
        got = want.copy()
        got["ch"][name][1, 0] += 1
        assert {m[0] for m in ref.mismatches(got, want)} == {"ch." + name}
    for name in ("window", "reserved"):
        got = want.copy()
        got[name][1] += 1
        assert {m[0] for m in ref.mismatches(got, want)} == {name}
    for name in ref.HZ_FIELDS:
        got = want.copy()
        got["ch"][name][0, 0] *= 1.0 + 1e-10
        assert ref.mismatches(got, want) == []
        got["ch"][name][0, 0] *= 1.0 + 1e-8
        assert [m[0] for m in ref.mismatches(got, want)] == ["ch." + name]
    got = want.copy()
    got["ch"]["product_db"][0, 0, 1] = -400.0  # an infinity is matched by an infinity alone
    assert [m[0] for m in ref.mismatches(got, want)] == ["ch.product_db"]
    got = want.copy()
    got["ch"]["imd_db"][0, 0] = np.nan
    assert [m[0] for m in ref.mismatches(got, want)] == ["ch.imd_db"]
    assert ref.mismatches(want[:1], want)[0][0] == "shape"


# ---- the conditions of the device comparison ----------------------------------------------------------------------------------------

def test_the_gpu_cases_meet_the_conditions_of_the_bound():
    """on the very seeds and shapes of tests/test_gpu_imd.py: the runner-up of either argmax lies at least 1e-6 relative below its
    winner, every product's and every harmonic's centre is at least 1e-6 from a half-integer, F_b / F_a is at least 1e-6 relative
    from the 30 dB threshold, and numpy.fft and the radix-2 transform agree on every dB field to 1e-7 dB; the window the device
    reads wraps the ring.  With these, one float32 rounding is all that can separate the device from the restatement"""
    seen, windows = set(), []
    for case in ref.GPU_CASES:
        fft, sr, kw, w, channels = case
        p = ref.window_frames(w)
        windows.append(p)
        x = ref.case_audio(case)
        ring = ref.ring_frames(w)
        assert x.shape == (len(ref.STREAM_KINDS), channels, ring + p // 2 + 3) and x.shape[-1] % 4 != 0
        assert (x.shape[-1] - p) % ring + p > ring  # the window wraps the ring
        a, b = ref.imd(x, w, sr), ref.imd(x, w, sr, ref.fft_radix2)
        assert ref.mismatches(b, a) == []
        for s, pair in enumerate(ref.STREAM_KINDS):
            for c, kind in enumerate(pair[:channels]):
                r, vals = ref.analyse(x[s, c, -p:], sr)
                _, other = ref.analyse(x[s, c, -p:], sr, ref.fft_radix2)
                assert r.tobytes() == a["ch"][s, c].tobytes()
                seen.add(kind)
                if kind == "silence":
                    assert r["tones"] == 0 and not r.tobytes().strip(b"\0") and not vals
                    continue
                assert vals["margin_ka"] >= 1e-6 and vals["margin_ratio"] >= 1e-6, (case, kind, vals)
                if kind == "single" or (kind == "twin" and p == 512):  # (at P = 512 the twin's tones are 10 bins apart: one region)
                    assert r["tones"] == 1 and r["valid"] == 0 and not r.tobytes().replace(b"\1\0\0\0", b"", 1).strip(b"\0")
                    continue
                assert r["valid"] == 1 and r["tones"] == 2, (case, kind)
                worst = 0.0
                for name in ref.DB_FIELDS:
                    u, v = np.atleast_1d(vals[name]), np.atleast_1d(other[name])
                    assert np.array_equal(np.isinf(u), np.isinf(v)) and not np.isnan(u).any(), (case, kind, name)
                    fin = np.isfinite(u)
                    if fin.any():
                        worst = max(worst, float(np.max(np.abs(u[fin] - v[fin]))))
                print(f"{ref.case_id(case)} stream {s} ch {c} {kind}: P {p}, bins {int(r['lo_bin'])} + {int(r['hi_bin'])} ({vals['lo_bins']:.4f}, "
                      f"{vals['hi_bins']:.4f}), products {int(r['products']):#07x}, imd {float(r['imd_db']):.2f}, dfd2 {float(r['dfd2_db']):.2f}, "
                      f"mod {float(r['mod_db']):.2f}, td+n {float(r['tdn_db']):.2f}, noise {float(r['noise_db']):.2f}; margins k_a "
                      f"{vals['margin_ka']:.3g}, k_b {vals['margin_kb']:.3g}, 30 dB {vals['margin_ratio']:.3g}, half-integer "
                      f"{vals['margin_half']:.3g}; two orderings {worst:.3g} dB")
                assert vals["margin_kb"] >= 1e-6 and vals["margin_half"] >= 1e-6, (case, kind)
                assert worst <= 1e-7, (case, kind, worst)
                assert other["product_bins"] == vals["product_bins"] and other["harmonic_bins"] == vals["harmonic_bins"]
                if kind == "twin":
                    assert int(r["products"]) & 1 and abs(r["ratio_db"]) < 0.05
                elif kind == "wide":
                    assert r["lo_bin"] == 19 and int(r["products"]) & 0xf == 0xf and abs(r["ratio_db"] + 12.04) < 0.05
                elif kind == "clean":
                    assert r["imd_db"] < -120.0
                elif kind == "octave":
                    assert not int(r["products"]) & 1
    assert seen == set(ref.KINDS)
    assert windows == [512, 2048, 8192, 8192, 2048, 4096, 1024]


def test_imd_kernels_have_no_scratch():
    res = kernel_usage("wf_hip_measure", "imd_read_kernel")
    assert len(res) == 2, res  # one and two captured channels
    for name, r in res.items():
        print(name, r)
        assert r.get("ScratchSize [bytes/lane]") == 0 and r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
        assert r.get("LDS Size [bytes/block]") <= 2048, (name, r)  # the cross-wave hand-over; the transform's LDS is dynamic
