"""Delay finder (WF_HIP_OUT_DELAY) without a device: the structured dtype against the C layout, the appended output number, the
host tables (wf::host::delay_tables, compiled into a program of their own) against the restatement (tests/delay_ref.py), how well the
definition recovers known delays on the restatement, the conditions of the device comparison on its own seeds and shapes, and a
gfx950 compile of the read kernel with no scratch, no spills and next to no static LDS."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import delay_ref as ref
from kernel_usage import kernel_usage

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "waveform_amd" / "csrc"


def test_delay_dtype_matches_the_c_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wf_hip.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %d %d %d %d", sizeof(wf_hip_delay), (int)WF_HIP_OUT_DELAY, (int)WF_HIP_OUT_THD,\n'
                   "         (int)WF_HIP_DELAY_MAX_WINDOW, (int)WF_HIP_DELAY_CURVE);\n"
                   + "".join(f'  printf(" %zu", offsetof(wf_hip_delay, {n}));\n' for n in ref.FIELDS) +
                   '  printf(" %d", (int)WF_HIP_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    dt = binding.DELAY_DTYPE
    assert got == [dt.itemsize, binding.OUT_DELAY, binding.OUT_THD, binding.DELAY_MAX_WINDOW, binding.DELAY_CURVE] \
        + [dt.fields[n][1] for n in ref.FIELDS] + [13]
    assert dt.itemsize == 320 and dt.itemsize % 16 == 0 and dt == ref.DELAY_DTYPE
    assert dt.names == ("delay_frames", "delay_ms", "peak", "corr", "corr_zero", "ambiguity", "lag", "polarity", "valid", "window",
                        "reserved", "curve", "reserved2")
    assert [dt.fields[n][1] for n in dt.names] == [0, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 308]
    assert dt.fields["delay_frames"][0] == np.float64 and dt.fields["lag"][0] == np.int32 and dt.fields["polarity"][0] == np.int32
    assert dt.fields["curve"][0].shape == (65,) and dt.fields["curve"][0].base == np.float32 and dt.fields["reserved2"][0].shape == (3,)
    assert (ref.MAX_WINDOW, ref.CURVE) == (binding.DELAY_MAX_WINDOW, binding.DELAY_CURVE) == (4096, 65)


# ---- the host tables ----------------------------------------------------------------------------------------------------------------

TABLE_SIZES = (128, 144, 2064, 4096, 16384, 65536)  # fft sizes: P = 128, 128, 2048, 4096, 4096, 4096

PROGRAM = r"""
#include <cstdio>
#include <initializer_list>
#include "wf_measure_tables.hpp"
using namespace wf::host;
int main() {
  for(unsigned n : {128u, 144u, 2064u, 4096u, 16384u, 65536u}) {
    const DelayTables t = delay_tables(n);
    if(t.P != delay_window(n) || t.tab.size() != 2 * (size_t)t.P || (1u << t.log2p) != t.P) return 2;
    std::printf("T %u %u %u", n, t.P, t.log2p);
    for(double x : t.tab) std::printf(" %.17g", x);
    std::printf("\n");
  }
  return 0;
}
"""


def _build_and_run(directory, name, extra=()):
    src = directory / "delay_tables_main.cpp"
    src.write_text(PROGRAM)
    exe = directory / name
    subprocess.run(["g++", "-std=c++20", "-O2", *extra, "-I", str(CSRC), "-I", str(ROOT / "include"), str(src),
                    str(CSRC / "wf_measure_tables.cpp"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    text = _build_and_run(tmp_path_factory.mktemp("delay_tables"), "tables")
    out = {"text": text}
    for line in text.splitlines():
        f = line.split()
        assert f[0] == "T"
        out[int(f[1])] = (int(f[2]), int(f[3]), np.array(f[4:], np.float64))
    assert sorted(k for k in out if k != "text") == sorted(TABLE_SIZES)
    return out


@pytest.mark.parametrize("n", TABLE_SIZES)
def test_delay_tables(tables, n):
    """P equal; the taper to 1e-15 relative, entry by entry (both sides round the same long double value); the twiddles to
    test_measure_tables_cpu.py's 1e-12"""
    p, log2p, tab = tables[n]
    assert p == ref.window_frames(n) and 1 << log2p == p and tab.size == 2 * p
    w = ref.taper(p)
    assert w[0] == 0.0 and tab[0] == 0.0 and w[p // 2] == 1.0 and np.all(w[1:] > 0)
    print(f"fft {n}: P {p}, taper worst relative difference {float(np.max(np.abs(tab[1:p] - w[1:]) / w[1:])):.3g}")
    np.testing.assert_allclose(tab[:p], w, rtol=1e-15, atol=0)
    x = 2.0 * np.pi * np.arange(p // 2, dtype=np.float64) / float(p)
    tw = tab[p:].reshape(p // 2, 2)
    np.testing.assert_allclose(tw[:, 0], np.cos(x), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(tw[:, 1], -np.sin(x), rtol=1e-12, atol=1e-15)
    assert tw[0, 0] == 1.0 and tw[0, 1] == 0.0


def test_the_tables_program_is_clean_under_the_sanitizers(tables, tmp_path):
    """the same program with -fsanitize=address,undefined, run directly: exit 0 and the same output"""
    text = _build_and_run(tmp_path, "tables_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert text == tables["text"]


def test_window_frames():
    assert [ref.window_frames(w) for w in (128, 144, 1024, 2064, 4095, 4096, 16384, 65536)] == [128, 128, 1024, 2048, 2048, 4096, 4096, 4096]


# ---- the definition on the restatement ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cases():
    """per GPU case: (the case, its audio, the restatement of it in every order): computed once"""
    out = []
    for case in ref.GPU_CASES:
        fft, sr, kw, w = case
        x = ref.case_audio(case)
        out.append((case, x, {o: ref.delay(x, w, sr, o) for o in ref.ORDERS}))
    return out


def test_the_definition_recovers_known_delays(cases):
    """every correlated kind within 0.05 frame of the truth at P >= 1024; at P = 128 within 0.1 frame for the kinds whose delay is
    at most P / 8 frames and within 0.2 for the one near L; polarity -1 exactly for the inverted kind; ambiguity > 0.5 for
    independent noise and < 0.2 for white noise at small delays; corr_zero of dual mono 1 to 1e-12; silence and the NaN read the
    zero record"""
    seen = set()
    for case, x, res in cases:
        fft, sr, kw, w = case
        p = ref.window_frames(w)
        seen.add(p)
        got = res["numpy"]
        for s, (name, truth, pol) in enumerate(ref.KINDS):
            r = got[s]
            if name in ref.INVALID:
                assert r.tobytes() == ref.zero_record(p, 1).tobytes(), (case, name)
                continue
            assert r["valid"] == 1 and r["window"] == p and r["lag"] == np.floor(r["delay_frames"] + 0.5)
            assert abs(r["delay_ms"] - 1000.0 * r["delay_frames"] / sr) <= 1e-6 * max(1.0, abs(float(r["delay_ms"])))
            assert abs(r["peak"]) <= 1.0 + 1e-6 and abs(r["corr"]) <= 1.0 + 1e-6 and r["curve"][ref.CURVE // 2] == r["peak"]
            if truth is None:
                assert name == "independent" and r["ambiguity"] > 0.5, (case, name, r["ambiguity"])
                continue
            d = truth(p // 4)
            err = abs(float(r["delay_frames"]) - d)
            bound = 0.05 if p >= 1024 else (0.2 if name == "inverted L-1" else 0.1) if p == 128 else 0.1
            print(f"{ref.case_id(case)} {name}: P {p}, truth {d}, read {float(r['delay_frames']):.5f} (error {err:.3g} of {bound}), "
                  f"polarity {int(r['polarity'])}, peak {float(r['peak']):.3f}, ambiguity {float(r['ambiguity']):.3f}")
            assert err <= bound, (case, name, err)
            assert r["polarity"] == pol and (r["peak"] < 0) == (pol < 0)
            if name in ("white +3", "white -7.3", "dual mono"):
                assert r["ambiguity"] < 0.2, (case, name)
            if name == "dual mono":
                c0 = ref.analyse(x[s, 0, -p:], x[s, 1, -p:], sr)[1]["corr_zero"]
                assert abs(c0 - 1.0) <= 1e-12 and r["lag"] == 0 and r["corr_zero"] == 1.0
    assert seen == {128, 512, 1024, 2048, 4096}


def test_a_pure_sine_is_computed_and_ambiguous():
    p, sr = 1024, 48000
    t = np.arange(p, dtype=np.float64)
    s = 0.5 * np.sin(2.0 * np.pi * 37.3 / p * t)
    x = np.stack([np.roll(s, 3), s]).astype(np.float32)
    r = ref.delay_one(x, p, sr)
    print({n: r[n].tolist() for n in ref.FIELDS if n != "curve"})
    assert r["valid"] == 1 and r["ambiguity"] > 0.9


def test_only_the_newest_frames_count():
    sr, w = 44100, 2064
    rng = np.random.default_rng(4)
    x = ref.stream("white +3", rng, 3001, 2048)
    older = x.copy()
    older[:, :3001 - 2048] = 7.0
    a = ref.delay(x[None], w, sr)
    assert a.tobytes() == ref.delay(older[None], w, sr).tobytes() == ref.delay(x[None, :, 3001 - 2048:], w, sr).tobytes()
    assert a["window"][0] == 2048 and a["valid"][0] == 1 and a["lag"][0] == 3
    for bad in (np.nan, np.inf, -np.inf):
        for c in (0, 1):
            y = x.copy()
            y[c, 3001 - 700] = bad
            assert ref.delay_one(y, w, sr).tobytes() == ref.zero_record(2048, 1).tobytes()
    y = x.copy()
    y[1] = -0.0
    assert ref.delay_one(y, w, sr).tobytes() == ref.zero_record(2048, 1).tobytes()


def test_mismatches_applies_the_bound(cases):
    want = cases[1][2]["numpy"][:7]
    assert ref.mismatches(want, want) == []
    for name in ref.FLOAT_FIELDS:
        where = (0, 3) if name == "curve" else (0,)
        got = want.copy()
        f = got[name]
        f[where] = np.nextafter(f[where], np.float32(1e9))  # one ulp: inside
        assert ref.mismatches(got, want) == [], name
        f[where] = f[where] + max(3.0 * float(np.spacing(np.abs(f[where]))), 3e-6)  # three: outside
        assert [m[0] for m in ref.mismatches(got, want)] == [name]
    for name in ref.INT_FIELDS:
        got = want.copy()
        got[name][1] += 1
        assert {m[0] for m in ref.mismatches(got, want)} == {name}
    got = want.copy()
    got["delay_frames"][2] += 5e-8
    assert ref.mismatches(got, want) == []
    got["delay_frames"][2] += 2e-7
    assert [m[0] for m in ref.mismatches(got, want)] == ["delay_frames"]
    got = want.copy()
    got["peak"][0] = np.nan
    assert [m[0] for m in ref.mismatches(got, want)] == ["peak"]
    assert ref.mismatches(want[:1], want)[0][0] == "shape"


# ---- the conditions of the device comparison ----------------------------------------------------------------------------------------

def test_the_gpu_cases_meet_the_conditions_of_the_bound(cases):
    """on the very seeds and shapes of tests/test_gpu_delay.py, for every stream of every case: the four orders agree to 1e-9 in
    every field, curve included; the winning |R| exceeds every other lag's by at least 1e-3 relative; no bin with u >= 1e-6 has
    |phi| within 1e-6 rad of pi; |f| before clamping is not within 1e-6 of 0.5; the window the device reads wraps the ring.  With
    these, one float32 rounding is all that can separate the device from the restatement"""
    windows, overall = [], 0.0
    for case, x, res in cases:
        fft, sr, kw, w = case
        if kw.get("meter"):
            assert w == int(sr * (kw["meter_ms"] / 1000.0)) & -16 == 2208
        else:
            assert w == fft
        p = ref.window_frames(w)
        windows.append(p)
        ring = ref.ring_frames(w)
        assert x.shape == (len(ref.KINDS), 2, ring + p // 2 + 3) and x.shape[0] == 9 and x.shape[-1] % 2 == 1
        assert (x.shape[-1] - p) % ring + p > ring  # the window wraps the ring
        for o in ref.ORDERS[1:]:
            bad = ref.mismatches(res[o], res["numpy"], float_tol=1e-9)
            figures = ref.worst(res[o], res["numpy"])
            overall = max(overall, max(figures.values()))
            print(f"{ref.case_id(case)}: {o} against numpy, worst {max(figures.values()):.3g}")
            assert not bad, (case, o, bad[:4])
        for s, (name, truth, pol) in enumerate(ref.KINDS):
            r, vals = ref.analyse(x[s, 0, -p:], x[s, 1, -p:], sr)
            assert r.tobytes() == res["numpy"][s].tobytes()
            if name in ref.INVALID:
                assert r["valid"] == 0 and not vals
                continue
            print(f"{ref.case_id(case)} stream {s} {name}: lag {vals['lag']}, f {vals['f_raw']:+.5f}, argmax margin "
                  f"{vals['margin_argmax']:.3g}, closest phase to pi {vals['margin_pi']:.3g} rad")
            assert r["valid"] == 1
            assert vals["margin_argmax"] >= 1e-3, (case, name)
            assert vals["margin_pi"] >= 1e-6, (case, name)
            assert abs(abs(vals["f_raw"]) - 0.5) >= 1e-6, (case, name)
            if truth is not None:
                assert vals["margin_argmax"] >= 0.1, (case, name)  # (0.16 of the peak was the prototype's smallest)
    print(f"the four orders agree to {overall:.3g} over every field of every case")
    assert windows == [128, 1024, 2048, 4096, 4096, 2048, 512]
    assert [ref.case_id(c) for c in ref.GPU_CASES] == ["w128_sr48000", "w1024_sr44100", "w2064_sr48000", "w4096_sr96000", "w16384_sr48000",
                                                       "w2208_sr48000_meter1", "w512_sr48000_stereo0"]
    # the curve leaves +-L at the smallest window: L = 32 is its half-width
    r = cases[0][2]["numpy"][2]
    assert r["lag"] == 31 and r["window"] == 128


def test_delay_kernel_has_no_scratch():
    res = kernel_usage("wf_hip_measure", "delay_read_kernel")
    assert len(res) == 1, res
    for name, r in res.items():
        print(name, r)
        assert r.get("ScratchSize [bytes/lane]") == 0 and r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
        assert r.get("LDS Size [bytes/block]") <= 2048, (name, r)  # the cross-wave hand-overs; the transforms' LDS is dynamic
    src = (CSRC / "wf_delay.hpp").read_text()
    assert "asm" not in src and "atomic" not in src.replace("no atomics", "")
    # at the cap both regions together are what setup_delay asks for: 128 KB
    assert 2 * binding.DELAY_MAX_WINDOW * 16 == 128 * 1024
