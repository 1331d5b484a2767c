"""The loudness producer without a device: the K-weighting design against BS.1770-4 Tables 1 and 2 and across rates, the
float64 reference (tests/loudness_ref.py) against analytic truth, the new exports, the ctypes mirror of struct
wf_hip_loudness against the C layout, and a gfx950 compile of the new kernels with no scratch."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import loudness_ref as ref
from kernel_usage import kernel_usage

ROOT = Path(__file__).resolve().parents[1]


def test_k_weighting_matches_the_48k_tables():
    shelf, hpf = ref.k_coefs(48000)
    np.testing.assert_allclose(shelf, ref.TABLE_SHELF, rtol=0, atol=1e-6)
    np.testing.assert_allclose(hpf, ref.TABLE_HPF, rtol=0, atol=1e-6)


def test_k_weighting_at_44k1_agrees_with_48k():
    for f in (997.0, 10000.0):
        assert abs(ref.response_db(44100, f) - ref.response_db(48000, f)) < 0.01, f


def test_library_design_matches_the_restatement(tmp_path):
    """the host design in the library (wf_loudness_tables.cpp), compiled on its own, gives the restated coefficients and taps"""
    csrc = ROOT / "waveform_amd" / "csrc"
    src = tmp_path / "design.cpp"
    src.write_text('#include <cstdio>\n#include <initializer_list>\n#include "wf_loudness_tables.hpp"\n'
                   "int main() {\n"
                   "  for(unsigned fs : {44100u, 48000u}) { double s[5], h[5]; wf::host::k_weighting(fs, s, h);\n"
                   '    for(double v : s) std::printf("%.17g ", v); for(double v : h) std::printf("%.17g ", v); }\n'
                   "  double f[4][12]; wf::host::true_peak_fir(f);\n"
                   '  for(auto &r : f) for(double v : r) std::printf("%.17g ", v);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "design"
    subprocess.run(["g++", "-std=c++20", "-O2", "-I", str(csrc), str(src), str(csrc / "wf_loudness_tables.cpp"), "-o", str(exe)], check=True)
    got = np.array([float(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()])
    want = np.concatenate([np.concatenate(ref.k_coefs(fs)) for fs in (44100, 48000)] + [ref.fir_taps().ravel()])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def _sine(fs, f, seconds, dbfs, channels, phase=0.0):
    t = np.arange(int(fs * seconds)) / fs
    x = 10.0 ** (dbfs / 20.0) * np.sin(2 * np.pi * f * t + phase)
    return np.broadcast_to(x, (1, channels, x.size)).copy()


def test_reference_reads_a_997hz_sine_at_its_level():
    fs = 48000
    r = ref.measure(_sine(fs, 997.0, 4.0, -23.0, 2), fs)
    for k in ("momentary", "short_term", "integrated"):
        assert abs(r[k][0] - (-23.0)) < 0.05, (k, r[k][0])
    assert r["frames"][0] == 4 * fs


def test_reference_one_channel_reads_3_01_lu_lower():
    fs = 48000
    x = _sine(fs, 997.0, 4.0, -23.0, 2)
    x[:, 1] = 0.0
    r = ref.measure(x, fs)
    for k in ("momentary", "short_term", "integrated"):
        assert abs(r[k][0] - (-26.01)) < 0.05, (k, r[k][0])


def test_reference_silence_and_short_input():
    r = ref.measure(np.zeros((2, 2, 48000)), 48000)
    assert np.all(r["momentary"] == -np.inf) and np.all(r["integrated"] == -np.inf) and np.all(r["true_peak"] == -np.inf)
    assert np.all(r["range"] == 0.0)
    r = ref.measure(np.full((1, 1, 1000), 0.5), 48000)  # under one 400 ms block
    assert r["momentary"][0] == -np.inf and r["true_peak"][0] > -6.03


def test_fir_passband_is_flat_to_a_quarter_of_the_rate():
    taps = ref.fir_taps()
    np.testing.assert_allclose(taps.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    for frac in (0.25, 1 / 6, 1 / 8, 997 / 48000):
        resp = np.abs(taps @ np.exp(-2j * np.pi * frac * np.arange(12)))
        assert np.all(np.abs(20 * np.log10(resp)) < 0.01), (frac, resp)


def test_ctypes_loudness_matches_the_c_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wf_hip.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %d", sizeof(wf_hip_loudness), (int)WF_HIP_OUT_LOUDNESS);\n'
                   + "".join(f'  printf(" %zu", offsetof(wf_hip_loudness, {n}));\n' for n, _ in binding.Loudness._fields_)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(binding.Loudness), binding.OUT_LOUDNESS] + [getattr(binding.Loudness, n).offset for n, _ in binding.Loudness._fields_]
    assert got == want
    assert binding.LOUDNESS_DTYPE.itemsize == C.sizeof(binding.Loudness) == 32
    assert binding.OUT_LOUDNESS == binding.OUT_WAVEFORM_TS + 1  # appended: the existing outputs keep their numbers


@pytest.mark.parametrize("so", ["libwaveform_hip.so", "libwaveform_hip_dev.so"])
def test_new_symbols_exported_and_null_handle_refused(so):
    path = ROOT / "waveform_amd" / so
    nm = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert "wf_hip_enable_loudness" in exported
    L = wf.lib()
    assert L.wf_hip_enable_loudness(None, 0, 1) == -1
    assert L.wf_hip_output_bytes(None, binding.OUT_LOUDNESS) == 0


def test_loudness_kernels_have_no_scratch():
    scratch = {name: r.get("ScratchSize [bytes/lane]") for name, r in kernel_usage("wf_hip_measure", "loudness_").items()}
    assert len(scratch) == 3, sorted(scratch)  # the push kernel for 1 and 2 channels, the read kernel
    assert all(v == 0 for v in scratch.values()), scratch
