"""Stereo image (WF_HIP_OUT_STEREO) without a device: the structured dtype against the C layout, the appended output number,
the properties the definition promises of its float64 restatement (tests/stereo_ref.py), the condition of the signals the
device test pushes, and a gfx950 compile of the read kernel with no scratch."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from waveform_amd import binding
import stereo_ref as ref
from kernel_usage import kernel_usage

ROOT = Path(__file__).resolve().parents[1]
# (fft_size, sample rate) of tests/test_gpu_stereo.py's comparison against the restatement
GPU_SHAPES = [(128, 48000), (2064, 44100), (4096, 48000), (16384, 96000), (1024, 48000)]
GPU_SEED = 20261017


def test_stereo_dtype_matches_the_c_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wf_hip.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %d %d %d", sizeof(wf_hip_stereo), (int)WF_HIP_OUT_STEREO, (int)WF_HIP_OUT_BANDS, (int)WF_HIP_STEREO_MAX_WINDOW);\n'
                   '  printf(" %zu %zu %zu %zu %zu %zu", offsetof(wf_hip_stereo, correlation), offsetof(wf_hip_stereo, coherence),\n'
                   "         offsetof(wf_hip_stereo, phase_deg), offsetof(wf_hip_stereo, balance_db), offsetof(wf_hip_stereo, covered),\n"
                   "         offsetof(wf_hip_stereo, window));\n"
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    dt = binding.STEREO_DTYPE
    assert got == [dt.itemsize, binding.OUT_STEREO, binding.OUT_BANDS, binding.STEREO_MAX_WINDOW] \
        + [dt.fields[n][1] for n in ("correlation", "coherence", "phase_deg", "balance_db", "covered", "window")]
    assert dt.itemsize == 504 and dt == ref.STEREO_DTYPE and ref.MAX_WINDOW == binding.STEREO_MAX_WINDOW == 4096
    assert all(dt.fields[n][0].shape == (31,) for n in ref.FIELDS)
    assert binding.MEASURES["stereo"] == (binding.OUT_STEREO, dt, False)


def test_window_is_the_largest_power_of_two():
    assert [ref.window_frames(n) for n in (64, 127, 128, 2064, 4096, 4112, 16384, 65536)] == [64, 64, 128, 2048, 4096, 4096, 4096, 4096]


def _noise(rng, p, streams=2):
    return rng.standard_normal((streams, p)).astype(np.float32) * np.float32(0.25)


@pytest.mark.parametrize("p,sr", [(64, 48000), (2048, 44100), (4096, 48000)])
def test_identical_inverted_and_scaled_channels(p, sr):
    rng = np.random.default_rng(p)
    l = _noise(rng, p)
    live = ref.overlapping(sr, p)
    assert live.any()
    same = ref.stereo(np.stack([l, l], axis=1), sr)
    assert np.all(same["correlation"][:, live] == 1.0) and np.all(same["coherence"][:, live] == 1.0)
    assert np.all(np.abs(same["phase_deg"][:, live]) < 1e-6) and np.all(np.abs(same["balance_db"][:, live]) < 1e-6)
    inv = ref.stereo(np.stack([l, -l], axis=1), sr)
    assert np.all(inv["correlation"][:, live] == -1.0) and np.all(inv["phase_deg"][:, live] == 180.0)
    assert np.all(inv["coherence"][:, live] == 1.0)
    half = ref.stereo(np.stack([l, np.float32(0.5) * l], axis=1), sr)
    assert np.all(np.abs(half["balance_db"][:, live] - 20.0 * np.log10(0.5)) < 1e-5)  # -6.0206 dB
    assert np.all(half["correlation"][:, live] == 1.0)
    for got in (same, inv, half):
        assert np.all(got["window"] == p) and np.all(got["covered"] == ref.bands_ref.covered(sr, p))
        for name in ref.FIELDS:  # bands without bins read 0
            assert np.all(got[name][:, ~live] == 0.0)


@pytest.mark.parametrize("f,d,band", [(1000.0, 6, 17), (250.0, 40, 11), (4000.0, -2, 23)])
def test_a_delayed_sine_reads_its_phase(f, d, band):
    """r delayed by d frames lags by 360 f d / sr degrees: the left channel leads, the phase is positive (45, 75 and -60 degrees:
    away from +-180)"""
    p, sr = 4096, 48000
    t = np.arange(p + 64)
    l = 0.5 * np.sin(2 * np.pi * f * t / sr)
    r = 0.5 * np.sin(2 * np.pi * f * (t - d) / sr)
    got = ref.stereo(np.stack([l, r])[None, :, 64:].astype(np.float32), sr)[0]
    want = 360.0 * f * d / sr
    print(f, d, got["phase_deg"][band], want, got["coherence"][band], got["balance_db"][band])
    assert abs(want) < 170 and abs(got["phase_deg"][band] - want) < 0.5
    assert got["coherence"][band] > 0.999 and abs(got["balance_db"][band]) < 0.01
    assert abs(got["correlation"][band] - np.cos(np.radians(want))) < 0.01


def test_silence_and_a_dead_channel():
    p, sr = 1024, 48000
    z = np.zeros((1, 2, p), np.float32)
    got = ref.stereo(z, sr)
    for name in ref.FIELDS:
        assert np.all(got[name] == 0.0), name
    assert got["window"][0] == p and got["covered"][0] == ref.bands_ref.covered(sr, p)
    l = _noise(np.random.default_rng(3), p, 1)
    live = ref.overlapping(sr, p)
    dead_r = ref.stereo(np.stack([l, np.zeros_like(l)], axis=1), sr)
    dead_l = ref.stereo(np.stack([np.zeros_like(l), l], axis=1), sr)
    assert np.all(np.isneginf(dead_r["balance_db"][:, live])) and np.all(np.isposinf(dead_l["balance_db"][:, live]))
    for got in (dead_r, dead_l):
        assert np.all(got["balance_db"][:, ~live] == 0.0)
        for name in ("correlation", "coherence", "phase_deg"):
            assert np.all(got[name] == 0.0), name


def test_independent_noise_is_incoherent_in_the_wide_bands():
    p, sr = 4096, 48000
    rng = np.random.default_rng(9)
    got = ref.stereo(np.stack([_noise(rng, p, 8), _noise(rng, p, 8)], axis=1), sr)
    # band 30 averages ~390 bins: |X| / sqrt(A B) is about 1 / sqrt(bins / 1.5)
    assert np.all(got["coherence"][:, 30] < 0.25) and np.all(np.abs(got["correlation"][:, 30]) < 0.25)
    assert np.all(got["coherence"] >= 0.0) and np.all(got["coherence"] <= 1.0) and np.all(np.abs(got["correlation"]) <= 1.0)
    assert np.all(np.abs(got["correlation"]) <= got["coherence"] + 1e-6)


def test_mismatches_bound():
    want = np.zeros(1, ref.STEREO_DTYPE)
    want["coherence"] = 0.5
    want["phase_deg"] = 30.0
    want["balance_db"][0, 3] = -np.inf
    got = want.copy()
    assert ref.mismatches(got, want) == []
    got["phase_deg"][0, 5] = np.nextafter(np.float32(30.0), np.float32(0))  # one ulp
    assert ref.mismatches(got, want) == []
    got["phase_deg"][0, 5] = np.nextafter(got["phase_deg"][0, 5], np.float32(0))  # two
    assert [m[0] for m in ref.mismatches(got, want)] == ["phase_deg"]
    want["coherence"][0, 5] = got["coherence"][0, 5] = 0.009  # under 0.01: the phase is not compared
    assert ref.mismatches(got, want) == []
    got["coherence"][0, 5] = 0.0091
    assert [m[0] for m in ref.mismatches(got, want)] == ["coherence"]
    got = want.copy()
    got["balance_db"][0, 3] = -700.0
    got["window"] = 1
    assert [m[0] for m in ref.mismatches(got, want)] == ["balance_db", "window"]
    got = want.copy()
    got["correlation"][0, 0] = np.nan
    assert [m[0] for m in ref.mismatches(got, want)] == ["correlation"]


@pytest.mark.parametrize("fft,sr", GPU_SHAPES, ids=[f"n{f}_sr{s}" for f, s in GPU_SHAPES])
def test_the_gpu_tests_signal_keeps_its_phase_comparable(fft, sr):
    """the condition of tests/test_gpu_stereo.py's comparison: on its own seeds and shapes at most 1 % of the overlapping bands
    have a coherence under 0.01, where the phase is left out"""
    p = ref.window_frames(fft)
    x = ref.audio(np.random.default_rng(GPU_SEED + fft), 3, p + 1600, sr)
    want = ref.stereo(x[..., -p:], sr)
    live = ref.overlapping(sr, p)
    coh = want["coherence"][:, live]
    share = ref.low_coherence_share(want, sr)
    print(f"fft {fft} sr {sr}: P {p}, {int(live.sum())} bands overlap, smallest coherence {coh.min():.3f}, share under 0.01: {share:.4f}, "
          f"under 0.1: {(coh < 0.1).mean():.4f}")
    assert share <= 0.01


def test_stereo_kernel_has_no_scratch_and_no_static_lds():
    res = kernel_usage("wf_hip_measure", "stereo_read_kernel")
    assert len(res) == 1, res
    for name, r in res.items():
        assert r.get("ScratchSize [bytes/lane]") == 0 and r.get("VGPRs Spill") == 0, (name, r)
        # the transform is the whole 64 KB a workgroup gets by default: all of it dynamic, nothing static beside it
        assert r.get("LDS Size [bytes/block]") == 0, (name, r)
        assert r.get("Occupancy [waves/SIMD]") >= 2, (name, r)  # two workgroups of 64 KB share a CU's 160 KB
