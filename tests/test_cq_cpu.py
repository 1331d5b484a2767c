"""Constant-Q spectrum (WF_HIP_OUT_CQ) without a device: the structured dtype against the C layout, the appended output number,
the geometry (covered, resolved, L_b) from the formulas, the properties the definition promises of its float64 restatement
(tests/cq_ref.py), the condition of the signals the device test pushes, and a gfx950 compile of the read kernel with no scratch."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from waveform_amd import binding
import cq_ref as ref
from kernel_usage import kernel_usage

ROOT = Path(__file__).resolve().parents[1]
RATES = (8000, 44100, 48000, 96000)


def test_cq_dtype_matches_the_c_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wf_hip.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %d %d %d %d", sizeof(wf_hip_cq), (int)WF_HIP_OUT_CQ, (int)WF_HIP_OUT_STEREO, (int)WF_HIP_CQ_BINS,\n'
                   "         (int)WF_HIP_CQ_MAX_WINDOW);\n"
                   '  printf(" %zu %zu %zu %zu %zu %d", offsetof(wf_hip_cq, db), offsetof(wf_hip_cq, end_covered),\n'
                   "         offsetof(wf_hip_cq, first_resolved), offsetof(wf_hip_cq, max_window), offsetof(wf_hip_cq, reserved),\n"
                   "         (int)WF_HIP_ABI_VERSION);\n"
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    dt = binding.CQ_DTYPE
    assert got == [dt.itemsize, binding.OUT_CQ, binding.OUT_STEREO, binding.CQ_BINS, binding.CQ_MAX_WINDOW] \
        + [dt.fields[n][1] for n in ("db", "end_covered", "first_resolved", "max_window", "reserved")] + [13]
    assert dt.itemsize == 976 and dt == ref.CQ_DTYPE and dt.fields["db"][0].shape == (2, 120)
    assert ref.BINS == binding.CQ_BINS == 120 and ref.MAX_WINDOW == binding.CQ_MAX_WINDOW == 16384
    assert binding.MEASURES["cq"] == (binding.OUT_CQ, dt, False)
    assert np.array_equal(binding.CQ_CENTRES_HZ, ref.centres())


def test_bin_centres():
    f = ref.centres()
    assert f[57] == 440.0 and abs(f[0] - 16.3516) < 1e-4 and abs(f[119] - 15804.27) < 1e-2
    assert abs(ref.Q - 16.817) < 1e-3


@pytest.mark.parametrize("sr", RATES)
def test_geometry_from_the_formulas(sr):
    """end_covered, first_resolved and L_b written out bin by bin in plain Python, for four ring sizes; and the margin that keeps
    numpy's and the C library's pow from disagreeing about a ceil: Q sr / f_b further than 1e-6 from an integer in every bin"""
    full = ref.full_windows(sr)
    margin = np.abs(full - np.rint(full)).min()
    print(f"sr {sr}: smallest distance of Q sr / f_b from an integer {margin:.3e}")
    assert margin > 1e-6
    q = 1.0 / (2.0 ** (1.0 / 12.0) - 1.0)
    for lmax in (128, 1024, 4096, 16384):
        want_l, end, first = [], 0, None
        for b in range(120):
            fb = 440.0 * 2.0 ** ((b - 57) / 12.0)
            if fb * 2.0 ** (1.0 / 24.0) < sr / 2.0:
                assert end == b  # a prefix
                end = b + 1
            n = int(np.ceil(q * sr / fb))
            if n <= lmax and first is None:
                first = b
            want_l.append(min(n, lmax))
        L, end_covered, first_resolved = ref.geometry(sr, lmax)
        assert list(L) == want_l and end_covered == end and first_resolved == (120 if first is None else first)
        assert np.all(np.diff(L) <= 0) and L.max() <= lmax
        s = ref.cq(np.zeros((1, 2, lmax), np.float32), sr, lmax)[0]
        assert (s["end_covered"], s["first_resolved"], s["max_window"], s["reserved"]) == (end, first_resolved, lmax, 0)
    assert ref.geometry(48000, 16384)[1:] == (120, 20) and ref.geometry(48000, 4096)[2] == 44  # G#1, 51.9 Hz; G#3, 207.7 Hz
    assert ref.geometry(8000, 4096)[1] == 95 and ref.max_window(32768) == 16384 and ref.max_window(128) == 128


def _sine(f, amp, sr, frames, phase=0.3):
    return (amp * np.sin(2.0 * np.pi * f * np.arange(frames) / sr + phase)).astype(np.float32)


@pytest.mark.parametrize("sr", (44100, 48000))
def test_a_sine_at_a_bin_centre_reads_its_amplitude(sr):
    """every fourth resolved bin up to f_b = sr / 8.  (Above that the bin also hears the sine's own mirror image at -f_b, which
    aliases to sr - 2 f_b above f_b: closer than the 2 Q = 33.6 window bins it keeps below, where the Hann window's skirt
    is under 1e-5.)"""
    lmax = 16384
    L, end, first = ref.geometry(sr, lmax)
    f = ref.centres()
    bins = [b for b in range(first, end, 4) if f[b] <= sr / 8]
    assert len(bins) >= 15 and 57 in range(first, end)
    worst = 0.0
    for b in bins + [57]:
        amp = 0.5 if b == 57 else 0.1 + 0.01 * b
        x = np.stack([_sine(f[b], amp, sr, lmax), _sine(f[b], 2.0 * amp, sr, lmax, 1.1)])[None]
        got = ref.cq(x, sr, lmax)[0]["db"]
        worst = max(worst, abs(got[0, b] - 20.0 * np.log10(amp)))
        assert abs(got[0, b] - 20.0 * np.log10(amp)) < 1e-3, (b, got[0, b])
        assert abs(got[1, b] - got[0, b] - 6.0206) < 1e-3  # doubling the input adds 6.0206 dB
        assert int(np.argmax(got[0])) == b
        if b == 57 and sr == 48000:
            assert L[b] == 1835 and abs(got[0, b] - -6.02056) < 2e-5
            assert 5.0 < got[0, b] - got[0, b - 1] < 7.0 and 5.0 < got[0, b] - got[0, b + 1] < 7.0  # the Hann bank's overlap
    print(f"sr {sr}: {len(bins) + 1} bins, worst |db - 20 log10 A| {worst:.2e} dB")


def test_zeros_and_a_mono_input():
    sr, lmax = 48000, 1024
    z = ref.cq(np.zeros((2, 2, lmax), np.float32), sr, lmax)
    assert np.all(np.isneginf(z["db"])) and np.all(z["max_window"] == lmax)
    x = ref.audio(np.random.default_rng(1), 2, lmax, sr)
    mono = ref.cq(x[:, :1], sr, lmax)
    both = ref.cq(x, sr, lmax)
    assert np.all(np.isneginf(mono["db"][:, 1])) and np.array_equal(mono["db"][:, 0], both["db"][:, 0])
    assert np.all(np.isfinite(both["db"]))  # 48 kHz: every bin covered
    low = ref.cq(x, 8000, lmax)
    assert np.all(np.isneginf(low["db"][:, :, 95:])) and np.all(np.isfinite(low["db"][:, :, :95]))
    # only the newest L_b frames count: older ones may be anything
    longer = np.concatenate([np.ones((2, 2, 7), np.float32), x], axis=2)
    assert ref.cq(longer, sr, lmax).tobytes() == both.tobytes()


def test_mismatches_bound():
    sr, lmax = 48000, 1024
    x = ref.audio(np.random.default_rng(2), 2, lmax + 5, sr)
    want = ref.cq(x, sr, lmax)
    assert ref.mismatches(want, x, sr, lmax) == []
    a = ref.amplitudes(x, sr, lmax)
    pk = ref.peak(x, lmax)
    s = tuple(np.argwhere(ref.strong(a, pk))[0])
    got = want.copy()
    v = got["db"][s]
    got["db"][s] = np.nextafter(np.nextafter(v, np.float32(0)), np.float32(0))  # two ulps
    assert ref.mismatches(got, x, sr, lmax) == []
    got["db"][s] = np.nextafter(got["db"][s], np.float32(0))  # three: a strong bin has no second arm
    assert [m[0] for m in ref.mismatches(got, x, sr, lmax)] == ["db"]
    # a weak bin (a sine's far skirt) may differ by 1e-10 pk, however many ulps of dB that is
    tone = np.stack([_sine(ref.centres()[57], 0.5, sr, lmax)] * 2)[None]
    wt = ref.cq(tone, sr, lmax)
    at = ref.amplitudes(tone, sr, lmax)
    weak = tuple(np.argwhere(~ref.strong(at, ref.peak(tone, lmax)))[-1])
    got = wt.copy()
    got["db"][weak] = np.float32(20.0 * np.log10(at[weak] + 0.4e-10))
    assert abs(float(got["db"][weak]) - float(wt["db"][weak])) > 2 * np.spacing(abs(wt["db"][weak]))  # outside the first arm
    assert ref.mismatches(got, tone, sr, lmax) == []
    got["db"][weak] = np.float32(20.0 * np.log10(at[weak] + 2e-10))
    assert [m[0] for m in ref.mismatches(got, tone, sr, lmax)] == ["db"]
    got = want.copy()
    got["db"][0, 1, 3] = np.nan
    got["reserved"][1] = 1
    assert [m[0] for m in ref.mismatches(got, x, sr, lmax)] == ["reserved", "db"]
    got = ref.cq(x[:, :1], sr, lmax)
    got["db"][0, 1, 0] = -200.0  # the channel that was not captured reads -INFINITY exactly
    assert [m[0] for m in ref.mismatches(got, x[:, :1], sr, lmax)] == ["db exact"]


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=ref.case_id)
def test_the_gpu_tests_signal_is_mostly_strong(case):
    """the condition of tests/test_gpu_cq.py's comparison: on its own seeds and shapes at least 80 % of the covered bins of
    audio() have a_b >= 1e-3 max |x| and so must agree to two float32 ulps"""
    fft, sr, ring, ch, _, lmax = case
    fft, sr, ring, ch, kw, lmax = case
    if not kw.get("meter"):  # the ring of a spectrum batch: the next power of two of what was asked for, or of max(2 fft, 4096)
        assert lmax == ref.max_window(1 << ((max(ring, fft) if ring else max(2 * fft, 4096)) - 1).bit_length())
    x = ref.case_audio(case)
    assert x.shape == (3, ch, lmax + 1602)
    a = ref.amplitudes(x, sr, lmax)
    end = ref.geometry(sr, lmax)[1]
    share = ref.strong(a, ref.peak(x, lmax))[..., :end].mean()
    print(f"{ref.case_id(case)}: Lmax {lmax}, {end} covered bins, first resolved {ref.geometry(sr, lmax)[2]}, strong share {share:.3f}")
    assert share >= 0.8


def test_cq_kernel_has_no_scratch():
    res = kernel_usage("wf_hip_measure", "cq_read_kernel")
    assert len(res) == 2, res  # one and two captured channels
    for name, r in res.items():
        assert r.get("ScratchSize [bytes/lane]") == 0 and r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
        assert r.get("LDS Size [bytes/block]") == 0, (name, r)  # the staged windows are all of it, and dynamic
        # sixteen waves per workgroup, four per SIMD: 128 VGPRs at the most
        assert r.get("VGPRs") <= 128 and r.get("Occupancy [waves/SIMD]") >= 4, (name, r)
