"""Sonogram (WF_HIP_OUT_SONO) without a device: the structured dtype against the C layout, the appended output number, the
properties the definition promises of its float64 restatement (tests/sono_ref.py), the conditions of the signals the device test
pushes, and a gfx950 compile of the read kernels with no scratch, no spills and no static LDS.  (The host tables:
test_sono_tables_cpu.py.)"""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from waveform_amd import binding
import sono_ref as ref
from kernel_usage import kernel_usage

ROOT = Path(__file__).resolve().parents[1]
P, H = ref.P, ref.H
SR, RING = 48000, 8192  # T = 28


def test_sono_dtype_matches_the_c_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wf_hip.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %d %d %d %d %d %d", sizeof(wf_hip_sono), (int)WF_HIP_OUT_SONO, (int)WF_HIP_OUT_GONIO, (int)WF_HIP_SONO_WINDOW,\n'
                   "         (int)WF_HIP_SONO_HOP, (int)WF_HIP_SONO_COLUMNS, (int)WF_HIP_SONO_BANDS);\n"
                   + "".join(f'  printf(" %zu", offsetof(wf_hip_sono, {n}));\n' for n in ref.FIELDS) +
                   '  printf(" %d", (int)WF_HIP_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    dt = binding.SONO_DTYPE
    assert got == [dt.itemsize, binding.OUT_SONO, binding.OUT_GONIO, binding.SONO_WINDOW, binding.SONO_HOP, binding.SONO_COLUMNS,
                   binding.SONO_BANDS] + [dt.fields[n][1] for n in ref.FIELDS] + [13]
    assert dt.itemsize == 32800 and dt.itemsize % 16 == 0 and dt == ref.SONO_DTYPE and dt.names == ref.FIELDS
    assert dt.fields["columns"][1] == 32768 and dt.fields["reserved"][1] == 32792
    assert dt.fields["db"][0].shape == (2, 64, 64) and dt.fields["db"][0].base == np.float32
    assert (ref.WINDOW, ref.HOP, ref.COLUMNS, ref.BANDS) == (binding.SONO_WINDOW, binding.SONO_HOP, binding.SONO_COLUMNS, binding.SONO_BANDS) \
        == (1024, 256, 64, 64)
    assert np.array_equal(binding.SONO_EDGES_HZ, ref.EDGES_HZ) and binding.SONO_EDGES_HZ[0] == 62.5
    assert abs(binding.SONO_EDGES_HZ[64] - 16000.0) < 1e-9 and binding.SONO_EDGES_HZ[8] == 125.0


def _tone(freq, amp, frames, sr=SR):
    return (amp * np.sin(2.0 * np.pi * freq * np.arange(frames) / sr)).astype(np.float32)


@pytest.mark.parametrize("freq,amp", ((1000.0, 0.5), (5000.0, 0.5), (440.0, 0.031), (12000.0, 1.0)))
def test_a_sine_reads_its_amplitude(freq, amp):
    """the power sum of a column's bands is 20 log10 A: the Hann window's coherent gain and noise bandwidth in the cell's factor.
    1e-6 dB: the main lobe's four bins hold all but 1e-7 of the window's power, and float32 samples add 1e-7 relative at most"""
    x = np.stack([_tone(freq, amp, RING), _tone(freq, amp, RING)])[None]
    b = ref.band_powers(x, RING, SR, RING)
    total = 10.0 * np.log10(b[0, 0].sum(axis=-1) * ref.SCALE)
    print(freq, amp, total[0] - 20.0 * np.log10(amp))
    assert np.all(np.abs(total - 20.0 * np.log10(amp)) < 1e-4)
    if amp == 0.5 and freq in (1000.0, 5000.0):
        assert np.all(np.abs(total - (-6.0206)) < 1e-5)  # the header's figure


@pytest.mark.parametrize("k", (-20, -3, 1, 7))
def test_scaling_by_a_power_of_two_moves_every_cell_alike(k):
    rng = np.random.default_rng(1)
    x = np.stack([ref.signal(kind, rng, RING + 100) for kind in ref.KINDS])
    a = ref.sono(x, x.shape[-1], SR, RING)
    b = ref.sono(x * np.float32(2.0 ** k), x.shape[-1], SR, RING)
    fin = np.isfinite(a["db"])
    assert np.array_equal(fin, np.isfinite(b["db"])) and np.array_equal(a["db"][~fin], b["db"][~fin])
    want = a["db"][fin].astype(np.float64) + 20.0 * np.log10(2.0) * k
    # both sides are float32 roundings of float64 values that differ by the shift (the powers scale exactly): half an ulp each
    ulp = np.maximum(np.spacing(np.abs(a["db"][fin])), np.spacing(np.abs(b["db"][fin]))).astype(np.float64)
    assert np.all(np.abs(b["db"][fin].astype(np.float64) - want) <= ulp)
    for name in ref.FIELDS[1:]:
        assert np.array_equal(a[name], b[name])


def test_swapping_the_channels_swaps_the_pictures():
    rng = np.random.default_rng(2)
    x = np.stack([ref.signal(kind, rng, RING + 7) for kind in ref.KINDS])
    a, b = ref.sono(x, x.shape[-1], SR, RING), ref.sono(x[:, ::-1], x.shape[-1], SR, RING)
    assert np.array_equal(a["db"][:, 0], b["db"][:, 1]) and np.array_equal(a["db"][:, 1], b["db"][:, 0])
    assert np.all(np.isneginf(a["db"][1, 1])) and np.any(np.isfinite(a["db"][1, 0]))  # the burst's dead right channel


def test_only_the_frames_of_the_columns_matter():
    """frames older than newest H - (T - 1) H - P and the up-to-255 frames behind newest H change nothing"""
    rng = np.random.default_rng(3)
    t = ref.columns(RING)
    wpos = 3 * RING + 200  # 200 frames behind the newest column's end
    x = np.stack([ref.signal("noise", rng, wpos)])
    a = ref.sono(x, wpos, SR, RING)
    y = x.copy()
    first = wpos - 200 - (t - 1) * H - P
    y[:, :, :first] = 7.0
    y[:, :, wpos - 200:] = -3.0
    assert ref.sono(y, wpos, SR, RING).tobytes() == a.tobytes()
    assert ref.sono(y[:, :, first:], wpos, SR, RING).tobytes() == a.tobytes()
    for at in (first + 1, wpos - 201):  # the first and the last frame that do (frame `first` has the window's weight 0)
        z = x.copy()
        z[:, :, at] += 100.0
        assert ref.sono(z, wpos, SR, RING).tobytes() != a.tobytes()
    assert a["newest"][0] == wpos // H and ref.sono(x, wpos + (1 << 32), SR, RING)["newest"][0] == wpos // H


def test_a_burst_appears_in_the_columns_that_contain_it():
    t = ref.columns(RING)
    wpos = 2 * RING + 77
    x = np.zeros((1, 2, wpos), np.float32)
    f = wpos - 2000  # the burst: 40 frames from here
    x[0, :, f:f + 40] = np.random.default_rng(4).standard_normal((2, 40)).astype(np.float32)
    s = ref.sono(x, wpos, SR, RING)
    newest = wpos // H
    for a in range(t):
        lo, hi = (newest - a) * H - P, (newest - a) * H
        # (frame lo itself has the window's weight 0: a column sees frames lo + 1 .. hi - 1)
        inside = f + 40 > lo + 1 and f < hi
        assert np.any(np.isfinite(s["db"][0, :, a])) == inside, (a, lo, hi)
    assert 3 <= np.count_nonzero(np.isfinite(s["db"][0, 0]).any(axis=1)) <= 5


def test_silence_and_a_dead_channel_read_minus_infinity():
    z = np.zeros((2, 2, RING), np.float32)
    z[1, 0] = -0.0
    s = ref.sono(z, RING, SR, RING)
    assert np.all(np.isneginf(s["db"])) and s[0].tobytes() == s[1].tobytes()
    x = np.stack([ref.signal("noise", np.random.default_rng(5), RING)])
    x[:, 1] = 0
    s = ref.sono(x, RING, SR, RING)
    assert np.all(np.isneginf(s["db"][:, 1])) and np.all(np.isfinite(s["db"][:, 0, :28])) and np.all(np.isneginf(s["db"][:, :, 28:]))
    mono = ref.sono(x[:, :1], RING, SR, RING)  # one captured channel
    assert mono.tobytes() == s.tobytes()
    # a channel 2^-90 under the other is the transform's rounding to the definition; 2^-30 under it is a channel
    x[:, 1] = x[:, 0] * np.float32(2.0 ** -45)
    assert np.all(np.isneginf(ref.sono(x, RING, SR, RING)["db"][:, 1]))
    x[:, 1] = x[:, 0] * np.float32(2.0 ** -15)
    assert np.all(np.isfinite(ref.sono(x, RING, SR, RING)["db"][:, 1, :28]))


def test_bands_outside_the_spectrum():
    x = np.stack([ref.signal("noise", np.random.default_rng(6), RING)])
    low = ref.sono(x, RING, 8000, RING)      # bands from 47 up lie above 4 kHz
    assert (low["first_covered"][0], low["end_covered"][0]) == (0, 47)
    assert np.all(np.isfinite(low["db"][0, :, :28, :48])) and np.all(np.isneginf(low["db"][0, :, :28, 48:]))  # band 47: partly inside
    high = ref.sono(x, RING, 192000, RING)   # bands below 5 start under half a bin: they report what lies above it
    assert (high["first_covered"][0], high["end_covered"][0]) == (5, 64)
    assert np.all(np.isneginf(high["db"][0, :, :28, :4])) and np.all(np.isfinite(high["db"][0, :, :28, 4:]))


def test_mismatches_has_two_arms():
    rng = np.random.default_rng(7)
    x = np.stack([ref.signal(kind, rng, RING + 300) for kind in ref.KINDS])
    wpos = x.shape[-1]
    want = ref.sono(x, wpos, SR, RING)
    bad, arm2 = ref.mismatches(want, x, wpos, SR, RING)
    assert bad == [] and arm2[0] == 0 and arm2[2] > 0
    power = ref.band_powers(x, wpos, SR, RING)
    for name in ref.FIELDS[1:]:
        got = want.copy()
        got[name][1] += 1
        assert {m[0] for m in ref.mismatches(got, x, wpos, SR, RING)[0]} == {name}
    got = want.copy()  # three float32 ulps on a loud cell
    got["db"][0, 0, 3, 40] = np.nextafter(np.nextafter(np.nextafter(got["db"][0, 0, 3, 40], np.float32(9)), np.float32(9)), np.float32(9))
    assert [m[:2] for m in ref.mismatches(got, x, wpos, SR, RING)[0]] == [("db", (0, 0, 3, 40))]
    got["db"][0, 0, 3, 40] = np.nextafter(np.nextafter(want["db"][0, 0, 3, 40], np.float32(9)), np.float32(9))
    assert ref.mismatches(got, x, wpos, SR, RING)[0] == []
    # a cell far under its column's largest: the second arm holds its linear power, not its dB
    share = power[2] / power[2].max(axis=(0, 2), keepdims=True)
    c, a, b = (int(v) for v in np.argwhere((share < 1e-12) & (share > 0))[0])
    got = want.copy()
    got["db"][2, c, a, b] += np.float32(3.0)
    assert ref.mismatches(got, x, wpos, SR, RING)[0] == []
    got["db"][2, c, a, b] = want["db"][2].max()
    assert [m[:2] for m in ref.mismatches(got, x, wpos, SR, RING)[0]] == [("db", (2, c, a, b))]
    for wrong in (np.nan, np.inf):
        got["db"][2, c, a, b] = wrong
        assert len(ref.mismatches(got, x, wpos, SR, RING)[0]) == 1
    got = want.copy()  # a value where the restatement has none
    got["db"][1, 1, 0, 0] = -300.0
    got["db"][0, 0, 40, 0] = -300.0
    assert sorted(m[1] for m in ref.mismatches(got, x, wpos, SR, RING)[0]) == [(0, 0, 40, 0), (1, 1, 0, 0)]
    assert ref.mismatches(want[:1], x, wpos, SR, RING)[0][0][0] == "shape"


def test_noise_cells_lie_within_the_first_arm():
    """six seeds at T = 64: every cell of independent noise has a band power of at least 1e-9 of its column's largest"""
    lowest = 1.0
    for seed in range(6):
        x = np.stack([ref.signal("noise", np.random.default_rng(seed), 32768)])
        b = ref.band_powers(x, 32768, SR, 32768)
        lowest = min(lowest, float((b / b.max(axis=(1, 3), keepdims=True)).min()))
    print(f"smallest share of a noise cell in its column's largest: {lowest:.3g}")
    assert lowest >= ref.ARM1_RATIO


def test_the_gpu_cases_meet_the_comparisons_conditions():
    """on tests/test_gpu_sono.py's own seeds and shapes: the noise stream's covered cells lie within the first arm; the counter ends
    off the hop grid; the span read wraps the ring; and the chirp's neighbouring columns differ by more than 20 dB in some band, so
    that a misplaced column cannot pass"""
    for case in ref.GPU_CASES:
        fft, sr, ch, kw, ring_frames, ring_cap, t = case
        assert t == ref.columns(ring_cap) and (ring_frames == 0 or ring_frames == ring_cap)
        x = ref.case_audio(case)
        wpos = ref.case_wpos0(case) + x.shape[-1]
        assert x.shape == (3, ch, ring_cap + P // 2 + 3) and wpos % H != 0
        newest_end = wpos - wpos % H
        oldest = newest_end - (t - 1) * H - P
        assert oldest >= ref.case_wpos0(case)  # every frame read was pushed
        assert oldest // ring_cap != (newest_end - 1) // ring_cap  # ring positions run over the ring's end inside the span
        sizes = [hi - lo for lo, hi in ref.packets(np.random.default_rng(ring_cap), x.shape[-1])]
        assert sum(sizes) == x.shape[-1] and all(n % 2 == 1 for n in sizes) and len(set(sizes)) > len(sizes) // 2
        hist = np.concatenate([np.zeros((3, ch, ref.case_wpos0(case)), np.float32), x], axis=2)
        b = ref.band_powers(hist, wpos, sr, ring_cap)
        first, end = ref.covered(sr)
        assert (first, end) == (0, 64)
        share = b[0, :ch] / b[0].max(axis=(0, 2), keepdims=True)
        s = ref.sono(hist, wpos, sr, ring_cap)
        db = s["db"][2, 0, :t].astype(np.float64)
        step = np.abs(db[1:] - db[:-1]).max(axis=1)
        print(f"{ref.case_id(case)}: smallest noise share {share.min():.3g}, smallest step between neighbouring chirp columns {step.min():.1f} dB, "
              f"{len(sizes)} packets")
        assert share.min() >= ref.ARM1_RATIO and step.min() > 20.0
        assert np.any(np.isfinite(s["db"][1, 0, 0]))  # tones last
        if t >= 28:  # (the silence is a quarter of the span: shorter than a window and a hop below that)
            assert np.all(np.isneginf(s["db"][1, 0, t - 1]))  # silence first
        if ch == 2:
            assert np.all(np.isneginf(s["db"][1, 1]))
    assert [c[6] for c in ref.GPU_CASES] == [4, 12, 28, 64, 60, 28] and [c[2] for c in ref.GPU_CASES].count(1) == 1
    assert [ref.case_id(c) for c in ref.GPU_CASES] == ["ring2048_sr48000_ch2_fft128", "ring4096_sr48000_ch1_fft1024", "ring8192_sr44100_ch2_fft4096",
                                                      "ring32768_sr48000_ch2_fft4096", "ring16384_sr48000_ch2_fft4096", "ring8192_sr48000_ch2_meter"]


def test_sono_kernels_have_no_scratch():
    res = kernel_usage("wf_hip_measure", "sono_read_kernel")
    assert len(res) == 2 and any("ILi1E" in n for n in res) and any("ILi2E" in n for n in res), res  # <1> and <2>
    for name, r in res.items():
        assert r.get("ScratchSize [bytes/lane]") == 0 and r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
        assert r.get("LDS Size [bytes/block]") == 0, (name, r)  # the four columns' transforms are dynamic LDS
        # two workgroups of four waves to a CU: two waves to a SIMD, and twice 64 KB within a CU's 160 KB of LDS
        assert r.get("Occupancy [waves/SIMD]") >= 2, (name, r)
    assert 2 * 4 * P * 16 <= 160 * 1024
    res = kernel_usage("wf_hip_measure", "stereo_read_kernel")
    assert len(res) == 1, res
    for name, r in res.items():
        assert r.get("ScratchSize [bytes/lane]") == 0 and r.get("VGPRs Spill") == 0, (name, r)
