"""Band levels (WF_HIP_OUT_BANDS) without a device: the structured dtype against the C layout, the appended output number, the
properties of the float64 restatement (tests/bands_ref.py) the definition promises, sines on the exact
spectrum against analytic truth, and a gfx950 compile of the read kernel with no scratch."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import bands_ref as ref
from kernel_usage import kernel_usage

ROOT = Path(__file__).resolve().parents[1]


def test_bands_dtype_matches_the_c_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wf_hip.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %d %d %d", sizeof(wf_hip_bands), (int)WF_HIP_OUT_BANDS, (int)WF_HIP_OUT_PITCH, (int)WF_HIP_NUM_BANDS);\n'
                   '  printf(" %zu %zu %zu %zu %zu %zu", offsetof(wf_hip_bands, band_db), offsetof(wf_hip_bands, covered),\n'
                   "         offsetof(wf_hip_bands, total_db), offsetof(wf_hip_bands, a_db), offsetof(wf_hip_bands, c_db),\n"
                   "         offsetof(wf_hip_bands, reserved));\n"
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    dt = binding.BANDS_DTYPE
    assert got == [dt.itemsize, binding.OUT_BANDS, binding.OUT_PITCH, binding.NUM_BANDS] \
        + [dt.fields[n][1] for n in ("band_db", "covered", "total_db", "a_db", "c_db", "reserved")]
    assert dt.itemsize == 144 and dt == ref.BANDS_DTYPE and binding.NUM_BANDS == ref.NUM_BANDS == 31
    assert dt.fields["band_db"][0].shape == (31,)


def test_bands_output_is_appended_after_pitch():
    assert binding.OUT_BANDS == binding.OUT_PITCH + 1 == 14  # the existing outputs keep their numbers


def test_the_restatement_floors_at_the_librarys_db_min():
    assert np.float32(wf.db_min()) == ref.DB_MIN


def test_grid_is_iec_61260_base_ten():
    c, e = ref.centres_hz(), ref.edges_hz()
    assert np.array_equal(c, binding.BAND_CENTRES_HZ) and c.shape == (31,) and e.shape == (32,)
    assert c[17] == 1000.0 and abs(c[0] - 19.953) < 1e-3 and abs(c[30] - 19952.6) < 0.1 and abs(c[27] / c[17] - 10.0) < 1e-12
    # the edges meet: band b ends where band b + 1 begins (one array), each the geometric mean of the centres beside it,
    # and every band is a tenth of a decade wide
    assert np.allclose(e[1:-1], np.sqrt(c[:-1] * c[1:]), rtol=1e-14)
    assert np.allclose(e[1:] / e[:-1], 10.0 ** 0.1, rtol=1e-14)
    assert np.allclose(e[:-1] * 10.0 ** 0.05, c, rtol=1e-14)


@pytest.mark.parametrize("n,sr", [(128, 48000), (800, 44100), (4096, 48000), (4800, 96000), (65536, 48000), (65536, 8000)])
def test_bin_weights_partition_the_grid(n, sr):
    m = n // 2
    w = ref.bin_weights(sr, n)
    e = ref.edges_bins(sr, n)
    assert w.shape == (31, m) and np.all(w >= 0.0) and np.all(w <= 1.0)
    k = np.arange(m)
    inside = (k - 0.5 >= e[0]) & (k + 0.5 <= e[31])
    assert np.allclose(w.sum(axis=0)[inside], 1.0, rtol=0, atol=1e-9)  # a bin inside the grid is shared out wholly
    assert np.all(w.sum(axis=0) <= 1.0 + 1e-9)
    # a band's weights add up to its width, as far as the band lies on the bins' axis [-0.5, M - 0.5]
    want = np.clip(np.minimum(e[1:], m - 0.5) - np.maximum(e[:-1], -0.5), 0.0, None)
    assert np.allclose(w.sum(axis=1), want, rtol=0, atol=1e-8)
    # the bins of a band are contiguous and the bands ascend
    for b in range(31):
        nz = np.nonzero(w[b])[0]
        if len(nz):
            assert np.array_equal(nz, np.arange(nz[0], nz[-1] + 1))


def test_covered_for_a_few_shapes():
    def bands_of(bits):
        return [b for b in range(32) if bits >> b & 1]
    # 48 kHz, FFT 4096: a bin is 11.7 Hz; band 0 begins at 17.8 Hz = bin 1.52; band 30 ends at 22.39 kHz, under 24 kHz
    assert bands_of(ref.covered(48000, 4096)) == list(range(31))
    # FFT 128: a bin is 375 Hz, the first edge at or above bin 0.5 (187.5 Hz) is 223.9 Hz, the lower edge of band 11
    assert bands_of(ref.covered(48000, 128)) == list(range(11, 31))
    # 44.1 kHz: the row ends at bin M - 0.5 = 22.04 kHz, below band 30's upper edge
    assert bands_of(ref.covered(44100, 4096)) == list(range(30))
    assert bands_of(ref.covered(96000, 65536)) == list(range(31))
    assert bands_of(ref.covered(8000, 1024)) == list(range(23))  # 3.996 kHz: band 22 (3.16 kHz) ends at 3.55 kHz
    for sr, n in ((48000, 128), (44100, 800), (8000, 1024)):
        assert ref.covered(sr, n) >> 31 == 0


def test_weightings_are_one_at_1_khz_and_follow_the_standard():
    assert ref.a_weight(1000.0) == 1.0 and ref.c_weight(1000.0) == 1.0
    db = lambda w: 10.0 * np.log10(w)  # noqa: E731
    # IEC 61672-1 table 2 (rounded to 0.1 dB there; its nominal 31.5 Hz, 2 kHz and 20 kHz are the exact base-ten frequencies)
    for f, a, c in ((10.0 ** 1.5, -39.4, -3.0), (100.0, -19.1, -0.3), (1000.0, 0.0, 0.0), (10.0 ** 3.3, 1.2, -0.2), (10000.0, -2.5, -4.4),
                    (10.0 ** 4.3, -9.3, -11.2)):
        assert abs(db(ref.a_weight(f)) - a) < 0.06 and abs(db(ref.c_weight(f)) - c) < 0.06, f
    assert ref.a_weight(0.0) == 0.0 and ref.c_weight(0.0) == 0.0


def test_enbw_of_the_windows():
    n = 4096
    i = np.arange(n)
    hann = (0.5 * (1 - np.cos(2 * np.pi * i / (n - 1)))).astype(np.float32)
    assert abs(ref.enbw(hann, n) - 1.5 * n / (n - 1)) < 1e-6
    assert ref.enbw(None, n) == 1.0 and ref.enbw(np.ones(n, np.float32), n) == 1.0


def test_band_sums_add_up_to_the_total_of_their_bins():
    rng = np.random.default_rng(5)
    n, sr = 4096, 48000
    rows = rng.uniform(-90.0, -10.0, (3, 2, n // 2)).astype(np.float32)
    rows[0, 0, 100:200] = ref.DB_MIN  # no power
    rows[1, 1, :] = ref.DB_MIN
    got = ref.bands(rows, None, sr, n)
    p = ref.powers(rows)
    assert np.all(p[0, 0, 100:200] == 0.0) and np.all(p[..., 0] == 0.0)
    w = ref.bin_weights(sr, n)
    grid = w.sum(axis=0)
    with np.errstate(divide="ignore"):
        from_bands = 10.0 * np.log10(np.sum(10.0 ** (got["band_db"].astype(np.float64) / 10.0), axis=-1))
        from_bins = 10.0 * np.log10(np.sum(p * grid, axis=-1))
    assert np.allclose(from_bands[np.isfinite(from_bins)], from_bins[np.isfinite(from_bins)], rtol=0, atol=1e-5)
    assert np.all(np.isneginf(got["band_db"][1, 1])) and np.isneginf(got["total_db"][1, 1]) and np.isneginf(got["a_db"][1, 1])
    assert got["covered"][1, 1] == ref.covered(sr, n) and np.all(got["reserved"] == 0)
    assert np.all(got["total_db"][0] >= got["band_db"][0].max(axis=-1))
    # the two orders of addition agree within the contract's bound
    assert ref.mismatches(ref.bands(rows, None, sr, n, reverse=True), got) == []


def _exact_rows(bins, amp, n, window):
    """|X| 2 / window_sum in dB of sines at `bins` (cycles per n frames), from a float64 FFT: float32 [len(bins), M]"""
    t = np.arange(n)
    w = window.astype(np.float64)
    rows = []
    for b in bins:
        x = amp * np.sin(2 * np.pi * b / n * t + 0.3)
        mag = np.abs(np.fft.rfft(x * w))[:n // 2] * 2.0 / w.sum()
        rows.append(20.0 * np.log10(np.maximum(mag, 1e-30)))
    return np.asarray(rows, np.float32)


def test_sines_on_the_exact_spectrum_read_their_amplitude():
    """Hann, N = 4096, 48 kHz, amplitude 0.5 at bins 85.0, 85.37, 200.5 and 1000.25: total and the sine's band read 20 log10(0.5)
    whatever the offset between bins, and a - total, c - total read the curves at the sine's frequency."""
    n, sr, amp = 4096, 48000, 0.5
    bins = (85.0, 85.37, 200.5, 1000.25)
    hann = (0.5 * (1 - np.cos(2 * np.pi * np.arange(n) / (n - 1)))).astype(np.float32)
    got = ref.bands(_exact_rows(bins, amp, n, hann), hann, sr, n)
    truth = 20.0 * np.log10(amp)
    for i, (b, band) in enumerate(zip(bins, (17, 17, 21, 28))):
        f = b * sr / n
        e = ref.edges_bins(sr, n)
        assert e[band] + 3 <= b <= e[band + 1] - 3  # the main lobe is not split
        print(b, got["total_db"][i], got["band_db"][i, band], got["a_db"][i] - got["total_db"][i])
        assert abs(got["total_db"][i] - truth) < 1e-4 and abs(got["band_db"][i, band] - truth) < 1e-4
        assert abs((got["a_db"][i] - got["total_db"][i]) - 10 * np.log10(ref.a_weight(f))) < 2e-3
        assert abs((got["c_db"][i] - got["total_db"][i]) - 10 * np.log10(ref.c_weight(f))) < 2e-3
    assert np.all(got["covered"] == 0x7fffffff)


def test_mismatches_bound():
    want = np.zeros(1, ref.BANDS_DTYPE)
    want["band_db"] = -20.0
    want["band_db"][0, 3] = -np.inf
    got = want.copy()
    assert ref.mismatches(got, want) == []
    got["band_db"][0, 5] = np.nextafter(np.float32(-20.0), np.float32(0))  # one ulp
    assert ref.mismatches(got, want) == []
    got["band_db"][0, 5] = np.nextafter(got["band_db"][0, 5], np.float32(0))  # two
    assert len(ref.mismatches(got, want)) == 1
    got = want.copy()
    got["band_db"][0, 3] = -700.0
    got["covered"] = 1
    assert [m[0] for m in ref.mismatches(got, want)] == ["band_db", "covered"]
    got = want.copy()
    got["total_db"] = np.nan
    assert [m[0] for m in ref.mismatches(got, want)] == ["total_db"]


def test_bands_kernel_has_no_scratch():
    res = kernel_usage("wf_hip_measure", "bands_read_kernel")
    assert len(res) == 1, res
    for name, r in res.items():
        assert r.get("ScratchSize [bytes/lane]") == 0 and r.get("VGPRs Spill") == 0 and r.get("LDS Size [bytes/block]") == 0, (name, r)
        assert r.get("Occupancy [waves/SIMD]") >= 4, (name, r)
