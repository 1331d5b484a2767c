"""Spectral peaks (WF_HIP_OUT_PEAKS) without a device: the structured dtype against the C layout, the appended output number,
the float64 reference (tests/peaks_ref.py) against exact parabolas and hand-built rows, and a gfx950 compile
of the read kernel with no scratch."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import peaks_ref as ref
from kernel_usage import kernel_usage

ROOT = Path(__file__).resolve().parents[1]


def test_peaks_dtype_matches_the_c_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wf_hip.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %d %d", sizeof(wf_hip_peaks), sizeof(wf_hip_peak), WF_HIP_MAX_PEAKS, (int)WF_HIP_OUT_PEAKS);\n'
                   '  printf(" %zu %zu %zu", offsetof(wf_hip_peaks, count), offsetof(wf_hip_peaks, reserved), offsetof(wf_hip_peaks, peak));\n'
                   '  printf(" %zu %zu", offsetof(wf_hip_peak, hz), offsetof(wf_hip_peak, db));\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    dt, peak = binding.PEAKS_DTYPE, binding.PEAKS_DTYPE["peak"].base
    want = [dt.itemsize, peak.itemsize, binding.MAX_PEAKS, binding.OUT_PEAKS,
            dt.fields["count"][1], dt.fields["reserved"][1], dt.fields["peak"][1], peak.fields["hz"][1], peak.fields["db"][1]]
    assert got == want
    assert dt.itemsize == 72 and binding.MAX_PEAKS == ref.MAX_PEAKS == 8


def test_peaks_output_is_appended_after_loudness():
    assert binding.OUT_PEAKS == binding.OUT_LOUDNESS + 1  # the existing outputs keep their numbers


def test_reference_recovers_the_vertex_of_an_exact_parabola():
    M, fs, n = 512, 48000, 1024
    for k0, frac, top in ((100, 0.3, -12.0), (37, -0.45, -3.5), (400, 0.0, -60.0), (5, 0.5, -20.0)):
        x = np.arange(M, dtype=np.float64)
        row = (top - 0.02 * (x - (k0 + frac)) ** 2).astype(np.float32)
        count, k, hz, db = ref.peaks(row, -100, fs, n)
        # float32 rows: the vertex within what rounding the three values to float32 allows
        assert count == 1 and k[0] == k0, (k0, frac, count, k)  # (frac 0.5: a two-bin plateau, its first bin, p = +0.5)
        assert abs(hz[0] - (k0 + frac) * fs / n) < 1e-3 * fs / n, (k0, frac, hz[0])
        assert abs(db[0] - top) < 1e-4, (k0, frac, db[0])
        assert np.all(hz[1:] == 0) and np.all(np.isneginf(db[1:]))


def test_reference_tie_and_threshold_rules():
    floor = -70
    d = np.full(32, -80.0, np.float32)
    d[[3, 9, 15]] = -10.0         # equal values: lower bin first
    d[20] = -70.0                 # not above the floor
    d[22], d[23] = -30.0, -30.0   # a plateau: d[k] > d[k-1] and d[k] >= d[k+1] holds at its first bin only
    d[0], d[31] = 0.0, 0.0        # the edges are never candidates
    count, k, hz, db = ref.peaks(d, floor, 48000, 64)
    assert count == 4 and list(k[:4]) == [3, 9, 15, 22]
    assert np.all(k[4:] == -1)
    # more than eight candidates: the eight strongest, strongest first
    d = np.full(64, -90.0, np.float32)
    vals = -np.arange(12, dtype=np.float32)[::-1]  # -11 .. 0
    d[2:2 + 4 * 12:4] = vals
    count, k, hz, db = ref.peaks(d, floor, 48000, 128)
    assert count == 8 and list(k) == [2 + 4 * i for i in range(11, 3, -1)]
    assert np.all(np.diff(db) < 0)
    # a flat row and a row at DB_MIN have none
    for row in (np.full(64, -20.0, np.float32), np.full(64, wf.db_min(), np.float32)):
        count, k, hz, db = ref.peaks(row, floor, 48000, 128)
        assert count == 0 and np.all(hz == 0) and np.all(np.isneginf(db))


def test_peaks_kernel_has_no_scratch():
    found = kernel_usage("wf_hip_measure", "peaks_read_kernel")
    assert len(found) == 1, found
    (res,) = found.values()
    assert res.get("ScratchSize [bytes/lane]") == 0 and res.get("VGPRs Spill") == 0, res
    assert res.get("Occupancy [waves/SIMD]") == 8, res  # one row per wavefront: 8192 rows fill 256 CUs x 4 SIMDs x 8 at once
