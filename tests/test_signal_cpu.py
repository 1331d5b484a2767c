"""Signal statistics (WF_HIP_OUT_SIGNAL) without a device: the structured dtype against the C layout, the appended output
number, the float64 reference (tests/signal_ref.py) against analytic cases, and a gfx950 compile of the
read kernel with no scratch."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from waveform_amd import binding
import signal_ref as ref
from kernel_usage import kernel_usage

ROOT = Path(__file__).resolve().parents[1]


def test_signal_dtype_matches_the_c_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wf_hip.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %d", sizeof(wf_hip_signal), sizeof(wf_hip_channel_signal), (int)WF_HIP_OUT_SIGNAL);\n'
                   '  printf(" %zu %zu %zu %zu %zu", offsetof(wf_hip_signal, ch), offsetof(wf_hip_signal, correlation),\n'
                   "         offsetof(wf_hip_signal, balance_db), offsetof(wf_hip_signal, mid_db), offsetof(wf_hip_signal, side_db));\n"
                   '  printf(" %zu %zu %zu %zu", offsetof(wf_hip_channel_signal, rms_db), offsetof(wf_hip_channel_signal, peak_db),\n'
                   "         offsetof(wf_hip_channel_signal, dc), offsetof(wf_hip_channel_signal, clipped));\n"
                   '  printf(" %.17g", (double)WF_HIP_FULL_SCALE);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    got, full_scale = [int(v) for v in out[:-1]], float(out[-1])
    dt, ch = binding.SIGNAL_DTYPE, binding.CHANNEL_SIGNAL_DTYPE
    want = [dt.itemsize, ch.itemsize, binding.OUT_SIGNAL] + [dt.fields[n][1] for n in ("ch", "correlation", "balance_db", "mid_db", "side_db")] \
        + [ch.fields[n][1] for n in ("rms_db", "peak_db", "dc", "clipped")]
    assert got == want
    assert dt.itemsize == 48 and ch.itemsize == 16 and dt["ch"].shape == (2,)
    assert full_scale == 32767 / 32768 == float(binding.FULL_SCALE) == float(ref.FULL_SCALE)


def test_signal_output_is_appended_after_peaks():
    assert binding.OUT_SIGNAL == binding.OUT_PEAKS + 1  # the existing outputs keep their numbers


def _one(window):
    """the reference of one stream: window float32 [channels, W]"""
    r = ref.signal(np.asarray(window, np.float32)[None])
    return {k: v[0] for k, v in r.items()}


def test_reference_full_scale_sine_and_square():
    W = 4096
    n = np.arange(W)
    sine = np.sin(2 * np.pi * 7 * n / W).astype(np.float32)  # 7 whole periods
    r = _one(np.stack([sine, 0.5 * sine]))
    assert abs(r["rms_db"][0] - 10 * np.log10(0.5)) < 1e-6 and abs(r["rms_db"][0] + 3.0103) < 1e-4
    assert abs(r["rms_db"][1] - (10 * np.log10(0.125))) < 1e-6
    assert abs(r["dc"][0]) < 1e-7 and r["peak_db"][0] <= 0.0 and r["peak_db"][0] > -1e-6
    assert r["correlation"] == pytest.approx(1.0, abs=1e-12)
    assert r["balance_db"] == pytest.approx(20 * np.log10(0.5), abs=1e-9)  # right is 6 dB quieter
    square = np.where(n % 64 < 32, 1.0, -1.0).astype(np.float32)
    r = _one(np.stack([square, square]))
    assert r["rms_db"][0] == 0.0 and r["peak_db"][0] == 0.0 and r["dc"][0] == 0.0
    assert np.all(r["clipped"] == W)
    # the threshold: s16's positive extreme counts, u8's does not
    edge = np.array([32767 / 32768, 127 / 128, -1.0, 0.9999], np.float32)
    r = _one(edge[None])
    assert r["clipped"][0] == 2 and r["clipped"][1] == 0


def test_reference_stereo_phase():
    W = 1024
    rng = np.random.default_rng(1)
    x = rng.uniform(-0.5, 0.5, W).astype(np.float32)
    same = _one(np.stack([x, x]))
    assert same["correlation"] == 1.0 and same["balance_db"] == 0.0
    assert np.isneginf(same["side_db"]) and same["mid_db"] == same["rms_db"][0]
    inv = _one(np.stack([x, -x]))
    assert inv["correlation"] == -1.0 and inv["balance_db"] == 0.0
    assert np.isneginf(inv["mid_db"]) and inv["side_db"] == inv["rms_db"][0]
    # one side silent: balance +-inf, correlation 0; a silent stream: nothing to report
    right_only = _one(np.stack([np.zeros(W, np.float32), x]))
    assert right_only["balance_db"] == np.inf and right_only["correlation"] == 0.0
    assert np.isneginf(right_only["rms_db"][0]) and np.isneginf(right_only["peak_db"][0])
    left_only = _one(np.stack([x, np.zeros(W, np.float32)]))
    assert left_only["balance_db"] == -np.inf and left_only["correlation"] == 0.0
    # mid and side of uncorrelated channels each carry half of the mean power
    assert abs(left_only["mid_db"] - (left_only["rms_db"][0] - 10 * np.log10(4))) < 1e-9
    silent = _one(np.zeros((2, W), np.float32))
    assert silent["correlation"] == 0.0 and silent["balance_db"] == 0.0
    assert np.all(np.isneginf(silent["rms_db"])) and np.isneginf(silent["mid_db"]) and np.isneginf(silent["side_db"])
    # one captured channel
    mono = _one(x[None])
    assert np.isneginf(mono["rms_db"][1]) and np.isneginf(mono["peak_db"][1]) and mono["dc"][1] == 0 and mono["clipped"][1] == 0
    assert mono["correlation"] == 0.0 and mono["balance_db"] == 0.0 and np.isneginf(mono["mid_db"]) and np.isneginf(mono["side_db"])


def test_history_keeps_the_newest_window_zero_prefixed():
    h = ref.History(2, 1, 8)
    h.push(np.arange(1, 4, dtype=np.float32).reshape(1, 1, 3))
    assert h.window()[0, 0].tolist() == [0, 0, 0, 0, 0, 1, 2, 3]
    h.push(np.arange(10, 30, dtype=np.float32).reshape(1, 1, 20), first=1)  # longer than the window: its tail
    assert h.window()[1, 0].tolist() == list(range(22, 30))
    h.push(np.full((2, 1, 4), 5, np.float32), frames=[0, 2])
    assert h.window()[0, 0].tolist() == [0, 0, 0, 0, 0, 1, 2, 3] and h.window()[1, 0].tolist() == [24, 25, 26, 27, 28, 29, 5, 5]
    h.reset(1, 1)
    assert not h.window()[1].any()


def test_signal_kernel_has_no_scratch():
    res = kernel_usage("wf_hip_measure", "signal_read_kernel")
    assert len(res) == 2, res  # mono and stereo capture
    for name, r in res.items():
        assert r.get("ScratchSize [bytes/lane]") == 0 and r.get("VGPRs Spill") == 0, (name, r)
        assert r.get("Occupancy [waves/SIMD]") == 8, (name, r)
