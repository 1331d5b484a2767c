"""Oscilloscope (WF_HIP_OUT_SCOPE) without a device: the structured dtype against the C layout, the appended output number, the
properties the definition promises of its float64 restatement (tests/scope_ref.py), the condition of the signals the device test
pushes, and a gfx950 compile of the read kernel with no scratch and no static LDS."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from waveform_amd import binding
import scope_ref as ref
from kernel_usage import kernel_usage

ROOT = Path(__file__).resolve().parents[1]
FIELDS = ("lo", "hi", "window", "view", "columns", "start", "triggered", "period", "frac", "reserved")


def test_scope_dtype_matches_the_c_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wf_hip.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %d %d %d %d", sizeof(wf_hip_scope), (int)WF_HIP_OUT_SCOPE, (int)WF_HIP_OUT_CQ, (int)WF_HIP_SCOPE_MAX_WINDOW,\n'
                   "         (int)WF_HIP_SCOPE_COLUMNS);\n"
                   + "".join(f'  printf(" %zu", offsetof(wf_hip_scope, {n}));\n' for n in FIELDS) +
                   '  printf(" %d", (int)WF_HIP_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    dt = binding.SCOPE_DTYPE
    assert got == [dt.itemsize, binding.OUT_SCOPE, binding.OUT_CQ, binding.SCOPE_MAX_WINDOW, binding.SCOPE_COLUMNS] \
        + [dt.fields[n][1] for n in FIELDS] + [13]
    assert dt.itemsize == 4128 and dt == ref.SCOPE_DTYPE and dt.names == FIELDS
    assert dt.fields["lo"][0].shape == dt.fields["hi"][0].shape == (2, 256)
    assert ref.MAX_WINDOW == binding.SCOPE_MAX_WINDOW == 8192 and ref.COLUMNS == binding.SCOPE_COLUMNS == 256
    assert binding.MEASURES["scope"] == (binding.OUT_SCOPE, dt, False)


def _sine(f, amp, sr, frames, dc=0.0, phase=0.3):
    return (amp * np.sin(2.0 * np.pi * f * np.arange(frames) / sr + phase) + dc).astype(np.float32)


@pytest.mark.parametrize("f", (100.0, 440.0, 1234.5, 5000.0))
def test_a_sine_with_a_dc_offset_triggers(f):
    """a DC offset larger than the amplitude: no sample ever crosses zero, the 50 % level is crossed all the same"""
    sr, w = 48000, 4096
    x = np.stack([_sine(f, 0.2, sr, w, dc=0.5), _sine(f, 0.1, sr, w, dc=0.3)])
    s = ref.scope_one(x, w)
    u, hyst = ref.trigger_signal(x)
    start = int(s["start"])
    assert s["triggered"] == 1 and abs(int(s["period"]) - sr / f) <= 1.0
    assert 1 <= start <= w - w // 2 and u[start - 1] < 0.0 <= u[start] and hyst > 0.0
    assert 0.0 < s["frac"] <= 1.0 and s["frac"] == np.float32(u[start - 1] / (u[start - 1] - u[start]))
    assert x.min() > 0.0 and start + int(s["period"]) > w - w // 2  # the last trigger that leaves room for the view
    assert (s["window"], s["view"], s["columns"], s["reserved"]) == (w, w // 2, 256, 0)


def test_a_second_harmonic_does_not_halve_the_period():
    t, w = 100, 1024
    x = ref.table_periodic(t, w + 7)
    assert ref.rising_crossings(x[:10 * t]) == 20  # two upward crossings of the level per period ...
    for phase in range(0, t, 7):
        s = ref.scope_one(ref.table_periodic(t, w, phase)[None], w)
        assert s["triggered"] == 1 and s["period"] == t, (phase, s["period"])  # ... and one trigger
    # the picture stands still: whatever the phase, the trace is that of phase 0
    first = ref.scope_one(ref.table_periodic(t, w, 0)[None], w)
    for phase in (1, 13, 99):
        s = ref.scope_one(ref.table_periodic(t, w, phase)[None], w)
        assert np.array_equal(s["lo"], first["lo"]) and np.array_equal(s["hi"], first["hi"]) and s["frac"] == first["frac"]


def test_flat_signals_free_run():
    w = 1024
    ramp = np.linspace(-0.5, 0.5, w, dtype=np.float32)
    for name, x in (("silence", np.zeros((2, w), np.float32)), ("constant", np.full((2, w), 0.25, np.float32)),
                    ("l = -r", np.stack([ramp, -ramp])), ("mono constant", np.full((1, w), -0.5, np.float32))):
        s = ref.scope_one(x, w)
        assert (s["start"], s["triggered"], s["period"], s["frac"]) == (w - w // 2, 0, 0, 0.0), name
        edges = ref.column_edges(w // 2, 256)
        for ch in range(x.shape[0]):
            view = x[ch, w // 2:]
            assert np.array_equal(s["lo"][ch], np.minimum.reduceat(view, edges[:-1])), name
            assert np.array_equal(s["hi"][ch], np.maximum.reduceat(view, edges[:-1])), name
    assert not ref.scope_one(np.zeros((2, w), np.float32), w)["lo"].any()


def test_a_trigger_after_the_last_start_free_runs():
    w = 1024
    for at, triggered in ((w // 2 + 10, 0), (w // 2 + 1, 0), (w // 2, 1), (100, 1)):
        x = np.full((1, w), -1.0, np.float32)
        x[0, at:] = 1.0
        s = ref.scope_one(x, w)
        assert (s["triggered"], s["start"], s["period"]) == (triggered, at if triggered else w // 2, 0), at
        assert s["frac"] == (0.5 if triggered else 0.0)


@pytest.mark.parametrize("v", (32, 64, 500, 1000, 4096))
def test_columns_and_their_boundaries(v):
    w = 2 * v
    p, view, k = ref.geometry(w)
    assert (p, view, k) == (w, v, min(256, v))
    edges = ref.column_edges(v, k)
    assert edges[0] == 0 and edges[-1] == v and all(b > a for a, b in zip(edges, edges[1:]))  # never empty
    assert max(b - a for a, b in zip(edges, edges[1:])) <= 16
    x = np.random.default_rng(v).uniform(-1, 1, (2, w)).astype(np.float32)
    s = ref.scope_one(x, w)
    start = int(s["start"])
    for ch in range(2):
        for c in range(k):  # frame by frame, in plain Python
            frames = [x[ch, start + i] for i in range(c * v // k, (c + 1) * v // k)]
            assert s["lo"][ch, c] == min(frames) and s["hi"][ch, c] == max(frames)
    assert not s["lo"][:, k:].any() and not s["hi"][:, k:].any()
    assert ref.geometry(16384) == (8192, 4096, 256) and ref.geometry(65536)[0] == 8192 and ref.geometry(2193) == (2193, 1096, 256)


def test_only_the_newest_frames_count_and_mono_is_channel_0():
    w = 2000
    x = ref.audio(np.random.default_rng(3), 2, w + 11, w)
    both = ref.scope(x, w)
    assert ref.scope(x[..., 11:], w).tobytes() == both.tobytes()
    older = x.copy()
    older[..., :11] = 7.0
    assert ref.scope(older, w).tobytes() == both.tobytes()
    dual = np.stack([x[:, 0], x[:, 0]], axis=1)
    mono, two = ref.scope(x[:, :1], w), ref.scope(dual, w)
    assert np.array_equal(mono["lo"][:, 0], two["lo"][:, 0]) and np.array_equal(mono["hi"][:, 0], two["hi"][:, 0])
    for name in ("start", "triggered", "period", "frac"):  # t = 2 x_0: every comparison and the quotient are unchanged
        assert np.array_equal(mono[name], two[name]), name
    assert not mono["lo"][:, 1].any() and not mono["hi"][:, 1].any() and np.all(mono["triggered"] == 1)


def test_mismatches_compares_every_field():
    w = 1024
    x = ref.audio(np.random.default_rng(4), 2, w + 5, w)
    want = ref.scope(x, w)
    assert ref.mismatches(want, x, w) == [] and ref.frac_outcome(want, x, w) == "equal"
    for name in ref.INT_FIELDS:
        got = want.copy()
        got[name][1] += 1
        assert [m[0] for m in ref.mismatches(got, x, w)] == [name]
    for name in ("lo", "hi"):
        got = want.copy()
        got[name][0, 1, 255] = np.nextafter(got[name][0, 1, 255], np.float32(2))
        assert [m[0] for m in ref.mismatches(got, x, w)] == [name]
        got = want.copy()
        got[name][1, 0, 3] = np.nan
        assert [m[0] for m in ref.mismatches(got, x, w)] == [name]
    got = want.copy()
    got["frac"][0] = np.nextafter(got["frac"][0], np.float32(2))  # one ulp: the second outcome
    assert ref.mismatches(got, x, w) == [] and ref.frac_outcome(got, x, w) == "within one ulp"
    got["frac"][0] = np.nextafter(got["frac"][0], np.float32(2))
    assert [m[0] for m in ref.mismatches(got, x, w)] == ["frac"]
    z = np.zeros((1, 2, w), np.float32)
    got = ref.scope(z, w)
    got["lo"][0, 0, 0] = -0.0  # -0 equals +0
    assert ref.mismatches(got, z, w) == []


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=ref.case_id)
def test_the_gpu_tests_signal_triggers(case):
    """the condition of tests/test_gpu_scope.py's comparison: on its own seeds and shapes at least 90 % of the streams of every
    case read triggered == 1 and period > 0 in the restatement, so the device cannot pass on free-running streams alone"""
    fft, sr, ch, kw, w = case
    if kw.get("meter"):
        assert w == int(sr * (kw["meter_ms"] / 1000.0)) & -16 and w % 32 != 0
    else:
        assert w == fft
    p, v, _ = ref.geometry(w)
    x = ref.case_audio(case)
    assert x.shape == (3, ch, ref.ring_frames(w) + p // 2 + 3) and x.shape[-1] % 4 != 0
    s = ref.scope(x, w)
    share = np.mean((s["triggered"] == 1) & (s["period"] > 0))
    print(f"{ref.case_id(case)}: P {p}, V {v}, starts {s['start'].tolist()}, periods {s['period'].tolist()}, triggered share {share:.2f}")
    assert share >= 0.9
    assert np.all(s["period"] >= 7) and np.all(s["period"] <= (p - v) / 3.0 + 2)


def test_scope_kernel_has_no_scratch():
    res = kernel_usage("wf_hip_measure", "scope_read_kernel")
    assert len(res) == 2, res  # one and two captured channels
    for name, r in res.items():
        assert r.get("ScratchSize [bytes/lane]") == 0 and r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
        assert r.get("LDS Size [bytes/block]") == 0, (name, r)  # the staged windows and the working set behind them are dynamic
        assert r.get("Occupancy [waves/SIMD]") >= 4, (name, r)
