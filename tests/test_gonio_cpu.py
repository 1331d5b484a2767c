"""Vectorscope (WF_HIP_OUT_GONIO) without a device: the structured dtype against the C layout, the appended output number, the
properties the definition promises of its float64 restatement (tests/gonio_ref.py), the conditions of the signals the device test
pushes, and a gfx950 compile of the read kernel with no scratch and no static LDS."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from waveform_amd import binding
import gonio_ref as ref
from kernel_usage import kernel_usage

ROOT = Path(__file__).resolve().parents[1]
G = ref.GRID


def test_gonio_dtype_matches_the_c_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wf_hip.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %zu %d %d %d %d %d", sizeof(wf_hip_gonio), offsetof(wf_hip_gonio, window), offsetof(wf_hip_gonio, occupied),\n'
                   "         (int)WF_HIP_OUT_GONIO, (int)WF_HIP_OUT_SCOPE, (int)WF_HIP_GONIO_GRID, (int)WF_HIP_GONIO_MAX_WINDOW,\n"
                   "         (int)WF_HIP_GONIO_MIN_EXP);\n"
                   + "".join(f'  printf(" %zu", offsetof(wf_hip_gonio, {n}));\n' for n in ref.FIELDS) +
                   '  printf(" %d", (int)WF_HIP_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    dt = binding.GONIO_DTYPE
    assert got == [dt.itemsize, dt.fields["window"][1], dt.fields["occupied"][1], binding.OUT_GONIO, binding.OUT_SCOPE, binding.GONIO_GRID,
                   binding.GONIO_MAX_WINDOW, binding.GONIO_MIN_EXP] + [dt.fields[n][1] for n in ref.FIELDS] + [13]
    assert dt.itemsize == 8224 and dt.itemsize % 16 == 0 and dt == ref.GONIO_DTYPE and dt.names == ref.FIELDS
    assert dt.fields["window"][1] == 8192 and dt.fields["occupied"][1] == 8220
    assert dt.fields["cell"][0].shape == (64, 64) and dt.fields["cell"][0].base == np.uint16 and dt.fields["zoom"][0] == np.int32
    assert (ref.GRID, ref.MAX_WINDOW, ref.MIN_EXP) == (binding.GONIO_GRID, binding.GONIO_MAX_WINDOW, binding.GONIO_MIN_EXP) == (64, 8192, -24)


def _noise(seed, p, scale=1.0):
    return (ref.signal("noise", np.random.default_rng(seed), p).astype(np.float64) * scale).astype(np.float32)


@pytest.mark.parametrize("p", (1, 128, 2000, 8192))
def test_the_cells_add_up_to_the_window(p):
    for kind in ref.KINDS:
        s = ref.gonio_one(ref.signal(kind, np.random.default_rng(p), p + 5), p)
        assert s["window"] == p and int(s["cell"].astype(np.int64).sum()) == p, kind
        assert s["occupied"] == np.count_nonzero(s["cell"]) and s["in_phase"] + s["out_phase"] <= p
    assert ref.window_frames(16384) == 8192 and ref.gonio_one(np.zeros((2, 9000), np.float32), 16384)["window"] == 8192


@pytest.mark.parametrize("k", (-20, -3, 1, 2))
def test_scaling_by_a_power_of_two_moves_the_zoom_alone(k):
    x = _noise(1, 1024)
    a, b = ref.gonio_one(x, 1024), ref.gonio_one(x * np.float32(2.0 ** k), 1024)
    assert b["zoom"] == a["zoom"] - k and b["cell"].tobytes() == a["cell"].tobytes()
    assert b["peak"] == a["peak"] * np.float32(2.0 ** k) and b["mid_peak"] == a["mid_peak"] * np.float32(2.0 ** k)
    for name in ("in_phase", "out_phase", "occupied", "window"):
        assert a[name] == b[name]


def test_swapping_the_channels_mirrors_the_picture():
    x = _noise(2, 4096)
    keep = x[0] != x[1]  # a frame with side == 0 sits on the edge of cell 32 and does not mirror
    x = x[:, keep]
    a, b = ref.gonio_one(x, x.shape[1]), ref.gonio_one(x[::-1], x.shape[1])
    assert np.array_equal(b["cell"], a["cell"][:, ::-1]) and a["occupied"] >= 64
    # a side that falls on a cell's edge, k / 32, does not mirror either: there is none here, as the equality shows
    for name in ("zoom", "peak", "mid_peak", "side_peak", "in_phase", "out_phase", "occupied"):
        assert a[name] == b[name], name


def test_mono_and_antiphase_sources_draw_a_line():
    rng = np.random.default_rng(3)
    mono, anti, left = (ref.gonio_one(ref.signal(k, rng, 2048), 2048) for k in ("mono", "antiphase", "left"))
    assert mono["cell"][:, G // 2].sum() == 2048 and mono["side_peak"] == 0 and mono["mid_peak"] == mono["peak"]
    assert anti["cell"][G // 2, :].sum() == 2048 and anti["mid_peak"] == 0 and anti["side_peak"] == anti["peak"]
    assert mono["out_phase"] == 0 and anti["in_phase"] == 0 and mono["in_phase"] == anti["out_phase"] > 2000
    assert left["in_phase"] == left["out_phase"] == 0  # a zero counts in neither
    iy, ix = np.nonzero(left["cell"])
    assert np.all(np.abs((iy - G // 2) + (ix - G // 2) + 1) <= 1)  # up-left: mid = -side


def test_the_range_flips_at_powers_of_two():
    """one frame with r = -A in silence: side = mid = -A / 2, which the range puts between a quarter and a half of the deflection
    (cells 16 .. 24 of 0 .. 31 below the centre) unless the clamp holds it"""
    x = np.zeros((2, 256), np.float32)
    below_half = float(np.nextafter(np.float32(0.5), np.float32(0)))
    for peak, zoom, at in ((0.5, 0, 24), (below_half, 1, 16), (1.0, -1, 24), (0.999, 0, 16), (9.0, -4, 23), (2.0 ** -24, 23, 24),
                           (2.0 ** -25, 24, 24), (2.0 ** -30, 24, 31), (1e-45, 24, 32)):
        x[1, 7] = -peak
        s = ref.gonio_one(x, 256)
        assert s["zoom"] == zoom and s["peak"] == np.float32(peak) and s["peak"] > 0, (peak, s["zoom"])
        assert s["cell"].sum() == 256 and s["cell"][at, at] == (256 if at == G // 2 else 1), (peak, np.nonzero(s["cell"]))
        assert s["out_phase"] == 0 and s["in_phase"] == 0 and s["mid_peak"] == s["side_peak"] == np.float32(peak / 2)


def test_the_clamp_keeps_every_index_in_range():
    x = _noise(4, 1024, ref.CLAMP_SCALE)
    x[0, 5] = np.float32(2.0 ** -30)
    s = ref.gonio_one(x, 1024)
    assert s["zoom"] == 24 and 0 < s["peak"] < 2.0 ** -24 and s["cell"].sum() == 1024
    assert s["cell"][G // 2 - 1:G // 2 + 1, G // 2 - 1:G // 2 + 1].sum() == 1024  # everything next to the centre
    wild = np.array([[3e38, -3e38, np.inf, 1.0], [-3e38, 3e38, 1.0, -np.inf]], np.float32)
    for e in (ref.MIN_EXP, 0, 128):  # whatever the range, the min / max in floating point holds the index
        u, v = ref.coordinates(wild, e)
        assert np.all((ref.index(u) >= 0) & (ref.index(u) < G)) and np.all((ref.index(v) >= 0) & (ref.index(v) < G))
    big = np.array([[1.0, 0.0], [1.0, 0.0]], np.float32)  # one frame at l = r = 1 with the range held at e = -24: the border
    assert ref.index(ref.coordinates(big, ref.MIN_EXP)[1]).tolist() == [G - 1, G // 2]


def test_silence_is_one_cell():
    s = ref.gonio_one(np.zeros((2, 3000), np.float32), 2000)
    assert s["cell"][G // 2, G // 2] == 2000 and s["occupied"] == 1 and s["zoom"] == 0 and s["peak"] == 0
    assert s["mid_peak"] == 0 and s["side_peak"] == 0 and s["in_phase"] == 0 and s["out_phase"] == 0 and s["window"] == 2000
    z = np.zeros((2, 64), np.float32)
    z[0] = -0.0
    assert ref.gonio_one(z, 64).tobytes() == ref.gonio_one(np.zeros((2, 64), np.float32), 64).tobytes()


def test_only_the_newest_frames_count():
    x = _noise(5, 2011)
    older = x.copy()
    older[:, :11] = 7.0
    assert ref.gonio(x[None], 2000).tobytes() == ref.gonio(older[None], 2000).tobytes() == ref.gonio(x[None, :, 11:], 2000).tobytes()


def test_mismatches_compares_every_field():
    x = np.stack([_noise(6, 1024), _noise(7, 1024)])
    want = ref.gonio(x, 1024)
    assert ref.mismatches(want, x, 1024) == [] and ref.mismatches(want, x) == []
    for name in ref.FIELDS:
        got = want.copy()
        if name == "cell":
            got[name][1, 40, 41] += 1
        elif got[name].dtype == np.float32:
            got[name][1] = np.nextafter(got[name][1], np.float32(2))
        else:
            got[name][1] += 1
        assert [m[0] for m in ref.mismatches(got, x, 1024)] == [name]
    assert ref.mismatches(want[:1], x, 1024)[0][0] == "shape"


def test_the_generators_figures():
    """what the kinds look like at the smallest and the largest window (printed; the conditions below are those of the cases)"""
    for p in (128, 8192):
        for kind in ("noise", "mono", "left"):
            s = ref.gonio_one(ref.signal(kind, np.random.default_rng(p), p), p)
            print(f"P {p} {kind}: occupied {int(s['occupied'])}, largest cell {int(s['cell'].max())}, zoom {int(s['zoom'])}")
            assert s["occupied"] >= (64 if kind == "noise" else 8)


def test_the_gpu_cases_are_no_trivial_pictures():
    """the conditions of tests/test_gpu_gonio.py's comparison, on its own seeds and shapes: every noise and Lissajous stream
    occupies at least 64 cells and has no cell above P / 8, the three signs of zoom occur, every kind is pushed, and the window
    the device reads wraps the ring and ends at an odd position"""
    zooms, kinds_seen = [], set()
    for case in ref.GPU_CASES:
        fft, sr, kw, w, kinds = case
        if kw.get("meter"):
            assert w == int(sr * (kw["meter_ms"] / 1000.0)) & -16 == 2208 and w % 64 != 0
        else:
            assert w == fft
        p = ref.window_frames(w)
        x = ref.case_audio(case)
        assert x.shape == (3, 2, ref.ring_frames(w) + p // 2 + 3) and x.shape[-1] % 4 != 0 and len(set(kinds)) == 3
        s = ref.gonio(x, w)
        for k, r in zip(kinds, s):
            print(f"{ref.case_id(case)} {k}: P {p}, zoom {int(r['zoom'])}, occupied {int(r['occupied'])}, largest cell {int(r['cell'].max())}, "
                  f"in / out of phase {int(r['in_phase'])} / {int(r['out_phase'])}")
            assert r["cell"].astype(np.int64).sum() == p == r["window"]
            if k in ref.PICTURE_KINDS:
                assert r["occupied"] >= 64 and r["cell"].max() <= p // 8, (case, k)
            zooms.append(int(r["zoom"]))
        kinds_seen |= set(kinds)
    assert kinds_seen == set(ref.KINDS)
    assert min(zooms) < 0 and 0 in zooms and max(zooms) > 0, zooms
    assert [ref.case_id(c) for c in ref.GPU_CASES] == ["w128", "w1024", "w2000", "w4096", "w16384", "w2208_meter"]
    # the clamp is active in the case test_gpu_gonio.py makes by scaling: zoom 24 with the peak below 2^-24
    x = (ref.case_audio(ref.GPU_CASES[1]).astype(np.float64) * ref.CLAMP_SCALE).astype(np.float32)
    s = ref.gonio(x, 1024)
    assert np.all(s["zoom"][:2] == 24) and np.all(s["peak"][:2] < 2.0 ** -24) and np.all(s["peak"][:2] > 0) and s["occupied"][0] > 1


def test_gonio_kernel_has_no_scratch():
    res = kernel_usage("wf_hip_measure", "gonio_read_kernel")
    assert len(res) == 1, res
    for name, r in res.items():
        assert r.get("ScratchSize [bytes/lane]") == 0 and r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
        assert r.get("LDS Size [bytes/block]") == 0, (name, r)  # the staged windows and the image behind them are dynamic
        assert r.get("Occupancy [waves/SIMD]") >= 4, (name, r)
