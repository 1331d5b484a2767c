"""The host tables of the measurement outputs (waveform_amd/csrc/wf_measure_tables.cpp) without a device: the library's own
builders, compiled into a program of their own, against the float64 restatements (tests/bands_ref.py, stereo_ref.py, cq_ref.py)
and numpy; the same program once more under the address and undefined-behaviour sanitizers; the readers of the two batch
classes being the same functions over one table that is the C table's twin; and, once for all measurement outputs, the ABI version,
the exported entry points and every output's number.

Bound of the float64 comparisons: rtol 1e-12 (atol 1e-300 for exact zeros), the figure test_loudness_cpu.py uses for the filter
design: four orders of magnitude above what a handful of correctly rounded double operations and two libm calls can differ by,
eight below the float32 resolution of any output.  Integers and masks are compared exactly."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from waveform_amd import binding
import bands_ref
import cq_ref
import stereo_ref

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "waveform_amd" / "csrc"
RTOL, ATOL = 1e-12, 1e-300

BANDS_CASES = [(48000, 1024), (44100, 2000), (8000, 128), (96000, 4096)]  # (sample rate, fft size); also the stereo image's
CQ_RATES = (8000, 44100, 48000, 96000)
CQ_RINGS = (128, 4096, 16384, 32768)
WAVES, HEAD, BIN_DOUBLES, SCHED_WORDS = 16, 8, 8 + 64 * 4, 16 + 1 + 120  # WF_CQ_WAVES, _BIN_HEAD, _BIN_DOUBLES, _SCHED_WORDS

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include "wf_measure_tables.hpp"
using namespace wf::host;
static void row(const std::vector<double> &v) { for(double x : v) std::printf(" %.17g", x); }
int main() {
  static_assert(wf::WF_CQ_WAVES == 16 && wf::WF_CQ_BIN_HEAD == 8 && wf::WF_CQ_BIN_DOUBLES == 264 && wf::WF_CQ_SCHED_WORDS == 137);
  const unsigned cases[4][2] = {{48000, 1024}, {44100, 2000}, {8000, 128}, {96000, 4096}};
  for(auto &c : cases) {
    const unsigned sr = c[0], N = c[1], M = N / 2;
    for(int hann = 0; hann < 2; ++hann) {
      std::vector<float> w;  // (the same float32 Hann window the test makes; empty: no window)
      for(unsigned i = 0; hann && i < N; ++i) w.push_back((float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)i / (double)N)));
      const BandsTables b = bands_tables(sr, N, M, w);
      double e[WF_HIP_NUM_BANDS + 1];
      const unsigned cov = third_octave_edges(sr, N, M, e);
      for(int j = 0; j <= WF_HIP_NUM_BANDS; ++j) if(e[j] != b.edges[j]) return 2;
      if(b.edges.size() != WF_HIP_NUM_BANDS + 1 || b.weights.size() != 2 * (size_t)M || cov != b.covered) return 2;
      std::printf("B %u %u %d %u %.17g", sr, N, hann, b.covered, b.enbw); row(b.edges); row(b.weights); std::printf("\n");
    }
    const StereoTables s = stereo_tables(sr, N);
    if(s.P != stereo_window(N) || s.tab.size() != 2 * (size_t)s.P + WF_HIP_NUM_BANDS + 1) return 3;
    std::printf("S %u %u %u %u %u", sr, N, s.P, s.log2p, s.covered); row(s.tab); std::printf("\n");
  }
  for(unsigned sr : {8000u, 44100u, 48000u, 96000u}) for(unsigned ring : {128u, 4096u, 16384u, 32768u}) {
    const CqTables q = cq_tables(sr, ring);
    if(q.sched.size() != wf::WF_CQ_SCHED_WORDS || q.tab.size() != (size_t)q.end_covered * wf::WF_CQ_BIN_DOUBLES) return 4;
    std::printf("C %u %u %u %u %u", sr, ring, q.max_window, q.end_covered, q.first_resolved);
    for(unsigned v : q.sched) std::printf(" %u", v);
    row(q.tab); std::printf("\n");
  }
  return 0;
}
"""


def _build_and_run(directory, name, extra=()):
    src = directory / "tables_main.cpp"
    src.write_text(PROGRAM)
    exe = directory / name
    subprocess.run(["g++", "-std=c++20", "-O2", *extra, "-I", str(CSRC), "-I", str(ROOT / "include"), str(src),
                    str(CSRC / "wf_measure_tables.cpp"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """the program's output, and its lines by kind: {"B": {(sr, N, hann): fields}, "S": {(sr, N): fields}, "C": {(sr, ring): fields}}"""
    text = _build_and_run(tmp_path_factory.mktemp("measure_tables"), "tables")
    out = {"B": {}, "S": {}, "C": {}, "text": text}
    for line in text.splitlines():
        f = line.split()
        key = tuple(int(v) for v in f[1:4 if f[0] == "B" else 3])
        out[f[0]][key] = f[len(key) + 1:]
    assert len(out["B"]) == 8 and len(out["S"]) == 4 and len(out["C"]) == 16
    return out


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=str(what))


def _hann32(n):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / float(n))).astype(np.float32)


@pytest.mark.parametrize("hann", (0, 1), ids=("no_window", "hann"))
@pytest.mark.parametrize("sr,n", BANDS_CASES)
def test_bands_tables(tables, sr, n, hann):
    """edges, covered, ENBW and the A / C weights of every bin against tests/bands_ref.py; and the bins' shares of the bands that
    follow from the library's edges (the overlap the kernel forms from them) against bands_ref.bin_weights"""
    f = tables["B"][(sr, n, hann)]
    m = n // 2
    covered, enbw = int(f[0]), float(f[1])
    edges = np.array(f[2:2 + 32], np.float64)
    weights = np.array(f[2 + 32:], np.float64).reshape(m, 2)
    assert covered == bands_ref.covered(sr, n)
    _close(edges, bands_ref.edges_bins(sr, n), "edges")
    window = _hann32(n) if hann else None
    if hann:
        _close(enbw, bands_ref.enbw(window, n), "enbw")
        assert abs(enbw - 1.5) < 1e-6  # Hann
    else:
        assert enbw == 1.0
    hz = np.arange(m, dtype=np.float64) * float(sr) / float(n)
    _close(weights[:, 0], bands_ref.a_weight(hz), "A weights")
    _close(weights[:, 1], bands_ref.c_weight(hz), "C weights")
    assert weights[0, 0] == 0.0 and weights[0, 1] == 0.0
    k = np.arange(m, dtype=np.float64)
    share = np.maximum(np.minimum(k[None] + 0.5, edges[1:, None]) - np.maximum(k[None] - 0.5, edges[:-1, None]), 0.0)
    want = bands_ref.bin_weights(sr, n)
    # (a share is a difference of bin positions up to m, each within rtol: the bound is absolute, rtol times m)
    np.testing.assert_allclose(share, want, rtol=0, atol=RTOL * float(m))


@pytest.mark.parametrize("sr,n", BANDS_CASES)
def test_stereo_tables(tables, sr, n):
    f = tables["S"][(sr, n)]
    p, log2p, covered = int(f[0]), int(f[1]), int(f[2])
    tab = np.array(f[3:], np.float64)
    assert p == stereo_ref.window_frames(n) and 1 << log2p == p
    assert covered == bands_ref.covered(sr, p)  # (a spectrum of P / 2 bins of a P-point transform)
    assert tab.size == 2 * p + 32
    i = np.arange(p, dtype=np.float64)
    _close(tab[:p], 0.5 - 0.5 * np.cos(2.0 * np.pi * i / float(p)), "window")
    x = 2.0 * np.pi * np.arange(p // 2, dtype=np.float64) / float(p)
    tw = tab[p:2 * p].reshape(p // 2, 2)
    _close(tw[:, 0], np.cos(x), "twiddles re")
    _close(tw[:, 1], -np.sin(x), "twiddles im")
    assert tw[0, 0] == 1.0 and tw[0, 1] == 0.0
    _close(tab[2 * p:], bands_ref.edges_bins(sr, p), "edges")


def _cq_fields(f):
    max_window, end_covered, first_resolved = int(f[0]), int(f[1]), int(f[2])
    sched = np.array(f[3:3 + SCHED_WORDS], np.int64)
    tab = np.array(f[3 + SCHED_WORDS:], np.float64).reshape(end_covered, BIN_DOUBLES)
    return max_window, end_covered, first_resolved, sched, tab


@pytest.mark.parametrize("ring", CQ_RINGS)
@pytest.mark.parametrize("sr", CQ_RATES)
def test_cq_geometry_and_phasors(tables, sr, ring):
    max_window, end_covered, first_resolved, _, tab = _cq_fields(tables["C"][(sr, ring)])
    lmax = cq_ref.max_window(ring)
    L, end, first = cq_ref.geometry(sr, lmax)
    assert (max_window, end_covered, first_resolved) == (lmax, end, first)
    assert np.array_equal(tab[:, 5], L[:end].astype(np.float64))
    assert np.array_equal(tab[:, 4], 4.0 / L[:end].astype(np.float64))
    assert np.all(tab[:, 6:8] == 0.0)
    # the phasors: numpy's cos / sin of the same long double arguments, rounded to float64
    ld = np.longdouble
    two_pi = ld(2) * ld("3.14159265358979323846264338327950288")
    b = np.arange(end).astype(ld)
    wc = -two_pi * ld(440) * np.exp2((b - ld(57)) / ld(12)) / ld(sr)
    wh = two_pi / L[:end].astype(ld)
    for col, w in ((0, wc), (2, wh)):
        _close(tab[:, col], np.cos(ld(64) * w).astype(np.float64), ("step re", col))
        _close(tab[:, col + 1], np.sin(ld(64) * w).astype(np.float64), ("step im", col))
        arg = np.arange(64).astype(ld)[None, :] * w[:, None]
        lanes = tab[:, HEAD:].reshape(end, 64, 4)
        _close(lanes[:, :, col], np.cos(arg).astype(np.float64), ("lanes re", col))
        _close(lanes[:, :, col + 1], np.sin(arg).astype(np.float64), ("lanes im", col))
    assert np.all(tab[:, HEAD] == 1.0) and np.all(tab[:, HEAD + 1] == 0.0)  # n = 0


@pytest.mark.parametrize("ring", CQ_RINGS)
@pytest.mark.parametrize("sr", CQ_RATES)
def test_cq_schedule(tables, sr, ring):
    """what the longest-first rule implies: every covered bin once, each wave's list in non-increasing L_b, and loads -- the sum
    of ceil(L_b / 64) + 8 over a wave's bins -- that differ by no more than the largest single bin's cost (a bin always goes to
    the least loaded wave, so no wave ever leads the least loaded one by more than the bin it took last)"""
    _, end, _, sched, tab = _cq_fields(tables["C"][(sr, ring)])
    L = tab[:, 5].astype(np.int64)
    offsets, order = sched[:WAVES + 1], sched[WAVES + 1:]
    assert offsets[0] == 0 and np.all(np.diff(offsets) >= 0) and offsets[-1] == end
    assert sorted(order[:end].tolist()) == list(range(end)) and np.all(order[end:] == 0)
    cost = (L + 63) // 64 + 8
    loads = []
    for w in range(WAVES):
        bins = order[offsets[w]:offsets[w + 1]]
        assert np.all(np.diff(L[bins]) <= 0), (w, bins)
        loads.append(int(cost[bins].sum()))
    print(f"sr {sr} ring {ring}: {end} bins, loads {min(loads)} .. {max(loads)}, largest bin {int(cost.max())}")
    assert max(loads) - min(loads) <= int(cost.max())


def test_the_program_is_clean_under_the_sanitizers(tables, tmp_path):
    """the same program with -fsanitize=address,undefined, run directly: exit 0 and the same output"""
    text = _build_and_run(tmp_path, "tables_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert text == tables["text"]


NAMES = ["loudness", "peaks", "signal", "pitch", "bands", "stereo", "cq", "scope", "gonio", "sono", "bits", "thd", "delay", "onset", "xfer",
         "impulse", "click", "imd", "tempo", "hum"]
# wf_hip_output (include/wf_hip.h), every number written out: a new output is appended, the others keep theirs
OUTPUT_NUMBERS = {"OUT_DECIBELS": 0, "OUT_BARS": 1, "OUT_PREMIRROR": 2, "OUT_VERTICES": 3, "OUT_VERTEX_COUNTS": 4, "OUT_LAST_SILENT": 5,
                  "OUT_TSMOOTH": 6, "OUT_METER": 7, "OUT_INPUT_RMS": 8, "OUT_WAVEFORM_TS": 9, "OUT_LOUDNESS": 10, "OUT_PEAKS": 11,
                  "OUT_SIGNAL": 12, "OUT_PITCH": 13, "OUT_BANDS": 14, "OUT_STEREO": 15, "OUT_CQ": 16, "OUT_SCOPE": 17, "OUT_GONIO": 18,
                  "OUT_SONO": 19, "OUT_BITS": 20, "OUT_THD": 21, "OUT_DELAY": 22, "OUT_ONSET": 23, "OUT_XFER": 24, "OUT_IMPULSE": 25,
                  "OUT_CLICK": 26, "OUT_IMD": 27, "OUT_TEMPO": 28, "OUT_HUM": 29}


def test_both_batch_classes_share_the_readers():
    """all twenty readers: one function on both batch classes, documented, and the Python table the twin of the one C table, whose
    row i is output OUT_LOUDNESS + i"""
    assert list(binding.MEASURES) == NAMES
    for name in binding.MEASURES:
        reader = getattr(binding.SpectrumBatch, name)
        assert reader is getattr(binding.MultiBatch, name) is getattr(binding._MeasureReaders, name), name
        assert reader.__doc__ and name not in vars(binding.SpectrumBatch) and name not in vars(binding.MultiBatch)
    # the rows of MEASURES in wf_hip_measure.hip, from the source text: {WF_HIP_OUT_X, sizeof(wf_hip_x), per_row, ...}
    text = (CSRC / "wf_hip_measure.hip").read_text()
    internal = (CSRC / "wf_hip_internal.hpp").read_text()
    assert text.count("constexpr Measure ") == 1
    table = text[text.index("constexpr Measure MEASURES["):]
    table = table[:table.index("};")]
    rows = re.findall(r"\{WF_HIP_OUT_(\w+), sizeof\(wf_hip_(\w+)\), (true|false),", table)
    assert len(rows) == len(NAMES) == 20 == table.count("{WF_HIP_OUT_")
    assert [int(n) for n in re.findall(r"N_MEASURES = (\d+)", internal)] == [20]
    for (out, struct, per_row), (name, (what, dtype, py_per_row)) in zip(rows, binding.MEASURES.items()):
        assert out.lower() == struct == name, (out, struct, name)
        assert what == getattr(binding, "OUT_" + out) and dtype is getattr(binding, out + "_DTYPE"), name
        assert py_per_row is (per_row == "true") is (name in ("peaks", "bands")), name
    # every measurement output -- OUT_LOUDNESS up to the last output there is -- once, at its own position
    last = max(v for k, v in vars(binding).items() if k.startswith("OUT_") and isinstance(v, int))
    assert [what for what, _, _ in binding.MEASURES.values()] == list(range(binding.OUT_LOUDNESS, last + 1))
    # the newest row word for word, its kernel header in the unit and in the Makefile
    assert "{WF_HIP_OUT_HUM, sizeof(wf_hip_hum), false, why_no_hum, setup_hum, launch_hum}" in table
    assert '#include "wf_hum.hpp"' in text and "wf_hum.hpp" in (CSRC / "Makefile").read_text()
    # one table on either side: the continuations it once had are gone
    for source in (text, internal, (ROOT / "waveform_amd" / "binding.py").read_text()):
        assert "MEASURES_MORE" not in source and "MEASURES_REST" not in source and "N_MEASURES_ALL" not in source


def test_every_reader_is_pinned_to_its_output_its_dtype_and_its_shape():
    """what each output's own module said of its reader, written out and not read from the C text: the number it reads, the dtype
    by name, one entry per stream but for peaks and bands, and one documented function on both batch classes"""
    assert len(binding.MEASURES) == len(NAMES) == 20
    for name in NAMES:
        number, per_row = OUTPUT_NUMBERS["OUT_" + name.upper()], name in ("peaks", "bands")
        assert binding.MEASURES[name] == (number, getattr(binding, name.upper() + "_DTYPE"), per_row), name
        reader = getattr(binding._MeasureReaders, name)
        assert reader is getattr(binding.SpectrumBatch, name) is getattr(binding.MultiBatch, name) and reader.__doc__, name


def test_the_abi_and_the_output_numbers_are_unchanged():
    """ABI version 13, 75 exported entry points, and every output at its number"""
    assert {k: v for k, v in vars(binding).items() if k.startswith("OUT_") and isinstance(v, int)} == OUTPUT_NUMBERS
    assert [OUTPUT_NUMBERS["OUT_" + name.upper()] for name in NAMES] == list(range(10, 30))
    assert binding.lib().wf_hip_abi_version() == 13
    path = ROOT / "waveform_amd" / "libwaveform_hip.so"
    nm = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line and line.split()[-1].startswith("wf_hip_")}
    assert len(exported) == 75, sorted(exported)  # no new entry point


@pytest.mark.parametrize("name", NAMES)
def test_a_measurement_output_has_no_bytes_without_a_handle(name):
    assert binding.lib().wf_hip_output_bytes(None, OUTPUT_NUMBERS["OUT_" + name.upper()]) == 0
