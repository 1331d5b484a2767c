"""The sonogram's host tables (wf::host::sono_tables, waveform_amd/csrc/wf_measure_tables.cpp) without a device: the library's own
builder, compiled into a program of its own, against numpy; and the same program once more under the address and
undefined-behaviour sanitizers, run directly.

Bounds.  Window and twiddles are built from long double arguments and rounded to float64 once; numpy's long double cos / sin of
the same arguments, rounded the same way, can differ from them by the last bit of the long double result, which moves the float64
only when it sits on a rounding boundary: one float64 ulp (rtol 2.3e-16), and 1e-19 absolute for cos(pi / 2), which is 2.7e-20
in long double and not 0.  The edges are three float64 operations and one exp2 behind 62.5: rtol 1e-15.  Integers are equal."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sono_ref as ref

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "waveform_amd" / "csrc"
RATES = (8000, 44100, 48000, 192000)
RINGS = (2048, 4096, 8192, 16384, 32768, 65536)
P = ref.P

PROGRAM = r"""
#include <cstdio>
#include <initializer_list>
#include "wf_measure_tables.hpp"
using namespace wf::host;
int main() {
  static_assert(WF_HIP_SONO_WINDOW == 1024 && WF_HIP_SONO_HOP == 256 && WF_HIP_SONO_COLUMNS == 64 && WF_HIP_SONO_BANDS == 64);
  for(unsigned sr : {8000u, 44100u, 48000u, 192000u}) for(unsigned ring : {2048u, 4096u, 8192u, 16384u, 32768u, 65536u}) {
    const SonoTables s = sono_tables(sr, ring);
    if(s.tab.size() != 2 * (size_t)WF_HIP_SONO_WINDOW + WF_HIP_SONO_BANDS + 1) return 2;
    std::printf("%u %u %u %u %u", sr, ring, s.columns, s.first_covered, s.end_covered);
    for(double x : s.tab) std::printf(" %.17g", x);
    std::printf("\n");
  }
  for(unsigned ring : {0u, 128u, 1024u, 1280u}) std::printf("small %u %u\n", ring, sono_tables(48000, ring).columns);
  return 0;
}
"""


def _build_and_run(directory, name, extra=()):
    src = directory / "sono_tables_main.cpp"
    src.write_text(PROGRAM)
    exe = directory / name
    subprocess.run(["g++", "-std=c++20", "-O2", *extra, "-I", str(CSRC), "-I", str(ROOT / "include"), str(src),
                    str(CSRC / "wf_measure_tables.cpp"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """the program's output and its lines: {(sr, ring): (columns, first_covered, end_covered, tab)}, {"small": {ring: columns}}"""
    text = _build_and_run(tmp_path_factory.mktemp("sono_tables"), "tables")
    out, small = {}, {}
    for line in text.splitlines():
        f = line.split()
        if f[0] == "small":
            small[int(f[1])] = int(f[2])
        else:
            out[(int(f[0]), int(f[1]))] = (int(f[2]), int(f[3]), int(f[4]), np.array(f[5:], np.float64))
    assert len(out) == len(RATES) * len(RINGS)
    return dict(text=text, rows=out, small=small)


def test_window_and_twiddles(tables):
    ld = np.longdouble
    two_pi = ld(2) * ld("3.14159265358979323846264338327950288")
    i = np.arange(P).astype(ld)
    window = (ld(0.5) - ld(0.5) * np.cos(two_pi * i / ld(P))).astype(np.float64)
    x = two_pi * np.arange(P // 2).astype(ld) / ld(P)
    first = None
    for key, (_, _, _, tab) in tables["rows"].items():
        assert tab.size == 2 * P + 65
        np.testing.assert_allclose(tab[:P], window, rtol=2.3e-16, atol=1e-19, err_msg=str(key))
        tw = tab[P:2 * P].reshape(P // 2, 2)
        np.testing.assert_allclose(tw[:, 0], np.cos(x).astype(np.float64), rtol=2.3e-16, atol=1e-19, err_msg=str(key))
        np.testing.assert_allclose(tw[:, 1], (-np.sin(x)).astype(np.float64), rtol=2.3e-16, atol=1e-19, err_msg=str(key))
        assert tw[0, 0] == 1.0 and tw[0, 1] == 0.0 and tab[0] == 0.0 and tab[P // 2] == 1.0
        first = tab if first is None else first
        assert np.array_equal(tab[:2 * P], first[:2 * P])  # neither depends on the rate or the ring
    # what the restatement windows with, from float64 arguments: 2 pi i / P rounded to float64 is off by up to 6.3 * 1.1e-16, the
    # window's slope is at most 0.5, and its own rounding adds 1.1e-16: below 5e-16
    np.testing.assert_allclose(first[:P], ref.hann(), rtol=0, atol=5e-16)


@pytest.mark.parametrize("sr", RATES)
def test_edges_and_covered(tables, sr):
    want = {8000: (0, 47), 44100: (0, 64), 48000: (0, 64), 192000: (5, 64)}[sr]
    for ring in RINGS:
        _, first, end, tab = tables["rows"][(sr, ring)]
        np.testing.assert_allclose(tab[2 * P:], ref.edges_bins(sr), rtol=1e-15, atol=0)
        assert (first, end) == want == ref.covered(sr)
    e = tables["rows"][(sr, 8192)][3][2 * P:]
    assert np.all(np.diff(e) > 0) and abs(e[0] - 62.5 * P / sr) < 1e-12 and abs(e[64] - 16000.0 * P / sr) < 1e-9
    # a covered pair that sat on its threshold would depend on the last bit of an edge: none is near
    assert np.min(np.abs(e - 0.5)) > 1e-3 and np.min(np.abs(e - (P / 2 - 0.5))) > 1e-3


def test_columns_of_the_rings(tables):
    for sr in RATES:
        got = [tables["rows"][(sr, ring)][0] for ring in RINGS]
        assert got == [4, 12, 28, 60, 64, 64] == [ref.columns(r) for r in RINGS]
    assert tables["small"] == {0: 0, 128: 0, 1024: 0, 1280: 1}  # (refused by the library below 2048: no underflow all the same)
    for ring in RINGS:  # the oldest column read is still in the ring
        assert (ref.columns(ring) - 1) * ref.H + P + ref.H - 1 < ring


def test_the_program_is_clean_under_the_sanitizers(tables, tmp_path):
    """the same program with -fsanitize=address,undefined, run directly: exit 0 and the same output"""
    text = _build_and_run(tmp_path, "tables_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert text == tables["text"]
