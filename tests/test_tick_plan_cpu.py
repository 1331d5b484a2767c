"""The decisions of wf_hip_create that need no device (waveform_amd/csrc/wf_tick_plan.cpp) without one: the library's own
planner, compiled into a program of its own, over every legal fft size (the 4089 multiples of 16 from 128 to 65536) in three
channel layouts, against the records the GPU sweeps left under profiles/ -- which kernel family every size takes, the rows /
row length / container / radices of the sizes above 16384, the fixed-plan ids of the plugin's automatic sizes -- and the lane
counts the GPU tests assert; the same program once more under the address and undefined-behaviour sanitizers."""
import json
import re
import subprocess
from collections import Counter
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "waveform_amd" / "csrc"
PROFILES = ROOT / "profiles"

LAYOUTS = ("one", "stereo", "monomix")  # one captured channel; a stereo pair; mono mixdown of two
# wf::Family in the words of the sweeps' `path` (tests/sizes_large_sweep.py)
PATH = {"POW2": "fused tick kernel", "ZERO_PADDED": "fused tick kernel", "MIXED_RADIX": "fused tick kernel: mixed radix",
        "FIXED_PLAN": "fused tick kernel: mixed radix", "BLUESTEIN": "fused tick kernel: Bluestein", "WHOLE_65536": "one kernel",
        "MR_TWO_ROWS": "mixed radix: two rows in one kernel", "MR_ROWS": "mixed-radix rows", "BLUESTEIN_ROWS": "Bluestein rows in LDS"}
# the plugin's automatic sizes -> spectrum_tick_kernel's PLAN: the row of the table of fixed plans whose product is n / 2
FIXED_IDS = {800: 1, 960: 2, 720: 3, 880: 4, 1600: 5, 1920: 6, 2000: 7, 1760: 8}

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "wf_tick_plan.hpp"
#include "wf_geometry.hpp"
#include "wf_host_tables.hpp"
static const char *name(wf::Family f) {
  switch(f) {
  case wf::Family::POW2: return "POW2"; case wf::Family::ZERO_PADDED: return "ZERO_PADDED"; case wf::Family::MIXED_RADIX: return "MIXED_RADIX";
  case wf::Family::FIXED_PLAN: return "FIXED_PLAN"; case wf::Family::BLUESTEIN: return "BLUESTEIN"; case wf::Family::WHOLE_65536: return "WHOLE_65536";
  case wf::Family::MR_TWO_ROWS: return "MR_TWO_ROWS"; case wf::Family::MR_ROWS: return "MR_ROWS"; case wf::Family::BLUESTEIN_ROWS: return "BLUESTEIN_ROWS";
  default: return "NONE";
  }
}
static wf_config config(unsigned n, int layout) {
  wf_config c;
  std::memset(&c, 0, sizeof(c));
  c.fft_size = n;
  c.capture_channels = layout == 0 ? 1 : 2;
  c.stereo = layout == 1;
  return c;
}
// dynamic LDS of the power-of-two tick kernel (wf_kernels.hpp: tick_lds_bytes) and its threads, SPW spectra per workgroup
template<class G> static void workgroup(int spw, unsigned *lds, unsigned *threads) {
  *lds = (unsigned)(spw * G::LDS_CF * 8 + G::R2 * G::R3 * 8 + 2 * spw * (G::T / 64) * 4 + 16);
  *threads = (unsigned)(G::T * spw);
}
int main() {
  const wf::PlanOverrides ov;
  for(unsigned n = 128; n <= 65536; n += 16)
    for(int layout = 0; layout < 3; ++layout) {
      const wf::TransformPlan t = wf::plan_transform(config(n, layout), ov);
      std::printf("T %u %d %s %u %d %u %u %u %u %d %d %d %d %d %d %d %d %d %a\n", n, layout, name(t.family), t.geom_n, (int)t.blu, t.big_l, t.big_rows,
                  t.br_l, t.br_rs, t.passes, t.radix[0], t.radix[1], t.radix[2], t.radix[3], (int)t.mr_small, t.plan_id, (int)t.want_split,
                  (int)t.split_mono, (double)t.in_scale);
    }
  // the lanes: (fft size, stereo streams, bars) of the shapes bench.py names and of the GPU tests' lane assertions, 256 compute units
  const unsigned shapes[][3] = {{4096, 4096, 0}, {16384, 1024, 26}, {4096, 8192, 26}, {2048, 256, 0}, {4096, 8192, 0}, {4096, 16384, 0}, {65536, 256, 0},
                                {800, 8192, 0}, {65536, 264, 0}, {32768, 520, 0}, {32768, 256, 0}, {4096, 64, 0}, {65536, 24, 0}, {32768, 24, 0}};
  for(auto &s : shapes) {
    const wf::TransformPlan t = wf::plan_transform(config(s[0], 1), ov);
    unsigned lds = 0, threads = 0; // (the transforms beyond a CU's LDS leave both 0)
    if(s[0] == 4096) workgroup<wf::G4096>(2, &lds, &threads);
    if(s[0] == 2048) workgroup<wf::G2048>(2, &lds, &threads);
    if(s[0] == 16384) workgroup<wf::G16384>(1, &lds, &threads);
    if(s[0] == 32768) workgroup<wf::G32768>(1, &lds, &threads);
    if(s[0] == 800) { // 400 complex points in the 2048-sample container, fixed plan, no display: wf_tick_geom.hip, setup_launch_blu
      workgroup<wf::G2048>(2, &lds, &threads);
      const int half = (int)wf::mr_exchange_half(400), s3 = half / 4 + 4;
      int cf = (int)wf::mr_exchange_cf(400, (unsigned)wf::G2048::LDS_CF);
      if(half > 4 * s3 ? cf > half : cf > 4 * s3) cf = half > 4 * s3 ? half : 4 * s3;
      lds -= 2u * (unsigned)(wf::G2048::LDS_CF - cf) * 8u;
    }
    std::printf("L %u %u %u %d\n", s[0], s[1], s[2], wf::plan_lanes(t, s[1], 2, s[2], lds, threads, 256, ov));
  }
  return 0;
}
"""


def _build_and_run(directory, name, extra=()):
    src = directory / "plan_main.cpp"
    src.write_text(PROGRAM)
    exe = directory / name
    subprocess.run(["g++", "-std=c++20", "-O2", *extra, "-I", str(CSRC), "-I", str(ROOT / "include"), str(src), str(CSRC / "wf_tick_plan.cpp"),
                    str(CSRC / "wf_host_tables.cpp"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """the program's output: {"text", "T": {(n, layout): fields}, "L": {(n, streams, bars): lanes}}"""
    text = _build_and_run(tmp_path_factory.mktemp("tick_plan"), "plan")
    out = {"text": text, "T": {}, "L": {}}
    keys = ("family", "geom_n", "blu", "big_l", "big_rows", "br_l", "br_rs", "passes", "r0", "r1", "r2", "r3", "mr_small", "plan_id", "want_split",
            "split_mono", "in_scale")
    for line in text.splitlines():
        f = line.split()
        if f[0] == "T":
            rec = dict(zip(keys, f[3:]))
            rec = {k: (v if k == "family" else float.fromhex(v) if k == "in_scale" else int(v)) for k, v in rec.items()}
            rec["radices"] = [rec[f"r{i}"] for i in range(rec["passes"])]
            out["T"][(int(f[1]), LAYOUTS[int(f[2])])] = rec
        else:
            out["L"][(int(f[1]), int(f[2]), int(f[3]))] = int(f[4])
    return out


def test_every_legal_size_gets_one_family(plans):
    """none is refused (NONE is what the library has no kernel for), the layout does not change the family, every size above 16384
    -- but 32768, the last power of two inside a CU's LDS -- takes the one kernel of 65536 or rows of one kind or the other (what
    retiring the chain through device memory rests on), and the counts per family are those of the GPU sweep over all 4089 sizes"""
    sizes = range(128, 65536 + 1, 16)
    assert len(plans["T"]) == 3 * len(sizes) == 3 * 4089
    for n in sizes:
        fams = {plans["T"][(n, lay)]["family"] for lay in LAYOUTS}
        assert len(fams) == 1 and fams <= set(PATH), (n, fams)
        if n > 16384:
            assert fams <= ({"POW2"} if n == 32768 else {"WHOLE_65536", "MR_TWO_ROWS", "MR_ROWS", "BLUESTEIN_ROWS"}), (n, fams)
    got = Counter("ok: " + PATH[plans["T"][(n, "stereo")]["family"]] for n in sizes)
    want = json.loads((PROFILES / "r06z_sizes_all_parity.json").read_text())["by_path"]
    assert dict(got) == want
    assert sorted(want.values()) == sorted([9, 385, 624, 148, 275, 2647, 1])


def test_families_up_to_16384_match_the_gpu_sweep(plans):
    recs = [json.loads(line) for line in (PROFILES / "r06t_sizes_upto16384_parity.jsonl").read_text().splitlines()]
    assert len(recs) == 1017
    for r in recs:
        assert PATH[plans["T"][(r["fft_size"], "stereo")]["family"]] == r["path"], r


def test_large_sizes_match_the_recorded_kernels(plans):
    """rows, row length, container and radices of the slider's 768 positions above 16384, from the kernel names the GPU sweep recorded"""
    recs = [json.loads(line) for line in (PROFILES / "r05_sizes_large.jsonl").read_text().splitlines()]
    assert len(recs) == 768
    for r in recs:
        n, k = r["fft_size"], r["kernel"]
        t = plans["T"][(n, "stereo")]
        if m := re.search(r"(\d+) rows of (\d+) complex points by Bluestein over (\d+) points inside LDS", k):
            assert t["family"] == "BLUESTEIN_ROWS" and (t["big_rows"], n // 2 // t["big_rows"], t["br_l"]) == tuple(map(int, m.groups())), (r, t)
            assert t["br_rs"] == (n // 2 // t["big_rows"] + 1) // 2 * 2 and t["big_l"] == n // 2 and not t["blu"]
        elif m := re.search(r"big_mr_whole_kernel<N=\d+: both of its (\d+) rows of (\d+) complex points as mixed radix ([\dx]+) ", k):
            assert t["family"] == "MR_TWO_ROWS" and (t["big_rows"], n // 2 // t["big_rows"]) == (int(m[1]), int(m[2])) == (2, n // 4), (r, t)
            assert t["radices"] == list(map(int, m[3].split("x"))), (r, t)
        elif m := re.search(r"big_mr_rows_kernel \+ big_epilogue_kernel<N=\d+: (\d+) rows of (\d+) complex points as mixed radix ([\dx]+),", k):
            assert t["family"] == "MR_ROWS" and (t["big_rows"], n // 2 // t["big_rows"]) == (int(m[1]), int(m[2])), (r, t)
            assert t["radices"] == list(map(int, m[3].split("x"))), (r, t)
        elif "big_whole_kernel" in k:
            assert n == 65536 and t["family"] == "WHOLE_65536" and (t["big_l"], t["big_rows"], t["geom_n"]) == (32768, 2, 32768), (r, t)
        else:
            assert n == 32768 and "spectrum_tick_kernel<N=32768" in k and ",split>" in k, r
            assert t["family"] == "POW2" and t["geom_n"] == 32768 and t["want_split"] and t["big_l"] == 0, (r, t)
        if n != 32768:
            assert t["want_split"] and t["geom_n"] == 32768, (r, t)  # the epilogue couples the channels through the rotating verdict words


def test_automatic_sizes_get_their_fixed_plans(plans):
    """the sizes the plugin picks by itself (48 kHz and 44.1 kHz at the usual frame rates): plans 1-4 of the 2048-sample container,
    5-8 of the 4096-sample one, in the order of wf_tick_plan.cpp's table"""
    fixed = [(5, 10, 8), (5, 12, 8), (10, 6, 6), (11, 5, 8), (10, 8, 10), (10, 8, 12), (10, 10, 10), (10, 8, 11)]
    for n in (720, 800, 880, 960, 1600, 1760, 1920, 2000):
        for lay in LAYOUTS:
            t = plans["T"][(n, lay)]
            assert t["family"] == "FIXED_PLAN" and t["mr_small"] and 1 <= t["plan_id"] <= 8, (n, t)
            assert tuple(t["radices"]) == fixed[t["plan_id"] - 1] and t["geom_n"] == (2048 if n < 1024 else 4096), (n, t)
            a, b, c = fixed[FIXED_IDS[n] - 1]
            assert a * b * c == n // 2 and t["plan_id"] == FIXED_IDS[n], (n, t)
    others = [n for n in range(128, 16384 + 1, 16) if plans["T"][(n, "stereo")]["family"] == "FIXED_PLAN" and n not in FIXED_IDS]
    assert not others, others


def test_split_and_scale(plans):
    """which layouts run split, and the power of two the window tables carry"""
    for n in range(128, 65536 + 1, 16):
        one, st, mm = (plans["T"][(n, lay)] for lay in LAYOUTS)
        big = st["big_l"] != 0
        assert st["want_split"] == (st["geom_n"] >= 8192) and not st["split_mono"]
        assert one["want_split"] == big and not one["split_mono"]
        assert mm["split_mono"] == (mm["geom_n"] >= 32768) and mm["want_split"] == (mm["split_mono"] or big)
        lg = (n - 1).bit_length()
        assert st["in_scale"] == 2.0 ** min(40, 52 - lg)  # (no legal size runs Bluestein through device memory: 2^24 there)


def test_lanes(plans):
    """what the GPU tests assert (test_gpu_fullsize.py, test_gpu_prologue_args.py), on 256 compute units"""
    lanes = plans["L"]
    assert lanes[(4096, 4096, 0)] == 3    # the headline batch
    assert lanes[(65536, 264, 0)] == 2
    assert lanes[(32768, 520, 0)] == 3
    assert lanes[(32768, 256, 0)] == 3
    assert lanes[(4096, 64, 0)] == 1      # a 64-stream handle
    assert lanes[(65536, 24, 0)] == 1 and lanes[(32768, 24, 0)] == 1
    assert all(1 <= v <= 4 for v in lanes.values()), lanes


def test_same_output_under_the_sanitizers(plans, tmp_path):
    text = _build_and_run(tmp_path, "plan_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    assert text == plans["text"]
