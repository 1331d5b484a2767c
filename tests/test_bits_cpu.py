"""Bit meter (WF_HIP_OUT_BITS) without a device: the structured dtype against the C layout, the appended output number, the
properties the definition promises of its numpy restatement (tests/bits_ref.py), the conditions of the signals the device test
pushes, and a gfx950 compile of the read kernels with no scratch, no spills and no static LDS."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from waveform_amd import binding
import bits_ref as ref
from kernel_usage import kernel_usage

ROOT = Path(__file__).resolve().parents[1]


def test_bits_dtype_matches_the_c_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wf_hip.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %d %d %d", sizeof(wf_hip_bits), sizeof(wf_hip_bits_channel), (int)WF_HIP_OUT_BITS, (int)WF_HIP_OUT_SONO,\n'
                   "         (int)WF_HIP_BITS_MAX_WINDOW);\n"
                   + "".join(f'  printf(" %zu", offsetof(wf_hip_bits_channel, {n}));\n' for n in ref.CHANNEL_FIELDS)
                   + "".join(f'  printf(" %zu", offsetof(wf_hip_bits, {n}));\n' for n in ref.FIELDS) +
                   '  printf(" %zu %d", offsetof(wf_hip_bits, ch[1]), (int)WF_HIP_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    dt, ch = binding.BITS_DTYPE, binding.BITS_CHANNEL_DTYPE
    assert got == [dt.itemsize, ch.itemsize, binding.OUT_BITS, binding.OUT_SONO, binding.BITS_MAX_WINDOW] \
        + [ch.fields[n][1] for n in ref.CHANNEL_FIELDS] + [dt.fields[n][1] for n in ref.FIELDS] + [ch.itemsize, 13]
    assert dt.itemsize == 1360 and ch.itemsize == 672 and dt.itemsize % 16 == 0
    assert dt == ref.BITS_DTYPE and dt.names == ref.FIELDS and ch == ref.BITS_CHANNEL_DTYPE and ch.names == ref.CHANNEL_FIELDS
    assert [ch.fields[n][1] for n in ref.CHANNEL_FIELDS] == [0, 512, 576, 640, 644, 648, 652, 656, 660, 664, 668]
    assert [dt.fields[n][1] for n in ref.FIELDS] == [0, 1344, 1348]
    assert ch.fields["hist"][0].shape == (256,) and ch.fields["hist"][0].base == np.uint16 and ch.fields["max_run_value"][0] == np.float32
    assert ref.MAX_WINDOW == binding.BITS_MAX_WINDOW == 8192


def _one(kind, p, seed=1):
    return ref.bits_channel(ref.signal(kind, np.random.default_rng(seed), p))


@pytest.mark.parametrize("p", (128, 2000, 8192))
def test_the_word_lengths(p):
    for kind, wl in (("s16", 16), ("u8", 8), ("s24", 24)):
        s = _one(kind, p)
        assert s["word_length"] == wl and s["fine"] == 0 and s["over"] == 0, kind
        assert not s["ones"][:32 - wl].any() and s["ones"][32 - wl] > 0, kind  # nothing below the grid's last bit
    s = _one("float", p)
    assert s["word_length"] == 32 and s["fine"] > 0 and s["over"] == 0
    s = _one("stuck", p)
    assert s["word_length"] == 16 and s["ones"][16] == p and 0 < s["ones"][17] < p  # the stuck bit reads P


@pytest.mark.parametrize("p", (1024, 2000, 8192))
def test_the_clipped_sine(p):
    s = _one("clipped", p)
    assert s["over"] > 0 and s["max_run"] >= 30 and s["max_run_value"] == np.float32(1.0)
    assert s["hist"][255] == s["over"]      # +1.0 is over and lands in the last bin; nothing else is there
    assert s["hist"][0] > 0 and s["magnitude_bits"] == 31  # -1.0 fits: v = -2^31, bin 0
    assert s["repeats"] >= s["over"] - (p // 200 + 1)


@pytest.mark.parametrize("p", (1, 64, 2000, 8192))
def test_silence(p):
    s = _one("silence", p)
    assert s["word_length"] == 0 and s["magnitude_bits"] == 0 and s["max_run"] == p and s["repeats"] == p - 1
    assert s["hist"][128] == s["mag"][0] == p and s["max_run_start"] == 0 and s["max_run_value"] == 0 and not s["ones"].any()
    assert s["over"] == 0 and s["fine"] == 0


@pytest.mark.parametrize("p", (128, 2000, 8192))
def test_the_invariants_hold_on_every_kind(p):
    for kind in ref.KINDS:
        x = ref.signal(kind, np.random.default_rng(p), p + 7, p)
        s = ref.bits_one(x[None], p)
        c = s["ch"][0]
        v = ref.code(x[-p:])[0]
        assert s["window"] == p and not s["reserved"].any() and not s["ch"][1].tobytes().strip(b"\0"), kind
        assert int(c["hist"].astype(np.int64).sum()) == int(c["mag"].astype(np.int64).sum()) == p, kind
        assert c["ones"][31] == np.count_nonzero(v < 0), kind
        assert 1 <= c["max_run"] <= p and c["max_run_start"] + c["max_run"] <= p and c["repeats"] <= p - 1, kind
        assert c["magnitude_bits"] <= 31 and c["word_length"] <= 32 and c["over"] + c["fine"] <= p, kind
    assert ref.window_frames(16384) == 8192 and ref.bits_one(np.zeros((2, 9000), np.float32), 16384)["window"] == 8192


def test_the_exotic_values():
    f = np.float32
    below_one = np.nextafter(f(1), f(0))
    tiny = np.float32(1e-45)  # the smallest denormal
    rows = [  # x, v, over, fine, hist bin, m
        (f(0.0), 0, False, False, 128, 0),
        (f(-0.0), 0, False, False, 128, 0),
        (tiny, 0, False, True, 128, 0),
        (-tiny, -1, False, True, 127, 0),
        (f(1e-39), 0, False, True, 128, 0),            # a denormal
        (f(2.0 ** -31), 1, False, False, 128, 1),
        (f(-2.0 ** -31), -1, False, False, 127, 0),
        (f(2.0 ** -32), 0, False, True, 128, 0),
        (f(-2.0 ** -32), -1, False, True, 127, 0),
        (f(-1.0), -2 ** 31, False, False, 0, 31),
        (f(1.0), 2 ** 31 - 1, True, False, 255, 31),
        (below_one, 2 ** 31 - 128, False, False, 255, 31),
        (f(np.inf), 2 ** 31 - 1, True, False, 255, 31),
        (f(-np.inf), -2 ** 31, True, False, 0, 31),
        (f(-1.5), -2 ** 31, True, False, 0, 31),
        (f(0.5), 2 ** 30, False, False, 192, 31),
        (f(-0.5), -2 ** 30, False, False, 64, 30),
        (f(2.0 ** -9) + f(2.0 ** -32), 2 ** 22, False, True, 128, 23),
    ]
    x = np.array([r[0] for r in rows], np.float32)
    assert x[2] > 0 and x[2].view(np.uint32) == 1
    v, over, fine = ref.code(x)
    assert v.tolist() == [r[1] for r in rows]
    assert over.tolist() == [r[2] for r in rows] and fine.tolist() == [r[3] for r in rows]
    assert ((v >> 24) + 128).tolist() == [r[4] for r in rows]
    assert ref.significant_bits(v).tolist() == [r[5] for r in rows]
    s = ref.bits_channel(x)
    assert s["over"] == 4 and s["fine"] == 6 and s["word_length"] == 32 and s["magnitude_bits"] == 31
    z = np.zeros(64, np.float32)
    z[1::2] = -0.0  # +0 and -0 differ as patterns: no repeats, though every code is 0
    s = ref.bits_channel(z)
    assert s["repeats"] == 0 and s["max_run"] == 1 and s["word_length"] == 0 and s["hist"][128] == 64


def test_the_first_of_equal_runs_wins():
    x = ref.signal("two_runs", np.random.default_rng(3), 1024)
    s = ref.bits_channel(x)
    assert s["max_run"] == ref.RUN and s["max_run_start"] == 1024 // 3 and s["max_run_value"] == np.float32(0.125)
    assert np.all(x[2 * 1024 // 3:2 * 1024 // 3 + ref.RUN] == np.float32(-0.375))  # the second one is as long
    x[2 * 1024 // 3 + ref.RUN] = -0.375  # one frame longer: now it wins
    s = ref.bits_channel(x)
    assert s["max_run"] == ref.RUN + 1 and s["max_run_start"] == 2 * 1024 // 3 and s["max_run_value"] == np.float32(-0.375)
    s = ref.bits_channel(ref.signal("float", np.random.default_rng(4), 512))  # no two frames equal: the first frame
    assert s["max_run"] == 1 and s["max_run_start"] == 0 and s["repeats"] == 0


def test_runs_at_the_ends_of_the_window():
    first = ref.bits_one(ref.signal("run_first", np.random.default_rng(5), 2011, 2000)[None], 2000)["ch"][0]
    assert first["max_run"] == ref.RUN and first["max_run_start"] == 0 and first["max_run_value"] == np.float32(0.0625)
    assert first["repeats"] == ref.RUN - 1  # the five equal frames in front of the window do not count
    last = ref.bits_one(ref.signal("run_last", np.random.default_rng(5), 2011, 2000)[None], 2000)["ch"][0]
    assert last["max_run"] == ref.RUN and last["max_run_start"] == 2000 - ref.RUN and last["max_run_value"] == np.float32(-0.5)
    whole = _one("constant", 8192)
    assert whole["max_run"] == 8192 and whole["max_run_start"] == 0 and whole["repeats"] == 8191 and whole["word_length"] == 5


def test_only_the_newest_frames_count():
    x = np.stack([ref.signal("float", np.random.default_rng(6), 2011), ref.signal("s16", np.random.default_rng(7), 2011)])
    older = x.copy()
    older[:, :11] = 7.0
    assert ref.bits(x[None], 2000).tobytes() == ref.bits(older[None], 2000).tobytes() == ref.bits(x[None, :, 11:], 2000).tobytes()
    assert ref.bits(x[None], 2000)["ch"]["over"].sum() == 0


def test_mismatches_compares_every_field():
    rng = np.random.default_rng(8)
    x = np.stack([np.stack([ref.signal(a, rng, 1024), ref.signal(b, rng, 1024)]) for a, b in (("float", "s16"), ("gap", "clipped"))])
    want = ref.bits(x, 1024)
    assert ref.mismatches(want, x, 1024) == [] and ref.mismatches(want, x) == []
    for name in ref.CHANNEL_FIELDS:
        got = want.copy()
        f = got["ch"][name]
        if name in ("hist", "ones", "mag"):
            f[1, 1, 7] += 1
        elif f.dtype == np.float32:
            f[1, 1] = np.nextafter(f[1, 1], np.float32(2))
        else:
            f[1, 1] += 1
        assert [m[0] for m in ref.mismatches(got, x, 1024)] == ["ch." + name]
    for name in ("window", "reserved"):
        got = want.copy()
        got[name][1] += 1
        assert {m[0] for m in ref.mismatches(got, x, 1024)} == {name}
    got = want.copy()
    got["ch"]["max_run_value"][0, 0] = -got["ch"]["max_run_value"][0, 0] if got["ch"]["max_run_value"][0, 0] else np.float32(-0.0)
    assert [m[0] for m in ref.mismatches(got, x, 1024)] == ["ch.max_run_value"]  # by its bits
    assert ref.mismatches(want[:1], x, 1024)[0][0] == "shape"


def test_the_gpu_cases_are_no_trivial_entries():
    """the conditions of tests/test_gpu_bits.py's comparison, on its own seeds and shapes: every kind is pushed, every noise stream
    occupies at least 100 bins of its histogram, every run kind has the run it was built for, and the window the device reads
    wraps the ring and ends at an odd position"""
    seen = set()
    for case in ref.GPU_CASES:
        fft, sr, kw, w, kinds = case
        if kw.get("meter"):
            assert w == int(sr * (kw["meter_ms"] / 1000.0)) & -16 == 2208 and w % 64 != 0
        else:
            assert w == fft
        p = ref.window_frames(w)
        x = ref.case_audio(case)
        assert x.shape == (3, 2, ref.ring_frames(w) + p // 2 + 3) and x.shape[-1] % 4 != 0 and len(set(kinds)) == 3
        assert (x.shape[-1] - p) % ref.ring_frames(w) + p > ref.ring_frames(w)  # the window wraps the ring
        s = ref.bits(x, w)
        for pair, r in zip(ref.case_kinds(case), s):
            assert r["window"] == p
            for k, c in zip(pair, r["ch"]):
                bins = int(np.count_nonzero(c["hist"]))
                print(f"{ref.case_id(case)} {k}: P {p}, word length {int(c['word_length'])}, magnitude bits {int(c['magnitude_bits'])}, over "
                      f"{int(c['over'])}, fine {int(c['fine'])}, repeats {int(c['repeats'])}, longest run {int(c['max_run'])} at "
                      f"{int(c['max_run_start'])} of {float(c['max_run_value'])}, bins {bins}")
                assert int(c["hist"].astype(np.int64).sum()) == int(c["mag"].astype(np.int64).sum()) == p
                if k in ref.NOISE_KINDS:
                    assert bins >= 100, (case, k)
                run = min(ref.RUN, p // 8)
                if k == "constant":
                    assert (c["max_run"], c["max_run_start"]) == (p, 0) and c["max_run_value"] == np.float32(0.3125)
                elif k == "silence":
                    assert (c["max_run"], c["max_run_start"], c["word_length"]) == (p, 0, 0)
                elif k == "gap":
                    g = min(ref.GAP, p // 2)
                    assert c["max_run"] == g and c["max_run_value"] == 0
                    if p >= 512:  # across a multiple of 256: a step of the workgroup
                        assert g == 300 and c["max_run_start"] < 256 < c["max_run_start"] + g
                elif k == "two_runs":
                    assert (c["max_run"], c["max_run_start"]) == (run, p // 3) and c["max_run_value"] == np.float32(0.125)
                    assert c["repeats"] >= 2 * (run - 1)
                elif k == "run_first":
                    assert (c["max_run"], c["max_run_start"]) == (run, 0) and c["max_run_value"] == np.float32(0.0625)
                elif k == "run_last":
                    assert (c["max_run"], c["max_run_start"]) == (run, p - run) and c["max_run_value"] == np.float32(-0.5)
                elif k == "clipped":
                    assert c["over"] > 0 and c["max_run"] >= 30 and abs(c["max_run_value"]) == 1
                elif k == "stuck":
                    assert c["word_length"] == 16 and c["ones"][16] == p
                elif k in ("s16", "u8", "s24"):
                    assert c["word_length"] == {"s16": 16, "u8": 8, "s24": 24}[k] and c["fine"] == 0
                elif k == "float":
                    assert c["word_length"] == 32 and c["fine"] > 0
            seen |= set(pair)
    assert seen == set(ref.KINDS)
    assert {k for case in ref.GPU_CASES for k in case[4]} == set(ref.KINDS)  # every kind is some stream's channel 0 as well
    assert [ref.case_id(c) for c in ref.GPU_CASES] == ["w128", "w1024", "w2000", "w4096", "w16384", "w2208_meter"]
    assert not any(k in ref.NOISE_KINDS for k in sum(map(list, ref.case_kinds(ref.GPU_CASES[0])), []))  # 128 frames cannot fill 100 bins


def test_bits_kernels_have_no_scratch():
    res = kernel_usage("wf_hip_measure", "bits_read_kernel")
    assert len(res) == 2, res  # one and two captured channels
    for name, r in res.items():
        assert r.get("ScratchSize [bytes/lane]") == 0 and r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
        assert r.get("LDS Size [bytes/block]") == 0, (name, r)  # the staged windows and the entry's image behind them are dynamic
        assert r.get("Occupancy [waves/SIMD]") >= 4, (name, r)
