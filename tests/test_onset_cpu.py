"""Onset detector (WF_HIP_OUT_ONSET) without a device: the structured dtype against the C layout, the appended output number, the
columns and the decided range per ring, the properties the definition promises of its float64 restatement (tests/onset_ref.py) on
committed seeds, the picking rule on hand-made curves, the conditions of the device comparison on its own seeds and shapes --
above all that no decision lies within four float32 ulps of flipping --, and a gfx950 compile of the read kernels with no scratch,
no spills and no static LDS."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from waveform_amd import binding
import onset_ref as ref
from kernel_usage import kernel_usage

ROOT = Path(__file__).resolve().parents[1]
P, H = ref.P, ref.H
SR = ref.SR


def test_onset_dtype_matches_the_c_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wf_hip.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %d %d %d %d %d %d", sizeof(wf_hip_onset), (int)WF_HIP_OUT_ONSET, (int)WF_HIP_OUT_DELAY, (int)WF_HIP_ONSET_WINDOW,\n'
                   "         (int)WF_HIP_ONSET_HOP, (int)WF_HIP_ONSET_COLUMNS, (int)WF_HIP_ONSET_BANDS);\n"
                   + "".join(f'  printf(" %zu", offsetof(wf_hip_onset, {n}));\n' for n in ref.FIELDS) +
                   '  printf(" %d", (int)WF_HIP_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    dt = binding.ONSET_DTYPE
    assert got == [dt.itemsize, binding.OUT_ONSET, binding.OUT_DELAY, binding.ONSET_WINDOW, binding.ONSET_HOP, binding.ONSET_COLUMNS,
                   binding.ONSET_BANDS] + [dt.fields[n][1] for n in ref.FIELDS] + [13]
    assert got[:3] == [2240, 23, 22]
    assert dt.itemsize == 2240 and dt.itemsize % 16 == 0 and dt == ref.ONSET_DTYPE and dt.names == ref.FIELDS
    assert [dt.fields[n][1] for n in dt.names] == [0, 512, 2048, 2176, 2180, 2184, 2188, 2192, 2196, 2200, 2204, 2208, 2212, 2216]
    assert dt.fields["strength"][0].shape == (128,) and dt.fields["group"][0].shape == (3, 128) and dt.fields["flags"][0].base == np.uint8
    assert dt.fields["last_strength"][0] == np.float32 and dt.fields["reserved"][0].shape == (6,)
    assert (ref.WINDOW, ref.HOP, ref.COLUMNS, ref.BANDS) == (binding.ONSET_WINDOW, binding.ONSET_HOP, binding.ONSET_COLUMNS, binding.ONSET_BANDS) \
        == (1024, 256, 128, 64)
    assert (binding.ONSET_FLAG_TOTAL, binding.ONSET_FLAG_LOW, binding.ONSET_FLAG_MID, binding.ONSET_FLAG_HIGH, binding.ONSET_FLAG_DECIDED) \
        == (ref.F_TOTAL, ref.F_LOW, ref.F_MID, ref.F_HIGH, ref.F_DECIDED) == (1, 2, 4, 8, 128)
    assert binding.ONSET_NONE == ref.NONE == 0xFFFFFFFF
    # the groups' edges: 62.5 Hz, 250 Hz, 2 kHz, 16 kHz
    e = binding.SONO_EDGES_HZ
    assert [float(round(e[i], 6)) for i in (0, 16, 40, 64)] == [62.5, 250.0, 2000.0, 16000.0] and ref.GROUPS == ((0, 16), (16, 40), (40, 64))


def test_columns_and_the_decided_range_per_ring():
    assert [ref.columns(r) for r in (8192, 16384, 32768, 65536, 131072, 1 << 20)] == [27, 59, 123, 128, 128, 128]
    assert [ref.spectral(r) for r in (8192, 65536)] == [28, 129]
    assert [ref.decided(ref.columns(r)) for r in (8192, 16384, 32768, 65536)] == [(3, 11), (3, 43), (3, 107), (3, 112)]
    assert ref.decided(19) == (3, 0) and ref.decided(20) == (3, 4)  # fewer than 20 columns: none is decided
    assert ref.columns(4096) == 11 and ref.decided(11)[1] == 0       # which is why rings under 8192 frames are refused
    for ring in (8192, 65536):
        ts = ref.spectral(ring)
        assert ts * H + P <= ring  # the oldest spectral column is in the ring wherever in a hop the counter stands
    # the smallest ring: ages 3 .. 10 are decided, 2048 frames: a reader every 2000 frames (24 Hz at 48 kHz) sees every column decided
    assert (11 - 3) * H == 2048 >= SR // 24
    e = ref.onset(np.zeros((1, 2, 100), np.float32), 100, SR, 8192)
    assert np.all(e["flags"][0, 3:11] == ref.F_DECIDED) and np.all(e["flags"][0, :3] == 0) and np.all(e["flags"][0, 11:] == 0)


def test_silence_reads_exact_zeros_and_no_flag():
    z = np.zeros((2, 2, 70000), np.float32)
    z[1, 0] = -0.0
    for ring in (8192, 65536):
        e = ref.onset(z, 70000, SR, ring)
        t = ref.columns(ring)
        assert not np.any(e["strength"]) and not np.any(e["group"]) and not np.any(np.signbit(e["strength"]))
        assert np.all((e["flags"] & 0x7F) == 0) and np.all(e["onsets"] == 0) and np.all(e["last_age"] == ref.NONE)
        assert np.all(e["last_frame"] == 0) and np.all(e["last_strength"] == 0) and not np.any(e["reserved"])
        assert np.all(e["columns"] == t) and np.all(e["newest"] == 70000 // H) and np.all(e["decided_end"] == t - 16)
        assert np.all(e["window"] == P) and np.all(e["hop"] == H) and e[0].tobytes() == e[1].tobytes()


def _curve(values):
    """[1, 4, T] by age from a list oldest first, the same curve four times"""
    o = np.asarray(values, np.float32)[::-1]
    return np.broadcast_to(o, (1, 4, len(o))).copy()


def test_the_picking_rule_on_hand_made_curves():
    base = [0.0] * 40
    v = list(base)
    v[20] = 3.0  # mean = 3 / 20 = 0.15: 3 >= 2.15
    f = ref.pick(_curve(v))[0][::-1]  # oldest first
    assert f[20] == 0x8F and np.count_nonzero(f & 0x0F) == 1
    assert np.all(f[16:37] & 0x80) and not np.any(f[:16] & 0x80) and not np.any(f[37:] & 0x80)  # n - 16 .. n + 3 in view
    v[20] = 2.1  # mean 0.105: 2.1 < 2.105
    assert not np.any(ref.pick(_curve(v)) & 0x0F)
    v[20] = 40.0 / 19.0 + 1e-3  # v >= v / 20 + 2 from v = 40 / 19 up
    assert np.count_nonzero(ref.pick(_curve(v)) & 1) == 1
    v = list(base)
    v[20], v[21] = 5.0, 5.0   # a plateau: the first of two equal columns is the onset (>= after, > before)
    f = ref.pick(_curve(v))[0][::-1]
    assert f[20] & 1 and not f[21] & 1
    v[20], v[23] = 5.0, 5.5   # a higher column within three hops behind: it takes the onset
    f = ref.pick(_curve(v))[0][::-1]
    assert not f[20] & 1 and f[23] & 1
    v = list(base)
    v[20], v[24] = 5.0, 5.5   # four hops behind: both
    f = ref.pick(_curve(v))[0][::-1]
    assert f[20] & 1 and f[24] & 1
    v = list(base)
    v[14], v[20] = 6.0, 5.0   # six hops before: 5 is not above it; seven hops before: it is
    assert not ref.pick(_curve(v))[0][::-1][20] & 1
    v[14], v[13] = 0.0, 6.0
    assert ref.pick(_curve(v))[0][::-1][20] & 1
    # the curves are picked independently
    o = _curve(base)
    o[0, 2, ::-1][20] = 3.0
    f = ref.pick(o)[0][::-1]
    assert f[20] == 0x80 | ref.F_MID
    assert ref.pick(np.zeros((2, 4, 19), np.float32)).tolist() == np.zeros((2, 19), np.uint8).tolist()


def test_margins_measure_the_distance_from_flipping():
    v = [0.0] * 40
    v[20] = 3.0
    assert ref.margins(_curve(v)) > 1e5
    ulp = float(np.spacing(np.float32(3.0)))
    v[21] = 3.0 - 2 * ulp     # the onset's ">= after" holds by two ulps
    assert abs(ref.margins(_curve(v)) - 2.0) < 1e-6
    v[21] = 3.0 + 2 * ulp     # the onset moves to column 21, whose "> before" holds by two ulps
    assert ref.pick(_curve(v))[0][::-1][21] & 1 and abs(ref.margins(_curve(v)) - 2.0) < 1e-6
    v[21] = 0.0
    v[20] = np.float32(40.0 / 19.0) + 3 * np.spacing(np.float32(2.1))  # the threshold holds by about three ulps
    assert 1.0 < ref.margins(_curve(v)) < 4.0
    # columns that are no onsets by a wide margin somewhere do not count, however close their other comparisons are
    assert ref.margins(_curve([1e-15 * (i % 3) for i in range(40)])) > 1e5
    assert ref.margins(np.zeros((1, 4, 19), np.float32)) == np.inf


EVENTS = (("kicks", ref.kicks), ("bursts", ref.bursts), ("legato", ref.legato))
SEEDS = (0, 2)


@pytest.mark.parametrize("name,make", EVENTS, ids=[e[0] for e in EVENTS])
def test_every_synthetic_event_is_found(name, make):
    """4 s each on the committed seeds: one onset of the total per event and none besides, its column's position n H - 384 within
    +-256 frames of where the event starts"""
    for seed in SEEDS:
        x, starts = make(np.random.default_rng(seed))
        o, flags = ref.scan(x, SR)
        cols = np.flatnonzero(flags & ref.F_TOTAL) + 1  # scan's first column is n = 1
        frames = cols * H - 3 * P // 8
        off = [int(frames[np.argmin(np.abs(frames - s))] - s) for s in starts]
        print(name, seed, "events", len(starts), "onsets at", frames.tolist(), "off by", off)
        assert len(cols) == len(starts) and all(abs(d) <= 256 for d in off)
        # what a read would report: the event in view of a ring of 65536 frames that ends 2000 frames behind the last event
        wpos = starts[-1] + 2000
        e = ref.onset(x[None, None, :wpos], wpos, SR, 65536)[0]
        assert e["onsets"] >= 1 and abs(int(e["last_frame"]) - starts[-1]) <= 256 and e["last_age"] == (wpos // H) - cols[-1]
        assert e["last_strength"] == e["strength"][e["last_age"]] == o[0, cols[-1] - 1]


def test_stationary_signals_have_no_onset():
    for seed in SEEDS:
        for db in (-20.0, -60.0):
            x, _ = ref.stationary(np.random.default_rng(seed), db)
            o, flags = ref.scan(x, SR)
            assert np.count_nonzero(flags & ref.F_DECIDED) > 700 and not np.any(flags & 0x0F), (seed, db)
    x, _ = ref.steady_sine(None)
    o, flags = ref.scan(x, SR)
    assert not np.any(flags & 0x0F) and o[0, 0] > 5.0  # (its start out of silence is an event, in no decided column)


def test_decided_flags_stand_still_when_frames_are_appended():
    rng = np.random.default_rng(3)
    x, _ = ref.bursts(rng)
    x = np.stack([x, x[::-1]])[None, :, :60000]
    for ring in (8192, 32768):
        t = ref.columns(ring)
        for wpos in (40000, 40101, 43211):
            one = ref.onset(x[:, :, :wpos], wpos, SR, ring)[0]
            two = ref.onset(x[:, :, :wpos + 300], wpos + 300, SR, ring)[0]
            d = int(two["newest"]) - int(one["newest"])
            assert d in (1, 2)
            assert np.array_equal(two["strength"][d:t], one["strength"][:t - d]) and np.array_equal(two["group"][:, d:t], one["group"][:, :t - d])
            both = np.arange(3, t - 16 - d)  # decided in both reads
            assert np.array_equal(two["flags"][both + d], one["flags"][both]) and np.all(one["flags"][both] & 0x80)
    assert np.any(ref.onset(x[:, :, :40000], 40000, SR, 32768)["flags"] & 1)


def test_mismatches_holds_what_the_contract_says():
    case = ref.GPU_CASES[2]
    fft, sr, ch, kw, ring_frames, ring_cap, t = case
    x = ref.case_audio(case)
    wpos = x.shape[-1]
    want = ref.onset(x, wpos, sr, ring_cap)
    assert ref.mismatches(want, x, wpos, sr, ring_cap) == ([], 0.0)
    got = want.copy()  # one ulp on a strength that no decision hangs on by less: within the contract
    a = int(np.argmax(want["strength"][0]))
    got["strength"][0, a] = np.nextafter(got["strength"][0, a], np.float32(99))
    if want["last_age"][0] == a:
        got["last_strength"][0] = got["strength"][0, a]
    bad, worst = ref.mismatches(got, x, wpos, sr, ring_cap)
    assert bad == [] and abs(worst - 1.0) < 1e-6
    got["strength"][0, a] = np.nextafter(got["strength"][0, a], np.float32(99))
    assert any(m[0] == "strength" for m in ref.mismatches(got, x, wpos, sr, ring_cap)[0])
    for name in ("columns", "newest", "decided_first", "decided_end", "window", "hop", "onsets", "last_age", "last_frame", "reserved"):
        got = want.copy()
        got[name][1] += 1
        assert name in {m[0].split(" ")[0] for m in ref.mismatches(got, x, wpos, sr, ring_cap)[0]}, name
    got = want.copy()
    got["flags"][2, 5] ^= 1
    assert {m[0].split(" ")[0] for m in ref.mismatches(got, x, wpos, sr, ring_cap)[0]} >= {"flags"}
    got = want.copy()  # something where the entry has nothing
    got["group"][0, 1, t] = 1e-20
    assert [m[:2] for m in ref.mismatches(got, x, wpos, sr, ring_cap)[0]] == [("group", (0, 1, t))]
    got = want.copy()
    got["strength"][1, 3] = np.nan
    assert ref.mismatches(got, x, wpos, sr, ring_cap)[0]
    assert ref.mismatches(want[:1], x, wpos, sr, ring_cap)[0][0][0] == "shape"


def test_the_gpu_cases_meet_the_comparisons_conditions():
    """on tests/test_gpu_onset.py's own seeds and shapes: no decision of the restatement lies within four float32 ulps of flipping,
    so that strengths one ulp apart cannot flip a flag; the counter ends off the hop grid; the span read wraps the ring; every
    frame read was pushed; the packets are odd and unequal; and there is something to find"""
    for case in ref.GPU_CASES:
        fft, sr, ch, kw, ring_frames, ring_cap, t = case
        assert t == ref.columns(ring_cap) and (ring_frames == 0 or ring_frames == ring_cap) and ring_cap >= ref.MIN_RING
        x = ref.case_audio(case)
        wpos0 = ref.case_wpos0(case)
        wpos = wpos0 + x.shape[-1]
        assert x.shape == (3, ch, ring_cap + P // 2 + 3) and wpos % H != 0
        newest_end = wpos - wpos % H
        oldest = newest_end - t * H - P
        assert oldest >= wpos0  # every frame read was pushed
        assert oldest // ring_cap != (newest_end - 1) // ring_cap  # ring positions run over the ring's end inside the span
        sizes = [hi - lo for lo, hi in ref.packets(np.random.default_rng(ring_cap), x.shape[-1])]
        assert sum(sizes) == x.shape[-1] and all(n % 2 == 1 for n in sizes) and len(set(sizes)) > len(sizes) // 2
        hist = np.concatenate([np.zeros((3, ch, wpos0), np.float32), x], axis=2)
        o = ref.strengths(hist, wpos, sr, ring_cap)
        m = [ref.margins(o[s:s + 1]) for s in range(3)]
        e = ref.entries(o, wpos)
        print(f"{ref.case_id(case)}: margins {[round(v, 1) for v in m]} ulps, onsets {e['onsets'].tolist()}, last_age {e['last_age'].tolist()}, "
              f"flagged columns per curve {[[int(np.count_nonzero(e['flags'][s] & b)) for b in (1, 2, 4, 8)] for s in range(3)]}")
        assert min(m) >= 4.0
        assert e["onsets"][0] == 0 and e["onsets"][1] >= 1 and np.any(e["flags"][2] & 0x0F)  # noise: none; the burst; the chirp
        assert np.all(o[0, 0] > 0) and np.any(o[1, 0] == 0) and np.all(np.isfinite(o))  # the burst's silence reads exact zeros
    assert [c[6] for c in ref.GPU_CASES] == [27, 27, 59, 123, 128, 128, 27] and [c[2] for c in ref.GPU_CASES].count(1) == 2
    assert [ref.case_id(c) for c in ref.GPU_CASES] == ["ring8192_sr48000_ch2_fft1024", "ring8192_sr48000_ch1_fft4096", "ring16384_sr44100_ch2_fft4096",
                                                      "ring32768_sr48000_ch2_fft4096", "ring65536_sr48000_ch2_fft4096", "ring65536_sr48000_ch1_fft2048",
                                                      "ring8192_sr48000_ch2_meter"]


def test_onset_kernels_have_no_scratch():
    res = kernel_usage("wf_hip_measure", "onset_read_kernel")
    assert len(res) == 2 and any("ILi1E" in n for n in res) and any("ILi2E" in n for n in res), res  # <1> and <2>
    for name, r in res.items():
        assert r.get("ScratchSize [bytes/lane]") == 0 and r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
        assert r.get("LDS Size [bytes/block]") == 0, (name, r)  # the transforms, the levels and the entry's image are dynamic LDS
        # two workgroups of four waves to a CU: two waves to a SIMD
        assert r.get("Occupancy [waves/SIMD]") >= 2, (name, r)
    lds = 4 * P * 16 + 5 * 64 * 8 + 4 * 128 * 4 + 128
    assert lds == 70272 and 2 * lds <= 160 * 1024
