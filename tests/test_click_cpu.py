"""Click detector (WF_HIP_OUT_CLICK) without a device: the structured dtype against the C layout, the appended output number, the
readings include/wf_hip.h's definition promises of its numpy restatement (tests/click_ref.py) at P = 256, 800, 4096 and 8192, and
the conditions the bit-for-bit comparison of tests/test_gpu_click.py rests on, for every window that test reads.

Zeros followed by noise at P = 256 are why a window of one block leans on the medians of its two halves: with the block's own median
alone, which stands on the eighth-lowest residual of the noise there, the restatement read 1 to 3 events of 24.3 to 34.8 dB on 18 of
click_ref's seeds 0 .. 23.  With the halves at half their weight all 24 read none (peak_db 11.7 to 16.1), and every other reading at
P = 256 is the same bits, since half a half's median lies under the block's own wherever the block is of one kind."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from waveform_amd import binding
import click_ref as ref

ROOT = Path(__file__).resolve().parents[1]
WINDOWS = (256, 800, 4096, 8192)  # FFT 256, 800, 4096 and 16384
CHANNEL_FIELDS = ("valid", "events", "hit_frames", "listed", "rate", "peak_db", "floor_db", "prediction_gain_db", "ev")
EVENT_FIELDS = ("start", "length", "peak", "frame", "strength_db", "amplitude")
FIELDS = ("ch", "window", "order", "reserved")


def test_click_dtype_matches_the_c_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wf_hip.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %zu %d %d %d %d %d %d", sizeof(wf_hip_click), sizeof(wf_hip_click_channel), sizeof(wf_hip_click_event),\n'
                   "         (int)WF_HIP_OUT_CLICK, (int)WF_HIP_OUT_IMPULSE, (int)WF_HIP_CLICK_MAX_WINDOW, (int)WF_HIP_CLICK_ORDER,\n"
                   "         (int)WF_HIP_CLICK_GAP, (int)WF_HIP_CLICK_MAX_EVENTS);\n"
                   + "".join(f'  printf(" %zu", offsetof(wf_hip_click_event, {n}));\n' for n in EVENT_FIELDS)
                   + "".join(f'  printf(" %zu", offsetof(wf_hip_click_channel, {n}));\n' for n in CHANNEL_FIELDS)
                   + "".join(f'  printf(" %zu", offsetof(wf_hip_click, {n}));\n' for n in FIELDS) +
                   '  printf(" %zu %d %d", offsetof(wf_hip_click, ch[1]), (int)WF_HIP_ABI_VERSION, WF_HIP_CLICK_THRESHOLD == 16.0);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    dt, ch, ev = binding.CLICK_DTYPE, binding.CLICK_CHANNEL_DTYPE, binding.CLICK_EVENT_DTYPE
    assert got == [dt.itemsize, ch.itemsize, ev.itemsize, binding.OUT_CLICK, binding.OUT_IMPULSE, binding.CLICK_MAX_WINDOW, binding.CLICK_ORDER,
                   binding.CLICK_GAP, binding.CLICK_MAX_EVENTS] + [ev.fields[n][1] for n in EVENT_FIELDS] \
        + [ch.fields[n][1] for n in CHANNEL_FIELDS] + [dt.fields[n][1] for n in FIELDS] + [ch.itemsize, 13, 1]
    assert dt.itemsize == 464 and ch.itemsize == 224 and ev.itemsize == 24 and dt.itemsize % 16 == 0
    assert dt.names == FIELDS and ch.names == CHANNEL_FIELDS and ev.names == EVENT_FIELDS
    assert binding.CLICK_THRESHOLD == 16.0 and ref.MAX_WINDOW == 8192 and ref.ORDER == 16


def _read(kind, p):
    rec, ratio, det = ref.analyse(ref.signal(kind, p))
    print(f"{kind} P={p}: events {rec['events']}, hit_frames {rec['hit_frames']}, peak_db {rec['peak_db']:.2f}, floor_db {rec['floor_db']:.2f}, "
          f"gain {rec['prediction_gain_db']:.2f} dB, listed {[(int(e['start']), int(e['length']), float(e['strength_db'])) for e in rec['ev'][:rec['listed']]]}")
    return rec, ratio, det


@pytest.mark.parametrize("p", WINDOWS)
def test_clean_noise_gives_no_event(p):
    rec = _read("noise", p)[0]
    assert rec["valid"] == 1 and rec["events"] == 0 and rec["hit_frames"] == 0 and rec["listed"] == 0 and rec["rate"] == 0
    assert 6.0 < rec["peak_db"] < 15.0 and not rec["ev"].tobytes().strip(b"\0")


@pytest.mark.parametrize("p", WINDOWS)
def test_a_clean_sine_gives_no_event(p):
    rec = _read("sine", p)[0]
    assert rec["valid"] == 1 and rec["events"] == 0 and abs(rec["peak_db"]) < 1.0 and rec["prediction_gain_db"] > 20.0


@pytest.mark.parametrize("p", WINDOWS)
def test_two_clicks_in_noise_are_found_at_their_frames(p):
    rec = _read("noise clicks", p)[0]
    assert rec["events"] == 2 and rec["listed"] == 2
    first, second = rec["ev"][0], rec["ev"][1]
    assert first["start"] == first["peak"] == p // 2 and second["start"] == second["peak"] == p // 4
    assert 1 <= first["length"] <= 2 and 1 <= second["length"] <= 2
    assert 34.0 < second["strength_db"] < first["strength_db"] < 40.0
    assert abs(first["amplitude"] - 0.3) < 0.02 and abs(second["amplitude"] + 0.2) < 0.02  # the sign of each
    assert rec["rate"] == np.float32(2.0 * 48000.0 / (p - 16))


@pytest.mark.parametrize("p", (4096, 8192))
def test_a_small_click_on_a_sine_is_found(p):
    rec = _read("sine click", p)[0]
    assert rec["events"] == 1 and rec["ev"][0]["start"] == p // 3 and abs(rec["ev"][0]["strength_db"] - (36.0 if p == 4096 else 42.6)) < 1.0


@pytest.mark.parametrize("p", WINDOWS)
def test_a_lone_click_in_silence(p):
    rec = _read("lone", p)[0]
    assert rec["valid"] == 1 and rec["events"] == 1 and rec["ev"][0]["start"] == p // 2 and rec["ev"][0]["length"] == 1
    assert 140.0 <= rec["ev"][0]["strength_db"] < 142.0 and rec["ev"][0]["amplitude"] == np.float32(0.25)
    assert abs(rec["prediction_gain_db"]) < 1e-6 and rec["floor_db"] == -np.inf


@pytest.mark.parametrize("p", WINDOWS)
def test_zeros_followed_by_noise_give_no_event(p):
    rec = _read("half", p)[0]
    assert rec["valid"] == 1 and rec["events"] == 0, (int(rec["events"]), rec["ev"]["strength_db"][:int(rec["listed"])].tolist())


@pytest.mark.parametrize("p", (256, 400, 527))
def test_a_lone_block_leans_on_its_halves(p):
    """windows of one block (P - 16 < 512): zeros followed by noise read no event on 24 seeds, well under the threshold, and where
    the block is of one kind -- noise with two clicks -- the halves change nothing: s_0 is 1.4826 times the block's own median"""
    peaks = []
    for seed in range(24):
        rec = ref.analyse(ref.signal("half", p, seed))[0]
        assert rec["events"] == 0, (seed, int(rec["events"]))
        peaks.append(float(rec["peak_db"]))
        rec, ratio, det = ref.analyse(ref.signal("noise clicks", p, seed))
        assert rec["events"] == 2 and len(det["med"]) == 3 and det["s"][0] == 1.4826 * det["med"][0] and det["med"][0] > max(det["med"][1:])
    print(f"P={p}: zeros then noise, peak_db {min(peaks):.1f} to {max(peaks):.1f}")
    assert max(peaks) < 20.0  # 4 dB under the threshold of 24.1


def test_twelve_clicks_list_the_eight_strongest():
    p = 8192
    rec, ratio, det = _read("crackle", p)
    pos = ref.crackle_positions(p)
    assert len(pos) == 12 and np.min(np.diff(pos)) >= ref.CRACKLE_SPACING
    assert rec["events"] == 12 and rec["listed"] == 8 and rec["hit_frames"] >= 12
    assert sorted(e[0] for e in det["events"]) == pos.tolist()
    s = rec["ev"]["strength_db"].astype(np.float64)
    assert np.all(np.diff(s) < 0)  # descending (and no two equal here)
    want = sorted(range(12), key=lambda i: (-det["strengths"][i], det["events"][i][0]))[:8]
    assert rec["ev"]["start"].tolist() == [det["events"][i][0] for i in want]
    assert min(det["strengths"][i] for i in want) >= max(det["strengths"][i] for i in range(12) if i not in want)
    assert rec["ev"]["frame"].tolist() == rec["ev"]["start"].tolist()  # the counter stands at P by default


def test_equal_strengths_list_the_earlier_start_first():
    x = np.zeros(1024, np.float32)
    x[300] = x[700] = 0.25
    rec = ref.analyse(x)[0]
    assert rec["events"] == 2 and rec["ev"]["strength_db"][0] == rec["ev"]["strength_db"][1] and rec["ev"]["start"][:2].tolist() == [300, 700]


@pytest.mark.parametrize("p", WINDOWS)
@pytest.mark.parametrize("kind", ("skip", "repeat"))
def test_a_splice_gives_an_event_at_the_splice(kind, p):
    rec = _read(kind, p)[0]
    c = ref.splice_at(p)
    assert rec["events"] == 1 and c <= rec["ev"][0]["start"] <= c + 2 and rec["ev"][0]["strength_db"] > 30.0
    clean = ref.analyse((ref.note(p) + ref.pink(np.random.default_rng(1), p, 1e-4)).astype(np.float32))[0]
    assert clean["events"] == 0  # the note without its splice


@pytest.mark.parametrize("p", WINDOWS)
def test_silence_and_a_nan_are_invalid(p):
    for kind in ref.INVALID + ("inf",):
        x = ref.signal("noise", p) if kind == "inf" else ref.signal(kind, p)
        if kind == "inf":
            x[p - 1] = -np.inf
        rec = ref.analyse(x)[0]
        assert rec["valid"] == 0 and rec["peak_db"] == rec["floor_db"] == rec["prediction_gain_db"] == -np.inf
        rec["peak_db"] = rec["floor_db"] = rec["prediction_gain_db"] = 0.0
        assert not rec.tobytes().strip(b"\0")  # every other field 0


def test_hits_within_the_gap_form_one_event():
    rng = np.random.default_rng(3)
    x = ref.pink(rng, 2048)
    x[1000] += 0.3
    x[1000 + ref.GAP] -= 0.3   # a gap of exactly GAP: the same event
    x[1500] += 0.3
    x[1500 + ref.GAP + 1] += 0.3  # one more: two events
    rec, ratio, det = ref.analyse(x.astype(np.float32))
    starts = sorted((e[0], e[1]) for e in det["events"])
    assert [s for s, _ in starts] == [1000, 1500, 1500 + ref.GAP + 1] and starts[0][1] >= 1000 + ref.GAP
    assert rec["events"] == 3


def test_the_sums_order_is_the_headers_and_barely_matters():
    """r in the header's order against math.fsum: the residual of the ill-conditioned case, a sine with a click, moves by less than
    1e-8 of its median"""
    import math
    x = ref.signal("sine click", 4096).astype(np.float64)
    r = ref.autocorrelation(x)
    exact = np.array([math.fsum(x[k:] * x[:len(x) - k]) for k in range(ref.ORDER + 1)])
    assert np.max(np.abs(r - exact)) <= 1e-13 * exact[0]

    def residual(rr):
        a, _ = ref.levinson(rr)
        acc = np.zeros(len(x) - ref.ORDER)
        for k in range(1, ref.ORDER + 1):
            acc = acc + a[k] * x[ref.ORDER - k:len(x) - k]
        return x[ref.ORDER:] - acc
    e0, e1 = residual(r), residual(exact)
    moved = float(np.max(np.abs(e0 - e1)) / np.median(np.abs(e0)))
    print(f"residual moved by {moved:.3g} of its median")
    assert moved < 1e-8


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=ref.case_id)
def test_the_margin_condition_holds_for_every_window_the_device_reads(case):
    """no judged frame's ratio within 1e-3 of the threshold, no two listed strengths within 1e-4 dB, and the same hits with every
    median and g one float32 ulp up and one down: what keeps the bit-for-bit comparison of the integers honest.  The seeds are fixed
    (click_ref.SEED, SEED_STEPS) so that this holds; it fails for a seed where it does not"""
    fft, ch, kw, w = case
    windows, wpos = ref.gpu_final_windows(case)
    p = ref.window_frames(w)
    assert windows.shape == (ref.STREAMS, ch, p) and len(set((wpos % 4).tolist())) == 4
    ring = ref.ring_frames(w)
    assert (wpos[1] % ring) < p and wpos[0] % ring == p + 5 and wpos[ref.RESET_STREAM] - (0 if kw.get("meter") else w) < p
    designed = ref.gpu_windows(case)
    for s in range(ref.STREAMS):
        for c in range(ch):
            if s == ref.RESET_STREAM:  # zeros, then the tail of its window
                assert not windows[s, c, :p // 2].any() and np.array_equal(windows[s, c, p // 2:], designed[s, c, p // 2:])
            else:
                assert windows[s, c].tobytes() == designed[s, c].tobytes(), (s, c)
            m = ref.margins(windows[s, c])
            print(f"stream {s} channel {c} ({ref.GPU_KINDS[s][c]}): least |ratio / threshold - 1| {m[0]:.4g}, listed strengths apart {m[1]:.4g} dB, "
                  f"the hits stand one ulp either way: {m[2]}")
            assert ref.margins_hold(m), (s, c, m)
    want = ref.click(windows, 48000, wpos)
    assert want["ch"]["valid"][:, 0].tolist() == [1, 1, 1, 1, 1, 1, 0] and want["ch"]["events"][0, 0] >= 1  # no trivial entries
    assert want["ch"]["events"][3, 0] == 1 and want["ch"]["ev"]["frame"][3, 0, 0] == (wpos[3] - p + p // 2) % (1 << 32)
    if ch == 2:
        assert want["ch"]["valid"][:, 1].tolist() == [1, 1, 1, 0, 1, 1, 1]
