"""The batches of tests/test_gpu_ring_stage.py and tests/test_ring_stage_cpu.py: eight stereo streams whose windows start at every
alignment of the ring's 16-byte groups, wholly inside the ring and across its end, for the outputs that stage their window through
waveform_amd/csrc/wf_ring_stage.hpp -- scope, gonio and bits.  (signal walks the same two runs with a loop of its own, and
tests/test_gpu_measure_stagger.py has it.)

A window of P frames that starts at ring position s is staged as the run [s, min(s + P, cap)) and, where s + P > cap, the run
[0, s + P - cap); each run as its at most 3 frames up to the next 16-byte boundary, its 16-byte words, in an unrolled loop of
4 x 256 words and a loop of 256, and its at most 3 frames behind the last boundary.

  w64_ring128     P = 64 in a ring of 128: runs of 1 to 64 frames, so the heads and tails dominate and a body can be empty.  The
                  smallest ring in which a window of 64 frames lies inside at a start other than 0, so that all eight combinations
                  of (start & 3, inside / across the end) exist.
  w64_ring64      P = 64 in the smallest ring wf_hip_create gives for it, 64 frames: the ring is the window.  Only a start of 0
                  lies inside; every other start crosses the end, at all four alignments.
  fft16384        P = 8192, the cap, in the default ring of 32768: a run of 4096 frames or more enters the unrolled loop.
A window of 64 frames is a meter batch's (8 ms at 8 kHz: wf_hip_fft_size() = 64, the least the oscilloscope takes); a spectrum
batch starts at fft_size 128.

One script per batch: uneven odd common packets that fill the ring and more, then one ragged push whose counts leave stream i's
window at STARTS[i].  The audio is scope_ref.audio's (a wave with two harmonics, DC and noise 30 dB under it, the channels
different in gain and noise), read by all three outputs."""
import numpy as np

import measure_stagger as ms
import scope_ref

STREAMS = 8
SEED = 20261120
OUTPUTS = ("scope", "gonio", "bits")
_KW = dict(sample_rate=48000, capture_channels=2, stereo=1, bars=1, slope=1.0, floor_db=-70)
_W64 = dict(fft_size=1024, sample_rate=8000, capture_channels=2, stereo=1, meter=1, bars=0, meter_ms=8, slope=1.0, floor_db=-70)

# (case, the window's frames P, where each stream's window starts in the ring)
BATCHES = (
    (ms.Case("w64_ring128", _W64, 128, 64, 128, 2), 64, (8, 21, 42, 63, 68, 65, 66, 127)),
    (ms.Case("w64_ring64", _W64, 1, 64, 64, 2), 64, (0, 1, 2, 3, 4, 5, 62, 63)),
    (ms.Case("fft16384", dict(fft_size=16384, **_KW), 0, 16384, 32768, 2), 8192, (4096, 9, 20002, 12291, 28676, 24581, 32766, 27579)),
)
BATCH_IDS = [b[0].name for b in BATCHES]
COMMON = (801, 1, 333, 77)  # the packets that follow the one that fills the ring


def runs(start, p, ring):
    """[(first ring position, frames)] of the window's one or two runs"""
    end = start + p
    return [(start, min(end, ring) - start)] + ([(0, end - ring)] if end > ring else [])


def parts(b0, n):
    """(head frames, 16-byte words, tail frames) of the run [b0, b0 + n), as ring_stage splits it"""
    b1 = b0 + n
    h = min((b0 + 3) & ~3, b1)
    e = max(b1 & ~3, h)
    return h - b0, (e - h) // 4, b1 - e


def combinations(case, p, counters):
    """{(window start & 3, whether the window crosses the ring's end)} of the streams, from their counters"""
    return {(int((c - p) % 4), int((c - p) % case.ring_cap + p > case.ring_cap)) for c in np.asarray(counters, np.int64)}


def plan(batch):
    """the common packets and the ragged counts that leave the windows at the batch's starts"""
    case, p, starts = batch
    common = (case.ring_cap + 3,) + COMMON
    at = case.wpos0 + sum(common)
    counts = [(s + p - at) % case.ring_cap for s in starts]
    counts = [c if c else case.ring_cap for c in counts]  # (every stream takes part in the ragged push)
    return common, np.asarray(counts, np.uint32)


def script(batch):
    """measure_stagger.replay's steps: ("push", 0, x) ..., ("ragged", x, counts), ("read", "the end")"""
    case, p, _ = batch
    common, counts = plan(batch)
    total = sum(common) + int(counts.max())
    bank = scope_ref.audio(np.random.default_rng(SEED + case.ring_cap), STREAMS, total, case.W)
    steps, at = [], 0
    for n in common:
        steps.append(("push", 0, np.ascontiguousarray(bank[:, :, at:at + n])))
        at += n
    x = np.zeros((STREAMS, 2, int(counts.max())), np.float32)
    for s in range(STREAMS):
        x[s, :, :int(counts[s])] = bank[s, :, at:at + int(counts[s])]
    return steps + [("ragged", x, counts), ("read", "the end")]
