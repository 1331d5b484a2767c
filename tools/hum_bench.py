"""Cost of reading WF_HIP_OUT_HUM, 4096 stereo streams at 48 kHz: ring_frames = 16384 (N = 16384, sixteen transforms of 512 points
per channel) and 32768 (N = 32768, sixteen of 1024 points, the LDS at its cap), for three contents of the rings: hum over noise
(tests/hum_ref.py's lines at 50.13 Hz under white noise at -40 dBFS, 64 different streams repeated), noise alone, and digital
silence (the kernel stages the window, sums it and leaves).
In one process, per shape and content: (a) wf_hip_read of the whole batch back to back into page-locked memory (wf_hip_host_alloc:
what the copy in (b) gets as well) and hum() of the Python binding, which reads into a fresh numpy array, both by device events on
the handle's stream (wf_hip_time_begin / _end around the calls; the read's copy of 304 bytes per stream to the host is inside the
bracket) and by the host clock; (b) the alternative a host has: the N-frame windows of both channels copied to the host -- a device
block of that size (the library has no reader for the rings) by hipMemcpy into page-locked memory, in parts of at most 512 MB whose
times add up.  The transform and the rule the host would then run are not counted.  Every figure is the median of `rounds` rounds
of `reads` calls after `warmup` calls, with the smallest and largest round beside it.  One JSON line.  The kernel's own time
without the copy is not measured here.
usage: python tools/hum_bench.py [--streams 4096] [--rings 16384,32768] [--warmup 2] [--reads 5] [--rounds 5] [--out FILE.json]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import waveform_amd as wf

import hum_ref as ref
from bench_common import emit, parser, rounds, windows_copy_in_parts

SR = 48000
DISTINCT = 64


def _fill(b, kind, frames):
    if kind == "silence":
        return
    rng = np.random.default_rng(29)
    if kind == "hum":
        x = np.stack([np.stack([ref.comb(rng, 50.13, ref.LEVELS, frames, SR, -40.0) for _ in range(2)]) for _ in range(DISTINCT)])
    else:
        x = np.stack([np.stack([ref.noise(rng, -40.0, frames) for _ in range(2)]) for _ in range(DISTINCT)])
    for first in range(0, b.streams, DISTINCT):
        b.push_audio(np.ascontiguousarray(x[:min(DISTINCT, b.streams - first)]), first=first)
    b.sync()


def one_shape(a, streams, ring_frames):
    cfg = wf.Config.defaults(fft_size=1024, sample_rate=SR, stereo=1, slope=1.0, bars=1, floor_db=-70)
    L = wf.lib()
    B = wf.binding
    pl = ref.plan(SR, ring_frames)
    per_stream = 2 * pl.N * 4
    res = dict(streams=streams, ring_frames=ring_frames, window=pl.N, decimation=pl.D, points=pl.M, bins=pl.K,
               windows_MB=round(streams * per_stream / 1e6, 1), hum_MB=round(streams * B.HUM_DTYPE.itemsize / 1e6, 2))
    for kind in ("hum", "noise", "silence"):
        with wf.SpectrumBatch(cfg, streams, ring_frames=ring_frames) as b:
            assert b.ring_frames == ring_frames
            _fill(b, kind, pl.N + 777)  # an odd count: the window starts at no aligned place and wraps the ring's end
            out = wf.PinnedBuffer((streams,), B.HUM_DTYPE)

            def read_pinned():
                assert L.wf_hip_read(b.h, B.OUT_HUM, 0, streams, C.c_void_p(out.ptr)) == 0

            got = b.hum()
            read_pinned()
            assert out.array.tobytes() == got.tobytes() and np.all(got["window"] == pl.N)
            want = {"hum": (1, 50), "noise": (1, 0), "silence": (0, 0)}[kind]
            assert np.all(got["ch"]["valid"] == want[0]) and np.mean(got["ch"]["family"] == want[1]) > 0.95, kind
            r = dict(lines=int(got["ch"]["lines"].sum()), family_found=round(float(np.mean(got["ch"]["family"] != 0)), 4))
            r["read_pinned"] = rounds(b, read_pinned, a.warmup, a.reads, a.rounds)
            r["read"] = rounds(b, b.hum, a.warmup, a.reads, a.rounds)
            out.close()
            res[kind] = r
    res["windows_copy_parts"], res["windows_copy_pinned"] = windows_copy_in_parts(streams, pl.N, max(a.reads // 2, 3), a.rounds)
    copy = res["windows_copy_pinned"]["host_us"][0]
    for kind in ("hum", "noise", "silence"):
        res[kind]["copy_over_read_pinned"] = round(copy / res[kind]["read_pinned"]["host_us"][0], 2)
    return res


def main():
    a = parser(2, 5, streams=4096, rings="16384,32768").parse_args()
    res = dict(sample_rate=SR, reads=a.reads, warmup=a.warmup, rounds=a.rounds,
               shapes=[one_shape(a, a.streams, int(r)) for r in a.rings.split(",")])
    emit(a, res)


if __name__ == "__main__":
    main()
