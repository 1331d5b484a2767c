"""Cost of reading WF_HIP_OUT_ONSET at the headline shape, 4096 stereo streams at 48 kHz and FFT 4096: with the default ring of 8192
frames (T = 27 strength columns from 28 spectral ones) and with ring_frames = 65536 (T = 128 from 129).  The rings hold independent
noise (the kernel's work does not depend on the audio).
In one process, per ring: (a) wf_hip_read of the whole batch back to back into page-locked memory (wf_hip_host_alloc: what the copy
in (b) gets as well) and onset() of the Python binding, which reads into a fresh numpy array, both by device events on the handle's
stream (wf_hip_time_begin / _end around the calls; the read's 9.2 MB copy to the host is inside the bracket) and by the host clock,
with sono() -- the reader that transforms the same columns, up to 64 of them, and returns every cell -- and signal() beside it;
(b) the alternative a host has: the span of both rings that the columns cover, T H + P + H - 1 frames per channel, copied to the
host -- a device block of that size (the library has no reader for the rings) by hipMemcpy into page-locked memory.  The transforms
the host would then run are not counted.  Every figure is the median of `rounds` rounds of `reads` calls after `warmup` calls, with
the smallest and largest round beside it.  One JSON line.  The kernel's own time without its copy is not measured here.
usage: python tools/onset_bench.py [--streams 4096] [--rings 0,65536] [--warmup 3] [--reads 10] [--rounds 5] [--out FILE.json]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import waveform_amd as wf

from bench_common import emit, parser, rounds, windows_copy


def one_ring(a, ring_frames):
    cfg = wf.Config.defaults(fft_size=4096, sample_rate=48000, stereo=1, slope=1.0, bars=1, floor_db=-70)
    seed = 0x5741564546524D31
    L = wf.lib()
    B = wf.binding
    with wf.SpectrumBatch(cfg, a.streams, ring_frames=ring_frames) as b:
        b.push_synth(seed, 0, b.ring_frames + 801)  # the counter ends off the hop grid
        b.sync()
        first = b.onset(0, 1)
        t = int(first["columns"][0])
        span = t * B.ONSET_HOP + B.ONSET_WINDOW + B.ONSET_HOP - 1
        nbytes = a.streams * 2 * span * 4
        entry = B.ONSET_DTYPE.itemsize
        res = dict(ring_frames=b.ring_frames, columns=t, spectral_columns=t + 1, span_frames=span, span_MB=round(nbytes / 1e6, 1),
                   onset_MB=round(a.streams * entry / 1e6, 2))
        out = wf.PinnedBuffer((a.streams,), B.ONSET_DTYPE)

        def read_pinned():
            assert L.wf_hip_read(b.h, B.OUT_ONSET, 0, a.streams, C.c_void_p(out.ptr)) == 0

        got = b.onset()
        read_pinned()
        assert out.array.tobytes() == got.tobytes()
        assert np.all(got["strength"][:, :t] > 0) and not np.any(got["strength"][:, t:]) and np.all(got["columns"] == t)
        res["mean_strength"] = round(float(np.mean(got["strength"][:, :t])), 3)
        res["onsets"] = int(got["onsets"].sum())
        res["onset_read_pinned"] = rounds(b, read_pinned, a.warmup, a.reads, a.rounds)
        res["onset_read"] = rounds(b, b.onset, a.warmup, a.reads, a.rounds)
        out.close()
        res["sono_read"] = rounds(b, b.sono, 1, max(a.reads // 3, 2), max(a.rounds // 2, 2))
        res["signal_read"] = rounds(b, b.signal, a.warmup, a.reads, a.rounds)
        res["span_copy_pinned"] = windows_copy((a.streams, 2, span), max(a.reads // 2, 3), a.rounds)
    copy = res["span_copy_pinned"]["host_us"][0]
    res["copy_over_read_pinned"] = round(copy / res["onset_read_pinned"]["host_us"][0], 2)
    res["copy_over_read"] = round(copy / res["onset_read"]["host_us"][0], 2)
    return res


def main():
    a = parser(3, 10, streams=4096, rings="0,65536").parse_args()
    res = dict(streams=a.streams, fft=4096, reads=a.reads, warmup=a.warmup, rounds=a.rounds,
               rings=[one_ring(a, int(r)) for r in a.rings.split(",")])
    emit(a, res)


if __name__ == "__main__":
    main()
