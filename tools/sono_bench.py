"""Cost of reading WF_HIP_OUT_SONO at the headline shape, 4096 stereo streams at 48 kHz and FFT 4096: with the default ring of 8192
frames (T = 28 columns) and with ring_frames = 32768 (T = 64).  The rings hold independent noise.
In one process, per ring: (a) wf_hip_read of the whole batch back to back into page-locked memory (wf_hip_host_alloc: what the copy
in (b) gets as well) and sono() of the Python binding, which reads into a fresh numpy array -- pageable memory that is touched for
the first time by the copy --, both by device events on the handle's stream (wf_hip_time_begin / _end around the calls; the read's
134.3 MB copy to the host is inside the bracket) and by the host clock, with signal() -- another reader of the rings, 0.2 MB
back -- beside it; (b) the alternative a host has: the span of both rings that the columns cover, (T - 1) H + P + H - 1 frames
per channel, copied to the host -- a device block of that size (the library has no reader for the rings) by hipMemcpy into
page-locked memory.  The transforms the host would then run are not counted.  Every figure is the median of `rounds` rounds of
`reads` calls after `warmup` calls, with the smallest and largest round beside it.  One JSON line.
usage: python tools/sono_bench.py [--streams 4096] [--rings 0,32768] [--warmup 3] [--reads 10] [--rounds 5] [--out FILE.json]"""
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
        first = b.sono(0, 1)
        t = int(first["columns"][0])
        span = (t - 1) * B.SONO_HOP + B.SONO_WINDOW + B.SONO_HOP - 1
        nbytes = a.streams * 2 * span * 4
        entry = B.SONO_DTYPE.itemsize
        res = dict(ring_frames=b.ring_frames, columns=t, span_frames=span, span_MB=round(nbytes / 1e6, 1),
                   sono_MB=round(a.streams * entry / 1e6, 1))
        out = wf.PinnedBuffer((a.streams,), B.SONO_DTYPE)

        def read_pinned():
            assert L.wf_hip_read(b.h, B.OUT_SONO, 0, a.streams, C.c_void_p(out.ptr)) == 0

        got = b.sono()
        read_pinned()
        assert out.array.tobytes() == got.tobytes()
        assert np.all(np.isfinite(got["db"][:, :, :t])) and np.all(np.isneginf(got["db"][:, :, t:]))
        res["mean_db"] = round(float(np.mean(got["db"][:, :, :t])), 2)
        res["sono_read_pinned"] = rounds(b, read_pinned, a.warmup, a.reads, a.rounds)
        res["sono_read"] = rounds(b, b.sono, a.warmup, a.reads, a.rounds)
        res["signal_read"] = rounds(b, b.signal, a.warmup, a.reads, a.rounds)
        out.close()
        res["span_copy_pinned"] = windows_copy((a.streams, 2, span), max(a.reads // 2, 3), a.rounds)
    copy = res["span_copy_pinned"]["host_us"][0]
    res["copy_over_read_pinned"] = round(copy / res["sono_read_pinned"]["host_us"][0], 2)
    res["copy_over_read"] = round(copy / res["sono_read"]["host_us"][0], 2)
    return res


def main():
    a = parser(3, 10, streams=4096, rings="0,32768").parse_args()
    res = dict(streams=a.streams, fft=4096, reads=a.reads, warmup=a.warmup, rounds=a.rounds,
               rings=[one_ring(a, int(r)) for r in a.rings.split(",")])
    emit(a, res)


if __name__ == "__main__":
    main()
