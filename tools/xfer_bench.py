"""Cost of reading WF_HIP_OUT_XFER at the headline shape, 4096 stereo streams at 48 kHz and FFT 4096: with the default ring of 8192
frames (P = 1024, K = 13 segments) and with ring_frames = 65536 (P = 2048, K = 32).  The kernel's work depends on one thing in the
audio, whether the lag it finds is 0: then the sums of the first pass stand (K + 1 transforms), otherwise a second pass follows
(2 K + 1).  So two legs per ring: independent noise in the two channels, whose lag is noise (both passes), and dual mono (one).
In one process, per ring and leg: (a) wf_hip_read of the whole batch back to back into page-locked memory (wf_hip_host_alloc: what the
copy in (b) gets as well) and xfer() of the Python binding, which reads into a fresh numpy array, both by device events on the
handle's stream (wf_hip_time_begin / _end around the calls; the read's 50.5 MB copy to the host is inside the bracket) and by the host
clock, with delay() and signal() beside it; (b) the alternative a host has: the span of both rings that the segments cover,
(K - 1) H + P + 2 L + H - 1 frames per channel, copied to the host -- a device block of that size (the library has no reader for the
rings) by hipMemcpy into page-locked memory.  The transforms the host would then run are not counted.  Every figure is the median of
`rounds` rounds of `reads` calls after `warmup` calls, with the smallest and largest round beside it.  One JSON line.  The kernel's
own time without its copy is not measured here.
usage: python tools/xfer_bench.py [--streams 4096] [--rings 0,65536] [--warmup 2] [--reads 5] [--rounds 5] [--out FILE.json]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import waveform_amd as wf

from bench_common import emit, parser, rounds, windows_copy

CHUNK = 2053  # frames per push of the dual-mono leg


def one_leg(a, ring_frames, dual):
    cfg = wf.Config.defaults(fft_size=4096, sample_rate=48000, stereo=1, slope=1.0, bars=1, floor_db=-70)
    seed = 0x5741564546524D31
    L = wf.lib()
    B = wf.binding
    with wf.SpectrumBatch(cfg, a.streams, ring_frames=ring_frames) as b:
        if dual:  # the same noise in both channels of every stream, chunk by chunk
            mono = (0.25 * np.random.default_rng(1).standard_normal(CHUNK)).astype(np.float32)
            x = np.ascontiguousarray(np.broadcast_to(mono, (a.streams, 2, CHUNK)))
            for _ in range(b.ring_frames // CHUNK + 2):
                b.push_audio(x)
        else:
            b.push_synth(seed, 0, b.ring_frames + 801)  # the counter ends off the hop grid
        b.sync()
        first = b.xfer(0, 1)
        p, k = int(first["window"][0]), int(first["segments"][0])
        span = (k - 1) * (p // 2) + p + 2 * (p // 4) + p // 2 - 1
        nbytes = a.streams * 2 * span * 4
        entry = B.XFER_DTYPE.itemsize
        res = dict(leg="dual mono" if dual else "independent noise", ring_frames=b.ring_frames, window=p, segments=k, span_frames=span,
                   span_MB=round(nbytes / 1e6, 1), xfer_MB=round(a.streams * entry / 1e6, 2))
        out = wf.PinnedBuffer((a.streams,), B.XFER_DTYPE)

        def read_pinned():
            assert L.wf_hip_read(b.h, B.OUT_XFER, 0, a.streams, C.c_void_p(out.ptr)) == 0

        got = b.xfer()
        read_pinned()
        assert out.array.tobytes() == got.tobytes()
        assert np.all(got["valid"] == 1) and np.all(got["window"] == p) and np.all(got["segments"] == k)
        res["lag_zero_streams"] = int(np.count_nonzero(got["lag"] == 0))
        res["transforms_per_stream"] = round(float(np.mean(np.where(got["lag"] == 0, k + 1, 2 * k + 1))), 2)
        res["mean_coherence"] = round(float(np.mean(got["mean_coherence"])), 4)
        assert (res["lag_zero_streams"] == a.streams) == dual
        res["xfer_read_pinned"] = rounds(b, read_pinned, a.warmup, a.reads, a.rounds)
        res["xfer_read"] = rounds(b, b.xfer, a.warmup, a.reads, a.rounds)
        out.close()
        res["delay_read"] = rounds(b, b.delay, a.warmup, a.reads, a.rounds)
        res["signal_read"] = rounds(b, b.signal, a.warmup, a.reads, a.rounds)
        res["span_copy_pinned"] = windows_copy((a.streams, 2, span), max(a.reads // 2, 3), a.rounds)
    copy = res["span_copy_pinned"]["host_us"][0]
    res["copy_over_read_pinned"] = round(copy / res["xfer_read_pinned"]["host_us"][0], 2)
    res["copy_over_read"] = round(copy / res["xfer_read"]["host_us"][0], 2)
    return res


def main():
    a = parser(2, 5, streams=4096, rings="0,65536").parse_args()
    res = dict(streams=a.streams, fft=4096, reads=a.reads, warmup=a.warmup, rounds=a.rounds,
               legs=[one_leg(a, int(r), dual) for r in a.rings.split(",") for dual in (False, True)])
    emit(a, res)


if __name__ == "__main__":
    main()
