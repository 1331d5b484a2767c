"""Cost of reading WF_HIP_OUT_TEMPO, stereo streams at 48 kHz and FFT 1024: 4096 streams with ring_frames = 131072 (T = 507 strength
columns, eight chunks of the columns kernel per stream) and 64 streams with ring_frames = 2^19 (T = 2043, 32 chunks: the batch a
kernel with one workgroup per stream would leave most of the chip idle on).  The rings hold independent noise (the columns kernel's
work does not depend on the audio; the rule's phase sums do, a little).
In one process, per shape: (a) wf_hip_read of the whole batch back to back into page-locked memory (wf_hip_host_alloc: what the copy
in (b) gets as well) and tempo() of the Python binding, which reads into a fresh numpy array, both by device events on the handle's
stream (wf_hip_time_begin / _end around the calls; the read's copy of 10592 bytes per stream to the host is inside the bracket) and
by the host clock; (b) the alternatives a host has: the span of both rings that the columns cover, (T + 1) H + P + H - 1 frames per
channel, copied to the host -- a device block (the library has no reader for the rings) by hipMemcpy into page-locked memory, in
parts of at most 512 MB whose times add up -- and T / 128 reads of WF_HIP_OUT_ONSET, the polling that covers the same columns (one
read is timed and scaled).  The transforms and the stitching the host would then run are not counted.  Every figure is the median
of `rounds` rounds of `reads` calls after `warmup` calls, with the smallest and largest round beside it.  One JSON line.  The
kernels' own times without the copy are not measured here.
usage: python tools/tempo_bench.py [--shapes 4096:131072,64:524288] [--warmup 2] [--reads 5] [--rounds 5] [--out FILE.json]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import waveform_amd as wf

from bench_common import emit, parser, rounds, windows_copy_in_parts



def one_shape(a, streams, ring_frames):
    cfg = wf.Config.defaults(fft_size=1024, sample_rate=48000, stereo=1, slope=1.0, bars=1, floor_db=-70)
    seed = 0x5741564546524D31
    L = wf.lib()
    B = wf.binding
    with wf.SpectrumBatch(cfg, streams, ring_frames=ring_frames) as b:
        for at in range(0, b.ring_frames + 801, 65536):  # the counter ends off the hop grid
            b.push_synth(seed, at, min(65536, b.ring_frames + 801 - at))
        b.sync()
        t = int(b.tempo(0, 1)["columns"][0])
        span = (t + 1) * B.TEMPO_HOP + B.TEMPO_WINDOW + B.TEMPO_HOP - 1
        per_stream = 2 * span * 4
        entry = B.TEMPO_DTYPE.itemsize
        res = dict(streams=streams, ring_frames=b.ring_frames, columns=t, chunks=(t + 63) // 64, span_frames=span,
                   span_MB=round(streams * per_stream / 1e6, 1), tempo_MB=round(streams * entry / 1e6, 2),
                   onset_reads=round(t / B.ONSET_COLUMNS, 2))
        out = wf.PinnedBuffer((streams,), B.TEMPO_DTYPE)

        def read_pinned():
            assert L.wf_hip_read(b.h, B.OUT_TEMPO, 0, streams, C.c_void_p(out.ptr)) == 0

        got = b.tempo()
        read_pinned()
        assert out.array.tobytes() == got.tobytes()
        assert np.all(got["strength"][:, :t] > 0) and not np.any(got["strength"][:, t:]) and np.all(got["columns"] == t)
        res["valid"] = int(got["valid"].sum())
        res["mean_strength"] = round(float(np.mean(got["strength"][:, :t])), 3)
        res["tempo_read_pinned"] = rounds(b, read_pinned, a.warmup, a.reads, a.rounds)
        res["tempo_read"] = rounds(b, b.tempo, a.warmup, a.reads, a.rounds)
        out.close()
        res["onset_read"] = rounds(b, b.onset, a.warmup, a.reads, a.rounds)
        res["span_copy_parts"], res["span_copy_pinned"] = windows_copy_in_parts(streams, span, max(a.reads // 2, 3), a.rounds)
    copy = res["span_copy_pinned"]["host_us"][0]
    polls = res["onset_read"]["host_us"][0] * t / B.ONSET_COLUMNS
    res["onset_polling_us"] = round(polls, 1)
    res["copy_over_read_pinned"] = round(copy / res["tempo_read_pinned"]["host_us"][0], 2)
    res["polling_over_read_pinned"] = round(polls / res["tempo_read_pinned"]["host_us"][0], 2)
    return res


def main():
    a = parser(2, 5, shapes="4096:131072,64:524288").parse_args()
    shapes = [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]
    res = dict(fft=1024, sample_rate=48000, reads=a.reads, warmup=a.warmup, rounds=a.rounds, shapes=[one_shape(a, s, r) for s, r in shapes])
    emit(a, res)


if __name__ == "__main__":
    main()
