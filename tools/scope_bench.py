"""Cost of reading WF_HIP_OUT_SCOPE at the headline shape, 4096 stereo streams at 48 kHz: at FFT 4096 (P = 4096) and at FFT 16384
(P = 8192, the cap).
In one process, per FFT size: (a) scope() back to back, by device events on the handle's stream (wf_hip_time_begin / _end around
the calls; the read's 16.9 MB copy to the host is inside the bracket) and by the host clock, with signal() -- the other reader of
the same windows, 0.2 MB back -- beside it; (b) the alternative a host has: the windows themselves copied to the host -- a device
block of their size (streams x 2 x P float32; the library has no reader for the rings) by hipMemcpy into page-locked memory.
The trigger search and the column minima the host would then run are not counted.  Every figure is the median of `rounds` rounds of
`reads` calls after `warmup` calls, with the smallest and largest round beside it.  The bytes are counted from the shapes: the
kernel reads the windows once and writes the entries.  One JSON line.  The kernel's own time comes from a
rocprofv3 --kernel-trace --stats run of this tool (a run of its own).
usage: python tools/scope_bench.py [--streams 4096] [--ffts 4096,16384] [--warmup 3] [--reads 10] [--rounds 5] [--out FILE.json]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import waveform_amd as wf

from bench_common import emit, parser, rounds, windows_copy


def one_fft(a, fft):
    cfg = wf.Config.defaults(fft_size=fft, sample_rate=48000, stereo=1, slope=1.0, bars=1, floor_db=-70)
    seed = 0x5741564546524D31
    with wf.SpectrumBatch(cfg, a.streams) as b:
        b.push_synth(seed, 0, b.ring_frames)
        b.push_synth(seed, b.ring_frames, 801)
        b.tick()
        b.sync()
        window = int(b.scope(0, 1)["window"][0])
        nbytes = a.streams * 2 * window * 4
        entry = wf.binding.SCOPE_DTYPE.itemsize
        res = dict(fft=fft, ring_frames=b.ring_frames, window=window, windows_MB=round(nbytes / 1e6, 1),
                   scope_MB=round(a.streams * entry / 1e6, 2),
                   scope_read=rounds(b, b.scope, a.warmup, a.reads, a.rounds),
                   signal_read=rounds(b, b.signal, a.warmup, a.reads, a.rounds))
        res["windows_copy_pinned"] = windows_copy((a.streams, 2, window), max(a.reads // 2, 3), a.rounds)
        got = b.scope()
        res["triggered_share"] = float(np.mean(got["triggered"]))
        res["mean_swing"] = float(np.mean(got["hi"][:, 0, :int(got["columns"][0])] - got["lo"][:, 0, :int(got["columns"][0])]))
    res["copy_over_read"] = round(res["windows_copy_pinned"]["host_us"][0] / res["scope_read"]["host_us"][0], 2)
    res["kernel_GB_moved"] = round((nbytes + a.streams * entry) / 1e9, 4)
    return res


def main():
    a = parser(3, 10, streams=4096, ffts="4096,16384").parse_args()
    res = dict(streams=a.streams, reads=a.reads, warmup=a.warmup, rounds=a.rounds, ffts=[one_fft(a, int(f)) for f in a.ffts.split(",")])
    emit(a, res)


if __name__ == "__main__":
    main()
