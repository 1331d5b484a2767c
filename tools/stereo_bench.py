"""Cost of reading WF_HIP_OUT_STEREO at the headline shape: 4096 stereo streams, 48 kHz, FFT 4096.
In one process: (a) stereo() back to back, by device events on the handle's stream (wf_hip_time_begin / _end around the calls;
the read's 2 MB copy to the host is inside the bracket) and by the host clock; signal() and pitch(), which read the same
windows, the same way; (b) the alternative a host has: the windows themselves copied to the host -- a device block of their
size (streams x 2 x P float32; the library has no reader for the rings) by hipMemcpy into page-locked and into pageable memory.
The transform the host would then run is not counted.  Every figure is the median of `rounds` rounds of `reads` calls after
`warmup` calls, with the smallest and largest round beside it.  One JSON line.  The kernel's own time comes from a
rocprofv3 --kernel-trace --stats run of this tool (a run of its own).
usage: python tools/stereo_bench.py [--streams 4096] [--fft 4096] [--warmup 5] [--reads 20] [--rounds 5] [--out FILE.json]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import waveform_amd as wf

from bench_common import emit, parser, rounds, windows_copy


def main():
    a = parser(5, 20, streams=4096, fft=4096).parse_args()
    cfg = wf.Config.defaults(fft_size=a.fft, sample_rate=48000, stereo=1, slope=1.0, bars=1, floor_db=-70)
    seed = 0x5741564546524D31
    with wf.SpectrumBatch(cfg, a.streams) as b:
        b.push_synth(seed, 0, a.fft + 801)
        b.tick()
        b.sync()
        p = int(b.stereo(0, 1)["window"][0])
        nbytes = a.streams * 2 * p * 4
        res = dict(streams=a.streams, fft=a.fft, window=p, windows_MB=round(nbytes / 1e6, 1), stereo_MB=round(a.streams * 504 / 1e6, 2),
                   reads=a.reads, warmup=a.warmup, rounds=a.rounds,
                   stereo_read=rounds(b, b.stereo, a.warmup, a.reads, a.rounds),
                   signal_read=rounds(b, b.signal, a.warmup, a.reads, a.rounds),
                   pitch_read=rounds(b, b.pitch, 2, max(a.reads // 4, 3), a.rounds))
        res["windows_copy_pinned"], res["windows_copy_pageable"] = windows_copy((a.streams, 2, p), max(a.reads // 4, 3), a.rounds, pageable=True)
        got = b.stereo()
        res["mean_coherence"] = float(np.mean(got["coherence"]))
        res["mean_correlation"] = float(np.mean(got["correlation"]))
    res["speedup_over_pinned_copy"] = round(res["windows_copy_pinned"]["host_us"][0] / res["stereo_read"]["host_us"][0], 1)
    emit(a, res)


if __name__ == "__main__":
    main()
