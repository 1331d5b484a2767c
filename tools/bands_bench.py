"""Cost of reading WF_HIP_OUT_BANDS at the headline shape: 4096 stereo streams, 48 kHz, FFT 4096, slope, bars.
In one process: (a) the bands read kernel back to back and behind a push and a tick, by device events on the handle's stream
(wf_hip_time_begin / _end around the calls; the read's 1.2 MB copy to the host is inside the bracket) and by the host clock;
(b) the yardsticks from code that already exists: peaks() over the same rows the same way, and decibels(), the 67.1 MB copy of
the rows to the host that the output replaces.  Every figure is the median of `rounds` rounds of `reads` calls after `warmup`
calls, with the smallest and largest round beside it.  One JSON line.  The kernels' own times come from a
rocprofv3 --kernel-trace --stats run of this tool (a run of its own).
usage: python tools/bands_bench.py [--streams 4096] [--fft 4096] [--warmup 10] [--reads 50] [--rounds 5] [--out FILE.json]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import waveform_amd as wf

from bench_common import emit, parser, rounds


def main():
    a = parser(10, 50, streams=4096, fft=4096).parse_args()
    cfg = wf.Config.defaults(fft_size=a.fft, sample_rate=48000, stereo=1, slope=1.0, bars=1, floor_db=-70)
    seed = 0x5741564546524D31
    with wf.SpectrumBatch(cfg, a.streams, ring_frames=a.fft + 800) as b:
        b.push_synth(seed, 0, a.fft + 800)
        b.tick()
        b.sync()
        rows = a.streams * b.output_channels
        pos = [a.fft + 800]

        def hop(read):
            def fn():
                b.push_synth(seed, pos[0], 800)
                pos[0] += 800
                b.tick()
                if read is not None:
                    read()
            return fn
        res = dict(streams=a.streams, fft=a.fft, rows=rows, row_MB=round(rows * (a.fft // 2) * 4 / 1e6, 1),
                   bands_MB=round(rows * 144 / 1e6, 2), peaks_MB=round(rows * 72 / 1e6, 2), reads=a.reads, warmup=a.warmup, rounds=a.rounds,
                   bands_read=rounds(b, b.bands, a.warmup, a.reads, a.rounds),
                   peaks_read=rounds(b, b.peaks, a.warmup, a.reads, a.rounds),
                   push_tick=rounds(b, hop(None), a.warmup, a.reads, a.rounds),
                   push_tick_bands_read=rounds(b, hop(b.bands), a.warmup, a.reads, a.rounds),
                   push_tick_peaks_read=rounds(b, hop(b.peaks), a.warmup, a.reads, a.rounds),
                   decibels_read=rounds(b, b.decibels, 2, max(a.reads // 5, 5), a.rounds))
        got = b.bands()
        res["mean_total_db"] = float(np.mean(got["total_db"]))
        res["mean_a_minus_total_db"] = float(np.mean(got["a_db"] - got["total_db"]))
    res["speedup_over_row_copy"] = round(res["decibels_read"]["host_us"][0] / res["bands_read"]["host_us"][0], 1)
    emit(a, res)


if __name__ == "__main__":
    main()
