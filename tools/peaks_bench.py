"""Cost of reading WF_HIP_OUT_PEAKS at the headline shape: 4096 stereo streams, 48 kHz, FFT 4096, slope, bars, after one tick.
Times `reads` calls of peaks() (the read kernel over 8192 rows of 2048 bins, then 0.6 MB device -> host) against the same
number of decibels() reads (67.1 MB device -> host, what a host that scans the rows itself must copy).  Host clock around calls
that end in a synchronise; one JSON line.  The read kernel's own time comes from a rocprofv3 --kernel-trace run of this tool.
usage: python tools/peaks_bench.py [--streams 4096] [--fft 4096] [--warmup 20] [--reads 200] [--out FILE.json]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import waveform_amd as wf

from bench_common import emit, parser, timed


def main():
    a = parser(20, 200, rounds=None, streams=4096, fft=4096).parse_args()
    cfg = wf.Config.defaults(fft_size=a.fft, sample_rate=48000, stereo=1, slope=1.0, bars=1, floor_db=-70)
    with wf.SpectrumBatch(cfg, a.streams, ring_frames=a.fft + 800) as b:
        b.push_synth(0x5741564546524D31, 0, a.fft + 800)
        b.tick()
        b.sync()
        rows = a.streams * b.output_channels
        t_peaks = timed(b.peaks, a.warmup, a.reads)
        t_rows = timed(b.decibels, max(a.warmup // 4, 2), max(a.reads // 4, 10))
        counts = b.peaks()["count"]
    row_bytes = rows * (a.fft // 2) * 4
    res = dict(streams=a.streams, fft=a.fft, rows=rows, row_MB=round(row_bytes / 1e6, 1), peaks_MB=round(rows * 72 / 1e6, 2),
               ms_per_peaks_read=round(t_peaks * 1e3, 4), ms_per_decibels_read=round(t_rows * 1e3, 4),
               speedup=round(t_rows / t_peaks, 2), mean_count=float(np.mean(counts)), reads=a.reads, warmup=a.warmup)
    emit(a, res)


if __name__ == "__main__":
    main()
