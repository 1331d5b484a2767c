"""Cost of reading WF_HIP_OUT_CQ at the headline shape: 4096 stereo streams, 48 kHz, FFT 4096, at the default ring (8192 frames,
so Lmax = 8192) and at ring_frames = 16384 (the cap).
In one process, per ring size: (a) cq() back to back, by device events on the handle's stream (wf_hip_time_begin / _end around
the calls; the read's 4 MB copy to the host is inside the bracket) and by the host clock; (b) the alternative a host has: the
windows themselves copied to the host -- a device block of their size (streams x 2 x Lmax float32; the library has no reader
for the rings) by hipMemcpy into page-locked memory.  The sums the host would then run are not counted.  Every figure is the
median of `rounds` rounds of `reads` calls after `warmup` calls, with the smallest and largest round beside it.  The work is
counted from the shapes: sample pairs = streams x sum of L_b over the covered bins, 15 float64 operations per pair and captured
channel pair (two complex rotations, the window, the product and four multiply-adds).  One JSON line.  The kernel's own time
comes from a rocprofv3 --kernel-trace --stats run of this tool (a run of its own).
usage: python tools/cq_bench.py [--streams 4096] [--fft 4096] [--warmup 3] [--reads 10] [--rounds 5] [--rings 0,16384] [--out FILE.json]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import waveform_amd as wf

from bench_common import emit, parser, rounds, windows_copy

OPS_PER_PAIR = 15
Q = 1.0 / (2.0 ** (1.0 / 12.0) - 1.0)


def pairs_per_stream(sr, lmax):
    """sum of L_b over the covered bins"""
    f = 440.0 * 2.0 ** ((np.arange(wf.binding.CQ_BINS) - 57.0) / 12.0)
    covered = f * 2.0 ** (1.0 / 24.0) < sr / 2.0
    return int(np.minimum(np.ceil(Q * sr / f), lmax)[covered].sum())


def one_ring(a, ring):
    cfg = wf.Config.defaults(fft_size=a.fft, sample_rate=48000, stereo=1, slope=1.0, bars=1, floor_db=-70)
    seed = 0x5741564546524D31
    with wf.SpectrumBatch(cfg, a.streams, ring_frames=ring) as b:
        b.push_synth(seed, 0, b.ring_frames)
        b.push_synth(seed, b.ring_frames, 801)
        b.tick()
        b.sync()
        lmax = int(b.cq(0, 1)["max_window"][0])
        nbytes = a.streams * 2 * lmax * 4
        pairs = pairs_per_stream(48000, lmax)
        res = dict(ring_frames=b.ring_frames, max_window=lmax, windows_MB=round(nbytes / 1e6, 1),
                   cq_MB=round(a.streams * wf.binding.CQ_DTYPE.itemsize / 1e6, 2), sample_pairs_per_stream=pairs,
                   float64_Gops=round(a.streams * pairs * OPS_PER_PAIR / 1e9, 2),
                   cq_read=rounds(b, b.cq, a.warmup, a.reads, a.rounds),
                   signal_read=rounds(b, b.signal, a.warmup, a.reads, a.rounds))
        res["windows_copy_pinned"] = windows_copy((a.streams, 2, lmax), max(a.reads // 2, 3), a.rounds)
        got = b.cq()
        res["mean_db"] = float(np.mean(got["db"][np.isfinite(got["db"])]))
        res["first_resolved"] = int(got["first_resolved"][0])
    res["copy_over_read"] = round(res["windows_copy_pinned"]["host_us"][0] / res["cq_read"]["host_us"][0], 2)
    res["float64_Tops_per_s_of_the_read"] = round(res["float64_Gops"] / res["cq_read"]["device_us_incl_copy"][0] * 1e3, 2)
    return res


def main():
    a = parser(3, 10, streams=4096, fft=4096, rings="0,16384").parse_args()
    res = dict(streams=a.streams, fft=a.fft, reads=a.reads, warmup=a.warmup, rounds=a.rounds, ops_per_pair=OPS_PER_PAIR,
               rings=[one_ring(a, int(r)) for r in a.rings.split(",")])
    emit(a, res)


if __name__ == "__main__":
    main()
