"""Cost of reading WF_HIP_OUT_SIGNAL at the headline shape: 4096 stereo streams, 48 kHz, FFT 4096, after one push and one tick.
Times `reads` calls of signal() (the read kernel over each stream's newest 4096 frames of both channels, 134.2 MB, then
0.2 MB device -> host) against the same number of decibels() reads (the rows a host would otherwise copy to learn anything
about the streams; the audio itself has no output).  Host clock around calls that end in a synchronise; one JSON line.  The
read kernel's own time comes from a rocprofv3 --kernel-trace run of this tool.
--mode hop: every read follows a push of one 800-frame hop and a tick instead (what a monitor does once per video frame),
so the window has just been written; the host time is then of the whole hop.
usage: python tools/signal_bench.py [--mode repeat|hop] [--streams 4096] [--fft 4096] [--warmup 20] [--reads 200] [--out FILE.json]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import waveform_amd as wf

from bench_common import emit, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--fft", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reads", type=int, default=200)
    ap.add_argument("--mode", choices=("repeat", "hop"), default="repeat")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = wf.Config.defaults(fft_size=a.fft, sample_rate=48000, stereo=1, slope=1.0, bars=1, floor_db=-70)
    with wf.SpectrumBatch(cfg, a.streams, ring_frames=a.fft + 800) as b:
        b.push_synth(0x5741564546524D31, 0, a.fft + 800)
        b.tick()
        b.sync()
        hop = [a.fft + 800]

        def one_hop():
            b.push_synth(0x5741564546524D31, hop[0], 800)
            hop[0] += 800
            b.tick()
            b.signal()
        t_signal = timed(b.signal if a.mode == "repeat" else one_hop, a.warmup, a.reads)
        t_rows = timed(b.decibels, max(a.warmup // 4, 2), max(a.reads // 4, 10))
        sig = b.signal()
        ring_frames = b.ring_frames
    window_bytes = a.streams * 2 * a.fft * 4
    res = dict(mode=a.mode, streams=a.streams, fft=a.fft, ring_frames=ring_frames, window_MB=round(window_bytes / 1e6, 1),
               ring_MB=round(a.streams * 2 * ring_frames * 4 / 1e6, 1), signal_MB=round(a.streams * 48 / 1e6, 2),
               **{"ms_per_signal_read" if a.mode == "repeat" else "ms_per_hop_push_tick_signal": round(t_signal * 1e3, 4)}, ms_per_decibels_read=round(t_rows * 1e3, 4),
               mean_rms_db=float(np.mean(sig["ch"]["rms_db"])), mean_abs_correlation=float(np.mean(np.abs(sig["correlation"]))),
               reads=a.reads, warmup=a.warmup)
    emit(a, res)


if __name__ == "__main__":
    main()
