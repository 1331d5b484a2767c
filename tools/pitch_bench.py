"""Cost of reading WF_HIP_OUT_PITCH at the headline shape: 4096 stereo streams, 48 kHz, FFT 4096, after one push and one tick.
Times `reads` calls of pitch() (the YIN kernel over each stream's newest 4096 frames, then 64 KB device -> host) and sets them
against two yardsticks measured in the same process by tools/micro/pitch_yardstick.hip: independent float64 FMAs issued from
registers at the kernel's occupancy (the rate this part sustains, as measured), and one hipMemcpy of the windows themselves to
the host (P x channels x 4 x streams bytes: what a host that estimates the pitch on the CPU has to copy first).  The kernel
computes r(tau) and e(tau) as direct sums, so it issues 2 H^2 + H FMAs per stream; both that and the H^2 of r(tau) alone are
reported as rates.  Host clock around calls that end in a synchronise; one JSON line.  The kernel's own time comes from a
rocprofv3 --kernel-trace --stats run of this tool.
--mode hop: every read follows a push of one 800-frame hop and a tick instead (what a monitor does once per video frame); the
host time is then of the whole hop.
usage: python tools/pitch_bench.py [--mode repeat|hop] [--streams 4096] [--fft 4096] [--warmup 3] [--reads 20] [--no-yardstick] [--out FILE.json]"""
import argparse
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import waveform_amd as wf

from bench_common import emit, timed


def yardstick():
    """the helper library, built on first use"""
    src = os.path.join(ROOT, "tools", "micro", "pitch_yardstick.hip")
    lib = os.path.join(ROOT, "tools", "micro", "libpitch_yardstick.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-shared", "-fPIC", src, "-o", lib], check=True)
    L = C.CDLL(lib)
    L.yard_fma_per_thread.restype = C.c_double
    L.yard_fma_per_thread.argtypes = [C.c_int]
    L.yard_fma_ms.restype = C.c_double
    L.yard_fma_ms.argtypes = [C.c_int, C.c_int, C.c_int]
    L.yard_d2h_ms.restype = C.c_double
    L.yard_d2h_ms.argtypes = [C.c_size_t, C.c_int, C.c_int]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--fft", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reads", type=int, default=20)
    ap.add_argument("--mode", choices=("repeat", "hop"), default="repeat")
    ap.add_argument("--no-yardstick", action="store_true")
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
            b.pitch()
        t_pitch = timed(b.pitch if a.mode == "repeat" else one_hop, a.warmup, a.reads)
        t_signal = timed(b.signal, 3, 20)
        got = b.pitch()
        ring_frames = b.ring_frames
    P = min(a.fft, wf.binding.PITCH_MAX_WINDOW)
    H = P // 2
    window_bytes = a.streams * 2 * P * 4
    fma_r, fma_issued = H * H * a.streams, (2 * H * H + H) * a.streams
    res = dict(mode=a.mode, streams=a.streams, fft=a.fft, window_frames=P, ring_frames=ring_frames, window_MB=round(window_bytes / 1e6, 1),
               pitch_KB=round(a.streams * 16 / 1e3, 1), fma_r_G=round(fma_r / 1e9, 2), fma_issued_G=round(fma_issued / 1e9, 2),
               **{"ms_per_pitch_read" if a.mode == "repeat" else "ms_per_hop_push_tick_pitch": round(t_pitch * 1e3, 4)},
               ms_per_signal_read=round(t_signal * 1e3, 4), voiced=int(got["voiced"].sum()), mean_clarity=float(np.mean(got["clarity"])),
               reads=a.reads, warmup=a.warmup)
    if a.mode == "repeat":  # (host clock: the kernel and a 64 KB copy; the kernel alone is in the rocprofv3 run)
        res["host_TFMA_per_s_r"] = round(fma_r / t_pitch / 1e12, 3)
        res["host_TFMA_per_s_issued"] = round(fma_issued / t_pitch / 1e12, 3)
    if not a.no_yardstick:
        Y = yardstick()
        blocks = 1024  # 256 CUs x 4 workgroups of 256 threads: four waves per SIMD, as the pitch kernel runs
        iters = max(int(round(fma_issued / (blocks * 256 * Y.yard_fma_per_thread(1)))), 1)
        ms = Y.yard_fma_ms(blocks, iters, 5)
        n = blocks * 256 * Y.yard_fma_per_thread(iters)
        res["yardstick"] = dict(fma_G=round(n / 1e9, 2), fma_ms=round(ms, 4), TFMA_per_s=round(n / ms / 1e9, 3) if ms > 0 else None,
                                d2h_pageable_ms=round(Y.yard_d2h_ms(window_bytes, 0, 3), 3), d2h_pinned_ms=round(Y.yard_d2h_ms(window_bytes, 1, 3), 3))
    emit(a, res)


if __name__ == "__main__":
    main()
