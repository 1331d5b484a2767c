"""Cost of reading WF_HIP_OUT_CLICK at the headline shape, 4096 stereo streams at 48 kHz: at FFT 4096 (P = 4096) and at FFT 16384
(P = 8192, the cap), for three kinds of audio: independent noise (no events: the selections run, the event passes skip every word
of the bitmap), a 1 kHz sine with a 0.01 click in every stream (the ill-conditioned predictor, one event) and silence (the early
leave behind the autocorrelation: valid = 0).
In one process, per FFT size: (a) per kind, wf_hip_read back to back into page-locked memory (wf_hip_host_alloc: what the copy
in (b) gets as well) and click() of the Python binding, which reads into a fresh numpy array, both by device events on the
handle's stream (wf_hip_time_begin / _end around the calls; the read's 1.9 MB copy to the host is inside the bracket) and by the
host clock, with signal() -- another reader of the same windows -- beside it; (b) the alternative a host has: the windows
themselves copied to the host -- a device block of their size (streams x 2 x P float32; the library has no reader for the rings)
by hipMemcpy into page-locked memory.  The detection the host would then run is not counted.  Every figure is the median of
`rounds` rounds of `reads` calls after `warmup` calls, with the smallest and largest round beside it.  One JSON line.  The
kernel's own time without its copy is not measured here.
usage: python tools/click_bench.py [--streams 4096] [--ffts 4096,16384] [--warmup 3] [--reads 10] [--rounds 5] [--out FILE.json]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import waveform_amd as wf

from bench_common import emit, parser, rounds, windows_copy

KINDS = ("noise", "sine_click", "silence")
CHUNK = 256  # streams per host push of the sine


def _fill(b, kind, window, seed):
    """the newest `window` + 801 frames of every stream become `kind`: the window ends at an odd position"""
    frames = window + 801
    if kind == "noise":
        b.push_synth(seed, 0, frames)
    elif kind == "silence":
        b.push_silence(frames)
    else:
        n = np.arange(frames, dtype=np.float64)
        for first in range(0, b.streams, CHUNK):
            k = min(CHUNK, b.streams - first)
            phase = (first + np.arange(k))[:, None, None] * 0.37 + np.array([0.0, 0.9])[None, :, None]
            a = (0.5 * np.sin(2.0 * np.pi * 1000.0 / 48000.0 * n[None, None, :] + phase)).astype(np.float32)
            a[:, :, frames - window + window // 3] += np.float32(0.01)
            b.push_audio(a, first=first)
    b.sync()


def one_fft(a, fft):
    cfg = wf.Config.defaults(fft_size=fft, sample_rate=48000, stereo=1, slope=1.0, bars=1, floor_db=-70)
    seed = 0x5741564546524D31
    L = wf.lib()
    with wf.SpectrumBatch(cfg, a.streams) as b:
        window = int(b.click(0, 1)["window"][0])
        nbytes = a.streams * 2 * window * 4
        entry = wf.binding.CLICK_DTYPE.itemsize
        res = dict(fft=fft, ring_frames=b.ring_frames, window=window, windows_MB=round(nbytes / 1e6, 1),
                   click_MB=round(a.streams * entry / 1e6, 2), kinds={})
        out = wf.PinnedBuffer((a.streams,), wf.binding.CLICK_DTYPE)

        def read_pinned():
            assert L.wf_hip_read(b.h, wf.binding.OUT_CLICK, 0, a.streams, C.c_void_p(out.ptr)) == 0

        for kind in KINDS:
            _fill(b, kind, window, seed)
            got = b.click()
            read_pinned()
            assert out.array.tobytes() == got.tobytes()
            ch = got["ch"]
            res["kinds"][kind] = dict(click_read_pinned=rounds(b, read_pinned, a.warmup, a.reads, a.rounds),
                                      click_read=rounds(b, b.click, a.warmup, a.reads, a.rounds),
                                      valid=int(ch["valid"].sum()), mean_events=round(float(np.mean(ch["events"])), 3),
                                      max_peak_db=round(float(np.max(ch["peak_db"])), 1))
        out.close()
        res["signal_read"] = rounds(b, b.signal, a.warmup, a.reads, a.rounds)
        res["windows_copy_pinned"] = windows_copy((a.streams, 2, window), max(a.reads // 2, 3), a.rounds)
    copy = res["windows_copy_pinned"]["host_us"][0]
    for kind in KINDS:
        res["kinds"][kind]["copy_over_read_pinned"] = round(copy / res["kinds"][kind]["click_read_pinned"]["host_us"][0], 2)
        res["kinds"][kind]["copy_over_read"] = round(copy / res["kinds"][kind]["click_read"]["host_us"][0], 2)
    res["kernel_GB_moved"] = round((nbytes + a.streams * entry) / 1e9, 4)
    return res


def main():
    a = parser(3, 10, streams=4096, ffts="4096,16384").parse_args()
    res = dict(streams=a.streams, reads=a.reads, warmup=a.warmup, rounds=a.rounds, ffts=[one_fft(a, int(f)) for f in a.ffts.split(",")])
    emit(a, res)


if __name__ == "__main__":
    main()
