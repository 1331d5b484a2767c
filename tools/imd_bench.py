"""Cost of reading WF_HIP_OUT_IMD at the headline shape, 4096 stereo streams at 48 kHz: at FFT 4096 (P = 4096, 64 KB of LDS per
workgroup) and at FFT 16384 (P = 8192, the cap: 128 KB, one workgroup to a CU), over independent noise (the kernel's work does not
depend on the audio: the transform, two searches, 28 regions and one strided pass over the bins whatever they hold).
In one process, per FFT size: (a) wf_hip_read back to back into page-locked memory (wf_hip_host_alloc: what the copy in (b) gets
as well) and imd() of the Python binding, which reads into a fresh numpy array, both by device events on the handle's stream
(wf_hip_time_begin / _end around the calls; the read's 1.5 MB copy to the host is inside the bracket) and by the host clock, with
the same two reads of WF_HIP_OUT_THD -- the reader whose spectrum and tables this one shares -- beside it; (b) the alternative a host
has: the windows themselves copied to the host -- a device block of their size (streams x 2 x P float32; the library has no reader
for the rings) by hipMemcpy into page-locked memory.  The transforms the host would then run are not counted.  Every figure is the
median of `rounds` rounds of `reads` calls after `warmup` calls, with the smallest and largest round beside it.  One JSON line.
The kernel's own time without its copy is not measured here.
usage: python tools/imd_bench.py [--streams 4096] [--ffts 4096,16384] [--warmup 3] [--reads 10] [--rounds 5] [--out FILE.json]"""
import ctypes as C
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
    L = wf.lib()
    with wf.SpectrumBatch(cfg, a.streams) as b:
        window = int(b.imd(0, 1)["window"][0])
        b.push_synth(seed, 0, window + 801)  # the window ends at an odd position
        b.sync()
        nbytes = a.streams * 2 * window * 4
        entry = wf.binding.IMD_DTYPE.itemsize
        res = dict(fft=fft, ring_frames=b.ring_frames, window=window, lds_KB=window * 16 // 1024, windows_MB=round(nbytes / 1e6, 1),
                   imd_MB=round(a.streams * entry / 1e6, 2), thd_MB=round(a.streams * wf.binding.THD_DTYPE.itemsize / 1e6, 2))
        out = wf.PinnedBuffer((a.streams,), wf.binding.IMD_DTYPE)
        out_thd = wf.PinnedBuffer((a.streams,), wf.binding.THD_DTYPE)

        def read_pinned():
            assert L.wf_hip_read(b.h, wf.binding.OUT_IMD, 0, a.streams, C.c_void_p(out.ptr)) == 0

        def read_thd_pinned():
            assert L.wf_hip_read(b.h, wf.binding.OUT_THD, 0, a.streams, C.c_void_p(out_thd.ptr)) == 0

        got = b.imd()
        read_pinned()
        assert out.array.tobytes() == got.tobytes() and np.all(got["window"] == window) and np.all(got["ch"]["tones"] >= 1)
        res["imd_read_pinned"] = rounds(b, read_pinned, a.warmup, a.reads, a.rounds)
        res["imd_read"] = rounds(b, b.imd, a.warmup, a.reads, a.rounds)
        res["thd_read_pinned"] = rounds(b, read_thd_pinned, a.warmup, a.reads, a.rounds)
        res["thd_read"] = rounds(b, b.thd, a.warmup, a.reads, a.rounds)
        res["two_tones_found"] = int(np.count_nonzero(got["ch"]["tones"] == 2))
        out.close()
        out_thd.close()
        res["windows_copy_pinned"] = windows_copy((a.streams, 2, window), max(a.reads // 2, 3), a.rounds)
    copy = res["windows_copy_pinned"]["host_us"][0]
    res["copy_over_read_pinned"] = round(copy / res["imd_read_pinned"]["host_us"][0], 2)
    res["copy_over_read"] = round(copy / res["imd_read"]["host_us"][0], 2)
    res["imd_over_thd_pinned"] = round(res["imd_read_pinned"]["host_us"][0] / res["thd_read_pinned"]["host_us"][0], 2)
    res["kernel_GB_moved"] = round((nbytes + a.streams * entry) / 1e9, 4)
    return res


def main():
    a = parser(3, 10, streams=4096, ffts="4096,16384").parse_args()
    res = dict(streams=a.streams, reads=a.reads, warmup=a.warmup, rounds=a.rounds, ffts=[one_fft(a, int(f)) for f in a.ffts.split(",")])
    emit(a, res)


if __name__ == "__main__":
    main()
