"""TEST HARNESS (child of tests/test_gpu_imd.py::test_across_the_2_to_the_32_wrap): runs against the DEVELOPMENT build of the
library (libwaveform_hip_dev.so via WF_HIP_LIB -- the release library does not export wf_hip_debug_age).

Twin handles in the manner of tests/bits_wrap_child.py, whose schedule this uses: `old` has had its 32-bit write positions moved to
just below 2^32 (wf_hip_debug_age), `fresh` has not; both are fed the same audio, and from just before old's positions overflow
imd() is read after every hop and must be the same bits on both -- with the window before 2^32, straddling it (0 < wpos < P),
starting at position 0 exactly (wpos = P) and behind it -- and within the bound of the restatement of the frames pushed.

usage: python tests/imd_wrap_child.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import waveform_amd as wf  # noqa: E402
import imd_ref as ref  # noqa: E402
from wrap_child import HOPS, Schedule, _dev  # noqa: E402

KINDS = (("twin", "wide"), ("octave", "single"), ("silence", "clean"))


def run():
    L = _dev()
    fft, ring, streams, sr = 2048, 8192, len(KINDS), 48000
    cfg = wf.Config.defaults(fft_size=fft, sample_rate=sr, stereo=1, slope=1.0, bars=1)
    with wf.SpectrumBatch(cfg, streams, ring_frames=ring) as fresh, wf.SpectrumBatch(cfg, streams, ring_frames=ring) as old:
        assert old.ring_frames == ring and old.fft_size == fft
        # a spectrum batch's wpos starts at fft (the zeros of create): aged by 2^32 - 2 rings it is 0 at T = 2 rings - fft and fft,
        # the window starting at position 0, at T = R
        R = 2 * ring
        sch = Schedule(R, fft, 0, big=ring // 2, fine=True)
        sch.check([0])
        wrap = R - fft
        assert L.wf_hip_debug_age(old.h, 0, streams, (1 << 32) - 2 * ring) == 0, L.wf_hip_last_error(old.h)
        rng = np.random.default_rng(ref.GPU_SEED)
        total = int(sum(sch.pushes))
        audio = np.stack([np.stack([ref.signal(k, rng, total, fft) for k in pair]) for pair in KINDS])  # one run of every signal
        hist = np.zeros((streams, 2, fft), np.float32)
        T, before, straddling, exact, behind = 0, 0, 0, 0, 0
        for i, p in enumerate(sch.pushes):
            a = np.ascontiguousarray(audio[:, :, T:T + p])
            T += p
            for b in (fresh, old):
                b.push_audio(a)
            hist = np.concatenate([hist, a], axis=2)[:, :, -fft:]
            if T < wrap - sum(HOPS):
                continue
            what = f"read {i} at wpos = 2^32{T - wrap:+d}"
            x, y = fresh.imd(), old.imd()
            assert x.tobytes() == y.tobytes(), f"{what}: the twins differ"
            bad = ref.mismatches(y, ref.imd(hist, fft, sr))
            assert not bad, (what, bad[:4])
            before += int(T <= wrap)
            straddling += int(0 < T - wrap < fft)
            exact += int(T == R)
            behind += int(T > R)
        assert before >= 2 and straddling >= 3 and exact == 1 and behind >= 3, (before, straddling, exact, behind)
        assert np.all(y["window"] == fft) and y["ch"]["tones"].tolist() == [[2, 2], [2, 1], [0, 2]]
        assert y["ch"]["lo_bin"][0].tolist() == [809, 19] and y["ch"]["products"][0].tolist() == [0x14115, 0x30cf]


if __name__ == "__main__":
    run()
    print("wrapped ok")
