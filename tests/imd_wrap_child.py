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
from wrap_child import Walk, slices, twins  # noqa: E402

KINDS = (("twin", "wide"), ("octave", "single"), ("silence", "clean"))


def run():
    fft, ring, streams, sr = 2048, 8192, len(KINDS), 48000
    cfg = wf.Config.defaults(fft_size=fft, sample_rate=sr, stereo=1, slope=1.0, bars=1)
    # a spectrum batch's wpos starts at fft (the zeros of create): aged by 2^32 - 2 rings it is 0 at T = 2 rings - fft and fft,
    # the window starting at position 0, at T = R
    with twins(cfg, streams, ring, fft, R=2 * ring, win=fft) as (fresh, old, sch):
        rng = np.random.default_rng(ref.GPU_SEED)
        total = int(sum(sch.pushes))
        audio = np.stack([np.stack([ref.signal(k, rng, total, fft) for k in pair]) for pair in KINDS])  # one run of every signal
        walk = Walk((fresh, old), sch.pushes, 2 * ring - fft, fft, slices(audio), hist=np.zeros((streams, 2, fft), np.float32))
        for i, T, what in walk:
            x, y = fresh.imd(), old.imd()
            assert x.tobytes() == y.tobytes(), f"{what}: the twins differ"
            bad = ref.mismatches(y, ref.imd(walk.hist, fft, sr))
            assert not bad, (what, bad[:4])
        assert walk.before >= 2 and walk.straddling >= 3 and walk.exact == 1 and walk.behind >= 3, walk.counts
        assert np.all(y["window"] == fft) and y["ch"]["tones"].tolist() == [[2, 2], [2, 1], [0, 2]]
        assert y["ch"]["lo_bin"][0].tolist() == [809, 19] and y["ch"]["products"][0].tolist() == [0x14115, 0x30cf]


if __name__ == "__main__":
    run()
    print("wrapped ok")
