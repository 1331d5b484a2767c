"""TEST HARNESS (child of tests/test_gpu_gonio.py::test_across_the_2_to_the_32_wrap): runs against the DEVELOPMENT build of the
library (libwaveform_hip_dev.so via WF_HIP_LIB -- the release library does not export wf_hip_debug_age).

Twin handles in the manner of tests/wrap_child.py, whose schedule this uses: `old` has had its 32-bit write positions moved to just
below 2^32 (wf_hip_debug_age), `fresh` has not; both are fed the same audio, and from just before old's positions overflow
gonio() is read after every hop and must be the same bits on both -- with the window before 2^32, straddling it (0 < wpos < P),
starting at position 0 exactly (wpos = P) and behind it -- and equal to the restatement of the frames pushed.

usage: python tests/gonio_wrap_child.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import waveform_amd as wf  # noqa: E402
import gonio_ref as ref  # noqa: E402
from wrap_child import Walk, twins  # noqa: E402

KINDS = ("noise", "lissajous", "left")


def run():
    fft, ring, streams = 2048, 8192, len(KINDS)
    cfg = wf.Config.defaults(fft_size=fft, stereo=1, slope=1.0, bars=1)
    # a spectrum batch's wpos starts at fft (the zeros of create): aged by 2^32 - 2 rings it is 0 at T = 2 rings - fft and fft,
    # the window starting at position 0, at T = R
    with twins(cfg, streams, ring, fft, R=2 * ring, win=fft) as (fresh, old, sch):
        rng = np.random.default_rng(ref.GPU_SEED)
        walk = Walk((fresh, old), sch.pushes, 2 * ring - fft, fft, hist=np.zeros((streams, 2, fft), np.float32),
                    audio=lambda i, T, p: np.stack([ref.signal(k, rng, p) for k in KINDS]))
        for i, T, what in walk:
            x, y = fresh.gonio(), old.gonio()
            assert x.tobytes() == y.tobytes(), f"{what}: the twins differ"
            bad = ref.mismatches(y, walk.hist, fft)
            assert not bad, (what, bad[:4])
        assert walk.before >= 2 and walk.straddling >= 3 and walk.exact == 1 and walk.behind >= 3, walk.counts
        assert np.all(y["occupied"] > 8) and np.all(y["window"] == fft)


if __name__ == "__main__":
    run()
    print("wrapped ok")
