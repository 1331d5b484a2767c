"""TEST HARNESS (child of tests/test_gpu_hum.py::test_across_the_2_to_the_32_wrap): runs against the DEVELOPMENT build of the
library (libwaveform_hip_dev.so via WF_HIP_LIB -- the release library does not export wf_hip_debug_age).

Twin handles in the manner of tests/tempo_wrap_child.py: `old` has had its 32-bit write positions moved to just below 2^32
(wf_hip_debug_age), `fresh` has not; both are fed the same audio -- hum_ref.wrap_audio in the packets of hum_ref.WRAP_PUSHES --
and hum() is read with the window before 2^32, ending at it, straddling it (0 < wpos < N) and behind it.  The entry holds nothing on
the counter, so the twins must read the same bytes, and fresh must equal the restatement of the frames pushed.

usage: python tests/hum_wrap_child.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import waveform_amd as wf  # noqa: E402
import hum_ref as ref  # noqa: E402
from wrap_child import Walk, slices, twins  # noqa: E402


def run():
    sr, ring, fft, streams = ref.SR, ref.RING, 1024, 3
    n = ref.plan(sr, ring).N
    cfg = wf.Config.defaults(fft_size=fft, sample_rate=sr, stereo=1, slope=1.0, bars=1)
    audio = ref.wrap_audio()
    # a spectrum batch's wpos starts at fft (the zeros of create): aged by 2^32 - 2 rings it is 0 at T = 2 rings - fft
    wrap = 2 * ring - fft
    with twins(cfg, streams, ring, fft) as (fresh, old, _):
        assert n == ring
        walk = Walk((fresh, old), ref.WRAP_PUSHES, wrap, n, slices(audio))
        for i, T, what in walk:
            x, y = fresh.hum(), old.hum()
            assert x.tobytes() == y.tobytes(), f"{what}: the twins differ"
            assert x["ch"]["family"].tolist() == [[50, 60], [60, 0], [0, 50]], (what, x["ch"]["family"].tolist())
            hist = np.concatenate([np.zeros((streams, 2, n), np.float32), audio[:, :, :T]], axis=2)
            bad = ref.mismatches(x, hist, sr, ring)
            assert not bad, (what, bad[:4])
        # (here `exact` is the read at the wrap itself, and a read that starts at position 0 counts as behind)
        before, exact, straddling, behind = walk.before - walk.at, walk.at, walk.straddling, walk.exact + walk.behind
        assert walk.T == audio.shape[-1] and before == 2 and exact == 1 and straddling >= 4 and behind >= 2, (before, exact, straddling, behind)
        print(f"{before} reads before the wrap, one at it, {straddling} with the window across it, {behind} behind it")


if __name__ == "__main__":
    run()
    print("wrapped ok")
