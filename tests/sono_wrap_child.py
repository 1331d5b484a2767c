"""TEST HARNESS (child of tests/test_gpu_sono.py::test_across_the_2_to_the_32_wrap): runs against the DEVELOPMENT build of the
library (libwaveform_hip_dev.so via WF_HIP_LIB -- the release library does not export wf_hip_debug_age).

Twin handles in the manner of tests/wrap_child.py, whose schedule this uses: `old` has had its 32-bit write positions moved to just
below 2^32 (wf_hip_debug_age), `fresh` has not; both are fed the same audio, and from just before old's positions overflow
sono() is read after every hop: the cells must be the same bytes on both -- with the span read before 2^32, straddling it
(0 < wpos < span), and behind it --, old's `newest` must be fresh's plus age / H modulo 2^32 / H, and fresh must equal the
restatement of the frames pushed.

usage: python tests/sono_wrap_child.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import waveform_amd as wf  # noqa: E402
import sono_ref as ref  # noqa: E402
from wrap_child import Walk, slices, twins  # noqa: E402


def run():
    fft, ring, streams = 1024, 8192, len(ref.KINDS)
    t = ref.columns(ring)
    span = (t - 1) * ref.H + ref.P + ref.H - 1  # the most frames a read looks back over
    cfg = wf.Config.defaults(fft_size=fft, stereo=1, slope=1.0, bars=1)
    # a spectrum batch's wpos starts at fft (the zeros of create): aged by 2^32 - 2 rings it is 0 at T = 2 rings - fft
    wrap, age = 2 * ring - fft, (1 << 32) - 2 * ring
    with twins(cfg, streams, ring, fft, R=wrap + ring, win=ring) as (fresh, old, sch):
        assert t == 28 and span == ring - 1
        rng = np.random.default_rng(ref.GPU_SEED)
        total = int(sum(sch.pushes))
        audio = np.stack([ref.signal(k, rng, total, 2, span) for k in ref.KINDS])
        walk = Walk((fresh, old), sch.pushes, wrap, span, slices(audio))
        for i, T, what in walk:
            x, y = fresh.sono(), old.sono()
            assert x["db"].tobytes() == y["db"].tobytes(), f"{what}: the twins' cells differ"
            assert np.all(x["newest"] == (fft + T) // ref.H), what
            assert np.all(y["newest"] == (x["newest"] + age // ref.H) % ((1 << 32) // ref.H)), (what, x["newest"], y["newest"])
            for name in ref.FIELDS[1:]:
                if name != "newest":
                    assert np.array_equal(x[name], y[name]), (what, name)
            hist = np.concatenate([np.zeros((streams, 2, fft), np.float32), audio[:, :, :T]], axis=2)
            bad, arm2 = ref.mismatches(x, hist, fft + T, 48000, ring)
            assert not bad, (what, bad[:4])
        before, straddling, behind = walk.before, walk.straddling, walk.exact + walk.behind  # (the exact hit counts as behind here)
        assert before >= 2 and straddling >= 3 and behind >= 3, (before, straddling, behind)
        assert np.all(np.isfinite(y["db"][0, :, :t]))
        print(f"{before} reads before the wrap, {straddling} with the span across it, {behind} behind it")


if __name__ == "__main__":
    run()
    print("wrapped ok")
