"""TEST HARNESS (child of tests/test_gpu_onset.py::test_across_the_2_to_the_32_wrap): runs against the DEVELOPMENT build of the
library (libwaveform_hip_dev.so via WF_HIP_LIB -- the release library does not export wf_hip_debug_age).

Twin handles in the manner of tests/sono_wrap_child.py, whose schedule this uses: `old` has had its 32-bit write positions moved to
just below 2^32 (wf_hip_debug_age), `fresh` has not; both are fed the same audio, and from just before old's positions overflow
onset() is read after every hop: strengths and flags must be the same bytes on both -- with the span read before 2^32, straddling it
(0 < wpos < span), and behind it --, old's `newest` and `last_frame` must be fresh's plus the age modulo 2^32, and fresh must equal
the restatement of the frames pushed.

usage: python tests/onset_wrap_child.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import waveform_amd as wf  # noqa: E402
import onset_ref as ref  # noqa: E402
from wrap_child import Walk, slices, twins  # noqa: E402


def run():
    fft, ring, streams = 1024, 8192, len(ref.KINDS)
    t = ref.columns(ring)
    span = t * ref.H + ref.P + ref.H - 1  # the most frames a read looks back over
    cfg = wf.Config.defaults(fft_size=fft, stereo=1, slope=1.0, bars=1)
    # a spectrum batch's wpos starts at fft (the zeros of create): aged by 2^32 - 2 rings it is 0 at T = 2 rings - fft
    wrap, age = 2 * ring - fft, (1 << 32) - 2 * ring
    with twins(cfg, streams, ring, fft, R=wrap + ring, win=ring) as (fresh, old, sch):
        assert t == 27 and span == ring - 1
        rng = np.random.default_rng(ref.GPU_SEED)
        total = int(sum(sch.pushes))
        # (the burst's events lie in the last two spans, where the reads are)
        audio = np.stack([ref.signal(k, rng, total, 2, 2 * span) for k in ref.KINDS])
        seen, worst = 0, 0.0
        walk = Walk((fresh, old), sch.pushes, wrap, span, slices(audio))
        for i, T, what in walk:
            x, y = fresh.onset(), old.onset()
            for name in ref.FIELDS:
                if name not in ("newest", "last_frame"):
                    assert x[name].tobytes() == y[name].tobytes(), f"{what}: the twins' {name} differ"
            assert np.all(x["newest"] == (fft + T) // ref.H), what
            assert np.all(y["newest"] == (x["newest"] + age // ref.H) % ((1 << 32) // ref.H)), (what, x["newest"], y["newest"])
            hit = x["last_age"] != ref.NONE
            assert np.array_equal(y["last_frame"][hit], x["last_frame"][hit] + np.uint32(age)), (what, x["last_frame"], y["last_frame"])
            assert np.all(y["last_frame"][~hit] == 0) and np.all(x["last_frame"][~hit] == 0), what
            seen += int(np.count_nonzero(hit))
            hist = np.concatenate([np.zeros((streams, 2, fft), np.float32), audio[:, :, :T]], axis=2)
            bad, w = ref.mismatches(x, hist, fft + T, 48000, ring)
            assert not bad, (what, bad[:4])
            worst = max(worst, w)
        before, straddling, behind = walk.before, walk.straddling, walk.exact + walk.behind  # (the exact hit counts as behind here)
        assert before >= 2 and straddling >= 3 and behind >= 3, (before, straddling, behind)
        assert seen >= 3 and np.all(y["strength"][0, :t] > 0)
        print(f"{before} reads before the wrap, {straddling} with the span across it, {behind} behind it; {seen} entries with an onset in view; "
              f"largest difference of a strength {worst:.2f} ulps")


if __name__ == "__main__":
    run()
    print("wrapped ok")
