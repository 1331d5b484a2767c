"""TEST HARNESS (child of tests/test_gpu_click.py::test_across_the_2_to_the_32_wrap): runs against the DEVELOPMENT build of the
library (libwaveform_hip_dev.so via WF_HIP_LIB -- the release library does not export wf_hip_debug_age).

Twin handles in the manner of tests/bits_wrap_child.py, whose schedule this uses: `old` has had its 32-bit write positions moved to
just below 2^32 (wf_hip_debug_age), `fresh` has not; both are fed the same audio -- noise with a click in every packet of at least 64
frames, so that clicks lie on either side of the wrap -- and from just before old's positions overflow click() is read after every
hop.  Each handle must equal the restatement of the frames pushed with its own counter (tests/click_ref.py: `frame` is the counter
position of an event, so the twins differ there, and the aged one's wraps), and the twins must be the same bits everywhere else --
with the window before 2^32, straddling it (0 < wpos < P), starting at position 0 exactly (wpos = P) and behind it.

usage: python tests/click_wrap_child.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import waveform_amd as wf  # noqa: E402
import click_ref as ref  # noqa: E402
from wrap_child import Walk, twins  # noqa: E402


def run():
    fft, ring, streams, sr = 2048, 8192, 3, 48000
    cfg = wf.Config.defaults(fft_size=fft, sample_rate=sr, stereo=1, slope=1.0, bars=1)
    # a spectrum batch's wpos starts at fft (the zeros of create): aged by 2^32 - 2 rings it is 0 at T = 2 rings - fft and fft,
    # the window starting at position 0, at T = R
    with twins(cfg, streams, ring, fft, R=2 * ring, win=fft) as (fresh, old, sch):
        age = (1 << 32) - 2 * ring
        rng = np.random.default_rng(ref.SEED)

        def audio(i, T, p):
            a = rng.uniform(-0.005, 0.005, (streams, 2, p)).astype(np.float32)
            if p >= 64:  # a click per packet, channel and stream, no two alike
                for s in range(streams):
                    for c in range(2):
                        a[s, c, p // 2 + 5 * s + 2 * c] += np.float32((0.3 + 0.011 * (i % 9) + 0.02 * s) * (-1) ** (i + c))
            return a

        walk = Walk((fresh, old), sch.pushes, 2 * ring - fft, fft, audio, hist=np.zeros((streams, 2, fft), np.float32))
        wrapped_frames = 0
        for i, T, what in walk:
            hist = walk.hist
            for s in range(streams):
                for c in range(2):
                    assert ref.margins_hold(ref.margins(hist[s, c], sr)), (what, s, c, ref.margins(hist[s, c], sr))
            x, y = fresh.click(), old.click()
            for got, wpos, who in ((x, fft + T, "fresh"), (y, (fft + T + age) & 0xFFFFFFFF, "aged")):
                bad = ref.mismatches(got, ref.click(hist, sr, [wpos] * streams))
                assert not bad, (what, who, bad[:4])
            wrapped_frames += int(np.count_nonzero(y["ch"]["ev"]["frame"][y["ch"]["ev"]["length"] > 0] > (1 << 31)))
            for z in (x, y):
                z["ch"]["ev"]["frame"] = 0
            assert x.tobytes() == y.tobytes(), f"{what}: the twins differ beyond `frame`"
            assert np.all(y["ch"]["events"] >= 1), what
        assert walk.before >= 2 and walk.straddling >= 3 and walk.exact == 1 and walk.behind >= 3, walk.counts
        assert wrapped_frames >= 3  # events whose counter position lies before 2^32 were read, and after it
        assert np.all(y["window"] == fft) and np.all(y["order"] == ref.ORDER) and np.all(y["ch"]["valid"] == 1)


if __name__ == "__main__":
    run()
    print("wrapped ok")
