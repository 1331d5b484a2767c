"""TEST HARNESS (child of tests/test_gpu_impulse.py::test_across_the_2_to_the_32_wrap): runs against the DEVELOPMENT build of the
library (libwaveform_hip_dev.so via WF_HIP_LIB -- the release library does not export wf_hip_debug_age).

Twin handles in the manner of tests/xfer_wrap_child.py, whose schedule this uses: `old` has had its 32-bit write positions moved to
just below 2^32 (wf_hip_debug_age), `fresh` has not; both are fed the same audio, and from just before old's positions overflow
impulse() is read after every hop and must be the same bits on both but for `newest`, which follows each handle's own counter --
with the span before 2^32, straddling it and behind it -- and within the bound of the restatement of the frames pushed.

usage: python tests/impulse_wrap_child.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import waveform_amd as wf  # noqa: E402
import impulse_ref as ref  # noqa: E402
import xfer_ref  # noqa: E402
from wrap_child import Walk, slices, twins  # noqa: E402

KINDS = ("three taps", "delay -(L-1), echo", "guarded echoes")  # (kinds whose every span reads far from a tie, wherever it is cut)


def run():
    fft, ring, streams, sr = 2048, 8192, len(KINDS), 48000
    p, k = xfer_ref.geometry(fft, ring)
    h = p // 2
    span = xfer_ref.span_frames(p, k) + h - 1  # the most frames a read looks back over
    cfg = wf.Config.defaults(fft_size=fft, sample_rate=sr, stereo=1, slope=1.0, bars=1)
    # a spectrum batch's wpos starts at fft (the zeros of create): aged by 2^32 - 2 rings it is 0 at T = 2 rings - fft
    wrap, age = 2 * ring - fft, (1 << 32) - 2 * ring
    with twins(cfg, streams, ring, fft, R=wrap + ring, win=ring) as (fresh, old, sch):
        assert (p, k) == (1024, 13) and span == ring - 1
        rng = np.random.default_rng(ref.GPU_SEED)
        total = int(sum(sch.pushes))
        audio = np.stack([ref.stream(name, rng, total, p) for name in KINDS])
        worst = 0.0
        walk = Walk((fresh, old), sch.pushes, wrap, span, slices(audio))
        for i, T, what in walk:
            x, y = fresh.impulse(), old.impulse()
            for name in ref.IMPULSE_DTYPE.names:
                if name != "newest":
                    assert x[name].tobytes() == y[name].tobytes(), f"{what}: the twins' {name} differ"
            assert np.all(x["newest"] == (fft + T) // h), what
            assert np.all(y["newest"] == (x["newest"] + age // h) % ((1 << 32) // h)), (what, x["newest"], y["newest"])
            hist = audio[:, :, max(T - ring, 0):T]
            want = ref.impulse(hist, fft, ring, sr, wpos=fft + T)
            assert np.all(ref.margins(hist, fft, ring, sr, wpos=fft + T) >= 1e-3), what
            bad = ref.mismatches(x, want)
            assert not bad, (what, bad[:4])
            worst = max(worst, max(ref.worst(x, want).values()))
        before, straddling, behind = walk.before, walk.straddling, walk.exact + walk.behind  # (the exact hit counts as behind here)
        assert before >= 2 and straddling >= 3 and behind >= 3, (before, straddling, behind)
        assert np.all(y["valid"] == 1) and y["lag"].tolist() == [37, -(p // 4 - 1), 12] and y["count"].tolist() == [3, 2, 2]
        print(f"{before} reads before the wrap, {straddling} with the span across it, {behind} behind it; largest difference of a field "
              f"{worst:.3g}")


if __name__ == "__main__":
    run()
    print("wrapped ok")
