"""TEST HARNESS (child of tests/test_gpu_tempo.py::test_across_the_2_to_the_32_wrap): runs against the DEVELOPMENT build of the
library (libwaveform_hip_dev.so via WF_HIP_LIB -- the release library does not export wf_hip_debug_age).

Twin handles in the manner of tests/onset_wrap_child.py: `old` has had its 32-bit write positions moved to just below 2^32
(wf_hip_debug_age), `fresh` has not; both are fed the same audio -- kicks at 120 BPM, bursts at 150 BPM and noise, the first case
of tempo_ref.GPU_CASES carried on -- and tempo() is read with the span before 2^32, straddling it (0 < wpos < span) and behind it:
every field but the three on the counter must be the same bytes on both, old's `newest`, `last_beat_frame` and `next_beat_frame`
must be fresh's plus the age modulo 2^32, and fresh must equal the restatement of the frames pushed.  The span is the whole ring,
so the reads are a dozen at uneven hops rather than one after every hop of a video frame.

usage: python tests/tempo_wrap_child.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import waveform_amd as wf  # noqa: E402
import tempo_ref as ref  # noqa: E402
from wrap_child import Walk, slices, twins  # noqa: E402

COUNTER = ("newest", "last_beat_frame", "next_beat_frame")


def run():
    fft, sr, ch, kw, ring, t, kinds = ref.GPU_CASES[0]
    streams = len(kinds)
    span = (t + 1) * ref.H + ref.P + ref.H - 1  # the most frames a read looks back over
    cfg = wf.Config.defaults(fft_size=fft, sample_rate=sr, stereo=1, slope=1.0, bars=1)
    # a spectrum batch's wpos starts at fft (the zeros of create): aged by 2^32 - 2 rings it is 0 at T = 2 rings - fft
    wrap, age = 2 * ring - fft, (1 << 32) - 2 * ring
    with twins(cfg, streams, ring, fft) as (fresh, old, _):
        assert t == 507 and span == ring + ref.H - 1
        # (frames pushed, read behind it): the approach in half rings, two reads before the wrap, the exact hit, the span across it
        # at uneven places, and behind it
        pushes = [(ring // 2, False)] * 3 + [(ring // 2 - fft - 1278, False), (800, True), (441, True), (37, True), (800, True), (30011, True),
                                             (50021, True), (40009, True), (10991, True), (441, True), (30011, True)]
        total = sum(p for p, _ in pushes)
        audio = np.stack([np.stack([x, np.float32(0.25) * x]) for x in (ref.kicks(np.random.default_rng(ref.GPU_SEED), 120.0, total, sr)[0],
                                                                       ref.bursts(np.random.default_rng(ref.GPU_SEED + 1), 150.0, total, sr)[0],
                                                                       ref.noise(np.random.default_rng(ref.GPU_SEED + 2), -20.0, total))])
        worst = 0.0
        walk = Walk((fresh, old), pushes, wrap, span, slices(audio))
        for i, T, what in walk:
            x, y = fresh.tempo(), old.tempo()
            for name in ref.FIELDS:
                if name not in COUNTER:
                    assert x[name].tobytes() == y[name].tobytes(), f"{what}: the twins' {name} differ"
            assert np.all(x["valid"] == 1), what
            assert np.all(x["newest"] == (fft + T) // ref.H), what
            assert np.all(y["newest"] == (x["newest"] + age // ref.H) % ((1 << 32) // ref.H)), (what, x["newest"], y["newest"])
            for name in COUNTER[1:]:
                assert np.array_equal(y[name], x[name] + np.uint32(age)), (what, name, x[name], y[name])
            assert np.array_equal(x["next_beat_frame"], x["last_beat_frame"] + x["period_frames"]), what
            if 0 < T - wrap < span:  # the newest beat of the aged handle lies behind 2^32 or just before it
                assert np.all((y["last_beat_frame"] < span) | (y["last_beat_frame"] > (1 << 32) - span)), (what, y["last_beat_frame"])
            hist = np.concatenate([np.zeros((streams, 2, fft), np.float32), audio[:, :, :T]], axis=2)
            # (this audio is no committed case: its integers are held to the rule on the device's own strengths)
            bad, w = ref.mismatches(x, hist, fft + T, sr, ring, integers=False)
            assert not bad, (what, bad[:4])
            worst = max(worst, w)
        # (here `exact` is the read at the wrap itself, and a read that starts at position 0 counts as behind)
        before, exact, straddling, behind = walk.before - walk.at, walk.at, walk.straddling, walk.exact + walk.behind
        assert walk.T == total and before == 2 and exact == 1 and straddling >= 4 and behind >= 2, (before, exact, straddling, behind)
        assert y["lag"][:2].tolist() == [94, 75] and np.all(y["strength"][:, :t].max(axis=1) >= 2.0)
        print(f"{before} reads before the wrap, one at it, {straddling} with the span across it, {behind} behind it; largest difference of a "
              f"strength {worst:.2f} ulps")


if __name__ == "__main__":
    run()
    print("wrapped ok")
