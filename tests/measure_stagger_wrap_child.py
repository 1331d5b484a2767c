"""TEST HARNESS (child of tests/test_gpu_measure_stagger.py::test_one_stream_across_the_2_to_the_32_wrap): runs against the DEVELOPMENT
build of the library (libwaveform_hip_dev.so via WF_HIP_LIB -- the release library does not export wf_hip_debug_age).

Twin handles in the manner of tests/thd_wrap_child.py, per output: both play the staggered plan of the fft-1024 case
(tests/measure_stagger.py) in the output's own signal kinds, then ONE stream of `old` -- stream 3 of the seven -- has its 32-bit write
position moved to just below 2^32 (wf_hip_debug_age(h, 3, 1, 2^32 - 2 rings)) while its neighbours stay young, and both are fed
whole-batch hops by wrap_child.Schedule.  From just before the aged position overflows the output is read after every hop -- with
the window before 2^32, straddling it, starting at position 0 exactly and behind it -- and must be the same bytes on both twins for
all seven streams (`newest` of sono and onset, and onset's last_frame, of the aged stream alone ahead by the aged amount), and the
aged stream within its output's bound of the restatement of its ring at its aged counter.

usage: python tests/measure_stagger_wrap_child.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import waveform_amd as wf  # noqa: E402
import measure_stagger as ms  # noqa: E402
import onset_ref  # noqa: E402
from wrap_child import _dev  # noqa: E402

S, A = ms.STREAMS, ms.AGED


def run_output(L, case, output, steps):
    cfg = wf.Config.defaults(**case.kw)
    rings = ms.Rings.of(case)
    amount = (1 << 32) - 2 * case.ring_cap
    reads = []
    with wf.SpectrumBatch(cfg, S, ring_frames=case.ring_frames) as fresh, wf.SpectrumBatch(cfg, S, ring_frames=case.ring_frames) as old:
        assert (old.fft_size, old.ring_frames) == (case.W, case.ring_cap)

        def on_age(first, count, frames):
            assert (first, count, frames) == (A, 1, amount)
            assert L.wf_hip_debug_age(old.h, first, count, frames) == 0, L.wf_hip_last_error(old.h)

        def on_read(i, at):
            what = f"{output}, read {i} at wpos[{A}] = 2^32{at:+d}"
            x, y = getattr(fresh, output)(), getattr(old, output)()
            assert int(rings.counter[A]) == at % (1 << 32), what
            if output in ("sono", "onset"):
                ahead = np.zeros(S, np.int64)
                ahead[A] = amount // 256
                assert np.array_equal(y["newest"], (x["newest"] + ahead) % ((1 << 32) // 256)), (what, x["newest"], y["newest"])
                x = x.copy()
                x["newest"] = y["newest"]
                if output == "onset" and x["last_age"][A] != onset_ref.NONE:
                    x["last_frame"][A] = (int(x["last_frame"][A]) + amount) % (1 << 32)
            assert x.tobytes() == y.tobytes(), f"{what}: the twins differ in stream(s) {[s for s in range(S) if x[s].tobytes() != y[s].tobytes()]}"
            bad = ms.mismatches(output, case, y[A:A + 1], rings.history(A)[None], rings.counter[A:A + 1])
            assert not bad, (what, bad[:4])
            reads.append(at)

        ms.replay(ms.script(case, output, steps), rings, (fresh, old), on_read, wf.PinnedBuffer, on_age=on_age)
    W = case.W
    before, straddling, behind = sum(t < 0 for t in reads), sum(0 < t < W for t in reads), sum(t > W for t in reads)
    assert before >= 2 and 0 in reads and straddling >= 2 and W in reads and behind >= 3, reads
    return len(reads)


def run():
    L = _dev()
    case = ms.CASES[0]
    steps, _ = ms.wrap_plan(case)
    for output in ms.OUTPUTS:
        n = run_output(L, case, output, steps)
        print(f"{output}: {n} reads equal on both twins, stream {A} within its bound across 2^32")


if __name__ == "__main__":
    run()
    print("wrapped ok")
