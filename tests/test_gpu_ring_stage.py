"""The copy of a ring window into LDS (waveform_amd/csrc/wf_ring_stage.hpp) on the device, through the three outputs that use it:
scope, gonio and bits on the batches of tests/ring_stage_cases.py -- eight stereo streams whose windows start at every alignment of
the ring's 16-byte groups, wholly inside the ring and across its end; runs of one frame and runs that go through the unrolled loop.

Every entry is compared with the output's own restatement by that module's own comparison (measure_stagger.mismatches): no
tolerance is defined here.  tests/test_ring_stage_cpu.py shows that the windows lie where the cases say, that the audio meets the
comparisons' conditions and that a frame out of place is reported."""
import numpy as np
import pytest

import waveform_amd as wf
import measure_stagger as ms
import ring_stage_cases as rs

pytestmark = pytest.mark.gpu
S = rs.STREAMS


@pytest.mark.parametrize("batch", rs.BATCHES, ids=rs.BATCH_IDS)
def test_every_alignment_inside_and_across_the_end(batch):
    case, p, starts = batch
    with wf.SpectrumBatch(wf.Config.defaults(**case.kw), S, ring_frames=case.ring_frames) as b:
        assert (b.fft_size, b.ring_frames, b.capture_channels) == (case.W, case.ring_cap, case.channels)
        rings = ms.Rings.of(case, S)
        got = {}

        def on_read(i, tag):
            for out in rs.OUTPUTS:
                got[out] = getattr(b, out)()

        assert ms.replay(rs.script(batch), rings, (b,), on_read, wf.PinnedBuffer) == 1
        hist, c = rings.histories(), rings.counter
        # the counters the host has pushed the streams to: all eight combinations, where the ring leaves room for them
        seen = rs.combinations(case, p, c)
        every = {(a, x) for a in range(4) for x in (0, 1)}
        assert seen == (every if case.ring_cap > p else every - {(1, 0), (2, 0), (3, 0)})
        assert ((c.astype(np.int64) - p) % case.ring_cap).tolist() == list(starts)
        for out in rs.OUTPUTS:
            assert got[out].shape == (S,) and np.all(got[out]["window"] == p)
            bad = ms.mismatches(out, case, got[out], hist, c)
            print(f"{case.name} {out}: counters {c.tolist()}, {len(bad)} beyond the bound")
            assert not bad, (out, bad[:6])
