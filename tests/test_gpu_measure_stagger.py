"""The outputs that read the audio rings, on a batch whose seven streams all stand at different write positions
(tests/measure_stagger.py): stereo, cq, scope, gonio, sono, bits, thd, delay and onset, with signal and pitch on the same script,
each stream against the float64 restatement of its own ring at its own counter -- at every read of the plan, straight after the reset
of one stream and after a packet longer than the ring among them --; slices as a handle's first read; the outputs read in either
order; a three-shard group; one stream of the seven carried across 2^32.  And, on a batch that has all twenty measurement outputs,
every one of them on one handle, forwards against backwards with slices first.

A kernel that takes the write position, the alignment of its float4 fetch or the column anchor from another stream than its own --
wpos[0], wpos[slice index], a shard's wpos at the group's index -- passes every other module, where all streams of a batch have
received the same number of frames before every read.  tests/test_measure_stagger_cpu.py shows that it cannot pass here, and that
every window compared meets the conditions of its module's bound.  No tolerance is defined here: every bound is the output's own
(measure_stagger.mismatches)."""

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import measure_stagger as ms
import sono_ref
from measure_common import run_wrap_child

pytestmark = pytest.mark.gpu
S = ms.STREAMS
OUT = {name: getattr(binding, "OUT_" + name.upper()) for name in ms.OUTPUTS}
SPREAD = "cq"  # the audio of the tests of bit identity: noise and two sines, different in every stream and channel


def _create(case, cls=wf.SpectrumBatch, *args):
    return cls(wf.Config.defaults(**case.kw), S, *args, ring_frames=case.ring_frames)


def _checked(case, b):
    assert (b.fft_size, b.ring_frames, b.capture_channels) == (case.W, case.ring_cap, case.channels)
    return b


def _outputs(case, b):
    """the outputs the case has; the others refuse, with wf_hip_output_bytes 0"""
    have = [o for o in ms.OUTPUTS if ms.available(o, case)]
    for o in ms.OUTPUTS:
        assert (int(wf.lib().wf_hip_output_bytes(b.h, OUT[o])) != 0) == (o in have), o
    return have


def _pinned(shape):
    return wf.PinnedBuffer(shape)


def _read_all(b, outputs, first=0, count=None):
    return {o: getattr(b, o)(first, count) for o in outputs}


@pytest.mark.parametrize("output", ms.OUTPUTS)
@pytest.mark.parametrize("case", ms.CASES, ids=ms.CASE_IDS)
def test_every_stream_equals_the_restatement_of_its_own_ring(case, output):
    """the plan in the output's own signal kinds; at every read every stream's entry against the restatement of Rings.history(s) at
    that stream's counter, by the output's own comparison; the header words exactly"""
    with _create(case) as b:
        _checked(case, b)
        if not ms.available(output, case):
            assert int(wf.lib().wf_hip_output_bytes(b.h, OUT[output])) == 0
            with pytest.raises(wf.WfHipError):
                getattr(b, output)()
            return
        assert int(wf.lib().wf_hip_output_bytes(b.h, OUT[output])) != 0
        rings = ms.Rings.of(case)
        seen = []

        def on_read(i, tag):
            got = getattr(b, output)()
            hist, c = rings.histories(), rings.counter
            assert got.shape == (S,)
            bad = ms.mismatches(output, case, got, hist, c)
            print(f"{case.name} {output}, read {i} after {tag}: counters {c.tolist()}, {len(bad)} beyond the bound")
            assert not bad, (tag, bad[:6])
            if output in ("sono", "onset"):
                assert np.array_equal(got["newest"], c // 256), tag
            if output == "sono":
                arm2 = sono_ref.mismatches(got, hist, c, case.sr, case.ring_cap)[1]
                assert all(arm2[s] == 0 for s in range(S) if ms.first_arm_only(case, s)), (tag, arm2.tolist())
            seen.append(tag)

        ms.replay(ms.script(case, output), rings, (b,), on_read, _pinned)
        assert "the reset of stream 5" in seen and "the packet longer than the ring" in seen and seen[-1] == "the end" and len(seen) >= 5
        assert rings.counter.tolist() == ms.final_counters(case).tolist()


@pytest.mark.parametrize("case", ms.CASES, ids=ms.CASE_IDS)
def test_slices_as_a_handles_first_read(case):
    """three handles fed the same plan: read(first=2, count=3) and read(first=6, count=1), each the first read of its output on its
    handle, are the bytes of the full read's entries -- an output index used where the stream index belongs would not be"""
    with _create(case) as full, _create(case) as mid, _create(case) as last:
        outputs = _outputs(case, _checked(case, full))
        ms.replay(ms.script(case, SPREAD), None, (full, mid, last), None, _pinned)
        a = _read_all(mid, outputs, 2, 3)
        z = _read_all(last, outputs, 6, 1)
        want = _read_all(full, outputs)
        again = _read_all(mid, outputs, 6, 1)
        for o in outputs:
            assert want[o].shape == (S,) and a[o].shape == (3,) and z[o].shape == (1,)
            assert a[o].tobytes() == want[o][2:5].tobytes(), o
            assert z[o].tobytes() == want[o][6:].tobytes(), o
            assert again[o].tobytes() == want[o][6:].tobytes(), o
            assert len({want[o][s].tobytes() for s in range(S)}) == S, o  # no two streams read alike: a wrong entry would show


@pytest.mark.parametrize("case", ms.CASES, ids=ms.CASE_IDS)
def test_the_order_of_the_reads_does_not_matter(case, monkeypatch):
    """all outputs once in enum order and once in reverse, nothing in between: the same bytes; guard bytes behind every block intact
    (wf_hip_sync checks them under WF_HIP_CANARY)"""
    monkeypatch.setenv("WF_HIP_CANARY", "1")
    with _create(case) as b:
        outputs = _outputs(case, _checked(case, b))
        ms.replay(ms.script(case, SPREAD), None, (b,), None, _pinned)
        up = {o: getattr(b, o)() for o in outputs}
        down = {o: getattr(b, o)() for o in reversed(outputs)}
        b.sync()
        for o in outputs:
            assert up[o].tobytes() == down[o].tobytes(), o


@pytest.mark.parametrize("case", ms.CASES, ids=ms.CASE_IDS)
def test_three_shards_match_one_handle(case):
    """MultiBatch(cfg, 7, [0, 0, 0]) fed the same plan through push_audio(first=...) -- the ragged steps per stream on both sides:
    a group has no ragged push --: every output the bytes of the single handle's, also over a range that spans two shards; and
    after a tick the group gathers the bars of the single handle (a meter batch has one per channel: such a group could not be
    created while its shards were asked to write the gather's buffers themselves, which a meter kernel does not)"""
    with _create(case) as one, _create(case, wf.MultiBatch, [0, 0, 0]) as m:
        outputs = _outputs(case, _checked(case, one))
        ms.replay(ms.script(case, SPREAD), None, (one, m), None, None, ragged=False)
        m.sync()
        for o in outputs:
            want = getattr(one, o)()
            assert getattr(m, o)().tobytes() == want.tobytes(), o
            assert getattr(m, o)(2, 4).tobytes() == want[2:6].tobytes(), o  # streams 2 .. 5: two shards at least
            assert getattr(m, o)(6, 1).tobytes() == want[6:].tobytes(), o
        one.tick()
        m.tick()
        m.allgather_bars()
        bars = one.bars()
        assert m.bars().tobytes() == bars.tobytes()
        for d in range(3):
            assert m.gathered(d).tobytes() == bars.tobytes(), d
        for o in outputs:  # (a tick does not move the rings)
            assert getattr(m, o)().tobytes() == getattr(one, o)().tobytes(), o


def test_all_twenty_outputs_on_one_handle_in_either_order(monkeypatch):
    """every row of binding.MEASURES on twin handles fed the same audio -- the smallest ring the tempo serves, filled once, then one
    tick --: `a` reads them in table order, `b` in reverse with the slice (first=1, count=2) as each output's first read there.  The
    bytes are the same, so no row, block or setup flag is another output's; no two streams read alike, so a wrong entry would
    show; guard bytes behind every block intact (wf_hip_sync checks them under WF_HIP_CANARY).  No tolerance: twin handles read
    the same bits"""
    monkeypatch.setenv("WF_HIP_CANARY", "1")
    names, streams, ring = list(binding.MEASURES), 3, 131072
    assert len(names) == 20
    cfg = wf.Config.defaults(fft_size=1024, sample_rate=48000, stereo=1, bars=1)
    rng = np.random.default_rng(20)
    t = np.arange(ring, dtype=np.float64) / 48000.0
    hz = 110.0 * (1.0 + np.arange(streams * 2, dtype=np.float64)).reshape(streams, 2, 1)
    audio = (0.1 * rng.standard_normal((streams, 2, ring)) + 0.3 * np.sin(2.0 * np.pi * hz * t)).astype(np.float32)
    with wf.SpectrumBatch(cfg, streams, ring_frames=ring) as a, wf.SpectrumBatch(cfg, streams, ring_frames=ring) as b:
        for h in (a, b):
            assert (h.fft_size, h.ring_frames, h.capture_channels) == (1024, ring, 2)
            h.enable_loudness()
            for at in range(0, ring, 32768):
                h.push_audio(audio[:, :, at:at + 32768])
            h.tick()
            for name in names:
                assert int(wf.lib().wf_hip_output_bytes(h.h, binding.MEASURES[name][0])) != 0, name
        up = {name: getattr(a, name)() for name in names}
        part, down = {}, {}
        for name in reversed(names):
            part[name] = getattr(b, name)(1, 2)
            down[name] = getattr(b, name)()
        a.sync()
        b.sync()
    for name in names:
        assert up[name].shape[0] == streams and part[name].shape[0] == 2, name
        assert down[name].tobytes() == up[name].tobytes(), name
        assert part[name].tobytes() == up[name][1:3].tobytes(), name
        assert len({up[name][s].tobytes() for s in range(streams)}) == streams, name


def test_one_stream_across_the_2_to_the_32_wrap():
    """tests/measure_stagger_wrap_child.py: twin handles on the development build play the fft-1024 case, stream 3 of one of them is
    aged to just below 2^32 and walked across the wrap in small hops while its neighbours stay young; every output equal on both
    twins for all streams, the aged stream within its bound of the restatement.  One child process (the release library has no test
    aids)"""
    run_wrap_child("measure_stagger_wrap_child.py", 60)
