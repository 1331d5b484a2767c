"""The batches of tests/ring_stage_cases.py without a device: that their scripts leave the eight windows where the cases say, on
every path of wf_ring_stage.hpp's copy; that the audio meets the conditions of the three outputs' own comparisons; and that the
comparisons can see what a mistake in the staging would leave behind -- a frame of a head, a tail or either side of the wrap that
holds something else, and a window that starts one frame off."""
import numpy as np
import pytest

import bits_ref
import gonio_ref
import measure_stagger as ms
import ring_stage_cases as rs
import scope_ref

S = rs.STREAMS
OTHER = np.float32(0.7071)  # no sample of the audio


def _played(batch):
    rings = ms.Rings.of(batch[0], S)
    assert ms.replay(rs.script(batch), rings) == 1
    return rings


@pytest.fixture(scope="module", params=rs.BATCHES, ids=rs.BATCH_IDS)
def played(request):
    return request.param, _played(request.param)


def test_the_windows_lie_where_the_cases_say(played):
    (case, p, starts), rings = played
    ring = case.ring_cap
    c = rings.counter.astype(np.int64)
    assert ((c - p) % ring).tolist() == list(starts) and p == min(case.W, scope_ref.MAX_WINDOW) == gonio_ref.window_frames(case.W) == bits_ref.window_frames(case.W)
    common, counts = rs.plan((case, p, starts))
    assert sum(common) > ring and all(n % 2 == 1 for n in common) and counts.min() >= 1 and len(set(counts.tolist())) == S
    got = rs.combinations(case, p, c)
    every = {(a, x) for a in range(4) for x in (0, 1)}
    if ring > p:
        assert got == every
        assert [(s % 4, int(s + p > ring)) for s in starts] == [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (1, 1), (2, 1), (3, 1)]
    else:  # the ring is the window: only a start of 0 lies inside
        assert got == every - {(1, 0), (2, 0), (3, 0)}
    split = [[rs.parts(*r) for r in rs.runs(s, p, ring)] for s in starts]
    print(f"{case.name}: counters {c.tolist()}, (head, words, tail) of the runs {split}")
    flat = [part for runs in split for part in runs]
    assert {h for h, _, _ in flat} == {0, 1, 2, 3} and {t for _, _, t in flat} == {0, 1, 2, 3}
    if p == 64:
        assert any(w == 0 for _, w, _ in flat)  # a run of a head or a tail alone
        assert all(w < 256 for _, w, _ in flat)
    else:
        assert sum(w >= 1024 for _, w, _ in flat) >= 8 and any(w >= 2048 for _, w, _ in flat)  # the unrolled loop, once and twice
        assert any(0 < w < 256 for _, w, _ in flat) and any(256 <= w < 1024 for _, w, _ in flat)  # some threads idle; the plain loop alone
    # the ring holds pushed audio only, and no two streams the same
    hist = rings.histories()
    assert np.all(hist != 0.0) and len({hist[s].tobytes() for s in range(S)}) == S


def test_the_audio_meets_the_conditions_of_the_comparisons(played):
    """scope: test_scope_cpu.py's condition, at least 90 % of the streams trigger with a period; gonio and bits count every frame
    once, and no frame of a window equals its neighbour, so a frame taken from beside its place is another value"""
    (case, p, _), rings = played
    hist = rings.histories()
    s = scope_ref.scope(hist, case.W)
    share = np.mean((s["triggered"] == 1) & (s["period"] > 0))
    print(f"{case.name} scope: starts {s['start'].tolist()}, periods {s['period'].tolist()}, triggered share {share:.2f}")
    assert share >= 0.9
    g = gonio_ref.gonio(hist, case.W)
    assert np.all(g["cell"].astype(np.int64).sum(axis=(1, 2)) == p) and np.all(g["window"] == p) and np.all(g["occupied"] >= 8)
    b = bits_ref.bits(hist, case.W)
    assert np.all(b["ch"]["hist"].astype(np.int64).sum(axis=2) == p) and np.all(b["window"] == p)
    w = hist[:, :, max(case.ring_cap - p - 1, 0):]
    assert np.all(w[:, :, 1:] != w[:, :, :-1]) and np.all(hist != OTHER)
    for out in rs.OUTPUTS:
        own = ms.restate(out, case, hist, rings.counter)
        assert ms.mismatches(out, case, own, hist, rings.counter) == [], out


def test_a_frame_that_holds_something_else_is_reported(played):
    """bits, which counts every bit of every sample: each frame of each run's head and tail, and the frames either side of every
    16-byte boundary next to them, replaced by another value in turn"""
    (case, p, starts), rings = played
    ring = case.ring_cap
    hist = rings.histories()
    own = ms.restate("bits", case, hist, rings.counter)
    tried = 0
    for s in range(S):
        at = []  # window indices
        first = 0
        for b0, n in rs.runs(starts[s], p, ring):
            head, words, tail = rs.parts(b0, n)
            at += list(range(first, first + min(head + 1, n))) + list(range(first + n - min(tail + 1, n), first + n))
            first += n
        for i in sorted(set(at)):
            wrong = hist[s:s + 1].copy()
            wrong[0, :, ring - p + i] = OTHER
            got = ms.restate("bits", case, wrong, rings.counter[s:s + 1])
            assert ms.mismatches("bits", case, got, hist[s:s + 1], rings.counter[s:s + 1]), (case.name, s, i)
            assert ms.mismatches("bits", case, own[s:s + 1], wrong, rings.counter[s:s + 1]), (case.name, s, i)
            tried += 1
    print(f"{case.name}: {tried} frames replaced, each reported")
    assert tried >= 4 * S


def test_a_window_one_frame_off_is_reported(played):
    """every output, every stream: the ring restated one frame early and one frame late.  (Where the ring is the window, that is
    the same frames in another order, which only the oscilloscope tells apart: gonio and bits count.)"""
    (case, p, _), rings = played
    hist, c = rings.histories(), rings.counter
    for out in rs.OUTPUTS if case.ring_cap > p else ("scope",):
        for s in range(S):
            for off in (-1, 1):
                wrong = ms.restate(out, case, rings.history(s, int(c[s]) + off)[None], c[s:s + 1])
                assert ms.mismatches(out, case, wrong, hist[s:s + 1], c[s:s + 1]), (case.name, out, s, off)
