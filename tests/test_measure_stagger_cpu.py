"""The staggered batch of tests/measure_stagger.py without a device: the ring model against signal_ref.History and against every
module's per-batch restatement; the counters the plan ends on; the conditions every module's bound rests on, for every stream's own
window at every read tests/test_gpu_measure_stagger.py and tests/measure_stagger_wrap_child.py compare; and that the cases can see
the mistake they are there for -- a stream read at another stream's write position is reported by that module's own comparison."""
import numpy as np
import pytest

import cq_ref
import gonio_ref
import measure_stagger as ms
import onset_ref
import scope_ref
import signal_ref
import sono_ref
import stereo_ref

S = ms.STREAMS


# ---- the ring model ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ms.CASES, ids=ms.CASE_IDS)
def test_the_ring_model_matches_signal_history(case):
    """the same random pushes, ragged pushes, pushes to sub-ranges, packets longer than the ring and resets: the newest W frames of
    Rings are signal_ref.History's, and the counters are the frames pushed since create or reset"""
    rng = np.random.default_rng(case.W)
    W, ring, ch = case.W, case.ring_cap, case.channels
    rings, hist = ms.Rings.of(case, 5), signal_ref.History(5, ch, W)
    count = np.full(5, case.wpos0, np.int64)
    for step in range(60):
        kind = int(rng.integers(0, 5))
        if kind == 0:
            n = int(rng.integers(1, 2 * W))
            x = rng.uniform(-1, 1, (5, ch, n)).astype(np.float32)
            rings.push(x), hist.push(x)
            count += n
        elif kind == 1:
            frames = rng.integers(0, W + 4, 5)
            frames[int(rng.integers(0, 5))] = 0
            x = rng.uniform(-1, 1, (5, ch, W + 3)).astype(np.float32)
            rings.push(x, frames=frames), hist.push(x, frames=frames)
            count += frames
        elif kind == 2:
            first = int(rng.integers(0, 5))
            x = rng.uniform(-1, 1, (int(rng.integers(1, 6 - first)), ch, int(rng.integers(1, 9)))).astype(np.float32)
            rings.push(x, first=first), hist.push(x, first=first)
            count[first:first + x.shape[0]] += x.shape[2]
        elif kind == 3:
            x = rng.uniform(-1, 1, (5, ch, ring + int(rng.integers(1, 300)))).astype(np.float32)
            rings.push(x), hist.push(x)
            count += x.shape[2]
        else:
            first = int(rng.integers(0, 4))
            rings.reset(first, 2), hist.reset(first, 2)
            count[first:first + 2] = case.wpos0
        assert rings.window(W).tobytes() == hist.window().tobytes(), step
        assert rings.counter.tolist() == count.tolist()
    # another counter turns the ring: what a kernel with the wrong index reads
    assert np.array_equal(rings.history(1, int(rings.counter[1]) + 3)[:, :-3], rings.history(1)[:, 3:])
    old = rings.history(2).copy()
    rings.age(2, 1, (1 << 32) - 2 * ring)
    assert int(rings.counter[2]) == (int(count[2]) - 2 * ring) % (1 << 32) and np.array_equal(rings.history(2), old)


@pytest.mark.parametrize("case", ms.CASES, ids=ms.CASE_IDS)
def test_one_history_through_each_restatement_equals_the_per_batch_call(case):
    """for a batch whose streams do share a counter, the unrolled histories and per-stream counters give what each module's
    existing per-batch call gives from the frames pushed and one scalar counter"""
    rng = np.random.default_rng(3)
    ring, sr, W = case.ring_cap, case.sr, case.W
    x = (0.3 * rng.standard_normal((3, case.channels, ring + 300))).astype(np.float32)
    rings = ms.Rings.of(case, 3)
    for lo in range(0, x.shape[2], 777):
        rings.push(x[:, :, lo:lo + 777])
    wpos = case.wpos0 + x.shape[2]
    assert rings.counter.tolist() == [wpos] * 3
    hist, pushed = rings.histories(), np.concatenate([np.zeros((3, case.channels, case.wpos0), np.float32), x], axis=2)
    assert np.array_equal(hist, pushed[:, :, -ring:])
    for out in ms.OUTPUTS:
        if not ms.available(out, case):
            continue
        got = ms.restate(out, case, hist, rings.counter)
        if out == "sono":
            want = sono_ref.sono(pushed, wpos, sr, ring)
        elif out == "onset":
            want = onset_ref.onset(pushed, wpos, sr, ring)
        else:
            want = np.concatenate([ms.restate(out, case, hist[s:s + 1], rings.counter[s:s + 1]) for s in range(3)])
        # (numpy's matrix products round differently for one stream and for three: bit for bit only where the module counts)
        if out in ("scope", "gonio", "bits"):
            assert got.tobytes() == want.tobytes(), out
        if out in ("sono", "onset"):
            assert np.array_equal(got["newest"], want["newest"]) and np.array_equal(got["columns"], want["columns"])
        assert ms.mismatches(out, case, want, hist, rings.counter) == [], out
        assert ms.mismatches(out, case, got, hist, rings.counter) == [], out


# ---- the plan ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ms.CASES, ids=ms.CASE_IDS)
def test_the_plan_staggers_the_counters(case):
    steps = ms.plan(case)
    ring, W = case.ring_cap, case.W
    c = ms.final_counters(case)
    print(f"{case.name}: counters {c.tolist()}, modulo the ring {(c % ring).tolist()}, start & 3 {((c - W) % 4).tolist()}, newest {(c // 256).tolist()}, "
          f"{len(steps)} steps, {sum(st[0] == 'read' for st in steps)} reads")
    assert len(set((c % ring).tolist())) == S                # pairwise distinct modulo the ring
    assert len(set((c % 4).tolist())) > 1                    # not all in one alignment class ...
    assert sorted(((c[:4] - W) % 4).tolist()) == [0, 1, 2, 3]  # ... streams 0 .. 3 cover all four
    assert len(set((c // 256).tolist())) >= 4                # the `newest` word of sono and onset
    assert (c[1:4] - c[0]).tolist() == [1, 2, 3]
    wraps = [(int(v) - W) % ring + W > ring for v in c]      # the newest W frames run over the ring's end
    assert wraps[4] and not any(wraps[:4])
    assert (c[4] - 512) % ring + 512 > ring                  # the shortest window of stream 4 wraps as well
    assert 0 < c[5] - case.wpos0 < ms.SHORTEST_WINDOW        # zeros and audio share every window of stream 5
    pushes = [st for st in steps if st[0] == "push"]
    ragged = [st for st in steps if st[0] == "ragged"]
    assert any(st[1:3] == (0, S) for st in pushes) and all(any(st[1:3] == (s, 1) for st in pushes) for s in range(S))
    assert sum(st[1][6] == 0 for st in ragged) == 1 and len(ragged) >= 3 and all(len(st[1]) == S for st in ragged)
    long_packet = ms.overlong(case)
    assert long_packet > ring and (long_packet - ring - ms.OVERLONG) % 256 == 0 and [st for st in pushes if st[3] > ring] == [("push", 6, 1, long_packet)]
    assert ((c[6] % ring) // 256) not in ((c[:6] % ring) // 256).tolist()  # stream 6 ends in a hop of its own
    common = [st[3] for st in pushes if st[1:3] == (0, S)]
    assert all(n % 2 == 1 for n in common) and len(set(common)) > len(common) // 2  # uneven odd packets
    tags = [st[1] for st in steps if st[0] == "read"]
    i = steps.index(("reset", 5, 1))
    assert steps[i + 1] == ("read", "the reset of stream 5") and tags[-1] == "the end" and len(tags) >= 5
    j = steps.index(("push", 6, 1, long_packet))
    assert steps[j + 1] == ("read", "the packet longer than the ring")
    # the script hands every stream all of its own audio, and a replay ends on the counters computed above
    rings = ms.Rings.of(case)
    assert ms.replay(ms.script(case, "cq"), rings) == len(tags) and rings.counter.tolist() == c.tolist()


def test_the_cases_are_the_smallest_with_every_output():
    a, b, m, b8 = ms.CASES
    assert (a.W, a.ring_cap, a.sr, a.channels) == (1024, 8192, 48000, 2) and onset_ref.columns(a.ring_cap) == 27
    assert all(ms.available(o, a) for o in ms.OUTPUTS) and all(ms.available(o, m) for o in ms.OUTPUTS)
    assert (b.W, b.ring_cap, b.sr, b.channels, b.ring_frames) == (2048, 4096, 44100, 1, 0)
    # one captured channel: the three outputs that take two channels refuse, and so does onset, whose ring is 8192 frames at least
    assert [o for o in ms.OUTPUTS if not ms.available(o, b)] == ["stereo", "gonio", "delay", "onset"]
    assert [o for o in ms.OUTPUTS if not ms.available(o, b8)] == ["stereo", "gonio", "delay"] and b8.kw == b.kw and b8.ring_cap == 8192
    assert m.meter and m.W == int(48000 * 0.05) & -16 == 2400 and m.wpos0 == 0 and m.ring_cap == 8192
    steps, wrap = ms.wrap_plan(a)
    tags = [st[1] for st in steps if st[0] == "read"]
    assert sum(t < 0 for t in tags) >= 2 and 0 in tags and sum(0 < t < a.W for t in tags) >= 2 and a.W in tags and sum(t > a.W for t in tags) >= 3
    assert sum(st[0] == "age" for st in steps) == 1 and (int(ms.final_counters(a)[ms.AGED]) - 2 * a.ring_cap + wrap) % (1 << 32) == 0


# ---- the conditions of every module's bound ---------------------------------------------------------------------------------------

CONDITIONED = ("pitch", "sono", "thd", "delay", "onset")


def _walk(case, out, steps, streams):
    """{what: the figure nearest its threshold} over every read of `steps` and every stream of `streams`, and the conditions that
    do not hold"""
    rings = ms.Rings.of(case)
    figures, missed = {}, []

    def on_read(i, tag):
        for s in streams:
            for what, fig, ok in ms.conditions(out, case, rings.history(s), rings.counter[s], s):
                key = what[5:] if what.startswith("ch ") else what
                worse = max if ("orders" in key or "orderings" in key or "second arm" in key) else min
                figures[key] = worse(figures.get(key, fig), fig)
                if not ok:
                    missed.append((tag, s, what, fig))

    reads = ms.replay(ms.script(case, out, steps), rings, on_read=on_read)
    return figures, missed, reads


@pytest.mark.parametrize("case", ms.CASES, ids=ms.CASE_IDS)
def test_every_read_meets_the_conditions_of_its_modules_bound(case):
    """for every stream's own window at every read of the plan, with the thresholds of each module's own CPU test: thd -- the
    runners-up of both argmaxes and every h f0 at least 1e-6 clear, numpy.fft and the radix-2 transform within 1e-7 dB; delay --
    its four orders within 1e-9, the argmax 1e-3, the phases 1e-6 from pi and the fraction 1e-6 from its clamp; onset -- no decision
    within four ulps of flipping; sono -- the noise streams wholly within the first arm; pitch -- both orders of addition agree"""
    for out in CONDITIONED:
        if not ms.available(out, case):
            continue
        figures, missed, reads = _walk(case, out, ms.plan(case), range(S))
        print(f"{case.name} {out}: {reads} reads x {S} streams: " + ", ".join(f"{k} {v:.3g}" for k, v in figures.items()))
        assert not missed, (out, missed[:6])
        assert figures


def test_the_aged_stream_meets_the_conditions_at_every_hop_across_the_wrap():
    case = ms.CASES[0]
    steps, wrap = ms.wrap_plan(case)
    for out in CONDITIONED:
        figures, missed, reads = _walk(case, out, steps, (ms.AGED,))
        print(f"{case.name} {out}, stream {ms.AGED} across 2^32: {reads} reads: " + ", ".join(f"{k} {v:.3g}" for k, v in figures.items()))
        assert not missed, (out, missed[:6])


# ---- the cases can see the mistake ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ms.CASES, ids=ms.CASE_IDS)
def test_a_stream_read_at_another_streams_counter_is_reported(case):
    """every output, every stream s >= 1 that is not silent: its ring restated at stream 0's counter -- what a kernel reading
    wpos[0], or wpos[slice index] in a slice, would make of it -- must be reported by the module's own comparison against the
    restatement at its own counter, with `newest` and `last_frame` of sono and onset set right, so that the columns themselves have
    to show it.  At least four streams per output; the other substitutions are counted and printed.  (sono and onset anchor their
    columns to multiples of 256 frames: two counters in the same hop read the same columns, which is why the plan runs the grid
    between streams 1 and 2.  YIN does not see a periodic stream move.)"""
    for out in ms.OUTPUTS:
        if not ms.available(out, case):
            continue
        rings = ms.Rings.of(case)
        ms.replay(ms.script(case, out), rings)
        hist, c = rings.histories(), rings.counter
        own = ms.restate(out, case, hist, c)
        assert ms.mismatches(out, case, own, hist, c) == []
        seen = np.zeros((S, S), bool)
        live = [s for s in range(1, S) if not ms.silent(out, case, s)]
        for s in live:
            for t in range(S):
                if t == s:
                    continue
                wrong = ms.restate(out, case, rings.history(s, c[t])[None], c[t:t + 1])
                if out in ("sono", "onset"):
                    wrong["newest"] = own["newest"][s]
                if out == "onset":
                    wrong["last_frame"] = own["last_frame"][s]
                seen[s, t] = bool(ms.mismatches(out, case, wrong, hist[s:s + 1], c[s:s + 1]))
        at0 = int(seen[:, 0].sum())
        every = int(sum(seen[s].sum() == S - 1 for s in live))
        print(f"{case.name} {out}: {len(live)} live streams; read at stream 0's counter {at0} are reported, at any other stream's {every}; "
              f"not reported (s, t): {[(s, t) for s in live for t in range(S) if t != s and not seen[s, t]]}")
        assert at0 >= 4, (out, seen[:, 0].tolist())


@pytest.mark.parametrize("case", ms.CASES, ids=ms.CASE_IDS)
def test_the_final_windows_are_no_trivial_entries(case):
    """the conditions tests/test_cq_cpu.py, test_stereo_cpu.py, test_scope_cpu.py and test_gonio_cpu.py put on their own GPU cases,
    with their thresholds, on every stream's own final window -- stream 5 apart, whose window is mostly the zeros of its reset: at
    least 80 % of cq's covered bins are strong (held to two ulps), at most 1 % of stereo's overlapping bands have a coherence under
    0.01 (where the phase is left out), at least 90 % of scope's streams trigger with a period, and gonio's picture kinds occupy at
    least 64 cells with no cell above P / 8"""
    full = [s for s in range(S) if s != 5]
    for out in ("cq", "stereo", "scope", "gonio"):
        if not ms.available(out, case):
            continue
        rings = ms.Rings.of(case)
        ms.replay(ms.script(case, out), rings)
        hist = rings.histories()[full]
        if out == "cq":
            lmax = cq_ref.max_window(case.ring_cap)
            end = cq_ref.geometry(case.sr, lmax)[1]
            share = cq_ref.strong(cq_ref.amplitudes(hist, case.sr, lmax), cq_ref.peak(hist, lmax))[..., :end].mean()
            print(f"{case.name} cq: strong share {share:.3f}")
            assert share >= 0.8
        elif out == "stereo":
            share = stereo_ref.low_coherence_share(stereo_ref.stereo(hist[..., case.ring_cap - case.W:], case.sr), case.sr)
            print(f"{case.name} stereo: share of bands with a coherence under 0.01 {share:.4f}")
            assert share <= 0.01
        elif out == "scope":
            s = scope_ref.scope(hist, case.W)
            share = np.mean((s["triggered"] == 1) & (s["period"] > 0))
            print(f"{case.name} scope: starts {s['start'].tolist()}, periods {s['period'].tolist()}, triggered share {share:.2f}")
            assert share >= 0.9
        else:
            g = gonio_ref.gonio(hist, case.W)
            p = gonio_ref.window_frames(case.W)
            for s, r in zip(full, g):
                print(f"{case.name} gonio {ms.GONIO_KINDS[s]}: zoom {int(r['zoom'])}, occupied {int(r['occupied'])}, largest cell {int(r['cell'].max())}")
                if ms.GONIO_KINDS[s] in gonio_ref.PICTURE_KINDS:
                    assert r["occupied"] >= 64 and r["cell"].max() <= p // 8, (case.name, s)
