"""The staggered batch: seven streams of one batch whose 32-bit write positions all differ, for the outputs that read the audio
rings through wf_ring_view.hpp -- stereo, cq, scope, gonio, sono, bits, thd, delay and onset, with signal and pitch on the same
script.  Shared by tests/test_measure_stagger_cpu.py (which shows, without a device, that the cases meet the conditions of every
module's bound and that a kernel reading another stream's position would be reported) and tests/test_gpu_measure_stagger.py and
tests/measure_stagger_wrap_child.py (which play the same steps into the device).

Rings       what the device keeps per stream, restated: the ring as it lies in memory and the uint32 counter.
plan(case)  the steps as frame counts: a common script of uneven odd packets through three push paths, and per stream what the
            table in its docstring adds to it.
script(...) the same steps with one output's own signal kinds in them, every stream's audio built for that stream's own end.
restate / mismatches / conditions: every output's own restatement, comparison and the conditions its bound rests on, called per
            stream with that stream's history and counter.  No tolerance is defined here: each comes from the output's *_ref.py
            (signal's from signal_ref.mismatches)."""
from dataclasses import dataclass, field

import numpy as np

import bits_ref
import cq_ref
import delay_ref
import gonio_ref
import onset_ref
import pitch_cases
import pitch_ref
import scope_ref
import signal_ref
import sono_ref
import stereo_ref
import thd_ref

STREAMS = 7
SEED = 20261102
OUTPUTS = ("signal", "pitch", "stereo", "cq", "scope", "gonio", "sono", "bits", "thd", "delay", "onset")  # enum order
TWO_CHANNEL = ("stereo", "gonio", "delay")
SHORTEST_WINDOW = 512  # the distortion window at fft 1024: stream 5 is refilled with fewer frames than this
TAIL = (151, 137, 101)  # the common packets behind the reset of stream 5
OVERLONG = 77          # stream 6's long packet is the ring, this many frames and the whole hops overlong() adds


@dataclass(frozen=True)
class Case:
    name: str
    kw: dict = field(hash=False)   # wf.Config.defaults(**kw)
    ring_frames: int               # asked of create (0: the default)
    W: int                         # wf_hip_fft_size() of the handle
    ring_cap: int
    channels: int

    @property
    def sr(self):
        return self.kw["sample_rate"]

    @property
    def meter(self):
        return bool(self.kw.get("meter"))

    @property
    def wpos0(self):
        """the counter of a fresh or reset stream: a spectrum batch holds N zeros, a meter batch nothing"""
        return 0 if self.meter else self.W


_COMMON = dict(slope=1.0, floor_db=-70)
CASES = (
    # onset's smallest ring (27 columns), above the distortion window's floor of 512
    Case("fft1024", dict(fft_size=1024, sample_rate=48000, capture_channels=2, stereo=1, bars=1, **_COMMON), 8192, 1024, 8192, 2),
    # the <1> instantiations; the default ring of 4096 frames
    Case("mono2048", dict(fft_size=2048, sample_rate=44100, capture_channels=1, stereo=0, bars=1, **_COMMON), 0, 2048, 4096, 1),
    # a meter batch: counters start at 0, W = 48000 * 0.05 = 2400 is no power of two
    Case("meter", dict(fft_size=1024, sample_rate=48000, capture_channels=2, stereo=1, meter=1, bars=0, meter_ms=50, **_COMMON), 0, 2400,
         8192, 2),
    # one captured channel once more, with the ring onset asks for: the default ring above leaves onset<1> out
    Case("mono2048_ring8192", dict(fft_size=2048, sample_rate=44100, capture_channels=1, stereo=0, bars=1, **_COMMON), 8192, 2048, 8192, 1),
)
CASE_IDS = [c.name for c in CASES]


def available(output, case):
    """whether a batch of this case has the output (include/wf_hip.h: two captured channels for stereo, gonio and delay; a ring of
    2048 frames for sono, of 8192 for onset; 512 frames for thd)"""
    if output in TWO_CHANNEL:
        return case.channels == 2
    if output == "onset":
        return case.ring_cap >= onset_ref.MIN_RING
    if output == "sono":
        return case.ring_cap >= 2 * sono_ref.P
    if output == "thd":
        return case.W >= SHORTEST_WINDOW
    return True


# ---- the ring model ---------------------------------------------------------------------------------------------------------------

class Rings:
    """Per stream the ring as the device holds it -- ring_cap float32 per captured channel, written at wpos & (ring_cap - 1) --
    and the uint32 counter."""

    def __init__(self, streams, channels, ring_cap, wpos0):
        assert ring_cap & (ring_cap - 1) == 0
        self.ring_cap, self.wpos0 = ring_cap, wpos0
        self.ring = np.zeros((streams, channels, ring_cap), np.float32)
        self.counter = np.full(streams, wpos0, np.uint32)

    @classmethod
    def of(cls, case, streams=STREAMS):
        return cls(streams, case.channels, case.ring_cap, case.wpos0)

    def push(self, samples, first=0, frames=None):
        """samples: float32 [count, channels, n]; frames: the per-stream counts of a ragged push (0 leaves a stream alone).  A
        packet longer than the ring keeps its newest frames; the counter moves by all of them"""
        samples = np.asarray(samples, np.float32)
        for i in range(samples.shape[0]):
            n = samples.shape[2] if frames is None else int(frames[i])
            if n == 0:
                continue
            s = first + i
            x = samples[i, :, :n]
            at = int(self.counter[s])
            keep = min(n, self.ring_cap)
            idx = (at + n - keep + np.arange(keep)) & (self.ring_cap - 1)
            self.ring[s][:, idx] = x[:, n - keep:]
            self.counter[s] = (at + n) & 0xFFFFFFFF

    def reset(self, first, count):
        """wf_hip_reset: a spectrum batch's N zeros with the counter at N, a meter batch's empty rings with the counter at 0"""
        self.ring[first:first + count] = 0.0
        self.counter[first:first + count] = self.wpos0

    def age(self, first, count, frames):
        """wf_hip_debug_age: the counters move, the rings stay (so whole rings only)"""
        assert frames % self.ring_cap == 0
        c = self.counter[first:first + count].astype(np.int64)
        self.counter[first:first + count] = ((c + frames) & 0xFFFFFFFF).astype(np.uint32)

    def history(self, s, counter=None):
        """float32 [channels, ring_cap]: stream s's ring unrolled, oldest frame first, ending at `counter` (default: its own;
        another stream's: what a kernel with the wrong index would see)"""
        c = int(self.counter[s] if counter is None else counter)
        idx = (c - self.ring_cap + np.arange(self.ring_cap)) & (self.ring_cap - 1)
        return self.ring[s][:, idx]

    def histories(self):
        return np.stack([self.history(s) for s in range(self.ring.shape[0])])

    def window(self, w):
        """float32 [streams, channels, w]: the newest w frames of every stream"""
        return self.histories()[:, :, self.ring_cap - w:]


# ---- the stagger plan -------------------------------------------------------------------------------------------------------------

def overlong(case):
    """frames of stream 6's long packet: ring_cap + 77 and as many hops of 256 frames as it takes to end stream 6, modulo the ring,
    in a hop of the sonogram's grid that no other stream ends in -- there its columns, not the `newest` word alone, tell it from
    every neighbour"""
    hop, ring = 256, case.ring_cap
    for extra in range(0, ring, hop):
        c = _counters(case, _steps(case, ring + OVERLONG + extra))
        if (c[6] % ring) // hop not in ((c[:6] % ring) // hop).tolist():
            return ring + OVERLONG + extra
    raise AssertionError("no free hop")


def plan(case):
    """the steps of the case as frame counts (_steps), stream 6's long packet sized by overlong()"""
    return _steps(case, overlong(case))


def _steps(case, long_packet):
    """the steps as frame counts: ("push", first, count, n) | ("ragged", counts[STREAMS]) | ("reset", first, count) | ("read", tag).

    The common script is one ring and a half of uneven odd packets (sono_ref.packets), handed over in turn by a whole-batch
    push_audio, one push_audio(first=s) per stream, one ragged push, and three push_audio to sub-ranges.  On top of it:
      stream 0  nothing
      stream 1, 2, 3  1, 2, 3 leading frames: with stream 0 all four classes of start & 3
      stream 4  ring_cap / 2 + 129 leading frames: its windows wrap the ring where its neighbours' do not
      stream 5  reset before the last three packets: 389 frames behind zeros, fewer than the shortest window
      stream 6  one packet of overlong(case) > ring_cap frames, and a count of 0 in the first ragged push
    A read follows every sixth packet, the long packet, the reset and the end."""
    ring, w0 = case.ring_cap, case.wpos0
    assert sum(TAIL) < SHORTEST_WINDOW
    # streams 0 .. 3 end at ring / 2 + 254 + s past a whole ring: their windows lie flat, and the hop grid of sono and onset (256)
    # runs between streams 1 and 2, where 1, 2 or 3 frames more would otherwise read the very same columns
    target = ring + ring // 2 + 254 - w0
    sizes = [hi - lo for lo, hi in sono_ref.packets(np.random.default_rng(SEED + ring + w0), target - sum(TAIL))]
    steps = [("push", 1, 1, 1), ("push", 2, 1, 2), ("push", 3, 1, 3), ("push", 4, 1, ring // 2 + 129)]
    ragged_seen = 0

    def common(path, n):
        nonlocal ragged_seen
        if path == 0:
            return [("push", 0, STREAMS, n)]
        if path == 1:
            return [("push", s, 1, n) for s in range(STREAMS)]
        if path == 2:
            counts = [n] * STREAMS
            if ragged_seen == 0:
                counts[6] = 0
            ragged_seen += 1
            return [("ragged", tuple(counts))]
        return [("push", 0, 2, n), ("push", 2, 3, n), ("push", 5, 2, n)]

    for i, n in enumerate(sizes):
        steps += common(i % 4, n)
        if i == len(sizes) // 3:
            steps += [("push", 6, 1, long_packet), ("read", "the packet longer than the ring")]
        elif i % 6 == 5:
            steps.append(("read", f"packet {i}"))
    steps += [("reset", 5, 1), ("read", "the reset of stream 5")]
    for j, n in enumerate(TAIL):
        steps += common((0, 2, 1)[j], n)  # whole batch, ragged, per stream
    steps.append(("read", "the end"))
    return steps


AGED = 3  # the stream tests/measure_stagger_wrap_child.py carries across 2^32 alone


def wrap_plan(case):
    """the plan without its reads, then ("age", AGED, 1, 2^32 - 2 ring_cap) -- one stream of the seven -- and whole-batch hops by
    wrap_child.Schedule across the point where that stream's counter overflows, with a read from just before it on.  Returns
    (steps, wrap): `wrap` frames of hops bring the aged counter to 0"""
    from wrap_child import HOPS, Schedule
    steps = [st for st in plan(case) if st[0] != "read"]
    amount = (1 << 32) - 2 * case.ring_cap
    wrap = int(-(int(final_counters(case)[AGED]) + amount) % (1 << 32))
    sch = Schedule(wrap + case.W, case.W, 0, big=case.ring_cap // 2, fine=True)
    sch.check([0])
    steps.append(("age", AGED, 1, amount))
    T = 0
    for n in sch.pushes:
        steps.append(("push", 0, STREAMS, n))
        T += n
        if T >= wrap - sum(HOPS):
            steps.append(("read", T - wrap))
    return steps, wrap


def totals(steps):
    """frames every stream receives over the steps"""
    t = np.zeros(STREAMS, np.int64)
    for st in steps:
        if st[0] == "push":
            t[st[1]:st[1] + st[2]] += st[3]
        elif st[0] == "ragged":
            t += np.asarray(st[1])
    return t


def final_counters(case):
    """by arithmetic, with no ring: where every stream's counter stands at the end of the plan"""
    return _counters(case, plan(case))


def _counters(case, steps):
    c = np.full(STREAMS, case.wpos0, np.int64)
    for st in steps:
        if st[0] == "push":
            c[st[1]:st[1] + st[2]] += st[3]
        elif st[0] == "ragged":
            c += np.asarray(st[1])
        elif st[0] == "reset":
            c[st[1]:st[1] + st[2]] = case.wpos0
    return c


# ---- each output's own signals ----------------------------------------------------------------------------------------------------

GONIO_KINDS = ("noise", "correlated", "lissajous", "quiet", "loud", "half", "antiphase")
BITS_KINDS = ("s16", "gap", "two_runs", "float", "run_first", "run_last", "stuck")  # channel 0; channel 1 the next of bits_ref.KINDS
# (one clean sine: its sfdr_db is one bin at -172 dBc, which two orderings of the transform place within 1e-7 dB of each other for
# most windows only -- thd_ref.GPU_SEED's comment -- and here every read of every case has to)
THD_KINDS = (("tone", "square"), ("square", "tone"), ("sine", "high"), ("high", "tone"), ("silence", "tone"), ("tone", "silence"),
             ("tone", "high"))
DELAY_KINDS = ("white +3", "white -7.3", "inverted L-1", "-100 dB +11", "tones +2.25", "dual mono", "independent")
SONO_KINDS = tuple(sono_ref.KINDS[s % 3] for s in range(STREAMS))   # noise, burst, chirp, noise, ...
ONSET_KINDS = tuple(onset_ref.KINDS[s % 3] for s in range(STREAMS))
SIGNAL_SCALES = (0.01, 0.5, 1.0, 1.2, 0.5, 1.0, 0.01)
# where the first seed left a window of some read outside a condition of its module's bound (test_measure_stagger_cpu.py prints
# the margins), the next seeds were tried in order: (output, case) -> how many were passed over
SEED_STEPS = {("thd", "fft1024"): 3, ("delay", "meter"): 1}


def silent(output, case, s):
    """the streams whose every captured channel is silence: a shift of silence cannot be seen"""
    return output == "thd" and all(k == "silence" for k in THD_KINDS[s][:case.channels])


def audio(output, case, frames):
    """the output's own signal kinds: a list of float32 [channels, frames[s]] per stream, each built for its own length, so that
    what a kind places against the end of the window (bits' runs, delay's pairs, the bursts of sono and onset) lies against
    that stream's own end"""
    ch, W, sr, ring = case.channels, case.W, case.sr, case.ring_cap
    rng = np.random.default_rng(SEED + OUTPUTS.index(output) * 1000 + case.W + 100000 * SEED_STEPS.get((output, case.name), 0))
    longest = int(max(frames))
    out = []
    if output in ("pitch", "stereo", "cq", "scope"):  # generators of a whole bank: every stream keeps the newest of its row
        if output == "pitch":
            bank = pitch_cases.bank(int(rng.integers(1 << 30)), STREAMS, ch, longest, sr)
        elif output == "stereo":
            bank = stereo_ref.audio(rng, STREAMS, longest, sr)
        elif output == "cq":
            bank = cq_ref.audio(rng, STREAMS, longest, sr)[:, :ch]
        else:
            bank = scope_ref.audio(rng, STREAMS, longest, W)[:, :ch]
        return [np.ascontiguousarray(bank[s, :, longest - int(frames[s]):]) for s in range(STREAMS)]
    for s in range(STREAMS):
        n = int(frames[s])
        if output == "signal":
            x = rng.uniform(-SIGNAL_SCALES[s], SIGNAL_SCALES[s], (ch, n)).astype(np.float32)
        elif output == "gonio":
            x = gonio_ref.signal(GONIO_KINDS[s], rng, n)
        elif output == "bits":
            k = BITS_KINDS[s]
            pair = (k, bits_ref.KINDS[(bits_ref.KINDS.index(k) + 1) % len(bits_ref.KINDS)])
            x = np.stack([bits_ref.signal(kk, rng, n, bits_ref.window_frames(W)) for kk in pair[:ch]])
        elif output == "thd":
            x = np.stack([thd_ref.signal(k, rng, n, thd_ref.window_frames(W)) for k in THD_KINDS[s][:ch]])
        elif output == "delay":
            x = delay_ref.stream(DELAY_KINDS[s], rng, n, delay_ref.window_frames(W))
        elif output == "sono":
            x = sono_ref.signal(SONO_KINDS[s], rng, n, ch, (sono_ref.columns(ring) - 1) * sono_ref.H + sono_ref.P)
        elif output == "onset":
            x = onset_ref.signal(ONSET_KINDS[s], rng, n, ch, onset_ref.columns(ring) * onset_ref.H + onset_ref.P)
        else:
            raise ValueError(output)
        assert x.shape == (ch, n) and x.dtype == np.float32
        out.append(x)
    return out


def script(case, output, steps=None):
    """the plan with the output's audio in it: ("push", first, x [count, channels, n]) | ("ragged", x [STREAMS, channels, widest],
    counts) | ("reset", first, count) | ("read", tag).  Every stream's frames come from its own signal, in order"""
    steps = plan(case) if steps is None else steps
    src = audio(output, case, totals(steps))
    at = [0] * STREAMS
    out = []

    def take(s, n):
        x = src[s][:, at[s]:at[s] + n]
        assert x.shape[1] == n
        at[s] += n
        return x

    for st in steps:
        if st[0] == "push":
            _, first, count, n = st
            out.append(("push", first, np.stack([take(s, n) for s in range(first, first + count)])))
        elif st[0] == "ragged":
            counts = np.asarray(st[1], np.uint32)
            x = np.zeros((STREAMS, case.channels, int(counts.max())), np.float32)
            for s in range(STREAMS):
                x[s, :, :int(counts[s])] = take(s, int(counts[s]))
            out.append(("ragged", x, counts))
        else:
            out.append(st)
    assert at == [a.shape[1] for a in src]
    return out


def replay(steps, rings=None, batches=(), on_read=None, pinned=None, ragged=True, on_age=None):
    """plays a script into a Rings and into every batch of `batches`; on_read(index, tag) at every read.  pinned: a factory of
    PinnedBuffer for the ragged pushes; ragged=False feeds those steps per stream with push_audio(first=s) instead (a MultiBatch
    has no ragged push); on_age(first, count, frames) ages the handles of wrap_plan's step"""
    reads = 0
    for st in steps:
        if st[0] == "push":
            _, first, x = st
            if rings is not None:
                rings.push(x, first=first)
            for b in batches:
                b.push_audio(x, first=first)
        elif st[0] == "ragged":
            _, x, counts = st
            if rings is not None:
                rings.push(x, frames=counts)
            for b in batches:
                if ragged:
                    pin = pinned(x.shape)
                    try:
                        b.ingest_done(0)
                        pin.array[...] = x
                        b.push_audio_ragged_async(pin, counts, x.shape[2], 0)
                        b.sync()
                    finally:
                        pin.close()
                else:
                    for s in range(STREAMS):
                        if counts[s]:
                            b.push_audio(np.ascontiguousarray(x[s:s + 1, :, :int(counts[s])]), first=s)
        elif st[0] == "reset":
            if rings is not None:
                rings.reset(st[1], st[2])
            for b in batches:
                b.reset(st[1], st[2])
        elif st[0] == "age":
            if rings is not None:
                rings.age(st[1], st[2], st[3])
            if on_age is not None:
                on_age(st[1], st[2], st[3])
        else:
            if on_read is not None:
                on_read(reads, st[1])
            reads += 1
    return reads


# ---- every output's own restatement, comparison and conditions ----------------------------------------------------------------------

def signal_struct(want):
    """signal_ref.signal's dict as [streams] of wf_hip_signal"""
    from waveform_amd import binding
    out = np.zeros(len(want["correlation"]), binding.SIGNAL_DTYPE)
    for name in ("rms_db", "peak_db", "dc", "clipped"):
        out["ch"][name] = want[name]
    for name in ("correlation", "balance_db", "mid_db", "side_db"):
        out[name] = want[name]
    return out


def restate(output, case, hist, wpos):
    """[streams] of the output's struct from hist, float32 [streams, channels, ring_cap] (Rings.history, the counter at its end),
    and the counters wpos [streams]"""
    hist = np.asarray(hist, np.float32)
    W, sr, ring = case.W, case.sr, case.ring_cap
    if output == "signal":
        return signal_struct(signal_ref.signal(hist[..., ring - W:]))
    if output == "pitch":
        return pitch_ref.pitch(hist[..., ring - pitch_ref.window_frames(W):], sr)
    if output == "stereo":
        return stereo_ref.stereo(hist[..., ring - W:], sr)
    if output == "cq":
        return cq_ref.cq(hist, sr, ring)
    if output == "scope":
        return scope_ref.scope(hist, W)
    if output == "gonio":
        return gonio_ref.gonio(hist, W)
    if output == "bits":
        return bits_ref.bits(hist, W)
    if output == "thd":
        return thd_ref.thd(hist, W, sr)
    if output == "delay":
        return delay_ref.delay(hist, W, sr)
    if output == "sono":
        return sono_ref.sono(hist, wpos, sr, ring)
    if output == "onset":
        return onset_ref.onset(hist, wpos, sr, ring)
    raise ValueError(output)


def mismatches(output, case, got, hist, wpos):
    """everything in `got` ([streams] of the output's struct) beyond the output's own bound of the restatement of hist and wpos: the
    list of that module's own comparison"""
    hist = np.asarray(hist, np.float32)
    W, sr, ring = case.W, case.sr, case.ring_cap
    if output == "signal":
        return signal_ref.mismatches(got, signal_ref.signal(hist[..., ring - W:]))
    if output == "pitch":
        want, well = pitch_ref.evaluate(hist[..., ring - pitch_ref.window_frames(W):], sr)
        idx, _ = pitch_ref.compare(got, want, well)
        return [("pitch", int(i), got[i].tolist(), want[i].tolist()) for i in idx]
    if output == "stereo":
        return stereo_ref.mismatches(got, stereo_ref.stereo(hist[..., ring - W:], sr))
    if output == "cq":
        return cq_ref.mismatches(got, hist, sr, ring)
    if output == "scope":
        return scope_ref.mismatches(got, hist, W)
    if output == "gonio":
        return gonio_ref.mismatches(got, hist, W)
    if output == "bits":
        return bits_ref.mismatches(got, hist, W)
    if output == "thd":
        return thd_ref.mismatches(got, thd_ref.thd(hist, W, sr))
    if output == "delay":
        return delay_ref.mismatches(got, delay_ref.delay(hist, W, sr))
    if output == "sono":
        return sono_ref.mismatches(got, hist, wpos, sr, ring)[0]
    if output == "onset":
        return onset_ref.mismatches(got, hist, wpos, sr, ring)[0]
    raise ValueError(output)


def first_arm_only(case, s):
    """the sonogram's noise streams: every live cell must pass by the first arm (tests/test_gpu_sono.py holds its noise stream to
    the same)"""
    return SONO_KINDS[s] == "noise"


def conditions(output, case, x, wpos, s):
    """the conditions the output's bound rests on, for one stream's history x [channels, ring_cap] and counter: a list of
    (what, figure, holds).  The thresholds are those of tests/test_thd_cpu.py, test_delay_cpu.py, test_onset_cpu.py,
    test_sono_cpu.py and test_pitch_cpu.py; the outputs held bit for bit, or by a bound that names its own exceptions (cq, stereo,
    signal), have none"""
    W, sr, ring = case.W, case.sr, case.ring_cap
    res = []
    if output == "thd":
        p = thd_ref.window_frames(W)
        for c in range(case.channels):
            w = x[c, ring - p:]
            r, vals = thd_ref.analyse(w, sr)
            _, other = thd_ref.analyse(w, sr, thd_ref.fft_radix2)
            if not vals:
                res.append((f"ch {c} invalid in both orderings", 0.0, not other))
                continue
            res.append((f"ch {c} margin k0", vals["margin_k0"], vals["margin_k0"] >= 1e-6))
            res.append((f"ch {c} margin ks", vals["margin_ks"], vals["margin_ks"] >= 1e-6))
            res.append((f"ch {c} margin half-integer", vals["margin_half"], vals["margin_half"] >= 1e-6))
            worst, same = 0.0, bool(other) and other["harmonic_bins"] == vals["harmonic_bins"]
            for name in thd_ref.DB_FIELDS:
                u, v = np.atleast_1d(vals[name]), np.atleast_1d(other[name]) if other else np.atleast_1d(np.nan)
                same = same and np.array_equal(np.isinf(u), np.isinf(v)) and not np.isnan(u).any()
                fin = np.isfinite(u) & np.isfinite(v)
                if fin.any():
                    worst = max(worst, float(np.max(np.abs(u[fin] - v[fin]))))
            res.append((f"ch {c} two orderings, dB", worst, same and worst <= 1e-7))
    elif output == "delay":
        p = delay_ref.window_frames(W)
        a, b = x[0, ring - p:], x[1, ring - p:]
        r, vals = delay_ref.analyse(a, b, sr)
        worst = 0.0
        ok = True
        for o in delay_ref.ORDERS[1:]:
            q = delay_ref.analyse(a, b, sr, o)[0]
            ok = ok and not delay_ref.mismatches(np.array([q]), np.array([r]), float_tol=1e-9)
            worst = max(worst, max(delay_ref.worst(np.array([q]), np.array([r])).values()))
        res.append(("four orders", worst, ok))
        if vals:
            res.append(("margin argmax", vals["margin_argmax"], vals["margin_argmax"] >= 1e-3))
            res.append(("margin pi", vals["margin_pi"], vals["margin_pi"] >= 1e-6))
            res.append(("margin clamp", abs(abs(vals["f_raw"]) - 0.5), abs(abs(vals["f_raw"]) - 0.5) >= 1e-6))
    elif output == "onset":
        m = onset_ref.margins(onset_ref.strengths(x[None], int(wpos), sr, ring))
        res.append(("margin of the decisions, ulps", m, m >= 4.0))
    elif output == "sono":
        if first_arm_only(case, s):
            arm2 = sono_ref.mismatches(sono_ref.sono(x[None], int(wpos), sr, ring), x[None], int(wpos), sr, ring)[1]
            res.append(("cells by the second arm", float(arm2[0]), arm2[0] == 0))
    elif output == "pitch":
        _, well = pitch_ref.evaluate(x[None, :, ring - pitch_ref.window_frames(W):], sr)
        res.append(("well conditioned", float(well[0]), bool(well[0])))
    return res
