"""TEST HARNESS (child of tests/test_gpu_fullsize.py::test_sample_counters_wrap_at_2_to_the_32 and of tests/test_gpu_wrap.py): runs
against the DEVELOPMENT build of the library (libwaveform_hip_dev.so via WF_HIP_LIB -- the release library does not export
wf_hip_debug_age).

Every kind runs twin handles: `old` has had its 32-bit sample counters moved to just below 2^32 (wf_hip_debug_age), `fresh` has
not; both are fed the same audio and must produce the same bits at every step while old's counters overflow.  The new kinds share
one schedule (Schedule): an approach in large pushes, then small hops with a tick after each through the three places where the
overflow can show -- the window straddling position 2^32 (0 < wpos < N), the exact hit (wpos = N: the window starts at
position 0) and the whole stretch wpos - N < A/V-sync delay, where only WF_STREAM_WRAPPED tells "wrapped" from "not enough audio
yet".  Each kind asserts by arithmetic on its own schedule that those positions occurred.

usage: python tests/wrap_child.py spectrum_normalize|meter|spectrum_delay_<fft>|push_paths|reset_after_wrap|meter_delay|rms_feed|
                                  waveform|measure"""
import contextlib
import os
import sys

import numpy as np

if len(sys.argv) > 1 and sys.argv[1] == "push_paths":
    import torch  # noqa: F401  (wf_hip_push_audio_device: torch brings its own HIP runtime and has to come before libwaveform_hip.so)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import waveform_amd as wf  # noqa: E402
from tools import synth  # noqa: E402

SEED = synth.DEFAULT_SEED


def run(kind):
    if kind == "meter":
        cfg = wf.Config.defaults(meter=1, meter_rms=1, meter_ms=150)
    else:
        cfg = wf.Config.defaults(fft_size=2048, stereo=1, slope=1.0, normalize_volume=1, bars=1, interp_mode=wf.INTERP["lanczos"])
    streams, ring = 3, 1 << 17
    push = 60000 if kind != "meter" else 6000
    pushes = 50 if kind != "meter" else 40
    rings_left = 8 if kind != "meter" else 1
    age = (1 << 32) - rings_left * ring  # the wrap falls inside the run
    L = wf.lib()
    assert hasattr(L, "wf_hip_debug_age"), "needs the development build (WF_HIP_LIB=waveform_amd/libwaveform_hip_dev.so)"
    with wf.SpectrumBatch(cfg, streams, ring_frames=ring) as fresh, wf.SpectrumBatch(cfg, streams, ring_frames=ring) as old:
        if kind != "meter":
            fresh.enable_input_rms()
            old.enable_input_rms()
        assert L.wf_hip_debug_age(old.h, 0, streams, age) == 0, L.wf_hip_last_error(old.h)
        total = 0
        for i in range(pushes):
            a = synth.block(SEED, 0, streams, fresh.capture_channels, i * push, push) * np.float32(0.05 if i % 7 else 0.8)
            for b in (fresh, old):
                b.push_audio(a)
                b.tick()
            total += push
            if kind == "meter":
                assert np.array_equal(fresh.meter(), old.meter()), f"push {i}: levels differ"
            else:
                assert np.array_equal(fresh.decibels(), old.decibels()), f"push {i}: rows differ ({total} frames in, wrap at {rings_left * ring})"
                assert np.array_equal(fresh.input_rms(), old.input_rms()), f"push {i}: m_input_rms differs"
            assert np.array_equal(fresh.bars(), old.bars()) and np.array_equal(fresh.last_silent(), old.last_silent())
        assert total > rings_left * ring + 4 * push


# ---- the common schedule of the kinds below ------------------------------------------------------------------------------------

HOPS = (800, 441, 37)                 # sum 1278: a video frame at 60 Hz, one at 44.1 kHz's rate, a scrap
TICK_DELAY = 960                      # TickParams.delay_frames of every tick
STREAM_DELAYS = (0, 441, 1443)        # wf_hip_set_stream_delay: aligned and unaligned, the streams' danger windows differ
RMS_SIZE, RMS_BLOCK = 48000, 256      # m_input_rms_size at 48 kHz, csrc/wf_rms.hpp


def _pow2(n):
    return 1 << (int(n) - 1).bit_length()


def _ring_for(n):
    """the smallest ring a spectrum batch of fft size n admits with every delay of this file"""
    return _pow2(max(2 * n, n + TICK_DELAY + max(STREAM_DELAYS)))


def _rms_cap(ring, n, feed=False):
    """the capacity of the device RMS producer's ring (enable_rms_producer, csrc/wf_hip.hip): wf_hip_debug_age wants a multiple"""
    return _pow2(2 * RMS_SIZE + 2 * RMS_BLOCK) if feed else _pow2(RMS_SIZE + ring - n + 2 * RMS_BLOCK)


class Schedule:
    """The frames of every push; a tick follows each.  R: the pushed frames after which an aged stream's wpos is w0 + win again
    modulo 2^32 (spectrum batches: w0 = win = N, so wpos = N + T - R); the aged wpos is 0 at T = R - win.  Small hops around
    T = R - win, through (R - win, R) -- all of it when `fine`, else its two ends with large pushes in between --, and from
    T = R in hops of 37 and 441 until every stream's delay has passed; then three ordinary hops."""

    def __init__(self, R, win, max_delay, big, fine=False):
        self.R, self.win = R, win
        self.pushes = []
        self.T = 0
        cycle = sum(HOPS)
        assert R - win > cycle, (R, win)
        self._big_to(R - win - cycle, big)
        self._hops(HOPS)                                   # -> T = R - win: wpos = 0
        assert self.T == R - win
        if fine or win < 3 * cycle:
            while R - self.T > cycle:
                self._hops(HOPS[::-1])
            for h in HOPS[::-1]:
                if h < R - self.T:
                    self._hops((h,))
            self._hops((R - self.T,))
        else:
            self._hops(HOPS[::-1])
            self._big_to(R - cycle, big)
            self._hops(HOPS)
        assert self.T == R                                  # the exact hit
        while self.T <= R + max_delay + HOPS[2]:
            self._hops((37, 441))
        self._hops((800, 441, 800))
        self.ticks = np.cumsum(self.pushes)                 # T at every tick

    def _hops(self, hops):
        for h in hops:
            self.pushes.append(int(h))
            self.T += int(h)

    def _big_to(self, target, big):
        while self.T < target:
            self._hops((min(big, target - self.T),))

    def danger(self, delay):
        """the ticks at which only WF_STREAM_WRAPPED keeps a stream of this delay from underflowing: 0 <= wpos - N < delay"""
        return (self.ticks >= self.R) & (self.ticks < self.R + delay)

    def check(self, delays):
        """the coverage the kinds rely on, by arithmetic: a schedule that misses the wrap fails here"""
        t, R, win = self.ticks, self.R, self.win
        assert np.any(t == R - win), "no tick at wpos = 0"
        assert np.any((t > R - win) & (t < R)), "no tick with the window straddling 2^32"
        assert np.any(t == R), "no tick at the exact hit"
        assert t[-1] > R + max(delays) + 2 * HOPS[0], "the run ends before every stream has recovered"
        assert set(HOPS) <= set(self.pushes)
        for d in delays:
            if d:
                assert np.count_nonzero(self.danger(d)) >= 3, f"delay {d}: fewer than 3 ticks in [R, R + delay)"
                if win >= 512:  # (hops of at most 441 cannot step over it) the DELAYED window straddles 2^32 as well
                    assert np.any((t > R + d - win) & (t < R + d)), f"delay {d}: the delayed window never straddles 2^32"


def _dev():
    L = wf.lib()
    assert hasattr(L, "wf_hip_debug_age"), "needs the development build (WF_HIP_LIB=waveform_amd/libwaveform_hip_dev.so)"
    return L


def _age(L, old, R):
    assert R % old.ring_frames == 0, (R, old.ring_frames)
    rc = L.wf_hip_debug_age(old.h, 0, old.streams, (1 << 32) - R)
    assert rc == 0, L.wf_hip_last_error(old.h)


@contextlib.contextmanager
def twins(cfg, streams, ring, fft, R=None, win=None):
    """The twins of the children of the measurement outputs (tests/<out>_wrap_child.py): spectrum batches `fresh` and `old` of this
    ring and fft size, old's write positions aged by 2^32 - 2 rings.  A spectrum batch's wpos starts at fft (the zeros of create), so
    the aged wpos is 0 after wrap = 2 rings - fft pushed frames.  With R and win, the fine Schedule of them, checked, else None."""
    L = _dev()
    with wf.SpectrumBatch(cfg, streams, ring_frames=ring) as fresh, wf.SpectrumBatch(cfg, streams, ring_frames=ring) as old:
        assert old.ring_frames == ring and old.fft_size == fft
        sch = None
        if R is not None:
            sch = Schedule(R, win, 0, big=ring // 2, fine=True)
            sch.check([0])
        assert L.wf_hip_debug_age(old.h, 0, streams, (1 << 32) - 2 * ring) == 0, L.wf_hip_last_error(old.h)
        yield fresh, old, sch


def slices(audio):
    """the audio of a push, for a child that draws one long run and cuts it"""
    return lambda i, T, p: np.ascontiguousarray(audio[:, :, T:T + p])


class Walk:
    """The twins' walk across the wrap.  Iterating it pushes audio(i, T, p) -- the child's audio of push i, p frames behind the T
    pushed so far -- to both twins and yields (i, T, what) behind every push that is read, T counting that push: every one from
    sum(HOPS) frames before the wrap on, or, where `pushes` holds (frames, read), those it marks.  `hist`, where given (the zeros
    of create), is kept as the newest frames of that length.  It counts the reads with the aged wpos = T - wrap at or before
    2^32 (`before`; `at`: those of them at it exactly), with the span read across it (`straddling`), starting at position 0
    exactly (`exact`) and behind it (`behind`); which of them a child needs, and how many, it asserts itself."""

    def __init__(self, both, pushes, wrap, span, audio, hist=None):
        self.both, self.pushes, self.wrap, self.span, self.audio, self.hist = both, pushes, wrap, span, audio, hist
        self.T = self.before = self.at = self.straddling = self.exact = self.behind = 0

    @property
    def counts(self):
        return self.before, self.straddling, self.exact, self.behind

    def __iter__(self):
        for i, p in enumerate(self.pushes):
            p, read = p if isinstance(p, tuple) else (p, None)
            a = self.audio(i, self.T, p)
            self.T = T = self.T + p
            for b in self.both:
                b.push_audio(a)
            if self.hist is not None:
                self.hist = np.concatenate([self.hist, a], axis=2)[:, :, -self.hist.shape[2]:]
            if (T < self.wrap - sum(HOPS)) if read is None else not read:
                continue
            d = T - self.wrap
            self.before += int(d <= 0)
            self.at += int(d == 0)
            self.straddling += int(0 < d < self.span)
            self.exact += int(d == self.span)
            self.behind += int(d > self.span)
            yield i, T, f"read {i} at wpos = 2^32{d:+d}"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(fresh, old, what, names):
    for n in names:
        a, b = getattr(fresh, n)(), getattr(old, n)()
        assert np.array_equal(_bits(a), _bits(b)), f"{what}: {n} differs, first at stream {int(np.argwhere(np.any((a != b).reshape(len(a), -1), axis=1))[0][0])}"


SPECTRUM_OUTPUTS = ("decibels", "bars", "last_silent", "tsmooth", "input_rms")


def _spectrum_cfg(n, **kw):
    return wf.Config.defaults(**{**dict(fft_size=n, stereo=1, slope=1.0, normalize_volume=1, bars=1, interp_mode=wf.INTERP["lanczos"]), **kw})


def _audio(streams, channels, t0, n, s16_exact=False):
    a = synth.block(SEED, 0, streams, channels, t0, n) * np.float32(0.5)
    if s16_exact:  # floats that a 16-bit packet holds exactly (x * 2^-15)
        a = np.round(a * np.float32(32768.0)).astype(np.int16).astype(np.float32) * np.float32(2.0 ** -15)
    return a


def _alive(b, s, what):
    """stream s shows audio: a stream that skipped its channels (rows left at DB_MIN) on both handles must not pass"""
    rows = b.decibels(s, 1)
    assert not np.all(rows == np.float32(wf.db_min())), f"{what}: stream {s}'s rows are all DB_MIN"
    assert not b.last_silent(s, 1)[0], f"{what}: stream {s} is marked silent"


# which kernel family a geometry is there for, as a part of kernel_name()
GEOMETRIES = {
    512: ("spectrum_tick_kernel<N=512,", None),                       # small power of two inside LDS
    800: ("mixed radix", "N=800:"),                                   # mixed radix
    1120: ("mixed radix", "N=1120:"),                                 # 560 = 7 x 5 x 16 points: mixed radix with a radix-7 pass
    2096: ("by Bluestein over", "N=2096 "),                           # 1048 = 8 x 131 points: Bluestein inside LDS
    4096: ("spectrum_tick_kernel<N=4096,", None),                     # the headline geometry and its prologue
    8192: ("spectrum_tick_kernel<N=8192,", "split"),                  # split: the stream flags rotate through three buffers
    32768: ("spectrum_tick_kernel<N=32768,", "split"),                # one spectrum per workgroup
    65536: ("big_whole_kernel<N=65536", None),                        # wf_big.hpp: its own underflow test and flag carry
    16400: ("big_br_{columns,rows}_kernel", "N=16400:"),              # wf_big.hpp, rows by Bluestein
    32000: ("big_mr_", "N=32000:"),                                   # wf_big.hpp, mixed-radix rows
}


def run_spectrum_delay(n):
    L = _dev()
    head, also = GEOMETRIES[n]
    streams = len(STREAM_DELAYS)
    ring = _ring_for(n)
    R = max(ring, _rms_cap(ring, n))
    cfg = _spectrum_cfg(n)
    delays = [TICK_DELAY + d for d in STREAM_DELAYS]
    sch = Schedule(R, n, max(delays), big=max(ring, 16384))
    sch.check(delays)
    with wf.SpectrumBatch(cfg, streams, ring_frames=ring) as fresh, wf.SpectrumBatch(cfg, streams, ring_frames=ring) as old:
        name = old.kernel_name()
        assert head in name and (also is None or also in name), (n, name)
        assert old.ring_frames == ring and old.fft_size == n
        for b in (fresh, old):
            b.enable_input_rms()
            b.set_stream_delay(np.array(STREAM_DELAYS, np.uint32))
        _age(L, old, R)
        T, seen = 0, 0
        for i, p in enumerate(sch.pushes):
            a = _audio(streams, 2, T, p)
            T += p
            for b in (fresh, old):
                b.push_audio(a)
                b.tick(delay_frames=TICK_DELAY)
            what = f"fft {n}, tick {i} at T = R{T - R:+d} (R = {R})"
            _same(fresh, old, what, SPECTRUM_OUTPUTS)
            for s, d in enumerate(delays):
                if R <= T < R + d:
                    _alive(old, s, what)
                    seen += 1
        assert T == sch.ticks[-1] and seen >= 3 * streams


# ---- every push path ---------------------------------------------------------------------------------------------------------

def run_push_paths():
    L = _dev()
    n, streams = 1024, len(STREAM_DELAYS)
    ring = _ring_for(n)
    delays = [TICK_DELAY + d for d in STREAM_DELAYS]
    R = _rms_cap(ring, n)  # (the muted pair runs the RMS producer; the same R for every pair, so that their rows can be compared)
    sch = Schedule(R, n, max(delays), big=16384)
    sch.check(delays)
    # the ragged paths deliver every hop in two pushes: stream s gets the first split[s] frames, then the rest; the splits differ, so
    # the streams wrap in different pushes, and stream 0 gets nothing (frames[i] == 0) in the first of them
    splits = (0.0, 0.4, 1.0)
    wrap_push = int(np.searchsorted(sch.ticks, R - n))  # the hop that takes wpos past 2^32 (it ends at wpos = 0 exactly)
    assert sch.ticks[wrap_push] == R - n

    def counts_of(p):
        return np.array([int(p * f) for f in splits], np.uint32)

    def ragged(b, a, p, push):
        first = counts_of(p)
        for cnt, off in ((first, np.zeros(streams, np.uint32)), (np.uint32(p) - first, first)):
            if cnt.any():
                push(b, a, cnt, off, int(cnt.max()))

    def ragged_float(b, a, cnt, off, mx):
        pin = wf.PinnedBuffer((streams, 2, mx))
        pin.array[...] = 0
        for s in range(streams):
            pin.array[s, :, :cnt[s]] = a[s, :, off[s]:off[s] + cnt[s]]
        b.push_audio_ragged_async(pin, cnt, mx, 0)
        b.sync()
        pin.close()

    def ragged_pcm(b, a, cnt, off, mx):
        pin = wf.PinnedBuffer((streams, mx, 2), np.int16)
        pin.array[...] = 0
        for s in range(streams):
            pin.array[s, :cnt[s]] = np.round(a[s, :, off[s]:off[s] + cnt[s]].T * np.float32(32768.0)).astype(np.int16)
        b.push_pcm(pin, interleaved=True, frames=cnt, slot=1)
        b.sync()
        pin.close()

    def to_s16(a):
        return np.ascontiguousarray(np.round(a * np.float32(32768.0)).astype(np.int16).transpose(0, 2, 1))

    def device(b, a, p):
        d = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        torch.cuda.synchronize()
        b.push_audio_device(d.data_ptr(), streams, p)
        b.sync()

    paths = {
        "blocking": lambda b, a, p, i, T: b.push_audio(a),
        "ragged_float": lambda b, a, p, i, T: ragged(b, a, p, ragged_float),
        "ragged_pcm": lambda b, a, p, i, T: ragged(b, a, p, ragged_pcm),
        "host_pcm": lambda b, a, p, i, T: b.push_pcm(to_s16(a), interleaved=True),
        "device": lambda b, a, p, i, T: device(b, a, p),
        "synth": lambda b, a, p, i, T: b.push_synth(SEED, T, p),
        # two hops in three are muted packets: zeros into the rings, the samples into the RMS producer -- the wrapping hop among them
        "muted": lambda b, a, p, i, T: b.push_audio(a) if (i - wrap_push) % 3 == 1 else b.push_audio_muted(a),
    }
    torch.cuda.set_device(0)
    results = {}
    for path, push in paths.items():
        rms = path == "muted"
        outputs = SPECTRUM_OUTPUTS if rms else SPECTRUM_OUTPUTS[:-1]
        cfg = _spectrum_cfg(n, normalize_volume=1 if rms else 0)
        with wf.SpectrumBatch(cfg, streams, ring_frames=ring) as fresh, wf.SpectrumBatch(cfg, streams, ring_frames=ring) as old:
            for b in (fresh, old):
                if rms:
                    b.enable_input_rms()
                b.set_stream_delay(np.array(STREAM_DELAYS, np.uint32))
            _age(L, old, R)
            T, rows, seen = 0, [], 0
            for i, p in enumerate(sch.pushes):
                a = _audio(streams, 2, T, p, s16_exact=True)
                for b in (fresh, old):
                    push(b, a, p, i, T)
                    b.tick(delay_frames=TICK_DELAY)
                T += p
                what = f"{path}, tick {i} at T = R{T - R:+d}"
                _same(fresh, old, what, outputs)
                if T > R - n - sum(HOPS):
                    rows.append((old.decibels(), old.bars(), old.last_silent()))
                for s, d in enumerate(delays):
                    if R <= T < R + d and not rms:
                        _alive(old, s, what)
                        seen += 1
            assert rms or seen >= 3 * streams
            results[path] = rows
    # the same floats through another entry point: the same rows
    for path in ("ragged_float", "ragged_pcm", "host_pcm", "device"):
        assert len(results[path]) == len(results["blocking"]) > 12
        for k, (got, want) in enumerate(zip(results[path], results["blocking"])):
            for g, w, out in zip(got, want, ("rows", "bars", "last_silent")):
                assert np.array_equal(_bits(g), _bits(w)), f"{path} against blocking, {out} at compared tick {k}"


# ---- wf_hip_reset behind the wrap -----------------------------------------------------------------------------------------------

def run_reset_after_wrap():
    L = _dev()
    n, streams, victim = 1024, 3, 1
    ring = _ring_for(n)
    R = _rms_cap(ring, n)
    sch = Schedule(R, n, TICK_DELAY, big=16384)
    sch.check([TICK_DELAY])
    db_min = np.float32(wf.db_min())
    with wf.SpectrumBatch(_spectrum_cfg(n), streams, ring_frames=ring) as fresh, wf.SpectrumBatch(_spectrum_cfg(n), streams, ring_frames=ring) as old:
        for b in (fresh, old):
            b.enable_input_rms()
        _age(L, old, R)
        T = 0

        def step(p, what):
            nonlocal T
            a = _audio(streams, 2, T, p)
            T += p
            for b in (fresh, old):
                b.push_audio(a)
                b.tick(delay_frames=TICK_DELAY)
            _same(fresh, old, what, SPECTRUM_OUTPUTS)

        for i, p in enumerate(sch.pushes):
            step(p, f"tick {i} at T = R{T + p - R:+d}")
            if T == R + 37 + 441:
                break
        assert T == R + 37 + 441 and T < R + TICK_DELAY  # inside the danger window: the aged victim carries WF_STREAM_WRAPPED
        _alive(old, victim, "before the reset")
        for b in (fresh, old):
            b.reset(victim, 1)
        since = 0
        for p in (441, 441):  # fewer than delay frames since the reset: the stream has not got the audio its delay asks for
            step(p, f"{since + p} frames after the reset")
            since += p
            assert since < TICK_DELAY
            for b in (fresh, old):
                # underflow leaves the channels alone (no transform, the smoothing state stays as the reset left it: zeros) and
                # the end-of-tick dB pass re-dBFSes the stale rows of DB_MIN: DB_MIN + slope + volume compensation (a few tens of
                # dB), hundreds of dB below anything a transform of this audio stores
                assert not b.tsmooth(victim, 1).any(), f"{since} frames after the reset: the reset stream did not underflow (smoothing state moved)"
                assert np.all(b.decibels(victim, 1) < db_min / 2), f"{since} frames after the reset: the reset stream did not underflow"
                assert not b.last_silent(victim, 1)[0]
                for s in range(streams):
                    if s != victim:
                        _alive(b, s, f"{since} frames after the reset")
        for p in (800, 441, 37, 800):
            step(p, f"{since + p} frames after the reset")
            since += p
        assert since > TICK_DELAY + n
        for b in (fresh, old):
            _alive(b, victim, "recovered")
            assert b.tsmooth(victim, 1).any() and np.all(b.decibels(victim, 1) > db_min / 2)


# ---- meter batches ----------------------------------------------------------------------------------------------------------------

def run_meter_delay():
    L = _dev()
    cfg = wf.Config.defaults(meter=1, meter_rms=1, meter_ms=150)
    streams, victim = len(STREAM_DELAYS), 1
    delays = [TICK_DELAY + d for d in STREAM_DELAYS]
    with wf.SpectrumBatch(cfg, streams) as fresh, wf.SpectrumBatch(cfg, streams) as old:
        ring, size = old.ring_frames, old.fft_size  # (a meter batch's fft_size: its meter buffer, 150 ms)
        assert size == 7200
        assert ring >= size + max(delays) and old.kernel_name() == "meter_tick_kernel"
        R = 2 * ring + size  # wpos starts at 0 here: it is 0 again at T = 2 rings, and `size` at T = R
        sch = Schedule(R, size, max(delays), big=ring, fine=True)
        sch.check(delays)
        for b in (fresh, old):
            b.set_stream_delay(np.array(STREAM_DELAYS, np.uint32))
        assert L.wf_hip_debug_age(old.h, 0, streams, (1 << 32) - 2 * ring) == 0, L.wf_hip_last_error(old.h)
        # once mend = wpos - delay of the victim is just past 2^32 (the cleared stretch [mend - size, mend) straddles it): capture
        # timed out, then hidden, then shown again
        at = int(np.searchsorted(sch.ticks, R - size + delays[victim], side="right"))
        assert R - size + delays[victim] < sch.ticks[at] < R - size + delays[victim] + size
        masks = {at: 2, at + 1: 1, at + 2: 0}  # WF_HIP_HIDDEN_TIMEOUT, WF_HIP_HIDDEN, shown
        T, loud = 0, 0
        for i, p in enumerate(sch.pushes):
            a = _audio(streams, old.capture_channels, T, p)
            T += p
            for b in (fresh, old):
                if i in masks:
                    b.set_hidden(np.array([masks[i]], np.uint8), first=victim)
                b.push_audio(a)
                b.tick(delay_frames=TICK_DELAY)
            what = f"tick {i} at T = R{T - R:+d}"
            _same(fresh, old, what, ("meter", "bars", "last_silent"))
            if i in (at, at + 1):
                assert np.all(old.meter(victim, 1) == np.float32(wf.db_min())) and old.last_silent(victim, 1)[0], what
            elif T > R - size:
                loud += int(np.all(old.meter() > np.float32(wf.db_min())))
        assert loud > len(sch.pushes) // 2


# ---- the RMS producer fed by the host -----------------------------------------------------------------------------------------------

def run_rms_feed():
    L = _dev()
    n, streams = 1024, 4
    ring = _ring_for(n)
    R = _rms_cap(ring, n, feed=True)  # rend starts at 0: the aged rend passes 2^32 once a stream has been fed R values
    sch = Schedule(R, n, TICK_DELAY, big=16384)
    sch.check([TICK_DELAY])
    rng = np.random.default_rng(20261018)
    most = 43000
    assert most <= RMS_SIZE
    pin = [wf.PinnedBuffer((streams, most)), wf.PinnedBuffer((streams, most))]
    # what every stream is fed per tick: an approach in three long feeds, then ragged counts (0 included) that differ between the
    # streams, so that rend crosses 2^32 in different feeds
    feeds = [np.full(streams, most, np.uint32)] * 3
    fed = np.full(streams, 3 * most, np.int64)
    crossed = [None] * streams
    while len(feeds) < len(sch.pushes):
        k = len(feeds)
        c = np.array([800, 441 if k % 2 else 0, 37 + 400 * (k % 3), 799 if k % 4 else 0], np.uint32)
        if k == 5:
            c[:] = 0  # nothing to consume in this frame, for any stream
        feeds.append(c)
        for s in range(streams):
            if crossed[s] is None and fed[s] < R <= fed[s] + c[s]:
                crossed[s] = k
        fed += c
    assert all(c is not None and c + 6 < len(feeds) for c in crossed), (crossed, len(feeds))
    assert len(set(crossed)) >= 3, crossed
    cfg = _spectrum_cfg(n)
    with wf.SpectrumBatch(cfg, streams, ring_frames=ring) as fresh, wf.SpectrumBatch(cfg, streams, ring_frames=ring) as old:
        for b in (fresh, old):
            b.enable_input_rms(feed=True)
        _age(L, old, R)
        T = 0
        for i, p in enumerate(sch.pushes):
            a = _audio(streams, 2, T, p)
            T += p
            c, slot = feeds[i], i & 1
            mx = max(int(c.max()), 1)
            for b in (fresh, old):
                b.ingest_done(slot)
            sq = (rng.uniform(0.0, 0.6, (streams, mx)).astype(np.float32)) ** 2
            pin[slot].array.reshape(-1)[:sq.size] = sq.reshape(-1)
            for b in (fresh, old):
                b.push_audio(a)
                b.push_rms_ragged_async(pin[slot], c, mx, slot)
                b.tick(delay_frames=TICK_DELAY)
            what = f"tick {i} at T = R{T - R:+d}, feed {c.tolist()}"
            _same(fresh, old, what, SPECTRUM_OUTPUTS)
            if i > 3:
                assert np.all(old.input_rms() > 0)
        for b in (fresh, old):
            b.sync()
    for p in pin:
        p.close()


# ---- waveform batches -------------------------------------------------------------------------------------------------------------

def run_waveform():
    L = _dev()
    cfg = wf.Config.defaults(waveform=1, width=800, stereo=1)
    streams = len(STREAM_DELAYS)
    delays = [TICK_DELAY + d for d in STREAM_DELAYS]
    with wf.SpectrumBatch(cfg, streams) as fresh, wf.SpectrumBatch(cfg, streams) as old:
        ring, w0 = old.ring_frames, old.fft_size
        assert old.kernel_name() == "waveform_tick_kernel" and w0 == 800
        win = ring // 2  # at least the history a tick looks back over (ring >= 2 * (waveform samples + width))
        R = 2 * ring - w0 + win  # wpos starts at `width`: 0 at T = 2 rings - width
        sch = Schedule(R, win, max(delays), big=ring // 2, fine=True)
        sch.check(delays)
        for b in (fresh, old):
            b.set_stream_delay(np.array(STREAM_DELAYS, np.uint32))
        assert L.wf_hip_debug_age(old.h, 0, streams, (1 << 32) - 2 * ring) == 0, L.wf_hip_last_error(old.h)
        T, idle, moved = 0, [], 0
        for i, p in enumerate(sch.pushes):
            a = _audio(streams, old.capture_channels, T, p)
            T += p
            ts = 10_000_000_000 + T * 1_000_000_000 // 48000  # the end of the newest captured sample
            for b in (fresh, old):
                b.push_audio(a)
                b.tick(delay_frames=TICK_DELAY, audio_ts_ns=ts)
            what = f"tick {i} at T = 2 rings - width {T - (R - win):+d}"
            _same(fresh, old, what, ("decibels", "waveform_ts", "last_silent"))
            before = old.waveform_ts()
            moved += int(np.any(before != 0))
            if i % 4 == 1:  # a tick without new audio: every stream holds exactly its reserve, nothing is consumed
                rows = old.decibels()
                for b in (fresh, old):
                    b.tick(delay_frames=TICK_DELAY, audio_ts_ns=ts)
                _same(fresh, old, what + ", idle tick", ("decibels", "waveform_ts", "last_silent"))
                assert np.array_equal(old.waveform_ts(), before) and np.array_equal(_bits(old.decibels()), _bits(rows)), what
                idle.append(T)
        idle = np.array(idle)
        assert np.any(idle < R - win) and np.count_nonzero(idle > R - win) >= 3 and moved > len(sch.pushes) // 2
        assert not np.all(old.decibels() == np.float32(wf.db_min()))


# ---- the measurement outputs ------------------------------------------------------------------------------------------------------

def run_measure():
    from signal_ref import History
    import pitch_ref
    import signal_ref
    from test_gpu_signal import _check as signal_check
    from test_gpu_pitch import Tally
    L = _dev()
    streams = 3
    for meter in (False, True):
        if meter:
            cfg = wf.Config.defaults(meter=1, meter_rms=1, capture_channels=1, stereo=0)
        else:
            cfg = wf.Config.defaults(fft_size=4096, stereo=1, slope=1.0, bars=1)
        with wf.SpectrumBatch(cfg, streams, ring_frames=0 if meter else 16384) as fresh, \
                wf.SpectrumBatch(cfg, streams, ring_frames=0 if meter else 16384) as old:
            ring, cap, fft = old.ring_frames, old.capture_channels, old.fft_size
            assert meter or ring == 16384  # CQ's longest window (WF_HIP_CQ_MAX_WINDOW) is the whole ring
            P = pitch_ref.window_frames(fft)
            w0 = 0 if meter else fft
            R = 2 * ring - w0 + ring  # the window of this schedule: the whole ring, the longest look back there is (CQ)
            sch = Schedule(R, ring, 0, big=ring // 2, fine=True)
            sch.check([0])
            wrap = R - ring  # T at which the aged wpos is 0
            for b in (fresh, old):
                b.enable_loudness()
            assert L.wf_hip_debug_age(old.h, 0, streams, (1 << 32) - 2 * ring) == 0, L.wf_hip_last_error(old.h)
            hist = History(streams, cap, max(fft, P))
            names = ["signal", "pitch", "cq", "scope", "loudness"] + ([] if meter or cap < 2 else ["stereo"])
            rng = np.random.default_rng(7)
            T, tied, voiced, triggered = 0, 0, 0, 0
            tally = Tally()
            for i, p in enumerate(sch.pushes):
                # 220 Hz and low noise, the channels differing in phase and level, one clipped sample per hop
                t = (T + np.arange(p)) / 48000.0
                a = np.empty((streams, cap, p), np.float32)
                for s in range(streams):
                    for c in range(cap):
                        a[s, c] = (0.5 - 0.2 * c - 0.05 * s) * np.sin(2 * np.pi * 220.0 * t + 0.7 * c + 0.3 * s)
                a += rng.normal(0.0, 0.003, a.shape).astype(np.float32)
                a[:, 0, p // 2] = 1.0
                T += p
                for b in (fresh, old):
                    b.push_audio(a)
                hist.push(a)
                if T < wrap - sum(HOPS):
                    continue
                what = f"{'meter' if meter else 'spectrum'} batch, read {i} at wpos = 2^32{T - wrap:+d}"
                got = {}
                for nm in names:
                    x, y = getattr(fresh, nm)(), getattr(old, nm)()
                    assert x.tobytes() == y.tobytes(), f"{what}: {nm} differs"
                    got[nm] = y
                voiced += int(got["pitch"]["voiced"].all())
                triggered += int(got["scope"]["triggered"].all())
                if 0 < T - wrap < P:  # the pitch window straddles 2^32 (the signal window, at least as long, with it)
                    signal_check(got["signal"], signal_ref.signal(hist.window()[:, :, -fft:]), what)
                    tally.check(got["pitch"], hist.window()[:, :, -P:], what)
                    tied += 1
            assert tied >= 3 and voiced >= tied and triggered >= tied, (tied, voiced, triggered)
            assert np.all(old.signal()["ch"]["clipped"][:, 0] > 0) and np.all(np.isfinite(old.loudness()["momentary"]))
            tally.close()


KINDS = {"push_paths": run_push_paths, "reset_after_wrap": run_reset_after_wrap, "meter_delay": run_meter_delay, "rms_feed": run_rms_feed,
         "waveform": run_waveform, "measure": run_measure}

if __name__ == "__main__":
    kind = sys.argv[1]
    if kind in ("spectrum_normalize", "meter"):
        run(kind)
    elif kind.startswith("spectrum_delay_"):
        run_spectrum_delay(int(kind.rsplit("_", 1)[1]))
    else:
        KINDS[kind]()
    print("wrapped ok")
