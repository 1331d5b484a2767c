"""wf_hip_reset against fresh twins: a stream re-initialised in the middle of a run (update() in the plugin, a slot rejoined
through wf_hip_reset, wf_hip_multi_reset on a group) must read and tick, bit for bit, as the same stream of a handle created at
that moment.  Three handles per case:
  A  history H1, then reset(first, count) on a slice, then history H2
  B  created fresh where A is reset, given the settings a reset leaves in force (include/wf_hip.h), then H2: A's reset streams
  C  never reset, H1 + H2: A's other streams
Every output the configuration has is compared after the reset (before any tick) and after every tick of H2, with
np.array_equal -- the mirror hand-over (wf_hip_bars_mirror_ready) included.  Also here: a readback in flight across a reset
returns the state before it, wf_hip_read_async refused for a bad rider leaves nothing behind, and a group reset that straddles
a shard boundary."""
import numpy as np
import pytest

import waveform_amd as wf
from tools import synth

pytestmark = pytest.mark.gpu
SEED = synth.DEFAULT_SEED
HOP = 800
SHOWN, HIDDEN, HIDDEN_TIMEOUT, PAUSED, STARVED = 0, 1, 2, 3, 4

FAMILIES = {
    "pow2_4096_ema_slope": dict(cfg=dict(fft_size=4096, stereo=1, slope=1.0), streams=12),
    # kernel: a part of kernel_name() that names the path the family is there for
    "mixed_800_bars": dict(cfg=dict(fft_size=800, stereo=1, tsmoothing=0, bars=1, interp_mode=1), streams=12, silent=True, kernel="mixed radix"),
    "bluestein_2096_curve": dict(cfg=dict(fft_size=2096, stereo=0, tsmoothing=2, curve=1, interp_mode=2, width=500), streams=10, kernel="Bluestein"),
    "big_65536_bars": dict(cfg=dict(fft_size=65536, stereo=1, bars=1, interp_mode=1), streams=5, kernel="big_whole_kernel"),
    "bars_mirror_gauss": dict(cfg=dict(fft_size=4096, stereo=1, bars=1, interp_mode=1, mirror_freq_axis=1, filter_mode=1, filter_radius=1.5),
                              streams=12, mirror=True),
    "curve_2048_vertices": dict(cfg=dict(fft_size=2048, stereo=1, curve=1, interp_mode=2, width=640, vertices=1), streams=10, mirror=True),
    "stepped_2048_mirror": dict(cfg=dict(fft_size=2048, stereo=1, slope=1.0, bars=1, interp_mode=1, channel_spacing=6, mirror_freq_axis=1,
                                         vertices=3), streams=10, mirror=True),
    "normalize_set_rms": dict(cfg=dict(fft_size=4096, stereo=1, bars=1, normalize_volume=1), streams=10, rms="set"),
    "normalize_device_rms": dict(cfg=dict(fft_size=4096, stereo=1, bars=1, interp_mode=1, normalize_volume=1), streams=10, rms="device"),
    "meter_rms": dict(cfg=dict(meter=1, meter_ms=50), streams=10),
    "waveform_normalize": dict(cfg=dict(waveform=1, stereo=1, width=400, normalize_volume=1), streams=10, rms="device"),
    # three lanes (two rounds of one-workgroup-per-CU workgroups): the reset and the hand-over follow a laned tick
    "lanes_32768_mirror": dict(cfg=dict(fft_size=32768, stereo=1, slope=1.0, bars=1, interp_mode=1), streams=520, mirror=True, lanes=True),
}


def _kind(cfg):
    return "meter" if cfg.meter else "wave" if cfg.waveform else "spectrum"


def same(a, b):
    """bit-exact where it matters: float arrays NaN-aware, records and integers byte for byte"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        return np.array_equal(a, b, equal_nan=True)
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


class _Hip:
    """the HIP runtime the library is linked against, looked up through the library's own handle (torch cannot share a process
    with it once it is loaded): device buffers and a consumer stream for the mirror hand-over"""

    def __init__(self):
        import ctypes as C
        L = wf.lib()
        self.C = C
        self.malloc, self.free, self.memset, self.memcpy = L["hipMalloc"], L["hipFree"], L["hipMemset"], L["hipMemcpy"]
        self.stream_create, self.stream_destroy, self.stream_sync = L["hipStreamCreate"], L["hipStreamDestroy"], L["hipStreamSynchronize"]
        self.malloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.free.argtypes = [C.c_void_p]
        self.memset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.stream_create.argtypes = [C.POINTER(C.c_void_p)]
        self.stream_destroy.argtypes = [C.c_void_p]
        self.stream_sync.argtypes = [C.c_void_p]

    def alloc(self, nbytes):
        p = self.C.c_void_p()
        assert self.malloc(self.C.byref(p), nbytes) == 0
        assert self.memset(p, 0xFF, nbytes) == 0  # NaN in every float: a hand-over nobody wrote shows
        return p.value

    def stream(self):
        s = self.C.c_void_p()
        assert self.stream_create(self.C.byref(s)) == 0
        return s.value

    def download(self, ptr, shape):
        out = np.empty(shape, np.float32)
        assert self.memcpy(out.ctypes.data_as(self.C.c_void_p), self.C.c_void_p(ptr), out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        return out


class Twin:
    """one handle plus the device buffers its bars mirror into (two sets of one buffer each) and the stream that consumes them"""

    def __init__(self, cfg, streams, fam):
        self.b = wf.SpectrumBatch(cfg, streams)
        self.kind = _kind(cfg)
        self.rms = fam.get("rms")
        self.sets = None
        if self.rms == "device":
            self.b.enable_input_rms()
        if fam.get("mirror"):
            self.hip = _Hip()
            self.shape = (streams, self.b.display_channels, self.b.num_bars)
            self.sets = [self.hip.alloc(int(np.prod(self.shape)) * 4) for _ in range(2)]
            self.consumer = self.hip.stream()
            self.b.set_bars_mirrors([self.sets[0]], [self.sets[1]])

    def handed_over(self):
        ptr = self.b.bars_mirror_ready(self.consumer)
        assert ptr in self.sets
        assert self.hip.stream_sync(self.consumer) == 0
        return self.hip.download(ptr, self.shape)

    def outputs(self):
        b, o = self.b, {}
        if self.kind == "meter":
            o.update(meter=b.meter(), last_silent=b.last_silent(), signal=b.signal())
            if b.num_bars:
                o["bars"] = b.bars()
        elif self.kind == "wave":
            o.update(decibels=b.decibels(), last_silent=b.last_silent(), waveform_ts=b.waveform_ts())
        else:
            o.update(decibels=b.decibels(), tsmooth=b.tsmooth(), last_silent=b.last_silent(), peaks=b.peaks(), signal=b.signal())
            if b.num_bars:
                o["bars"] = b.bars()
            if b.cfg.mirror_freq_axis:
                o["premirror"] = b.premirror()
            if b.cfg.vertices:
                o.update(vertices=b.vertices(), vertex_counts=b.vertex_counts())
        if self.rms == "device":
            o["input_rms"] = b.input_rms()
        if self.sets is not None:
            o["mirror_hand_over"] = self.handed_over()
            assert same(o["mirror_hand_over"], o["bars"]), "the mirror hand-over differs from the handle's own bars"
        return o

    def close(self):
        self.b.close()  # (waits for the ticks that write the mirrors)
        if self.sets is not None:
            self.hip.stream_destroy(self.consumer)
            for p in self.sets:
                self.hip.free(p)


class Script:
    """the calls of H1 / H2, the same on every handle they are played on"""

    def __init__(self, cfg, streams, fam):
        self.cfg, self.streams, self.fam = cfg, streams, fam
        self.kind = _kind(cfg)
        self.n = int(cfg.fft_size)
        self.index = np.zeros(streams, np.int64)  # next synth sample index per stream
        self.delay = ((np.arange(streams) * 37) % 161).astype(np.uint32)     # not all multiples of 4
        self.input_rms = (0.02 + 0.01 * np.arange(streams)).astype(np.float32)
        self.audio_ts = np.zeros(streams, np.uint64)
        self.t = 0

    def ragged_noise(self, handles, hop=HOP):
        """three contiguous chunks of different lengths: the rings end up unaligned"""
        bounds = [0, self.streams // 3, 2 * self.streams // 3, self.streams]
        for k in range(3):
            lo, hi = bounds[k], bounds[k + 1]
            if hi <= lo:
                continue
            frames = hop + ((k + self.t) % 3 - 1) * 3
            for h in handles:
                h.b.push_synth(SEED, int(self.index[lo]), frames, first=lo, count=hi - lo, stream_id0=lo)
            self.index[lo:hi] += frames

    def silence(self, handles, lo, hi, frames):
        for h in handles:
            h.b.push_silence(frames, first=lo, count=hi - lo)

    def tick(self, handles):
        if self.kind == "wave":
            self.audio_ts = (np.uint64(1_000_000_000) + np.uint64(16_666_667) * np.uint64(self.t + 1)
                             + np.arange(self.streams, dtype=np.uint64) * np.uint64(1000))
            for h in handles:
                h.b.set_stream_audio_ts(self.audio_ts)
        for h in handles:
            h.b.tick()
        self.t += 1

    def h1(self, handles):
        """noise, silence into the silent state, every hidden state, ragged pushes, per-stream delay and RMS; the mirror set is
        handed over after some ticks but not after the last one (the reset then finds a set the ticks wrote)"""
        half = self.streams // 2
        for t in range(12):
            if t == 1:
                for h in handles:
                    h.b.set_stream_delay(self.delay)
            if t == 2 and self.fam.get("rms") == "set":
                for h in handles:
                    h.b.set_input_rms(self.input_rms)
            if 3 <= t < 9:  # the first half falls silent for long enough to enter the silent state, the rest goes on
                self.silence(handles, 0, half, self.n + HOP if t == 3 else HOP)
                self._noise_range(handles, half, self.streams)
            else:
                self.ragged_noise(handles)
            if t == 9:
                mask = np.array([(SHOWN, HIDDEN, HIDDEN_TIMEOUT, PAUSED, STARVED)[i % 5] for i in range(self.streams)], np.uint8)
                if self.kind != "spectrum":
                    mask[mask == STARVED] = HIDDEN
                for h in handles:
                    h.b.set_hidden(mask)
            self.tick(handles)
            if t % 2 == 0:  # (t = 11, the last, is odd)
                for h in handles:
                    if h.sets is not None:
                        h.handed_over()
        if self.fam.get("silent"):
            assert any(h.b.last_silent()[:half].any() for h in handles), "H1 never reached the silent state"

    def _noise_range(self, handles, lo, hi):
        for h in handles:
            h.b.push_synth(SEED, int(self.index[lo]), HOP, first=lo, count=hi - lo, stream_id0=lo)
        self.index[lo:hi] += HOP

    def settings_in_force(self, twin):
        """what a reset leaves in force, given to the fresh twin explicitly"""
        twin.b.set_stream_delay(self.delay)
        if self.fam.get("rms") == "set":
            twin.b.set_input_rms(self.input_rms)
        if self.kind == "wave":
            twin.b.set_stream_audio_ts(self.audio_ts)

    def h2_tick(self, handles, k):
        if k == 2:
            for h in handles:
                h.b.set_hidden(np.full(2, HIDDEN, np.uint8), first=self.streams - 2)
        if k == 3:
            self.silence(handles, 0, self.streams, 2 * HOP)
        else:
            self.ragged_noise(handles)
        self.tick(handles)


def _compare(a, b, c, mask, when):
    oa, ob, oc = a.outputs(), b.outputs(), c.outputs()
    assert oa.keys() == ob.keys() == oc.keys()
    for k in oa:
        if mask.any():
            assert same(oa[k][mask], ob[k][mask]), f"{when}: {k} of the reset streams differ from a fresh handle's"
        if (~mask).any():
            assert same(oa[k][~mask], oc[k][~mask]), f"{when}: {k} of the streams outside the reset differ from a handle never reset"


def _inflight_read(a, kind, fam):
    """a readback of the state before the reset, issued before it: pinned destinations of every output the batch reads that way"""
    from waveform_amd import binding
    b, n = a.b, a.b.streams
    if kind != "meter":
        assert int(b.L.wf_hip_output_bytes(b.h, binding.OUT_DECIBELS)) == b.output_channels * b.bins * 4
    if kind == "meter":
        want = dict(meter=wf.PinnedBuffer((n, b.capture_channels)), last_silent=wf.PinnedBuffer((n,), np.uint8))
    else:
        want = dict(rows=wf.PinnedBuffer((n, b.output_channels, b.bins)), last_silent=wf.PinnedBuffer((n,), np.uint8))
        if b.num_bars:
            want["bars"] = wf.PinnedBuffer((n, b.display_channels, b.num_bars))
        if b.cfg.mirror_freq_axis and b.num_bars:
            want["premirror"] = wf.PinnedBuffer((n, b.display_channels))
        if b.cfg.vertices:
            want["vertices"] = wf.PinnedBuffer((n, b.display_channels, int(b.L.wf_hip_num_vertices(b.h)), 4))
            want["vertex_counts"] = wf.PinnedBuffer((n, b.display_channels), np.uint32)
        if fam.get("rms") == "device":
            want["input_rms"] = wf.PinnedBuffer((n,))
    for p in want.values():
        p.array[...] = np.nan if p.array.dtype.kind == "f" else 0xAB
    b.read_async(0, **want)
    snap = None
    if b.num_bars and kind != "meter":
        snap = wf.PinnedBuffer((n, b.display_channels, b.num_bars))
        snap.array[...] = np.nan
        b.read_bars_async(snap, 1)
    return want, snap


def _check_inflight(a, c, want, snap):
    a.b.readback_done(0)
    a.b.readback_done(1)
    cb = c.b
    truth = dict(rows=lambda: cb.decibels(), last_silent=lambda: cb.last_silent().astype(np.uint8), bars=cb.bars, premirror=cb.premirror,
                 vertices=cb.vertices, vertex_counts=cb.vertex_counts, input_rms=cb.input_rms, meter=cb.meter)
    for k, p in want.items():
        assert same(p.array, truth[k]()), f"a readback issued before the reset did not return the state before it: {k}"
        p.close()
    if snap is not None:
        assert same(snap.array, cb.bars()), "a bars snapshot read issued before the reset did not return the bars before it"
        snap.close()


def run_case(name, resets, h2_ticks=4):
    fam = FAMILIES[name]
    cfg = wf.Config.defaults(**fam["cfg"])
    streams = fam["streams"]
    s = Script(cfg, streams, fam)
    a, c = Twin(cfg, streams, fam), Twin(cfg, streams, fam)
    b = None
    try:
        if fam.get("lanes"):
            assert a.b.launches_per_tick() > 1, a.b.kernel_name()
        if fam.get("kernel"):
            assert fam["kernel"] in a.b.kernel_name(), a.b.kernel_name()
        if fam.get("rms") == "device":  # (the producer owns m_input_rms: per-stream values are refused while it runs)
            with pytest.raises(wf.WfHipError):
                a.b.set_input_rms(np.full(streams, 0.1, np.float32))
        s.h1([a, c])
        want, snap = _inflight_read(a, s.kind, fam)
        mask = np.zeros(streams, bool)
        for first, count in resets:
            a.b.reset(first, count)
            mask[first:first + count] = True
        b = Twin(cfg, streams, fam)
        s.settings_in_force(b)
        _check_inflight(a, c, want, snap)
        _compare(a, b, c, mask, "after the reset, before any tick")
        for k in range(h2_ticks):
            s.h2_tick([a, b, c], k)
            _compare(a, b, c, mask, f"H2 tick {k}")
    finally:
        for h in (a, b, c):
            if h is not None:
                h.close()


@pytest.mark.parametrize("name", list(FAMILIES))
def test_reset_slice_equals_a_fresh_handle(name):
    streams = FAMILIES[name]["streams"]
    run_case(name, [(streams // 3, max(1, streams // 3))])


@pytest.mark.parametrize("resets", [[(0, 1)], [(9, 1)], [(0, 10)], [(2, 4), (4, 4)]], ids=["first", "last", "whole", "overlapping"])
def test_reset_ranges(resets):
    run_case("stepped_2048_mirror", resets, h2_ticks=3)


@pytest.mark.parametrize("resets", [[(0, 1)], [(9, 1)], [(0, 10)], [(2, 4), (4, 4)]], ids=["first", "last", "whole", "overlapping"])
def test_reset_ranges_meter(resets):
    run_case("meter_rms", resets, h2_ticks=3)


def test_refused_read_async_leaves_nothing_behind():
    """wf_hip_read_async refused for a rider the batch does not have must not have enqueued the rows: the pinned destinations
    keep their sentinel, the slot is as if the call never happened, the next tick equals a twin's, and a valid read on the same
    slot returns the right data"""
    cfg = wf.Config.defaults(fft_size=2048, stereo=1, bars=1, interp_mode=1)
    n = 6
    with wf.SpectrumBatch(cfg, n) as a, wf.SpectrumBatch(cfg, n) as twin:
        for t in range(3):
            for h in (a, twin):
                h.push_synth(SEED, t * HOP, HOP)
                h.tick()
        rows = wf.PinnedBuffer((n, a.output_channels, a.bins))
        silent = wf.PinnedBuffer((n,), np.uint8)
        bars = wf.PinnedBuffer((n, a.display_channels, a.num_bars))
        rider = wf.PinnedBuffer((n, a.display_channels, 64, 4))
        counts = wf.PinnedBuffer((n, a.display_channels), np.uint32)
        try:
            for what in ("input_rms", "vertices", "vertex_counts", "premirror"):
                for p in (rows, bars, rider):
                    p.array[...] = np.nan
                silent.array[...] = 0xAB
                counts.array[...] = 0xDEADBEEF
                dst = dict(rows=rows, last_silent=silent, bars=bars)
                dst[what] = counts if what == "vertex_counts" else rider
                with pytest.raises(wf.WfHipError) as e:
                    a.read_async(0, **dst)
                assert e.value.code == -1, (what, e.value)
                a.sync()
                a.readback_done(0)
                assert np.isnan(rows.array).all() and np.isnan(bars.array).all() and np.isnan(rider.array).all(), \
                    f"a refused read_async with {what} wrote into the destinations"
                assert (silent.array == 0xAB).all() and (counts.array == 0xDEADBEEF).all(), f"a refused read_async with {what} wrote m_last_silent"
            for h in (a, twin):
                h.push_synth(SEED, 3 * HOP, HOP)
                h.tick()
            assert same(a.decibels(), twin.decibels()) and same(a.bars(), twin.bars()) and same(a.last_silent(), twin.last_silent())
            a.read_async(0, rows=rows, last_silent=silent, bars=bars)
            a.readback_done(0)
            assert same(rows.array, twin.decibels()) and same(bars.array, twin.bars())
            assert same(silent.array.astype(bool), twin.last_silent())
        finally:
            for p in (rows, silent, bars, rider, counts):
                p.close()


@pytest.mark.parametrize("mirror", [None, "0"], ids=["direct-peer", "copy"])
def test_group_reset_across_a_shard_boundary(mirror, monkeypatch):
    """wf_hip_multi_reset over a range that straddles shard boundaries equals a plain handle's reset; the gather right after it,
    with no tick in between, hands over the reset bars -- whether the tick kernels store into every device's result themselves
    (direct peer stores, the default where the devices address each other) or the bars are copied behind the tick"""
    if mirror is None:
        monkeypatch.delenv("WF_HIP_MULTI_MIRROR", raising=False)
    else:
        monkeypatch.setenv("WF_HIP_MULTI_MIRROR", mirror)
    cfg = wf.Config.defaults(fft_size=4096, stereo=1, slope=1.0, bars=1, interp_mode=1)
    streams = 13  # shards [0, 5), [5, 9), [9, 13)
    devices = [i % wf.device_count() for i in range(3)]
    with wf.SpectrumBatch(cfg, streams) as plain, wf.MultiBatch(cfg, streams, devices) as m:
        assert [s[2] for s in m.shards] == [0, 5, 9]
        for t in range(5):
            for b in (plain, m):
                b.push_synth(SEED, t * HOP, HOP)
                b.tick()
            if t < 4:
                m.allgather_bars()  # (none after the last tick: the reset finds a result the ticks wrote)
        for b in (plain, m):
            b.reset(3, 8)
        m.allgather_bars()
        want = plain.bars()
        assert same(m.bars(), want) and same(m.decibels(), plain.decibels()) and same(m.last_silent(), plain.last_silent())
        for i in range(m.n_devices):
            assert same(m.gathered(i), want), f"device index {i}: the gather after the reset handed over bars from before it"
        for t in range(5, 7):
            for b in (plain, m):
                b.push_synth(SEED, t * HOP, HOP)
                b.tick()
            m.allgather_bars()
            want = plain.bars()
            assert same(m.decibels(), plain.decibels())
            for i in range(m.n_devices):
                assert same(m.gathered(i), want), f"tick {t}, device index {i}"
        # which path the gathers took: the shard handles have mirror buffers (the tick kernels store into every device's result)
        # exactly when the group chose the direct peer stores.  (Asked last: a hand-over behind the group's back.)
        import ctypes as C
        assert m.transport == "peer", m.transport
        m.sync()
        direct = []
        for h, _dev, _first, _count in m.shards:
            out = C.c_void_p(0)
            direct.append(m.L.wf_hip_bars_mirror_ready(h, C.c_void_p(m.L.wf_hip_stream(h)), C.byref(out)) == 0)
        assert direct == [mirror is None] * 3, (mirror, direct)
