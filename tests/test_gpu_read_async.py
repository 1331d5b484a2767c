"""wf_hip_read_async where its slots are reused: a slot read again with another size (its snapshot and its silent bytes regrow,
then are reused for a smaller read), and a slot read again while the ticks run on behind the copies, nothing ever waiting for the
device but wf_hip_readback_done.  The truth is always the blocking reader of the same output (wf_hip_read), bit for bit.  The
reads in flight across a reset, on every family, and the refused read are in test_gpu_reset.py."""
import numpy as np
import pytest

import waveform_amd as wf
from tools import synth

pytestmark = pytest.mark.gpu
SEED = synth.DEFAULT_SEED
HOP = 800
SENTINEL = 0xAB  # every byte of a pinned destination before a read

METER = dict(meter=1, meter_ms=50)
BARS_512 = dict(fft_size=512, stereo=1, bars=1, interp_mode=1)
MANY = 300  # streams: more than the floor of the slots' blocks (256 elements, of the snapshot and of the silent bytes alike)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def shapes(b):
    """the Readback fields this batch can fill: (shape per stream, dtype)"""
    nv = int(b.L.wf_hip_num_vertices(b.h))
    return dict(rows=((b.output_channels, b.bins), np.float32), last_silent=((), np.uint8), bars=((b.display_channels, b.num_bars), np.float32),
                premirror=((b.display_channels,), np.float32), vertices=((b.display_channels, nv, 4), np.float32),
                vertex_counts=((b.display_channels,), np.uint32), input_rms=((), np.float32), meter=((b.capture_channels,), np.float32))


def pinned_set(b, names):
    """destinations for the whole batch, every byte the sentinel"""
    out = {}
    for k in names:
        shape, dtype = shapes(b)[k]
        out[k] = wf.PinnedBuffer((b.streams,) + shape, dtype)
        out[k].array.reshape(-1).view(np.uint8)[...] = SENTINEL
    return out


def blocking(b, names, first=0, count=None):
    """the same outputs through wf_hip_read (waits for the ticks issued so far)"""
    read = dict(rows=b.decibels, last_silent=lambda f, c: b.last_silent(f, c).astype(np.uint8), bars=b.bars, premirror=b.premirror,
                vertices=b.vertices, vertex_counts=b.vertex_counts, input_rms=b.input_rms, meter=b.meter)
    return {k: read[k](first, count) for k in names}


def close_all(sets):
    for s in sets:
        for p in s.values():
            p.close()


@pytest.mark.parametrize("cfg,names", [(METER, ("meter", "last_silent")), (BARS_512, ("bars",)), (BARS_512, ("rows", "last_silent", "bars"))],
                         ids=["meter", "bars_snapshot", "rows_bars"])
def test_slot_grows_and_is_reused(cfg, names):
    """one slot, read with 1, 40, all 300 and again 1 stream: both of its blocks regrow and are then reused for less; what lands
    is what the blocking readers return for that range, and nothing lands outside it"""
    with wf.SpectrumBatch(wf.Config.defaults(**cfg), MANY) as b:
        dst = pinned_set(b, names)
        try:
            for t, (first, count) in enumerate([(7, 1), (100, 40), (0, MANY), (7, 1)]):
                b.push_silence(HOP, first=0, count=120)  # (both values of m_last_silent inside the second range)
                b.push_synth(SEED, t * HOP, HOP, first=120, count=MANY - 120, stream_id0=120)
                b.tick()
                want = blocking(b, names, first, count)
                for p in dst.values():
                    p.array.reshape(-1).view(np.uint8)[...] = SENTINEL
                b.read_async(0, first, count, **dst)
                b.readback_done(0)
                for k in names:
                    got = dst[k].array
                    assert bits_equal(got[:count], want[k]), f"read {t} of [{first}, {first}+{count}): {k} differs from the blocking read"
                    assert (got[count:].reshape(-1).view(np.uint8) == SENTINEL).all(), f"read {t} of {count} streams wrote {k} past them"
        finally:
            close_all([dst])


# name -> configuration, streams, destinations, options
RUN_ON = {
    "curve_vertices_mirror": (dict(fft_size=2048, stereo=1, curve=1, interp_mode=2, width=640, vertices=1, mirror_freq_axis=1), 6,
                              ("rows", "last_silent", "bars", "premirror", "vertices", "vertex_counts"), {}),
    "normalize_input_rms": (dict(fft_size=4096, stereo=1, bars=1, interp_mode=1, normalize_volume=1), 6,
                            ("rows", "last_silent", "bars", "input_rms"), dict(rms=True)),
    "bars_snapshot": (BARS_512, MANY, ("bars",), {}),
    "meter": (METER, MANY, ("meter", "last_silent"), dict(kernel="meter_tick_kernel")),
    # the smallest split geometry: three flag buffers, the current one rotates with every tick
    "split_8192": (dict(fft_size=8192, stereo=1, bars=1, interp_mode=1), 6, ("rows", "last_silent"), dict(kernel="split", silent=3, lead_in=4)),
}
ROUNDS = 6


@pytest.mark.parametrize("name", list(RUN_ON))
def test_ticks_run_on_behind_a_read(name):
    """six rounds of push, tick, read_async on alternating slots with nothing waiting for the device except readback_done of the
    slot about to be reused: every round's destinations equal what a twin, read with the blocking readers after every tick, held
    in that round"""
    cfg, n, names, opt = RUN_ON[name]
    silent = opt.get("silent", 0)  # streams [0, silent) get silence throughout, the others noise
    with wf.SpectrumBatch(wf.Config.defaults(**cfg), n) as a, wf.SpectrumBatch(wf.Config.defaults(**cfg), n) as twin:
        if "kernel" in opt:
            assert opt["kernel"] in a.kernel_name(), a.kernel_name()
        sets, record = [], []
        try:
            if opt.get("rms"):
                a.enable_input_rms()
                twin.enable_input_rms()
            for t in range(opt.get("lead_in", 0) + ROUNDS):
                for h in (a, twin):
                    if silent:
                        h.push_silence(HOP, first=0, count=silent)
                    h.push_synth(SEED, t * HOP, HOP, first=silent, count=n - silent, stream_id0=silent)
                    h.tick()
                r = t - opt.get("lead_in", 0)
                if r < 0:
                    continue
                if r >= 2:
                    a.readback_done(r & 1)
                sets.append(pinned_set(a, names))
                a.read_async(r & 1, **sets[-1])
                record.append(blocking(twin, names))
            a.readback_done(0)
            a.readback_done(1)
            if silent:  # (on the twin's record: with one value only the wrong flag buffer could pass)
                ls = np.stack([rec["last_silent"] for rec in record])
                print("last_silent of the twin per round:", ls.tolist())
                assert ls.any() and not ls.all(), "m_last_silent took one value only over the rounds"
                assert any(row.any() and not row.all() for row in ls), "no round has streams in both states"
            for r in range(ROUNDS):
                for k in names:
                    assert bits_equal(sets[r][k].array, record[r][k]), f"round {r}: {k} differs from the twin's blocking read"
        finally:
            close_all(sets)
