"""The words the fused tick kernel reads in front of its fetch burst -- the leading 128 bytes of wf::TickArgs: wpos, stream_flags,
delay_stream, vol_comp_stream, stream_base, stream_count, cap_ch, mode, ring_mask, ring_stride, delay and the table pointers -- and
the order the burst is requested in (tables in front of the ring window on the geometries that take that order).  Every case is the
HIP path against the oracle's restatement of the reference, through the helpers the other GPU tests use; small batches, a few ticks."""
import numpy as np
import pytest

import scenarios
from helpers import assert_db_close

pytestmark = pytest.mark.gpu

HOP = 800
STREAMS = 3  # an odd number of stereo streams is an even number of spectra: the clamped, inactive spectrum shows with one channel


def _audio(streams, channels, frames):
    from tools import synth
    return synth.block(scenarios.SEED, 0, streams, channels, 0, frames)


def _run(cfg_dict, first_push, ticks, *, streams=STREAMS, ring_frames=0, delays=None, rms=None, events=None, common_delay=0):
    """Ticks a batch and one oracle per stream side by side and compares the rows after every tick.
    delays[i]: per-stream A/V-sync delay in frames (the oracle of that stream is fed that many frames late: it analyses the window
    that ends there); rms[i]: per-stream m_input_rms; events[tick][i]: 0 shown, 1 hidden, 3 paused (the source is not ticked)."""
    import waveform_amd as wf
    cfg = scenarios.make_config(cfg_dict)
    channels = int(cfg.capture_channels)
    total = first_push + HOP * (ticks - 1)
    audio = _audio(streams, channels, total)
    delays = [0] * streams if delays is None else delays
    oracles = [scenarios.OracleBackend(cfg, input_rms=None if rms is None else float(rms[i])) for i in range(streams)]
    with wf.SpectrumBatch(cfg, streams, ring_frames=ring_frames) as b:
        kernel = b.kernel_name()
        if any(delays):
            b.set_stream_delay(np.array(delays, np.uint32))
        if rms is not None:
            b.set_input_rms(np.array(rms, np.float32))
        pushed = 0
        fed = [0] * streams
        for k in range(ticks):
            n = first_push if k == 0 else HOP
            b.push_audio(audio[:, :, pushed:pushed + n])
            pushed += n
            state = [0] * streams if events is None else events[k]
            if events is not None:
                b.set_hidden(np.array(state, np.uint8))
            b.tick(delay_frames=common_delay)
            got = b.decibels()
            for i, o in enumerate(oracles):
                upto = pushed - delays[i] - common_delay
                o.set_hidden(state[i] == 1)
                o.push(audio[i][:, fed[i]:upto], muted=False)
                fed[i] = upto
                if state[i] != 3:
                    o.tick(1.0 / 60.0)
                assert_db_close(got[i], o.observe()["db"], f"{kernel}: tick {k}, stream {i} (state {state[i]}, delay {delays[i]})", deep=True)
    return kernel


# N = 4096: the ring holds 8192 samples and starts with its write position at 4096; 3200 frames, then 800 per tick, put the
# window at [3200, 7296), [4000, 8096), [4800, 8896), [5600, 9696): the third and fourth wrap the ring's end
CFG_4096 = dict(fft_size=4096, stereo=1, slope=1.0)


@pytest.mark.parametrize("delay", [4, 3], ids=["aligned", "unaligned"])
def test_n4096_window_wraps_with_a_per_stream_delay(delay):
    """delay_stream non-null; a multiple of four keeps the 16-byte fetch, three selects the unaligned instantiation"""
    _run(CFG_4096, 3200, 4, ring_frames=8192, delays=[0, delay, 0])


@pytest.mark.parametrize("delay", [4, 3], ids=["aligned", "unaligned"])
def test_n4096_every_word_of_the_prologue(delay):
    """the same batch with volume normalisation per stream (vol_comp_stream, mode), stream 0 hidden and stream 2 paused on the
    second tick (stream_flags), a common delay on top of the per-stream one"""
    cfg = dict(CFG_4096, normalize_volume=1, volume_target=-8.0, max_gain=30.0)
    events = [[0, 0, 0], [1, 0, 3], [0, 0, 0], [0, 0, 0]]
    _run(cfg, 3200, 4, ring_frames=8192, delays=[0, delay, 0], rms=[0.5, 0.0316, 1e-4], events=events, common_delay=8)


def test_n4096_mono_capture():
    """cap_ch = 1: stream and channel come from a shift by cap_ch - 1, and three spectra leave the last workgroup half empty"""
    _run(dict(fft_size=4096, capture_channels=1, stereo=0, slope=1.0), 3200, 3, ring_frames=8192, delays=[4, 0, 0])


@pytest.mark.parametrize("n", [512, 2048, 8192])
def test_other_geometries_behind_the_reordered_arguments(n):
    """one wavefront per spectrum with four and sixteen points per thread, and the 8192-sample geometry"""
    _run(dict(fft_size=n, stereo=1, slope=1.0), max(n - HOP, HOP), 2, delays=[0, 4, 0])


def test_three_lanes_equal_one_lane():
    """stream_base / stream_count: the smallest batch the plan ticks as three slices (one workgroup per CU: 32768 samples, 256
    stereo streams) against the same streams -- the first and last of every slice -- ticked in a small handle's single launch:
    bit-equal, and the first of them against the oracle"""
    import waveform_amd as wf
    n, streams, ticks = 32768, 256, 2
    cfg_dict = dict(fft_size=n, stereo=1, slope=1.0)
    cfg = scenarios.make_config(cfg_dict)
    with wf.SpectrumBatch(cfg, streams) as big:
        lanes = big.launches_per_tick()
        assert lanes == 3, (lanes, big.kernel_name())
        # (the slices: streams / lanes each, the last one takes the remainder)
        per = streams // lanes
        picks = sorted({0, per - 1, per, 2 * per - 1, 2 * per, streams - 1})
        with wf.SpectrumBatch(cfg, len(picks)) as small:
            assert small.launches_per_tick() == 1
            for k in range(ticks):
                frames = n - HOP if k == 0 else HOP
                index0 = 0 if k == 0 else n - HOP + HOP * (k - 1)
                big.push_synth(scenarios.SEED, index0, frames)
                for j, s in enumerate(picks):
                    small.push_synth(scenarios.SEED, index0, frames, first=j, count=1, stream_id0=s)
                big.tick()
                small.tick()
            want = small.decibels()
            for j, s in enumerate(picks):
                got = big.decibels(s, 1)[0]
                assert np.array_equal(got.view(np.uint32), want[j].view(np.uint32)), f"stream {s} differs between three lanes and one"
    from tools import synth
    total = n - HOP + HOP * (ticks - 1)
    audio = synth.block(scenarios.SEED, picks[0], 1, 2, 0, total)[0]
    ora = scenarios.OracleBackend(cfg)
    fed = 0
    for k in range(ticks):
        frames = n - HOP if k == 0 else HOP
        ora.push(audio[:, fed:fed + frames], muted=False)
        fed += frames
        ora.tick(1.0 / 60.0)
    assert_db_close(want[0], ora.observe()["db"], "stream 0 of the one-lane handle against the oracle", deep=True)
