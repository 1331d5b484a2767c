"""The mains hum detector on the device (WF_HIP_OUT_HUM) against the float64 restatement (tests/hum_ref.py) of the frames pushed:
batches of three streams -- hum at 50.13 Hz, hum at 59.84 Hz without its fundamental, noise alone -- at the plans that take each
path of the kernel: 48000 Hz with a ring of 16384 frames (M = 512) and of 32768 (M = 1024, the LDS at its cap, the guard bytes
on), 96000 Hz (D = 64) and 16000 Hz with a ring of 8192 (D = 8); one and two captured channels, the second channel with other
content and one of them digital silence; packets of unequal odd sizes, so that the window starts at no aligned place and wraps the
ring's end; a meter batch; a slice as the first read; streams at different write positions and a stream reset and refilled; bit identity across
push paths; silence, a NaN and an infinity; refusals; a two-shard group; the 2^32 wrap of the write positions.

The bound (hum_ref.mismatches): every integer field equal to the restatement's and every float32 field within one float32 rounding
of the restatement's float64 value -- mains_hz, hz[] and total_db included.  tests/test_hum_cpu.py asserts that every candidate
line of every window read here stands at least 3 dB from the 15 dB margin, so no rounding of the device can move an integer."""
import ctypes as C

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import hum_ref as ref
from tools import synth
from measure_common import check_abi_refusals, check_shards_match, run_wrap_child

pytestmark = pytest.mark.gpu
ERR_INVALID = -1
ENTRY = 304
SR, RING = ref.SR, ref.RING


def _cfg(sr=SR, channels=2, fft=1024, **kw):
    return wf.Config.defaults(**{**dict(fft_size=fft, sample_rate=sr, capture_channels=channels, stereo=1 if channels == 2 else 0, slope=1.0,
                                        bars=1, floor_db=-70), **kw})


def _packets(rng, total):
    """(lo, hi) of packets of unequal odd lengths of 1 .. 8001 frames that add up to `total`"""
    cuts, at = [], 0
    while at < total:
        n = min(2 * int(rng.integers(0, 4001)) + 1, total - at)
        cuts.append((at, at + n))
        at += n
    return cuts


def _check(got, x, sr, ring, what=""):
    assert got.dtype == binding.HUM_DTYPE and got.dtype == ref.HUM_DTYPE
    bad = ref.mismatches(got, x, sr, ring)
    print(f"{what}: family {got['ch']['family'].tolist()}, mask {got['ch']['mask'].tolist()}, mains_hz {got['ch']['mains_hz'].tolist()}, "
          f"ratio_db {got['ch']['ratio_db'].tolist()}, noise_db {got['ch']['noise_db'].tolist()}")
    assert not bad, bad[:6]


@pytest.mark.parametrize("channels", (1, 2))
@pytest.mark.parametrize("sr,ring", ref.GPU_PLANS)
def test_hum_equals_the_restatement_of_the_frames(sr, ring, channels, monkeypatch):
    if ring == 32768 and sr == 48000:  # guard bytes behind every block, checked by wf_hip_sync
        monkeypatch.setenv("WF_HIP_CANARY", "1")
    pl = ref.plan(sr, ring)
    x = ref.case_audio(sr, ring, channels)
    with wf.SpectrumBatch(_cfg(sr, channels), 3, ring_frames=ring) as b:
        assert b.ring_frames == ring and b.capture_channels == channels
        assert wf.lib().wf_hip_output_bytes(b.h, binding.OUT_HUM) == ENTRY  # before the first read
        fresh = b.hum()
        assert fresh.tobytes() == ref.fresh(3, sr, ring).tobytes() and not fresh["ch"]["valid"].any()  # freshly created: zeros
        for lo, hi in _packets(np.random.default_rng(ring + sr), x.shape[-1]):
            b.push_audio(np.ascontiguousarray(x[:, :, lo:hi]))
        got = b.hum()
        b.sync()
        again = b.hum()
        b.sync()
    assert got.tobytes() == again.tobytes()
    assert np.all(got["window"] == pl.N) and np.all(got["decimation"] == pl.D)
    assert got["ch"]["family"][:, 0].tolist() == [50, 60, 0] and got["ch"]["mask"][:, 0].tolist() == [0b10111, 0b101110, 0]
    if channels == 2:
        assert got["ch"]["family"][:, 1].tolist() == [60, 0, 50] and got["ch"]["valid"][:, 1].tolist() == [1, 0, 1]
    else:
        assert not got["ch"][:, 1].tobytes().strip(b"\0")  # a channel that is not captured reads zeros
    assert np.all(np.abs(got["ch"]["mains_hz"][:2, 0] - np.float32([50.13, 59.84])) < 0.05)
    _check(got, x, sr, ring, f"{sr} Hz, ring {ring}, {channels} ch")


def test_a_meter_batch_reads_the_same_entries():
    """a meter batch has rings and no spectrum: its counter starts at 0, not at fft_size, so the same frames lie elsewhere in the
    ring; the entries are those of the spectrum batch, bit for bit"""
    x = ref.case_audio(SR, RING, 2)
    reads = []
    for kw in (dict(), dict(meter=1, bars=0, meter_ms=46)):
        with wf.SpectrumBatch(_cfg(**kw), 3, ring_frames=RING) as b:
            assert b.ring_frames == RING
            b.push_audio(x)
            reads.append(b.hum())
    assert reads[0].tobytes() == reads[1].tobytes()
    _check(reads[1], x, SR, RING, "a meter batch")


def test_a_slice_first_streams_at_different_positions_and_a_reset_stream():
    """the first read of a handle is a slice (first = 1, count = 1): the block is allocated whole; then 5001 frames more for one
    stream, whose window then lies elsewhere in the ring and across its end, and a stream reset and refilled with N + 3 frames"""
    long, refill = ref.stagger_audio()
    n = ref.plan(SR, RING).N
    a = n + ref.GPU_EXTRA
    with wf.SpectrumBatch(_cfg(), 3, ring_frames=RING) as b:
        b.push_audio(np.ascontiguousarray(long[:, :, :a]))
        part = b.hum(1, 1)
        full = b.hum()
        assert part.shape == (1,) and part.tobytes() == full[1:2].tobytes()
        assert b.hum(2, 1).tobytes() == full[2:].tobytes()
        b.push_audio(np.ascontiguousarray(long[1:2, :, a:]), first=1)
        b.reset(2, 1)
        b.push_audio(refill, first=2)
        moved = b.hum()
        b.tick()
        assert b.hum().tobytes() == moved.tobytes()  # a tick does not move the rings
    # (a spectrum batch's counter starts at fft_size: these windows end at ring positions 1801, 6802 and 1027 + n, and all wrap)
    assert (1024 + a) % RING == 1801 and (1024 + a + ref.STAGGER_MORE) % RING == 6802
    _check(full, long[:, :, :a], SR, RING, "the whole batch behind a slice")
    assert moved[0:1].tobytes() == full[0:1].tobytes()
    _check(moved[1:2], long[1:2], SR, RING, "5001 frames more")
    _check(moved[2:3], refill, SR, RING, "reset and refilled")
    assert moved["ch"]["family"][2].tolist() == [50, 60]


def test_every_push_path_leaves_the_same_bits():
    """the same frames through push_audio, the pinned asynchronous push and wf_hip_push_pcm (s16 interleaved: every value exact in
    float32) read bit-identically; push_synth reads as the restatement of what it leaves in the rings"""
    pcm, conv = ref.paths_audio()
    streams, frames = conv.shape[0], conv.shape[-1]
    cuts = _packets(np.random.default_rng(7), frames)
    reads = {}
    for path in ("float", "pinned", "pcm", "synth"):
        with wf.SpectrumBatch(_cfg(), streams, ring_frames=RING) as b:
            if path == "synth":
                b.push_synth(synth.DEFAULT_SEED, ref.SYNTH_INDEX0, frames)
            for i, (lo, hi) in enumerate(cuts if path != "synth" else ()):
                if path == "float":
                    b.push_audio(np.ascontiguousarray(conv[:, :, lo:hi]))
                elif path == "pinned":
                    pin = wf.PinnedBuffer((streams, 2, hi - lo))
                    pin.array[...] = conv[:, :, lo:hi]
                    b.push_audio_async(pin, streams, hi - lo, i & 1)
                    b.sync()
                    pin.close()
                else:
                    b.push_pcm(np.ascontiguousarray(pcm[:, lo:hi]), interleaved=True)
            reads[path] = b.hum()
    for path in ("pinned", "pcm"):
        assert reads[path].tobytes() == reads["float"].tobytes(), path
    assert reads["float"]["ch"]["family"].tolist() == [[50, 60], [60, 0], [0, 50]]
    _check(reads["float"], conv, SR, RING, "s16 packets")
    _check(reads["synth"], synth.block(synth.DEFAULT_SEED, 0, streams, 2, ref.SYNTH_INDEX0, frames), SR, RING, "push_synth")
    assert not reads["synth"]["ch"]["family"].any() and reads["synth"]["ch"]["valid"].all()


def test_silence_a_nan_and_an_infinity():
    x = ref.case_audio(SR, RING, 2)
    x = np.concatenate([x, x[:1]])  # a fourth stream
    n = ref.plan(SR, RING).N
    x[0, 1, -5] = np.nan            # inside the window: the channel reads invalid, its neighbour does not
    x[2, 0, -n] = np.inf            # the window's oldest frame
    x[3, 0, -n - 1] = np.nan        # one frame in front of the window: no part of it
    with wf.SpectrumBatch(_cfg(), 4, ring_frames=RING) as b:
        b.push_audio(x)
        got = b.hum()
    assert got["ch"]["valid"].tolist() == [[1, 0], [1, 0], [0, 1], [1, 1]]
    zero = np.zeros((), binding.HUM_CHANNEL_DTYPE).tobytes()
    for s, c in ((0, 1), (1, 1), (2, 0)):
        assert got["ch"][s, c].tobytes() == zero, (s, c)
    assert got["ch"]["family"].tolist() == [[50, 0], [60, 0], [0, 50], [50, 60]]
    for name in ref.CHANNEL_FLOATS + ref.CHANNEL_ARRAYS:
        assert np.all(np.isfinite(got["ch"][name])), name
    _check(got, x, SR, RING, "a NaN, digital silence and an infinity")


def test_refusals():
    L = wf.lib()
    with wf.SpectrumBatch(wf.Config.defaults(waveform=1, stereo=1, width=640, meter_ms=100), 2) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_HUM) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.hum()
        assert e.value.code == ERR_INVALID and "waveform batch" in str(e.value) and "hum" in str(e.value), str(e.value)
    with wf.SpectrumBatch(_cfg(fft=4096), 2) as b:  # the default ring at FFT 4096: 8192 frames, 5.9 Hz bins
        assert b.ring_frames == 8192 and L.wf_hip_output_bytes(b.h, binding.OUT_HUM) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.hum()
        assert e.value.code == ERR_INVALID and "hum" in str(e.value) and "sample_rate / 3" in str(e.value) and "ring_frames" in str(e.value), str(e.value)
        out = np.empty(2, binding.HUM_DTYPE)
        assert L.wf_hip_read(b.h, binding.OUT_HUM, 0, 2, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID
        assert b"hum" in L.wf_hip_last_error(b.h)
        assert b.signal().shape == (2,)  # nothing was enqueued that would trouble the next call
    with wf.SpectrumBatch(_cfg(sr=192000), 1, ring_frames=1 << 17) as b:  # 5.9 Hz bins from the 32768 frames there are at most
        assert L.wf_hip_output_bytes(b.h, binding.OUT_HUM) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.hum()
        assert e.value.code == ERR_INVALID and "hum" in str(e.value) and "sample rate" in str(e.value), str(e.value)
    with wf.SpectrumBatch(_cfg(), 2, ring_frames=RING) as b:
        assert L.wf_hip_output_bytes(b.h, binding.OUT_HUM) == ENTRY
        check_abi_refusals(b, binding.OUT_HUM, binding.HUM_DTYPE, 2, ref.fresh(2, SR, RING))


def test_two_shards_match_one_handle():
    cfg = _cfg()
    x = ref.case_audio(SR, RING, 2)
    with wf.SpectrumBatch(cfg, 3, ring_frames=RING) as one, wf.MultiBatch(cfg, 3, [0, 0], ring_frames=RING) as m:
        one.push_audio(x)
        m.push_audio(x)
        m.sync()
        want = check_shards_match(one, m, "hum", (1, 2))
    assert want["ch"]["family"].tolist() == [[50, 60], [60, 0], [0, 50]]


def test_across_the_2_to_the_32_wrap():
    """tests/hum_wrap_child.py: twin handles on the development build, one aged to just below 2^32, read before the wrap, at it,
    with the window across it and behind it.  One child process (the release library has no test aids)"""
    run_wrap_child("hum_wrap_child.py", 120)
