"""Click detector on the device (WF_HIP_OUT_CLICK) against the numpy restatement (tests/click_ref.py) of the frames pushed: batches
of seven streams, each with another of the definition's inputs in its window and its own write position -- a flat window, one that
wraps round the ring, one behind a wf_hip_reset and a partial refill, one fed a packet longer than the ring, and three more so that
the windows start in all four classes of position modulo 4 -- at FFT 256, 800, 4096 and 16384 with one and with two captured
channels (channel 1 carries another input than channel 0), and one meter batch.  Then slices, refusals, a one-device group and the
2^32 wrap of the counters.

Every integer field is compared for equality and every float32 field within one float32 rounding (click_ref.mismatches);
tests/test_click_cpu.py asserts, for these very windows, the margins that make the integer comparison honest.  The restatement sums
r in the order include/wf_hip.h fixes, so the residual is the same bits on both sides and only log10 is left to differ.

wf_hip_read_async carries the eight outputs of the tick in a fixed record (wf_hip_readback) and no measurement output: there is
nothing of this output to compare through it without a new field, which the ABI does not get here."""
import ctypes as C

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import measure_stagger as ms
import click_ref as ref
from measure_common import check_abi_refusals, run_wrap_child

pytestmark = pytest.mark.gpu
OUT_CLICK = binding.OUT_CLICK  # (the output these tests are about: a library without it fails every one of them)
ERR_INVALID = -1
ENTRY = 464
SR = 48000


def _cfg(fft=4096, channels=2, **kw):
    return wf.Config.defaults(**{**dict(fft_size=fft, sample_rate=SR, capture_channels=channels, stereo=1 if channels == 2 else 0, slope=1.0,
                                        bars=1, floor_db=-70), **kw})


def _check(got, windows, wpos, what=""):
    want = ref.click(windows, SR, wpos)
    assert got.dtype == binding.CLICK_DTYPE and got.shape == want.shape
    c = got["ch"]
    print(f"{what}: P {got['window'].tolist()}, valid {c['valid'].tolist()}, events {c['events'].tolist()}, hit_frames {c['hit_frames'].tolist()}, "
          f"peak_db {c['peak_db'].tolist()}, worst |got - want| in ulps {ref.worst(got, want)}")
    bad = ref.mismatches(got, want)
    assert not bad, bad[:8]
    for s in range(len(got)):  # the slots behind the listed events are zero bytes
        for ch in range(2):
            assert not got["ch"]["ev"][s, ch, int(got["ch"]["listed"][s, ch]):].tobytes().strip(b"\0"), (s, ch)
    return want


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=ref.case_id)
def test_click_equals_the_restatement_of_the_frames(case):
    fft, ch, kw, w = case
    p = ref.window_frames(w)
    rings = ms.Rings(ref.STREAMS, ch, ref.ring_frames(w), 0 if kw.get("meter") else w)
    with wf.SpectrumBatch(_cfg(fft, ch, **kw), ref.STREAMS) as b:
        assert b.fft_size == w and b.ring_frames == rings.ring_cap and b.capture_channels == ch
        assert wf.lib().wf_hip_output_bytes(b.h, OUT_CLICK) == ENTRY  # before the first read
        ms.replay(ref.gpu_script(case), rings, (b,))
        part = np.frombuffer(b"\xff" * (3 * ENTRY), binding.CLICK_DTYPE).copy()  # the first read is a slice: the block is allocated whole
        assert wf.lib().wf_hip_read(b.h, OUT_CLICK, 2, 3, part.ctypes.data_as(C.c_void_p)) == 0
        got = b.click()
        assert part.tobytes() == got[2:5].tobytes() and b.click(6, 1).tobytes() == got[6:].tobytes()
        assert b.click().tobytes() == got.tobytes()  # the same frames, the same bits
    wpos = rings.counter.astype(np.int64)
    assert np.all(got["window"] == p) and np.all(got["order"] == ref.ORDER) and not got["reserved"].any()
    if ch == 1:
        assert not got["ch"][:, 1].tobytes().strip(b"\0")  # all zero bytes
    want = _check(got, rings.window(p), wpos, ref.case_id(case))
    assert want["ch"]["valid"][:, 0].tolist() == [1, 1, 1, 1, 1, 1, 0]
    lone = got["ch"][3, 0]  # behind the packet longer than the ring
    assert lone["events"] == 1 and lone["ev"]["start"][0] == p // 2 and lone["ev"]["frame"][0] == (wpos[3] - p + p // 2) % (1 << 32)
    assert lone["ev"]["strength_db"][0] >= 140.0 and lone["ev"]["amplitude"][0] == np.float32(0.25)
    two = got["ch"][0, 0]  # the two clicks in noise, at their frames and with their signs
    assert two["events"] == 2 and two["ev"]["start"][:2].tolist() == [p // 2, p // 4] and two["ev"]["amplitude"][0] > 0 > two["ev"]["amplitude"][1]
    nan = got["ch"][6, 0]
    assert nan["valid"] == 0 and nan["peak_db"] == nan["floor_db"] == nan["prediction_gain_db"] == -np.inf and not nan["ev"].tobytes().strip(b"\0")
    if p == 8192 and ch == 2:
        assert got["ch"]["events"][6, 1] == 12 and got["ch"]["listed"][6, 1] == 8  # the twelve clicks


def test_refusals():
    L = wf.lib()
    with wf.SpectrumBatch(wf.Config.defaults(waveform=1, stereo=1, width=640, meter_ms=100), 2) as b:
        assert L.wf_hip_output_bytes(b.h, OUT_CLICK) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.click()
        assert e.value.code == ERR_INVALID and "waveform batch" in str(e.value) and "click detector" in str(e.value), str(e.value)
        out = np.empty(2, binding.CLICK_DTYPE)
        assert L.wf_hip_read(b.h, OUT_CLICK, 0, 2, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID
        assert b"click detector" in L.wf_hip_last_error(b.h)
    with wf.SpectrumBatch(_cfg(128), 2) as b:  # W < 256
        assert b.fft_size == 128 and L.wf_hip_output_bytes(b.h, OUT_CLICK) == 0
        with pytest.raises(wf.WfHipError) as e:
            b.click()
        assert e.value.code == ERR_INVALID and "at least 256 frames" in str(e.value) and "click detector" in str(e.value), str(e.value)
        assert b.bits().shape == (2,)  # the other readers of such a batch are unharmed
    with wf.SpectrumBatch(_cfg(1024), 2) as b:
        assert L.wf_hip_output_bytes(b.h, OUT_CLICK) == ENTRY  # before the first read
        silent = ref.click(np.zeros((2, 2, 1024), np.float32), SR, [1024, 1024])  # freshly created: valid = 0
        check_abi_refusals(b, OUT_CLICK, binding.CLICK_DTYPE, 2, silent)


def test_a_one_device_group_reads_the_same():
    """wf_hip_multi_read on a group of one device, and of three shards of it, against the plain read of a twin"""
    case = ref.GPU_CASES[3]  # FFT 800, two channels
    fft, ch, kw, w = case
    cfg = _cfg(fft, ch, **kw)
    script = ref.gpu_script(case)
    with wf.SpectrumBatch(cfg, ref.STREAMS) as one, wf.MultiBatch(cfg, ref.STREAMS, [0]) as m1, wf.MultiBatch(cfg, ref.STREAMS, [0, 0, 0]) as m3:
        ms.replay(script, None, (one, m1, m3))
        for m in (m1, m3):
            m.sync()
        want = one.click()
        for m in (m1, m3):
            assert m.click().tobytes() == want.tobytes()
            assert m.click(2, 4).tobytes() == want[2:6].tobytes()
    assert np.all(want["window"] == w) and want["ch"]["events"][0, 0] == 2


def test_across_the_2_to_the_32_wrap():
    """tests/click_wrap_child.py: twin handles on the development build, one aged to just below 2^32, walked across the wrap in
    small hops with a click on each side; each equal to the restatement of its own ring and counter, `frame` included, at every hop.
    One child process (the release library has no test aids)"""
    run_wrap_child("click_wrap_child.py", 90)
