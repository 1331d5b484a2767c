"""The multi-device group (waveform_amd/csrc/wf_hip_multi.cpp) without a device and without a sanitizer: the product's source
over the host-only mock of the HIP runtime and of the wf_hip_* calls it makes (tests/mock/mock_device.cpp), built plain
(build/libwfmulti_plain.so, tests/mock/Makefile).  What create decides and says -- the note wf_hip_multi_last_error gives right
after it, the refusal of a bad WF_HIP_MULTI_TRANSPORT --, what a gather does when a shard's mirror buffers were handed over
behind the group's back, and ranges that do not cover the whole group.  The environment is read at create, so every case is a
child process with its own WF_HIP_MULTI_* / WF_MOCK_* variables; the test adds no sanitizer's runtime."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
MOCK = ROOT / "tests" / "mock"
LIB = ROOT / "build" / "libwfmulti_plain.so"

# every child: tests/mock/multi_stress.py's bindings (ms.L), its group() and its expected(), plus the calls it does not declare
PRELUDE = r"""
import ctypes as C, sys
import numpy as np
sys.argv = ["multi_stress.py", %r]
sys.path.insert(0, %r)
import multi_stress as ms
L, vp, u32, fp = ms.L, ms.vp, ms.u32, ms.fp
L.wf_hip_bars_mirror_ready.argtypes = [vp, vp, C.POINTER(vp)]
L.wf_hip_multi_gather_stream.restype = vp
L.wf_hip_multi_gather_stream.argtypes = [vp, u32]
L.mock_mirror_buffers.restype = u32
L.mock_mirror_buffers.argtypes = [vp]
P = ms.TickParams(1 / 60, 0, 0.0, 0, 0)
INVALID, RUNTIME = -1, -4  # WF_HIP_ERR_*
def err(m=None): return L.wf_hip_multi_last_error(m).decode()
def shard(m, i): return L.wf_hip_multi_shard(m, i, None, None, None)
def ticked(m, streams, n=1):
    assert L.wf_hip_multi_push_synth(m, 0, streams, 1, 0, 0, 800) == 0
    for _ in range(n):
        assert L.wf_hip_multi_tick(m, C.byref(P)) == 0
def gathered(m, i, streams):
    out = np.empty((streams, 2, 26), np.float32)
    assert L.wf_hip_multi_read_gathered(m, i, out.ctypes.data_as(fp)) == 0, err(m)
    return out
""" % (str(LIB), str(MOCK))


@pytest.fixture(scope="module", autouse=True)
def _library():
    if not LIB.exists():
        subprocess.run(["make", "-C", str(MOCK), str(Path("..") / ".." / "build" / LIB.name)], capture_output=True)
    assert LIB.exists(), f"{LIB} not built (make -C tests/mock)"


def _child(code, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith(("WF_HIP_MULTI_", "WF_MOCK_"))}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", PRELUDE + code], capture_output=True, text=True, timeout=120, env=e, cwd=ROOT)
    assert r.returncode == 0 and "done" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout


def test_the_stress_script_passes_over_the_plain_build():
    r = subprocess.run([sys.executable, str(MOCK / "multi_stress.py"), str(LIB)], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "multi stress ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# the note of a group on the peer transport: devices, streams, extra environment, what the note must (not) contain, buffers per
# mirror set on every shard's handle (the number of devices: the tick kernels store into every device's result themselves)
NOTES = {
    "peer access everywhere": ([0, 1, 2, 3], 13, {}, None, 4),
    "one pair denied": ([0, 1, 2, 3], 13, {"WF_MOCK_DENY_PEER": "2:1"}, ["peer access is not enabled from device 2 to device 1", "hipMemcpyPeerAsync"], 0),
    "nine shards": ([0, 1, 2, 3, 0, 1, 2, 3, 0], 20, {}, ["9 devices", "at most 8"], 0),
    "WF_HIP_MULTI_MIRROR=send": ([0, 1, 2, 3], 13, {"WF_HIP_MULTI_MIRROR": "send"}, ["WF_HIP_MULTI_MIRROR=send"], 1),
    "WF_HIP_MULTI_MIRROR=0": ([0, 1, 2, 3], 13, {"WF_HIP_MULTI_MIRROR": "0"}, ["WF_HIP_MULTI_MIRROR=0"], 0),
}


@pytest.mark.parametrize("case", list(NOTES))
def test_the_note_after_create_names_the_real_cause(case):
    """why the tick kernels do not store into every device's result themselves: the pair that has no peer access (that wording
    for that cause alone), the limit of wf_hip_set_bars_mirrors, or the variable that asked; "" where they do.  The gathered
    result is every stream's bars on every device either way."""
    devices, streams, env, want, buffers = NOTES[case]
    code = r"""
devices, streams, want, buffers = %r, %r, %r, %r
m = ms.group(devices, streams)
note = err(m)
assert L.wf_hip_multi_transport(m) == b"peer"
if want is None:
    assert note == "", note
else:
    assert all(w in note for w in want), note
    assert ("peer access" in note) == ("peer access" in want[0]), note
    assert "from device" not in want[0] or note.count("device ") == 2, note   # (exactly that pair: no other is named)
assert [L.mock_mirror_buffers(shard(m, i)) for i in range(len(devices))] == [buffers] * len(devices)
for t in (1, 2, 3):
    ticked(m, streams)
    assert L.wf_hip_multi_allgather_bars(m) == 0, err(m)
    for i in range(len(devices)):
        assert np.array_equal(gathered(m, i, streams), ms.expected(streams, t)), (i, t)
L.wf_hip_multi_destroy(m)
print("done")
""" % (devices, streams, want, buffers)
    _child(code, WF_HIP_MULTI_TRANSPORT="peer", **env)


def test_a_bad_transport_name_is_refused():
    _child(r"""
cfg = ms.Config()
cfg.fft_size, cfg.sample_rate, cfg.capture_channels, cfg.stereo, cfg.bars = 2048, 48000, 2, 1, 1
m = vp()
assert L.wf_hip_multi_create(C.byref(cfg), (C.c_int * 2)(0, 1), 2, 8, 0, C.byref(m)) == INVALID and not m.value
assert err() == "WF_HIP_MULTI_TRANSPORT=bogus: expected rccl or peer", err()
print("done")
""", WF_HIP_MULTI_TRANSPORT="bogus")


@pytest.mark.parametrize("timed", [False, True])
def test_a_mirror_handed_over_outside_the_group_fails_the_gather(timed):
    """wf_hip_bars_mirror_ready on ONE shard handle (the header forbids it): that shard's next hand-over is the other buffer, the
    pieces of a result would lie in different buffers.  wf_hip_multi_allgather_bars says so, and so does a gathering
    wf_hip_multi_time_ticks (after its workers are back); the exchange is then out of service and everything else goes on."""
    _child(r"""
timed, streams = %d, 10
m = ms.group([0, 1, 2], streams)
assert [L.mock_mirror_buffers(shard(m, i)) for i in range(3)] == [3, 3, 3]
ticked(m, streams)
assert L.wf_hip_multi_allgather_bars(m) == 0 and np.array_equal(gathered(m, 2, streams), ms.expected(streams, 1))
buf = vp()
assert L.wf_hip_bars_mirror_ready(shard(m, 1), L.wf_hip_multi_gather_stream(m, 1), C.byref(buf)) == 0
ms_, per = C.c_float(0), (C.c_float * 3)()
if timed:
    assert L.wf_hip_multi_time_ticks(m, C.byref(P), 4, 0, 1, C.byref(ms_), per) == RUNTIME
else:
    assert L.wf_hip_multi_tick(m, C.byref(P)) == 0
    assert L.wf_hip_multi_allgather_bars(m) == RUNTIME
assert "shard 1 handed over bars buffer" in err(m) and "handed over or replaced outside the group" in err(m), err(m)
ticks = 5 if timed else 2
assert L.wf_hip_multi_allgather_bars(m) == RUNTIME and "out of service" in err(m), err(m)
assert L.wf_hip_multi_time_ticks(m, C.byref(P), 2, 0, 1, C.byref(ms_), per) == RUNTIME and "out of service" in err(m)
out = np.empty((streams, 2, 26), np.float32)
assert L.wf_hip_multi_read_gathered(m, 0, out.ctypes.data_as(fp)) == RUNTIME and "out of service" in err(m)
assert L.wf_hip_multi_tick(m, C.byref(P)) == 0 and L.wf_hip_multi_sync(m) == 0
assert L.wf_hip_multi_read(m, ms.OUT_BARS, 0, streams, out.ctypes.data_as(vp)) == 0 and np.array_equal(out, ms.expected(streams, ticks + 1))
assert L.wf_hip_multi_time_ticks(m, C.byref(P), 3, 0, 0, C.byref(ms_), per) == 0
L.wf_hip_multi_destroy(m)
print("done")
""" % int(timed), WF_HIP_MULTI_TRANSPORT="peer", WF_HIP_MULTI_MIRROR="1")


def test_hidden_masks_over_ranges_that_span_and_that_stay_inside_shards():
    """wf_hip_multi_set_hidden and wf_hip_multi_read(WF_HIP_OUT_LAST_SILENT) with ranges cut at the shard boundaries: 10 streams in
    shards of 4, 3 and 3 -- a range that touches all three, one inside the middle shard, one stream at a boundary"""
    _child(r"""
streams = 10
m = ms.group([0, 1, 2], streams)
model = np.zeros(streams, np.uint8)
rng = np.random.default_rng(7)
for first, count in ((2, 7), (5, 2), (0, 10), (4, 1), (3, 2), (9, 1)):
    mask = rng.integers(0, 2, count).astype(np.uint8)
    mask[0] = 1
    assert L.wf_hip_multi_set_hidden(m, first, count, mask.ctypes.data_as(C.POINTER(C.c_uint8))) == 0, err(m)
    model[first:first + count] = mask
    for f, c in ((first, count), (0, streams), (5, 2), (2, 7)):
        back = np.full(c, 255, np.uint8)
        assert L.wf_hip_multi_read(m, ms.OUT_LAST_SILENT, f, c, back.ctypes.data_as(vp)) == 0, err(m)
        assert np.array_equal(back, model[f:f + c]), (first, count, f, c, back, model)
assert L.wf_hip_multi_set_hidden(m, 8, 3, model.ctypes.data_as(C.POINTER(C.c_uint8))) == INVALID and "outside 0..10" in err(m)
assert L.wf_hip_multi_set_hidden(m, 0, 2, None) == INVALID and err(m) == "mask is NULL"
L.wf_hip_multi_destroy(m)
print("done")
""", WF_HIP_MULTI_TRANSPORT="peer")
