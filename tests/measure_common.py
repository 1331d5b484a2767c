"""What the GPU tests of the measurement outputs (tests/test_gpu_<out>.py) share, written once.

A new output's test file takes from here:
  Hip                        device buffers for its push-path test (push_audio_device)
  packets                    uneven packet cuts for its cases against the restatement
  check_slices_and_repeats   the tail of test_repeated_reads_and_slices
  check_abi_refusals         the C-ABI tail of test_refusals: five refused wf_hip_read calls, then a good one
  check_shards_match         the tail of test_three_shards_match_one_handle
  run_wrap_child             test_across_the_2_to_the_32_wrap: tests/<out>_wrap_child.py, which is written over the twin walk of
                             tests/wrap_child.py (twins, Walk) and states only its audio and what it compares at a read
and writes itself what is the output's own knowledge: `_cfg` (the defaults differ between outputs), `_check` against its
tests/<out>_ref.py, its cases and signal kinds, the words its refusals must name, and every expected value it pins -- those stay at
the call site, behind the helper's return value."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

import waveform_amd as wf

ROOT = Path(__file__).resolve().parent.parent
ERR_INVALID = -1


class Hip:
    """device buffers from the HIP runtime the library is linked against, looked up through the library's own handle"""

    def __init__(self):
        L = wf.lib()
        self.malloc, self.free, self.memcpy = L["hipMalloc"], L["hipFree"], L["hipMemcpy"]
        self.malloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.free.argtypes = [C.c_void_p]
        self.memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def upload(self, arr):
        p = C.c_void_p()
        assert self.malloc(C.byref(p), arr.nbytes) == 0
        assert self.memcpy(p, arr.ctypes.data_as(C.c_void_p), arr.nbytes, 1) == 0  # hipMemcpyHostToDevice
        return p.value


def packets(rng, total, most):
    """(lo, hi) of uneven packets of 1..most frames that add up to `total`"""
    cuts, at = [], 0
    while at < total:
        n = min(int(rng.integers(1, most + 1)), total - at)
        cuts.append((at, at + n))
        at += n
    return cuts


def run_wrap_child(name, seconds):
    """tests/<name> in one child process on the development build (the release library has no test aids), ended after `seconds`"""
    env = dict(os.environ, WF_HIP_LIB=str(ROOT / "waveform_amd" / "libwaveform_hip_dev.so"))
    r = subprocess.run([sys.executable, str(ROOT / "tests" / name)], capture_output=True, text=True, timeout=seconds, env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "wrapped ok" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])


def check_abi_refusals(b, out_id, dtype, streams, zero=None):
    """wf_hip_read refuses a NULL `out`, a range past the batch from 0 and from behind the last stream, count 0 and a NULL handle;
    the good read after them is returned, and is `zero`'s bytes where the caller knows a fresh handle's entry"""
    L = wf.lib()
    assert L.wf_hip_read(b.h, out_id, 0, 1, None) == ERR_INVALID
    out = np.empty(streams + 1, dtype)
    ptr = out.ctypes.data_as(C.c_void_p)
    assert L.wf_hip_read(b.h, out_id, 0, streams + 1, ptr) == ERR_INVALID  # past the batch
    assert L.wf_hip_read(b.h, out_id, streams, 1, ptr) == ERR_INVALID
    assert L.wf_hip_read(b.h, out_id, 0, 0, ptr) == ERR_INVALID  # count 0
    assert L.wf_hip_read(None, out_id, 0, 1, ptr) == ERR_INVALID
    assert L.wf_hip_read(b.h, out_id, 0, streams, ptr) == 0
    if zero is not None:
        assert out[:streams].tobytes() == zero.tobytes()  # the next good read is correct
    return out[:streams]


def check_slices_and_repeats(b, reader):
    """on a batch of five streams nothing has read yet: a slice as the first read equals the entry of the full read, a tail slice
    its tail; repeated reads, and a read after a tick, are bit-identical.  Returns the full read"""
    read = getattr(b, reader)
    part = read(1, 1)  # the first read is a slice: the block is allocated whole
    full = read()
    assert part.shape == (1,) and part.tobytes() == full[1:2].tobytes()
    assert read(3, 2).tobytes() == full[3:].tobytes()
    for _ in range(3):
        assert read().tobytes() == full.tobytes()
    b.tick()
    assert read().tobytes() == full.tobytes()  # a tick does not move the rings
    return full


def check_shards_match(one, multi, reader, span):
    """a group's read equals one handle's: the whole, `span` = (first, count), a range that spans the shards, and the shape.
    Returns the one handle's read"""
    want = getattr(one, reader)()
    assert getattr(multi, reader)().tobytes() == want.tobytes()
    first, count = span
    assert getattr(multi, reader)(first, count).tobytes() == want[first:first + count].tobytes()
    assert getattr(multi, reader)().shape == (one.streams,)
    return want
