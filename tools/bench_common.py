"""What the read benches of the measurement outputs (tools/<out>_bench.py) share: the timing loops, the alternative a host has to
an output -- the ring windows themselves copied to the host --, and the command line with its one JSON line.  The only place in
tools/ that takes device memory from the HIP runtime the library is linked against.  A bench keeps its docstring, its defaults,
its shapes and the keys of its JSON."""
import argparse
import contextlib
import ctypes as C
import json
import time

import numpy as np
import waveform_amd as wf

PART_BYTES = 512 << 20


def timed(fn, warmup, reads):
    """seconds per call by the host clock, of calls that end in a synchronise"""
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(reads):
        fn()
    return (time.perf_counter() - t0) / reads


def _summary(v):
    return [round(float(np.median(v)), 2), round(min(v), 2), round(max(v), 2)]


def rounds(b, fn, warmup, reads, rounds):
    """per call, in us, [median, min, max] over the rounds: by the host clock, and by device events around the calls -- which
    bracket whatever the call enqueues, a read's copy to the host included: not a kernel's time"""
    L = wf.lib()
    for _ in range(warmup):
        fn()
    host, dev = [], []
    ms = C.c_float(0.0)
    for _ in range(rounds):
        b.sync()
        assert L.wf_hip_time_begin(b.h) == 0
        t0 = time.perf_counter()
        for _ in range(reads):
            fn()
        t1 = time.perf_counter()
        assert L.wf_hip_time_end(b.h, C.byref(ms)) == 0
        host.append((t1 - t0) / reads * 1e6)
        dev.append(float(ms.value) / reads * 1e3)
    return dict(host_us=_summary(host), device_us_incl_copy=_summary(dev))


def host_rounds(fn, warmup, reads, rounds):
    """per call, in us, [median, min, max] over the rounds, by the host clock alone"""
    for _ in range(warmup):
        fn()
    us = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(reads):
            fn()
        us.append((time.perf_counter() - t0) / reads * 1e6)
    return dict(host_us=_summary(us))


@contextlib.contextmanager
def device_block(nbytes):
    """a device block of `nbytes` (the library has no reader for the rings): yields its pointer and hipMemcpy(dst, src, bytes, kind)"""
    L = wf.lib()
    malloc, free, memcpy = L["hipMalloc"], L["hipFree"], L["hipMemcpy"]
    malloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    free.argtypes = [C.c_void_p]
    memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    d = C.c_void_p()
    assert malloc(C.byref(d), nbytes) == 0
    try:
        yield d, memcpy
    finally:
        assert free(d) == 0


def windows_copy(shape, reads, rounds, pageable=False):
    """the windows to the host: a device block of float32 `shape` by hipMemcpy into page-locked memory, host_rounds' figures after
    two warm-up copies -- and, with `pageable`, the same into pageable memory as a second value"""
    nbytes = int(np.prod(shape)) * 4
    with device_block(nbytes) as (d, memcpy):
        pinned = wf.PinnedBuffer(shape)
        try:
            res = host_rounds(lambda: memcpy(C.c_void_p(pinned.ptr), d, nbytes, 2), 2, reads, rounds)  # 2: hipMemcpyDeviceToHost
            if pageable:
                host = np.empty(shape, np.float32)
                res = res, host_rounds(lambda: memcpy(host.ctypes.data_as(C.c_void_p), d, nbytes, 2), 2, reads, rounds)
        finally:
            pinned.close()
    return res


def windows_copy_in_parts(streams, frames, reads, rounds):
    """windows_copy of [streams, 2, frames] in parts of at most PART_BYTES whose times add up: (parts, the figures)"""
    part = max(1, min(streams, PART_BYTES // (2 * frames * 4)))
    one = windows_copy((part, 2, frames), reads, rounds)
    scale = streams / part  # (every part but the last is full: the bytes are what counts)
    return -(-streams // part), {k: [round(v * scale, 1) for v in vals] for k, vals in one.items()}


def parser(warmup, reads, rounds=5, **options):
    """the command line of a bench: one option per keyword, of its default's type and in the keywords' order (--streams 4096,
    --ffts "4096,16384" ...), then --warmup, --reads, --rounds (unless None) and --out"""
    ap = argparse.ArgumentParser()
    for name, default in options.items():
        ap.add_argument("--" + name, type=type(default), default=default)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--reads", type=int, default=reads)
    if rounds is not None:
        ap.add_argument("--rounds", type=int, default=rounds)
    ap.add_argument("--out", default=None)
    return ap


def emit(a, res):
    """the one JSON line, and --out"""
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
