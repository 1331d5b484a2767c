"""numpy restatement of wf_hip_push_pcm's sample conversion (include/wf_hip.h) and channel pick: what the twin handle of
tests/test_gpu_pcm.py is fed through the float32 entry points.  Checked at the edges by tests/test_pcm_cpu.py."""
from __future__ import annotations

import numpy as np

DTYPES = (np.uint8, np.int16, np.int32, np.float32)


def to_float(x: np.ndarray) -> np.ndarray:
    """u8: (x - 128) * 2^-7, s16: x * 2^-15, s32: (float)x * 2^-31 (the int -> float cast rounds to nearest even), f32 as is"""
    if x.dtype == np.uint8:
        return (x.astype(np.int32) - 128).astype(np.float32) * np.float32(2.0 ** -7)
    if x.dtype == np.int16:
        return x.astype(np.float32) * np.float32(2.0 ** -15)
    if x.dtype == np.int32:
        return x.astype(np.float32) * np.float32(2.0 ** -31)
    assert x.dtype == np.float32, x.dtype
    return x.copy()


def captured(packet: np.ndarray, interleaved: bool, channel_base: int, capture_channels: int) -> np.ndarray:
    """the float32 planar packet [count][capture_channels][frames] the float entry points would be given"""
    planar = packet.transpose(0, 2, 1) if interleaved else packet
    return np.ascontiguousarray(to_float(planar[:, channel_base:channel_base + capture_channels, :]))


def random_packet(rng: np.random.Generator, dtype, count: int, channels: int, frames: int, interleaved: bool) -> np.ndarray:
    """full-scale noise in the packet's own format (float32: uniform in [-1, 1))"""
    shape = (count, frames, channels) if interleaved else (count, channels, frames)
    dt = np.dtype(dtype)
    if dt == np.float32:
        return rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)
