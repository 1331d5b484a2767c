"""numpy restatement of the wire formats' conversions (wf_hip_wire_format, include/wf_hip.h) and channel pick: what the twin
handle of tests/test_gpu_wire.py is fed through the float32 entry points.  A packet is a uint8 array whose last axis holds the
bytes of one sample as they lie in memory.  Checked at the edges by tests/test_wire_cpu.py."""
from __future__ import annotations

import numpy as np

WIRES = ("s24", "s24_be", "s16_be", "ulaw", "alaw")
BYTES = {"s24": 3, "s24_be": 3, "s16_be": 2, "ulaw": 1, "alaw": 1}


def decode_int(b: np.ndarray, wire: str) -> np.ndarray:
    """the signed integer of every sample of a uint8 [..., B] array, int64 [...]"""
    b = np.asarray(b)
    assert b.dtype == np.uint8 and b.shape[-1] == BYTES[wire], (b.dtype, b.shape, wire)
    x = b.astype(np.int64)
    if wire in ("s24", "s24_be"):
        lo, mid, hi = (x[..., 0], x[..., 1], x[..., 2]) if wire == "s24" else (x[..., 2], x[..., 1], x[..., 0])
        v = lo | mid << 8 | hi << 16
        return v - ((v & 0x800000) << 1)
    if wire == "s16_be":
        v = x[..., 0] << 8 | x[..., 1]
        return v - ((v & 0x8000) << 1)
    if wire == "ulaw":
        u = ~x[..., 0] & 0xFF
        e, m = (u >> 4) & 7, u & 15
        mag = (((m << 3) + 0x84) << e) - 0x84
        return np.where(u & 0x80, -mag, mag)
    assert wire == "alaw", wire
    a = x[..., 0] ^ 0x55
    e, m = (a >> 4) & 7, a & 15
    mag = np.where(e > 0, ((m << 4) + 0x108) << np.maximum(e - 1, 0), (m << 4) + 8)
    return np.where(a & 0x80, mag, -mag)


def decode(b: np.ndarray, wire: str) -> np.ndarray:
    """float32 [...] of a uint8 [..., B] array: the integer (exact in float32: 24 bits at most) times 2^-23 (s24, s24_be) or
    2^-15 (s16_be, G.711), one float32 multiply"""
    scale = np.float32(2.0 ** -23 if wire in ("s24", "s24_be") else 2.0 ** -15)
    return decode_int(b, wire).astype(np.float32) * scale


def captured(packet: np.ndarray, wire: str, interleaved: bool, channel_base: int, capture_channels: int) -> np.ndarray:
    """the float32 planar packet [count][capture_channels][frames] the float entry points would be given"""
    x = decode(packet, wire)
    planar = x.transpose(0, 2, 1) if interleaved else x
    return np.ascontiguousarray(planar[:, channel_base:channel_base + capture_channels, :])


def random_packet(rng: np.random.Generator, wire: str, count: int, channels: int, frames: int, interleaved: bool) -> np.ndarray:
    """uint8 [count][frames][channels][B] (interleaved) or [count][channels][frames][B]: every code equally likely.  Where the
    packet has room for them, the first samples are the format's extremes (s24: -2^23, 2^23 - 1, -1, 0) or, for G.711, every one
    of the 256 bytes."""
    shape = (count, frames, channels) if interleaved else (count, channels, frames)
    pkt = rng.integers(0, 256, shape + (BYTES[wire],), dtype=np.uint8)
    flat = pkt.reshape(-1, BYTES[wire])
    if wire in ("s24", "s24_be"):
        edges = np.array([[0x00, 0x00, 0x80], [0xFF, 0xFF, 0x7F], [0xFF, 0xFF, 0xFF], [0x00, 0x00, 0x00]], np.uint8)
        edges = edges if wire == "s24" else edges[:, ::-1]
    elif wire == "s16_be":
        edges = np.array([[0x80, 0x00], [0x7F, 0xFF], [0xFF, 0xFF], [0x00, 0x00]], np.uint8)
    else:
        edges = np.arange(256, dtype=np.uint8)[:, None]
    n = min(len(edges), len(flat))
    flat[:n] = edges[:n]
    return pkt
