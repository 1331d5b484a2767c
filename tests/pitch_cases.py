"""The seeded inputs of the pitch tests, shared by tests/test_pitch_cpu.py (which shows that every one of them is well
conditioned for the reference alone) and tests/test_gpu_pitch.py (which feeds the same frames to the device): analytic
windows, banks of pitched and unpitched streams, and the fuzz scripts -- lists of pushes, ragged pushes, resets, ticks and
reads that depend on the family alone, never on a device."""
import numpy as np

SR = 48000
SEED = 20261016


def sine(hz, n, amp=0.5, phase=0.0, sr=SR):
    return (amp * np.sin(2 * np.pi * hz * np.arange(n) / sr + phase)).astype(np.float32)


def harmonics_without_fundamental(n, f0=220.0, sr=SR):
    t = np.arange(n) / sr
    return (0.2 * sum(np.sin(2 * np.pi * k * f0 * t + 0.3 * k) for k in range(2, 6))).astype(np.float32)


def white_noise(n, seed=1):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, n).astype(np.float32)


SINES = (55.0, 110.0, 440.0, 997.3, 3000.0)


def analytic(n):
    """name -> mono float32 [n]"""
    c = {f"sine{hz:g}": sine(hz, n) for hz in SINES}
    c["missing_fundamental"] = harmonics_without_fundamental(n)
    c["noise"] = white_noise(n)
    c["silence"] = np.zeros(n, np.float32)
    c["constant"] = np.full(n, 0.1, np.float32)  # (0.1f squared is not a short binary fraction: its sums round)
    return c


def bank(seed, streams, cap, total, sr=SR):
    """float32 [streams, cap, total]: stream s is, by s mod 4, a pure sine, a sine with harmonics and noise, white noise, or
    a fundamental with harmonics whose second channel differs in level and phase; 40 Hz to 5 kHz, log-uniform"""
    rng = np.random.default_rng(seed)
    t = np.arange(total) / sr
    out = np.empty((streams, cap, total), np.float32)
    for s in range(streams):
        f0 = float(np.exp(rng.uniform(np.log(40.0), np.log(5000.0))))
        amp = float(rng.uniform(0.05, 0.9))
        kind = s % 4
        for c in range(cap):
            ph = float(rng.uniform(0, 2 * np.pi))
            if kind == 0:
                x = amp * np.sin(2 * np.pi * f0 * t + ph)
            elif kind == 1:
                x = amp * (np.sin(2 * np.pi * f0 * t + ph) + 0.5 * np.sin(4 * np.pi * f0 * t + 2 * ph) + 0.25 * np.sin(6 * np.pi * f0 * t))
                x = x / 1.75 + rng.normal(0, 0.02 * amp, total)
            elif kind == 2:
                x = rng.uniform(-amp, amp, total)
            else:
                g = 1.0 if c == 0 else 0.4
                x = g * amp * (0.6 * np.sin(2 * np.pi * f0 * t + ph) + 0.4 * np.sin(4 * np.pi * f0 * t + ph)) + rng.normal(0, 0.01, total)
            out[s, c] = x.astype(np.float32)
    return out


def ring_capacity(fft, ring_frames=0):
    want = max(ring_frames, fft) if ring_frames else max(2 * fft, 4096)
    return 1 << (want - 1).bit_length()


FUZZ = [  # (fft_size -- of a meter batch: the buffer meter_ms makes --, capture channels, config overrides, ring_frames of create)
    (128, 2, {}, 0), (800, 2, {}, 0), (800, 1, {}, 1000), (2048, 1, {}, 2048), (4096, 2, {}, 4896), (16384, 1, {}, 0),
    (65536, 2, {}, 0), (2400, 2, dict(meter=1, bars=0, meter_ms=50), 0), (960, 1, dict(meter=1, bars=0, meter_rms=1, meter_ms=20), 0),
]
FUZZ_IDS = [f"n{f}_cap{c}" + ("_meter" if k.get("meter") else "") for f, c, k, _ in FUZZ]
FUZZ_STREAMS = 4


def fuzz_script(fft, cap, kw, ring_frames):
    """the steps of one family: ("push", first, x) | ("ragged", x, frames) | ("reset", first, count) | ("tick",) | ("read",).
    Frames come from one long bank per stream, in order, so pitched streams stay continuous across pushes; the lengths leave
    the window at every alignment and across the ring's wrap."""
    streams = FUZZ_STREAMS
    rng = np.random.default_rng(SEED + fft * 3 + cap + (7 if kw.get("meter") else 0))
    W, ring = fft, ring_capacity(fft, ring_frames)
    P = min(W, 4096)
    total = 3 * ring + 8 * W + 64 * 1024
    src = bank(int(rng.integers(1 << 30)), streams, cap, total)
    at = np.zeros(streams, np.int64)  # frames of the bank consumed per stream
    steps = [("read",)]               # freshly created: zeros

    def take(first, n):
        """the next n frames of streams [first, streams)"""
        x = np.stack([src[s, :, at[s]:at[s] + n] for s in range(first, streams)])
        assert x.shape[2] == n
        at[first:] += n
        return x

    def ragged(width):
        frames = rng.integers(0, width + 1, streams).astype(np.uint32)
        x = np.zeros((streams, cap, width), np.float32)
        for s in range(streams):
            n = int(frames[s])
            x[s, :, :n] = src[s, :, at[s]:at[s] + n]
            at[s] += n
        return ("ragged", x, frames)

    steps += [("push", 0, take(0, int(rng.integers(1, P // 3 + 1)))), ("read",)]  # a window not yet filled
    steps += [("push", 0, take(0, W + int(rng.integers(1, 100)))), ("read",)]     # filled, at an odd offset
    steps += [ragged(min(W, 3000) + 3), ("read",)]                                # every stream at its own alignment
    for _ in range(3):                                                            # small odd hops to a slice of streams
        f0 = int(rng.integers(0, streams))
        steps.append(("push", f0, take(f0, int(rng.integers(1, 8)))))
    steps += [("tick",), ("read",)]
    steps += [("push", 0, take(0, ring + int(rng.integers(1, 300)))), ("read",)]  # longer than the ring
    steps += [("reset", 1, 2), ("push", 0, take(0, int(rng.integers(P // 2, P)))), ("read",)]  # a reset in the middle
    steps += [("push", 0, take(0, ring - int(rng.integers(1, 64)))), ("tick",), ("read",)]     # once round the ring
    steps += [ragged(min(W, 2000) + 1), ("read",)]
    return steps


def replay(steps, hist, on_read, batch=None, pinned=None):
    """runs a script against a signal_ref.History and, when given, a batch (`pinned`: a factory of PinnedBuffer for the
    ragged pushes); calls on_read(index) at every read"""
    reads = 0
    for st in steps:
        if st[0] == "push":
            _, first, x = st
            hist.push(x, first=first)
            if batch is not None:
                batch.push_audio(x, first=first)
        elif st[0] == "ragged":
            _, x, frames = st
            hist.push(x, frames=frames)
            if batch is not None:
                pin = pinned(x.shape)
                try:
                    batch.ingest_done(0)
                    pin.array[...] = x
                    batch.push_audio_ragged_async(pin, frames, x.shape[2], 0)
                    batch.sync()
                finally:
                    pin.close()
        elif st[0] == "reset":
            hist.reset(st[1], st[2])
            if batch is not None:
                batch.reset(st[1], st[2])
        elif st[0] == "tick":
            if batch is not None:
                batch.tick()
        else:
            on_read(reads)
            reads += 1
    return reads
