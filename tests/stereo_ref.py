"""Float64 restatement of WF_HIP_OUT_STEREO (include/wf_hip.h, "stereo image"): correlation, coherence, phase and balance
between captured channels 0 and 1 in each third-octave band, from the newest P frames of both channels and the sample rate
alone, with numpy's FFT.  The tests compare the device against it; nothing here knows how the device transforms or sums.  Also
the test signal the device tests push (audio)."""
import numpy as np

import bands_ref

NUM_BANDS = bands_ref.NUM_BANDS
MAX_WINDOW = 4096  # WF_HIP_STEREO_MAX_WINDOW
DEAD_RATIO = 2.0 ** -80  # WF_HIP_STEREO_DEAD_RATIO
FIELDS = ("correlation", "coherence", "phase_deg", "balance_db")
STEREO_DTYPE = np.dtype([(n, np.float32, (NUM_BANDS,)) for n in FIELDS] + [("covered", np.uint32), ("window", np.uint32)])


def window_frames(fft_size):
    """P: the largest power of two <= min(fft_size, MAX_WINDOW)"""
    p = 1
    while 2 * p <= min(fft_size, MAX_WINDOW):
        p *= 2
    return p


def band_sums(frames, sr):
    """frames: float32 [streams, 2, P], P a power of two.  A, B (float64 [streams, 31]) and X (complex128 [streams, 31])"""
    x = np.asarray(frames, np.float32).astype(np.float64)
    p = x.shape[-1]
    assert x.shape[1] == 2 and p & (p - 1) == 0
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(p) / p)
    z = np.fft.fft(w * (x[:, 0] + 1j * x[:, 1]), axis=-1)
    k = np.arange(1, p // 2)
    zk, zc = z[:, k], np.conj(z[:, p - k])
    l, r = (zk + zc) / 2.0, (zk - zc) / 2.0j
    wt = bands_ref.bin_weights(sr, p)[:, 1:]  # [31, P/2 - 1]: bins 1 .. P/2 - 1
    a = (np.abs(l) ** 2) @ wt.T
    b = (np.abs(r) ** 2) @ wt.T
    xx = (l * np.conj(r)) @ wt.T
    return a, b, xx


def fields_of_sums(a, b, xx, sr, p):
    """the struct of band sums A, B [..., 31] and X [..., 31]"""
    out = np.zeros(a.shape[:-1], STEREO_DTYPE)
    # a channel more than 2^-80 (-240.8 dB) under the other is the transform's rounding, not a signal: it counts as 0
    a, b = np.where(a > b * DEAD_RATIO, a, 0.0), np.where(b > a * DEAD_RATIO, b, 0.0)
    both = (a > 0) & (b > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.sqrt(a * b)
        out["correlation"] = np.where(both, np.clip(xx.real / d, -1.0, 1.0), 0.0)
        out["coherence"] = np.where(both, np.clip(np.abs(xx) / d, 0.0, 1.0), 0.0)
        ph = np.where(both, np.arctan2(xx.imag, xx.real) * (180.0 / np.pi), 0.0).astype(np.float32)
        out["phase_deg"] = np.where(ph == np.float32(-180.0), np.float32(180.0), ph)
        out["balance_db"] = np.where(both, 10.0 * np.log10(b / a), np.where(a > 0, -np.inf, np.where(b > 0, np.inf, 0.0)))
    out["covered"] = bands_ref.covered(sr, p)
    out["window"] = p
    return out


def stereo(frames, sr):
    """frames: float32 [streams, 2, W]: the newest W = fft_size frames of every stream's two rings, the newest last; the window
    is the newest P = window_frames(W) of them"""
    frames = np.asarray(frames, np.float32)
    p = window_frames(frames.shape[-1])
    a, b, xx = band_sums(frames[..., -p:], sr)
    return fields_of_sums(a, b, xx, sr, p)


def overlapping(sr, p):
    """[31] bool: the bands that overlap bins 1 .. P/2 - 1"""
    return bands_ref.bin_weights(sr, p)[:, 1:].sum(axis=1) > 0.0


def low_coherence_share(want, sr, below=0.01):
    """the share of the overlapping bands of `want` ([streams] structs) whose coherence is under `below`"""
    live = overlapping(sr, int(want["window"].flat[0]))
    return float((want["coherence"][:, live] < below).mean())


def mismatches(got, want):
    """(field, index, got, want) of every value outside the contract's bound: |got - want| <= max(1 float32 ulp of want, 1e-9) for
    correlation, coherence and balance_db -- infinities exactly where `want` has them --, the same for phase_deg in the bands where
    want's coherence is >= 0.01 (the phase is not compared below that), `covered` and `window` equal"""
    bad = []
    for name in FIELDS:
        g, w = got[name], want[name]
        inf = np.isinf(w)
        with np.errstate(invalid="ignore"):
            ok = np.where(inf, g == w, np.abs(g.astype(np.float64) - w.astype(np.float64))
                          <= np.maximum(np.spacing(np.abs(w)).astype(np.float64), 1e-9))
        ok &= np.isfinite(g) | inf
        if name == "phase_deg":
            ok |= want["coherence"] < 0.01
        bad += [(name, tuple(i), float(g[tuple(i)]), float(w[tuple(i)])) for i in np.argwhere(~ok)[:5]]
    for name in ("covered", "window"):
        bad += [(name, tuple(i), int(got[name][tuple(i)]), int(want[name][tuple(i)])) for i in np.argwhere(got[name] != want[name])[:5]]
    return bad


def audio(rng, streams, frames, sr):
    """float32 [streams, 2, frames]: l = 0.3 n + 0.2 sin(2 pi 997 t / sr), r = 0.2 roll(n, 3) + 0.15 m + 0.2 sin(2 pi 997 t / sr + 1),
    n and m independent unit Gaussian noise: partly coherent everywhere (r carries l's noise three frames late), a phase that
    turns with frequency, and a tone with a fixed phase"""
    t = np.arange(frames)
    n = rng.standard_normal((streams, frames))
    m = rng.standard_normal((streams, frames))
    l = 0.3 * n + 0.2 * np.sin(2.0 * np.pi * 997.0 * t / sr)
    r = 0.2 * np.roll(n, 3, axis=-1) + 0.15 * m + 0.2 * np.sin(2.0 * np.pi * 997.0 * t / sr + 1.0)
    return np.stack([l, r], axis=1).astype(np.float32)
