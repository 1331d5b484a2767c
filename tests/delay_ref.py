"""Numpy float64 restatement of WF_HIP_OUT_DELAY (include/wf_hip.h, "inter-channel delay"): by how many frames captured channel 0
lags channel 1 and whether one of them is inverted, from the floored-PHAT cross-correlation of the newest P frames of both rings
through the periodic Hann taper.  Nothing here knows how the device transforms, separates the channels or reduces: every channel is
transformed on its own by numpy.fft and the correlations come from an inverse transform of the weighted cross spectrum.  For the
comparison of orderings (tests/test_delay_cpu.py) three more orders of the same operations: "radix2", every transform by the
hand-written radix-2 of tests/thd_ref.py; "joint", both channels through one complex transform and separated behind it; "packed",
joint and then both correlations out of one forward transform of A + j G / g, with A taken back out of that spectrum for the phase
regression.  Also the signal kinds the tests push and the cases the CPU and the device tests share.

Bound of `mismatches`: lag, polarity, valid, window and the reserved words equal; delay_frames within 1e-7 frame; every float32
field and curve entry within max(1 float32 ulp of the wanted value, 1e-6).  It is derived, not measured: both sides work in float64
from the same float32 samples and differ only in the order of operations, the four orders here agree to some 1e-11 in every field
(test_delay_cpu.py asserts 1e-9 on the cases below and prints the figure), and no decision is near a tie there -- the winning |R|
exceeds every other lag's by at least 1e-3 relative, no weighted bin's phase is near +-pi, the fraction is not near its clamp -- so
one float32 rounding is all that can separate the device from the restatement."""
import numpy as np

from thd_ref import fft_radix2, ring_frames  # noqa: F401  (ring_frames: for the tests)

MAX_WINDOW = 4096  # WF_HIP_DELAY_MAX_WINDOW
CURVE = 65         # WF_HIP_DELAY_CURVE
BETA = 1e-3        # the floor of the PHAT weighting
DELAY_DTYPE = np.dtype([("delay_frames", np.float64), ("delay_ms", np.float32), ("peak", np.float32), ("corr", np.float32),
                        ("corr_zero", np.float32), ("ambiguity", np.float32), ("lag", np.int32), ("polarity", np.int32),
                        ("valid", np.uint32), ("window", np.uint32), ("reserved", np.uint32), ("curve", np.float32, (CURVE,)),
                        ("reserved2", np.uint32, (3,))])
FIELDS = DELAY_DTYPE.names
FLOAT_FIELDS = ("delay_ms", "peak", "corr", "corr_zero", "ambiguity", "curve")
INT_FIELDS = ("lag", "polarity", "valid", "window", "reserved", "reserved2")
ORDERS = ("numpy", "radix2", "joint", "packed")


def window_frames(w):
    """P of a handle whose wf_hip_fft_size() is w: the largest power of two <= min(w, MAX_WINDOW)"""
    p = 1
    while 2 * p <= min(int(w), MAX_WINDOW):
        p *= 2
    return p


def taper(p):
    """float64 [p]: the periodic Hann window, in long double with the argument reduced as an integer first"""
    ld = np.longdouble
    two_pi = ld(2) * ld("3.14159265358979323846264338327950288")
    i = np.arange(p, dtype=np.int64)
    return (ld("0.5") - ld("0.5") * np.cos(two_pi * (i % p).astype(ld) / ld(p))).astype(np.float64)


def _inverse(spec, forward):
    """sum_k spec[k] e^(+j 2 pi k n / P) for every n, through a forward transform"""
    return np.conj(forward(np.conj(spec)))


def analyse(x0, x1, sr, order="numpy"):
    """x0, x1: float32 [P], the whole windows of captured channels 0 and 1.  (one wf_hip_delay as a 0-d record, the float64 values
    behind its float32 fields and the margins of its decisions as a dict; the dict is empty for an invalid record)"""
    x0, x1 = np.ascontiguousarray(x0, np.float32), np.ascontiguousarray(x1, np.float32)
    p = x0.shape[0]
    m, lr = p // 2, p // 4
    out = np.zeros((), DELAY_DTYPE)
    out["window"] = p
    if not (np.all(np.isfinite(x0)) and np.all(np.isfinite(x1)) and np.any(x0 != 0.0) and np.any(x1 != 0.0)):
        return out, {}
    forward = fft_radix2 if order == "radix2" else np.fft.fft
    w = taper(p)
    if order in ("numpy", "radix2"):
        s0, s1 = forward(w * x0.astype(np.float64)), forward(w * x1.astype(np.float64))
    else:
        z = forward(w * x0.astype(np.float64) + 1j * (w * x1.astype(np.float64)))
        zr = np.conj(np.roll(z[::-1], 1))  # conj Z[P - k]
        s0, s1 = 0.5 * (z + zr), -0.5j * (z - zr)
    k = np.arange(1, m)
    x_0, x_1 = s0[1:m], s1[1:m]
    gk = x_0 * np.conj(x_1)
    mag = np.abs(gk)
    g = float(np.max(mag))
    e0, e1 = float(np.sum(np.abs(x_0) ** 2)), float(np.sum(np.abs(x_1) ** 2))
    if not (np.isfinite(g) and g > 0.0):
        return out, {}
    den = np.maximum(mag, BETA * g)
    u, ak = mag / den, gk / den
    full = np.zeros(p, np.complex128)
    if order == "packed":
        hk = gk / g
        full[1:m] = ak + 1j * hk
        full[p - k] = np.conj(ak) + 1j * np.conj(hk)
        y = np.roll(forward(full)[::-1], 1)  # y[(-n) mod P] at index n
        r_all, c_all = y.real / (2.0 * (m - 1)), g * y.imag / (2.0 * np.sqrt(e0 * e1))
        pk, qk = full[1:m], full[p - k]
        ak = 0.5 * (pk + np.conj(qk))
        u = np.abs(ak)
    else:
        full[1:m], full[p - k] = ak, np.conj(ak)
        r_all = _inverse(full, forward).real / (2.0 * (m - 1))
        full[1:m], full[p - k] = gk, np.conj(gk)
        c_all = _inverse(full, forward).real / (2.0 * np.sqrt(e0 * e1))
    lags = np.arange(-lr, lr + 1)
    r = r_all[lags % p]
    i0 = int(np.argmax(np.abs(r)))  # (the first of equal values: the scan runs from -L up)
    n0 = int(lags[i0])
    pol = 1 if r[i0] > 0.0 else -1
    b = pol * ak * np.exp(2j * np.pi * ((k * n0) % p) / p)
    phi = np.arctan2(b.imag, b.real)
    d = float(np.sum(u * k * k))
    f_raw = 0.0 if d == 0.0 else -(p / (2.0 * np.pi)) * float(np.sum(u * k * phi)) / d
    f = min(max(f_raw, -0.5), 0.5)
    far = np.abs(lags - n0) > 2
    top = abs(float(r[i0]))
    vals = {
        "delay_frames": n0 + f,
        "delay_ms": 1000.0 * (n0 + f) / float(sr),
        "peak": float(r[i0]),
        "corr": float(c_all[n0 % p]),
        "corr_zero": float(c_all[0]),
        "ambiguity": float(np.max(np.abs(r[far]))) / top if top > 0.0 else 0.0,
        "curve": r_all[(n0 - CURVE // 2 + np.arange(CURVE)) % p],
    }
    for name, v in vals.items():
        out[name] = v  # (float32 fields: rounded once)
    out["lag"], out["polarity"], out["valid"] = n0, pol, 1
    # the margins of the decisions: how far the runner-up of the argmax lies below the winner, relatively; how close to +-pi the
    # phase of a bin that carries weight comes; the fraction before it is clamped
    others = np.delete(np.abs(r), i0)
    vals["margin_argmax"] = 1.0 - float(np.max(others)) / top if top > 0.0 else 0.0
    heavy = u >= 1e-6
    vals["margin_pi"] = float(np.min(np.pi - np.abs(phi[heavy]))) if heavy.any() else np.pi
    vals["f_raw"] = f_raw
    vals["lag"], vals["polarity"] = n0, pol
    return out, vals


def delay_one(x, w, sr, order="numpy"):
    """x: float32 [2, >= P], the newest frame last.  One wf_hip_delay as a 0-d record"""
    p = window_frames(w)
    x = np.asarray(x, np.float32)
    assert x.shape[0] == 2 and x.shape[1] >= p
    return analyse(x[0, x.shape[1] - p:], x[1, x.shape[1] - p:], sr, order)[0]


def delay(frames, w, sr, order="numpy"):
    """frames: float32 [streams, 2, >= P]: the newest frames of the rings, the newest last"""
    return np.array([delay_one(x, w, sr, order) for x in frames], DELAY_DTYPE)


def zero_record(p, streams):
    s = np.zeros((), DELAY_DTYPE)
    s["window"] = p
    return np.repeat(s, streams)


def worst(got, want):
    """the largest |got - want| of every float field, for printing"""
    res = {"delay_frames": float(np.max(np.abs(got["delay_frames"] - want["delay_frames"]), initial=0.0))}
    for name in FLOAT_FIELDS:
        res[name] = float(np.max(np.abs(got[name].astype(np.float64) - want[name].astype(np.float64)), initial=0.0))
    return res


def mismatches(got, want, float_tol=None, frames_tol=1e-7):
    """(field, index, got, want) of everything in `got` ([streams] of wf_hip_delay) beyond the bound (the module's docstring) of
    `want`.  float_tol: an absolute bound for every float field instead (the comparison of orderings)"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return [("shape", (), (got.shape, got.dtype), (want.shape, want.dtype))]
    bad = []

    def note(name, where, g, f):
        bad.extend((name, tuple(i), g[tuple(i)].item(), f[tuple(i)].item()) for i in np.argwhere(where)[:5])

    for name in INT_FIELDS:
        note(name, got[name] != want[name], got[name], want[name])
    g, f = got["delay_frames"], want["delay_frames"]
    note("delay_frames", ~(np.abs(g - f) <= (frames_tol if float_tol is None else float_tol)), g, f)
    for name in FLOAT_FIELDS:
        g, f = got[name], want[name]
        tol = np.maximum(np.spacing(np.abs(f)).astype(np.float64), 1e-6) if float_tol is None else float_tol
        note(name, ~(np.abs(g.astype(np.float64) - f.astype(np.float64)) <= tol), g, f)
    return bad


# ---- the signals ------------------------------------------------------------------------------------------------------------------

def shifted(x, d):
    """x(t - d) of a real sequence of odd length, circular, for any real d: a phase ramp in the frequency domain, so that a
    fractional delay is exact"""
    n = x.shape[0]
    assert n & 1  # (no Nyquist bin to treat apart)
    spec = np.fft.rfft(x) * np.exp(-2j * np.pi * np.arange(n // 2 + 1) * d / n)
    return np.fft.irfft(spec, n)


# name, the true delay of channel 0 against channel 1 as a function of L (None: there is none), the true polarity
KINDS = (
    ("white +3", lambda lr: 3.0, 1),
    ("white -7.3", lambda lr: -7.3, 1),
    ("inverted L-1", lambda lr: lr - 1.0, -1),
    ("-100 dB +11", lambda lr: 11.0, 1),
    ("tones +2.25", lambda lr: 2.25, 1),
    ("dual mono", lambda lr: 0.0, 1),
    ("independent", None, 0),
    ("silent ch0", None, 0),
    ("one NaN", None, 0),
)
INVALID = ("silent ch0", "one NaN")
CORRELATED = tuple(name for name, d, _ in KINDS if d is not None)


def stream(kind, rng, frames, p):
    """float32 [2, frames] of one kind of stereo audio for a window of p frames: the delayed pairs are cut out of the middle of a
    longer sequence shifted as a whole, so that nothing wraps into the window"""
    pad = p // 4 + 16
    n = frames + 2 * pad
    n += 1 - (n & 1)
    noise = lambda: 0.25 * rng.standard_normal(n)  # noqa: E731
    cut = lambda x: x[pad:pad + frames]  # noqa: E731
    truth = dict((name, d) for name, d, _ in KINDS)[kind]
    d = truth(p // 4) if truth is not None else 0.0
    if kind in ("white +3", "white -7.3", "dual mono"):
        s = noise()
        pair = (shifted(s, d), s)
    elif kind == "inverted L-1":
        s = noise()
        pair = (-shifted(s, d), s)
    elif kind == "-100 dB +11":
        s = noise()
        pair = (shifted(s, d), 1e-5 * s)
    elif kind == "tones +2.25":  # two tones of whole periods in the long sequence, and noise 30 dB under each
        t = np.arange(n, dtype=np.float64)
        c1, c2 = round(0.0613 * n), round(0.1847 * n)
        s = 0.3 * np.sin(2.0 * np.pi * c1 * t / n + 0.4) + 0.3 * np.sin(2.0 * np.pi * c2 * t / n + 1.9)
        s = s + 0.3 * 10.0 ** (-30.0 / 20.0) * np.sqrt(0.5) * rng.standard_normal(n)
        pair = (shifted(s, d), s)
    elif kind == "independent":
        pair = (noise(), noise())
    elif kind == "silent ch0":
        pair = (np.zeros(n), noise())
    elif kind == "one NaN":
        s = noise()
        pair = (shifted(s, 2.0), s.copy())
        pair[1][pad + frames - p // 3] = np.nan  # inside the window
    else:
        raise ValueError(kind)
    return np.stack([cut(pair[0]), cut(pair[1])]).astype(np.float32)


# what tests/test_gpu_delay.py compares against the restatement: (fft_size asked for, sample rate, configuration overrides, the
# W = wf_hip_fft_size() that results); test_delay_cpu.py checks the conditions of the bound on them
GPU_SEED = 20261101
GPU_CASES = [
    (128, 48000, {}, 128),                                       # the smallest; log2 P odd: the single last stage; the curve leaves +-L
    (1024, 44100, {}, 1024),                                     # log2 P even
    (2064, 48000, {}, 2064),                                     # not a power of two: P = 2048 shorter than the FFT
    (4096, 96000, {}, 4096),                                     # the cap: both LDS regions at full size
    (16384, 48000, {}, 16384),                                   # the cap under a split-geometry tick
    (1024, 48000, dict(meter=1, bars=0, meter_ms=46), 2208),     # a meter batch: W = 48000 * 0.046 = 2208, P = 2048
    (512, 48000, dict(stereo=0), 512),                           # a mono mixdown display of two captured channels
]


def case_id(case):
    fft, sr, kw, w = case
    return f"w{w}_sr{sr}" + "".join(f"_{k}{v}" for k, v in kw.items() if k not in ("bars", "meter_ms"))


def case_audio(case):
    """the frames test_gpu_delay.py pushes for a case, float32 [streams, 2, frames]: one ring and P / 2 + 3 frames, so that the
    window wraps the ring and ends at an odd position"""
    fft, sr, kw, w = case
    rng = np.random.default_rng(GPU_SEED + w)
    p = window_frames(w)
    frames = ring_frames(w) + p // 2 + 3
    return np.stack([stream(name, rng, frames, p) for name, _, _ in KINDS])
