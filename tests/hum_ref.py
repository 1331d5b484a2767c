"""The float64 restatement of WF_HIP_OUT_HUM (include/wf_hip.h, "hum") in numpy: the plan, the spectrum as numpy's FFT of the
Hann-windowed newest N frames, the rule, and the entry; the polyphase form of the same bins that the kernel computes; the test
signals; and the bound of the device comparison (mismatches)."""
import math

import numpy as np

HARMONICS = 8        # WF_HIP_HUM_HARMONICS
MARGIN_DB = 15.0     # WF_HIP_HUM_MARGIN_DB
TOL_HZ = 0.5         # WF_HIP_HUM_TOL_HZ
FLOOR_SPAN = 20      # WF_HIP_HUM_FLOOR_SPAN
FLOOR_GUARD = 3      # WF_HIP_HUM_FLOOR_GUARD
MAX_WINDOW = 32768   # WF_HIP_HUM_MAX_WINDOW
FAMILIES = (50, 60)
TINY = 1e-300        # the least floor and the least power a level is taken of

CHANNEL_FLOATS = ("mains_hz", "hum_db", "total_db", "ratio_db", "odd_db", "even_db", "noise_db")
CHANNEL_UINTS = ("valid", "family", "lines", "mask")
CHANNEL_ARRAYS = ("hz", "level_db", "snr_db")
CHANNEL_FIELDS = CHANNEL_FLOATS + CHANNEL_UINTS + CHANNEL_ARRAYS + ("reserved",)
CHANNEL_DTYPE = np.dtype([(n, np.float32) for n in CHANNEL_FLOATS] + [(n, np.uint32) for n in CHANNEL_UINTS]
                         + [(n, np.float32, (HARMONICS,)) for n in CHANNEL_ARRAYS] + [("reserved", np.uint32)])
FIELDS = ("ch", "window", "decimation", "resolution_hz", "reserved")
HUM_DTYPE = np.dtype([("ch", CHANNEL_DTYPE, (2,)), ("window", np.uint32), ("decimation", np.uint32), ("resolution_hz", np.float32),
                      ("reserved", np.uint32)])


# ---- the plan (wf::host::hum_plan, in the same integer arithmetic) --------------------------------------------------------------

class Plan:
    def __init__(self, sr, ring):
        self.sr, self.ring = sr, ring
        self.D = 1 if sr >= 1280 else 0  # the largest power of two with 1280 D <= sr
        while self.D and 1280 * 2 * self.D <= sr:
            self.D *= 2
        self.N = min(ring, MAX_WINDOW, 1024 * self.D) if self.D else 0
        self.M = self.N // self.D if self.D else 0
        self.hz = sr / self.N if self.N else 0.0
        self.K = -(-484 * self.N // sr) + 22 if self.N else 0
        self.served = self.D >= 2 and self.N > 0 and sr <= 3 * self.N
        # the bins of noise_db: 20 Hz .. 8 * 60.5 Hz
        self.noise_lo = -(-20 * self.N // sr) if self.N else 0
        self.noise_hi = 484 * self.N // sr if self.N else 0

    def search(self, fam, h):
        """lo = max(ceil(h (fam - 0.5) / hz - 0.5), 6), hi = floor(h (fam + 0.5) / hz + 0.5), exactly"""
        lo = -(-(h * (2 * fam - 1) * self.N - self.sr) // (2 * self.sr))
        hi = (h * (2 * fam + 1) * self.N + self.sr) // (2 * self.sr)
        return max(lo, 6), hi


def plan(sr, ring):
    return Plan(sr, ring)


# ---- the spectrum ---------------------------------------------------------------------------------------------------------------

def spectrum(x, pl):
    """H[0 .. K-1] of the newest N frames (float32 taken to float64): numpy's FFT through the periodic Hann window, times 4 / N"""
    n = np.arange(pl.N)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / pl.N)
    return np.fft.fft(x.astype(np.float64) * w)[:pl.K] * (4.0 / pl.N)


def polyphase(x, pl):
    """the same bins as the kernel forms them: D / 2 complex M-point transforms of paired branches, the combination twiddles, and the
    Hann window across frequency"""
    N, D, M, K = pl.N, pl.D, pl.M, pl.K
    x = x.astype(np.float64)
    k = np.arange(-1, K + 1)
    km = k % M
    X = np.zeros(K + 2, np.complex128)
    for r in range(0, D, 2):
        Z = np.fft.fft(x[r::D] + 1j * x[r + 1::D])
        a, b = Z[km], np.conj(Z[(-km) % M])
        A, B = 0.5 * (a + b), -0.5j * (a - b)
        X += np.exp(-2j * np.pi * ((r * k) % N) / N) * A + np.exp(-2j * np.pi * (((r + 1) * k) % N) / N) * B
    return (0.5 * X[1:K + 1] - 0.25 * (X[0:K] + X[2:K + 2])) * (4.0 / N)


# ---- the rule -------------------------------------------------------------------------------------------------------------------

def _db(v):
    return 10.0 * math.log10(max(v, TINY))


def _floor(p, k):
    """the local floor of bin k: the element of rank n / 2 of the sorted powers beside it, over ln 2"""
    v = np.concatenate([p[max(2, k - FLOOR_SPAN):max(2, k - FLOOR_GUARD)], p[k + FLOOR_GUARD + 1:k + FLOOR_SPAN + 1]])
    return max(float(np.sort(v)[len(v) // 2]) / math.log(2.0), TINY)


def candidates(mag, p, pl):
    """every (family index, h, k, f, amp, snr_db) that reaches step 6, in family and harmonic order"""
    out = []
    for fi, fam in enumerate(FAMILIES):
        for h in range(1, HARMONICS + 1):
            lo, hi = pl.search(fam, h)
            if hi < lo:
                continue
            k = lo + int(np.argmax(mag[lo:hi + 1]))  # (the first of equal values: the lowest bin)
            peak = float(mag[k])
            if not (peak > mag[k - 1] and peak >= mag[k + 1]):
                continue
            below, above = float(mag[k - 1]), float(mag[k + 1])
            alpha = max(below, above) / peak
            d = min(max((2.0 * alpha - 1.0) / (alpha + 1.0), 0.0), 0.5)
            sinc = math.sin(math.pi * d) / (math.pi * d) if d > 0.0 else 1.0
            amp = peak * (1.0 - d * d) / sinc
            f = (k - d if below > above else k + d) * pl.hz / h
            if not abs(f - fam) <= TOL_HZ:
                continue
            snr = 10.0 * math.log10(amp * amp / _floor(p, k))
            out.append((fi, h, k, f, amp, snr))
    return out


def clearance(x, sr, ring):
    """how far, in dB, the nearest candidate of a channel's window stands from the margin (inf: there is none)"""
    pl = plan(sr, ring)
    x = np.asarray(x[-pl.N:], np.float32)
    if not np.all(np.isfinite(x)) or not np.any(x):
        return math.inf
    H = spectrum(x, pl)
    p = H.real * H.real + H.imag * H.imag
    return min([abs(c[5] - MARGIN_DB) for c in candidates(np.sqrt(p), p, pl)], default=math.inf)


def channel(x, sr, ring):
    """the entry of one captured channel (a dict of float64 and int values) from its frames, of which the newest N are read"""
    pl = plan(sr, ring)
    assert pl.served and len(x) >= pl.N
    x = np.asarray(x[-pl.N:], np.float32)
    e = {n: 0.0 for n in CHANNEL_FLOATS} | {n: 0 for n in CHANNEL_UINTS} | {n: np.zeros(HARMONICS) for n in CHANNEL_ARRAYS} | {"reserved": 0}
    if not np.all(np.isfinite(x)) or not np.any(x):
        return e
    x64 = x.astype(np.float64)
    total = float(np.sum(x64 * x64)) / pl.N
    H = spectrum(x, pl)
    p = H.real * H.real + H.imag * H.imag
    mag = np.sqrt(p)
    cand = [c for c in candidates(mag, p, pl) if c[5] >= MARGIN_DB]
    best = None
    for fi, fam in enumerate(FAMILIES):
        q = [c for c in cand if c[0] == fi]
        if not q:
            continue
        sw = sf = 0.0
        for _, h, k, f, amp, snr in q:  # ascending h
            w = (h * amp) * (h * amp)
            sw += w
            sf += w * f
        f0 = sf / sw
        kept = [c for c in q if abs(c[3] - f0) * c[1] <= pl.hz]
        hum = odd = even = 0.0
        for _, h, k, f, amp, snr in kept:
            v = amp * amp / 2.0
            hum += v
            if h >= 2 and h % 2 == 0:
                even += v
            elif h >= 3:
                odd += v
        if kept and (best is None or hum > best[1]):  # (50 on a tie)
            best = (fam, hum, odd, even, f0, kept)
    e["valid"] = 1
    e["total_db"] = _db(total)
    excluded = np.zeros(pl.K, bool)
    if best is not None:
        fam, hum, odd, even, f0, kept = best
        e["family"], e["lines"], e["mains_hz"] = fam, len(kept), f0
        e["hum_db"] = _db(hum)
        e["ratio_db"] = e["hum_db"] - e["total_db"]
        e["odd_db"] = _db(odd) if odd > 0.0 else 0.0
        e["even_db"] = _db(even) if even > 0.0 else 0.0
        for _, h, k, f, amp, snr in kept:
            e["mask"] |= 1 << (h - 1)
            e["hz"][h - 1], e["level_db"][h - 1], e["snr_db"][h - 1] = f, _db(amp * amp), snr
            excluded[max(0, k - FLOOR_GUARD):k + FLOOR_GUARD + 1] = True
    bins = np.arange(pl.noise_lo, pl.noise_hi + 1)
    v = p[bins[~excluded[bins]]]
    e["noise_db"] = _db(float(np.sort(v)[len(v) // 2]) / math.log(2.0)) if len(v) else _db(0.0)
    return e


def hum(x, sr, ring):
    """[streams] HUM_DTYPE entries of x [streams, channels, frames] (float32), as float32 of the float64 values"""
    pl = plan(sr, ring)
    out = np.zeros(x.shape[0], HUM_DTYPE)
    out["window"], out["decimation"], out["resolution_hz"] = pl.N, pl.D, pl.hz
    for s in range(x.shape[0]):
        for c in range(x.shape[1]):
            for n, v in channel(x[s, c], sr, ring).items():
                out[s]["ch"][c][n] = v
    return out


def fresh(streams, sr, ring):
    """what a batch reads whose windows are zeros"""
    return hum(np.zeros((streams, 1, plan(sr, ring).N), np.float32), sr, ring)


# ---- the bound of the device comparison -----------------------------------------------------------------------------------------

ABS_TOL = 1e-9


def mismatches(got, x, sr, ring):
    """(field, stream, channel, got, want) wherever the device's entries differ from the restatement of x [streams, channels, frames]:
    every integer equal, every float32 within one float32 rounding of the restatement's float64 value (or ABS_TOL)"""
    bad = []
    pl = plan(sr, ring)
    if got.shape != (x.shape[0],) or got.dtype != HUM_DTYPE:
        return [("shape", 0, 0, got.shape, x.shape[0])]
    for s in range(x.shape[0]):
        g = got[s]
        for name, want in (("window", pl.N), ("decimation", pl.D), ("reserved", 0)):
            if int(g[name]) != want:
                bad.append((name, s, -1, int(g[name]), want))
        if not abs(float(g["resolution_hz"]) - pl.hz) <= float(np.spacing(np.float32(pl.hz))):
            bad.append(("resolution_hz", s, -1, float(g["resolution_hz"]), pl.hz))
        for c in range(2):
            want = channel(x[s, c], sr, ring) if c < x.shape[1] else channel(np.zeros(pl.N, np.float32), sr, ring)
            for name in CHANNEL_UINTS + ("reserved",):
                if int(g["ch"][c][name]) != int(want[name]):
                    bad.append((name, s, c, int(g["ch"][c][name]), int(want[name])))
            for name in CHANNEL_FLOATS + CHANNEL_ARRAYS:
                a = np.atleast_1d(g["ch"][c][name]).astype(np.float64)
                w = np.atleast_1d(np.asarray(want[name], np.float64))
                tol = np.maximum(np.spacing(np.abs(w).astype(np.float32)).astype(np.float64), ABS_TOL)
                if not np.all(np.abs(a - w) <= tol):  # (a NaN fails)
                    bad.append((name, s, c, a.tolist(), w.tolist()))
    return bad


# ---- test signals ---------------------------------------------------------------------------------------------------------------

def noise(rng, db, frames):
    return (rng.standard_normal(frames) * 10.0 ** (db / 20.0)).astype(np.float32)


def pink(rng, db, frames):
    """noise of 1 / f power, of rms `db`"""
    s = np.fft.rfft(rng.standard_normal(frames))
    s[1:] /= np.sqrt(np.arange(1, len(s)))
    s[0] = 0.0
    y = np.fft.irfft(s, frames)
    return (y / np.sqrt(np.mean(y * y)) * 10.0 ** (db / 20.0)).astype(np.float32)


def comb(rng, f0, levels, frames, sr, noise_db=None):
    """sines of the amplitudes levels[h] dBFS at h f0 with random phases, over white noise of rms noise_db (None: none)"""
    n = np.arange(frames, dtype=np.float64)
    y = np.zeros(frames)
    for h, db in levels.items():
        y += 10.0 ** (db / 20.0) * np.sin(2.0 * np.pi * h * f0 * n / sr + rng.uniform(0.0, 2.0 * np.pi))
    if noise_db is not None:
        y += rng.standard_normal(frames) * 10.0 ** (noise_db / 20.0)
    return y.astype(np.float32)


LEVELS = {1: -40.0, 2: -46.0, 3: -43.0, 5: -52.0}          # the issue's hum
NO_FUNDAMENTAL = {2: -42.0, 3: -40.0, 4: -46.0, 6: -44.0}  # a comb without its fundamental

# the plans of the device comparison: (sample rate, ring frames), and what each exercises
GPU_PLANS = ((48000, 16384), (48000, 32768), (96000, 32768), (16000, 8192))
GPU_SEED = 2900
GPU_EXTRA = 777  # frames pushed beyond the window: an odd count, so that the window starts at no aligned place


def case_audio(sr, ring, channels, seed=GPU_SEED, frames=None):
    """[3, channels, N + GPU_EXTRA]: hum at 50.13 Hz, hum at 59.84 Hz without its fundamental, noise alone; with two channels the second
    carries other content: the 60 Hz comb, digital silence, and the 50 Hz hum"""
    pl = plan(sr, ring)
    frames = pl.N + GPU_EXTRA if frames is None else frames
    rng = np.random.default_rng(seed + sr // 1000 + ring // 1024)
    a = comb(rng, 50.13, LEVELS, frames, sr, -40.0)
    b = comb(rng, 59.84, NO_FUNDAMENTAL, frames, sr, -40.0)
    c = noise(rng, -40.0, frames)
    if channels == 1:
        return np.stack([a, b, c])[:, None, :]
    a2 = comb(rng, 59.84, NO_FUNDAMENTAL, frames, sr, -40.0)
    c2 = comb(rng, 50.13, LEVELS, frames, sr, -40.0)
    return np.stack([np.stack([a, a2]), np.stack([b, np.zeros(frames, np.float32)]), np.stack([c, c2])])


# the other audio of the device comparison, all at 48 kHz with a ring of 16384 frames and two captured channels
SR, RING = 48000, 16384
STAGGER_MORE = 5001  # frames that one stream gets on top of the others'
SYNTH_INDEX0 = 1000  # where push_synth's noise starts: the window from index 0 holds a candidate 2.5 dB under the margin
# (frames pushed, read behind it) of tests/hum_wrap_child.py: the approach, two reads before 2^32, the exact hit, the window across it
WRAP_PUSHES = ((RING // 2, False), (RING // 2, False), (RING // 2, False), (RING // 2 - 1024 - 1278, False), (800, True), (441, True), (37, True),
               (800, True), (3011, True), (5021, True), (4009, True), (10991, True), (441, True), (3011, True))


def stagger_audio():
    """(long [3, 2, N + GPU_EXTRA + STAGGER_MORE], refill [1, 2, N + 3]): every stream is pushed long[..., :N + GPU_EXTRA], stream 1 the rest on
    top, and stream 2 is reset and pushed `refill`"""
    n = plan(SR, RING).N
    return (case_audio(SR, RING, 2, GPU_SEED + 1, n + GPU_EXTRA + STAGGER_MORE), case_audio(SR, RING, 2, GPU_SEED + 2, n + 3)[0:1])


def paths_audio():
    """(pcm [3, frames, 2] int16, conv [3, 2, frames] float32): the first case rounded to 16 bits, and as the device widens it"""
    from pcm_convert import captured
    x = case_audio(SR, RING, 2, GPU_SEED + 3)
    pcm = np.round(np.transpose(x, (0, 2, 1)) * 32767.0).astype(np.int16)
    return pcm, np.ascontiguousarray(captured(pcm, True, 0, 2))


def wrap_audio():
    return case_audio(SR, RING, 2, GPU_SEED + 4, sum(p for p, _ in WRAP_PUSHES))


def gpu_windows():
    """(name, sample rate, ring, x [streams, channels, >= N frames]) of every window the device comparison reads: what
    tests/test_hum_cpu.py asserts the clearance of"""
    from tools import synth
    for sr, ring in GPU_PLANS:
        for ch in (1, 2):
            yield f"{sr}/{ring}/{ch}ch", sr, ring, case_audio(sr, ring, ch)
    n = plan(SR, RING).N
    long, refill = stagger_audio()
    yield "stagger", SR, RING, long[:, :, :n + GPU_EXTRA]
    yield "stagger more", SR, RING, long[1:2]
    yield "stagger refill", SR, RING, refill
    yield "s16", SR, RING, paths_audio()[1]
    yield "synth", SR, RING, synth.block(synth.DEFAULT_SEED, 0, 3, 2, SYNTH_INDEX0, n + GPU_EXTRA)
    x, at = wrap_audio(), 0
    for p, read in WRAP_PUSHES:
        at += p
        if read:
            yield f"wrap {at}", SR, RING, np.concatenate([np.zeros((3, 2, n), np.float32), x[:, :, :at]], axis=2)
