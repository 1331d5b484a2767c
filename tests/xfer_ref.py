"""Numpy float64 restatement of WF_HIP_OUT_XFER (include/wf_hip.h, "transfer function"): the gain, phase and coherence per bin of
captured channel 0 (measured) against channel 1 (reference), averaged over the K half-overlapped segments of P frames that the ring
holds, anchored to the sample counter, with the integer delay between the channels found by the floored PHAT of the averaged cross
spectrum and taken out.  Nothing here knows how the device transforms, separates the channels or reduces: every segment of every
channel is transformed on its own by numpy.fft -- so a segment of zeros has the spectrum 0 and two channels of the same bits the same
spectrum, to the bit, which the definition keeps --, and the lag search is an inverse transform of the weighted cross spectrum.  For the
comparison of orderings (tests/test_xfer_cpu.py) three more orders of the same sums -- "descending", "pairwise", "longdouble" -- in
which the correlations r[n] are also summed bin by bin instead of transformed.  Also the signal kinds the tests push and the cases
the CPU and the device tests share.

Bound of `mismatches`: valid, window, hop, segments, lag, newest and the reserved words equal; every float32 field and curve entry
within max(1 float32 ulp of the wanted value, 1e-6), the phase on the circle (+pi and -pi are one angle: an inverted channel reads
either), -INFINITY equal to itself.  It is derived, not measured: both sides work in float64 from the same float32 samples and differ
only in the order of operations; the four orders here agree to 1e-9 in every field on the committed cases (test_xfer_cpu.py asserts
it and prints the figure), and the one decision, the argmax of |r[n]|, is not near a tie there -- the winning |r| exceeds every other
lag's by at least 1e-3 on every stream whose lag is asserted; independent noise is exempt, its lag is noise, and the comparison
takes the device's lag for it -- so one float32 rounding is all that can separate the device from the restatement."""
import numpy as np

from delay_ref import BETA, taper

MAX_WINDOW = 2048   # WF_HIP_XFER_MAX_WINDOW
MAX_SEGMENTS = 32   # WF_HIP_XFER_MAX_SEGMENTS
BINS = 1024         # WF_HIP_XFER_BINS
DEAD_RATIO = 2.0 ** -80  # WF_HIP_STEREO_DEAD_RATIO
XFER_DTYPE = np.dtype([("valid", np.uint32), ("window", np.uint32), ("hop", np.uint32), ("segments", np.uint32), ("lag", np.int32),
                       ("newest", np.uint32), ("lag_peak", np.float32), ("mean_coherence", np.float32), ("reserved", np.uint32, (4,)),
                       ("gain_db", np.float32, (BINS,)), ("phase", np.float32, (BINS,)), ("coherence", np.float32, (BINS,))])
FIELDS = XFER_DTYPE.names
FLOAT_FIELDS = ("lag_peak", "mean_coherence", "gain_db", "phase", "coherence")
INT_FIELDS = ("valid", "window", "hop", "segments", "lag", "newest", "reserved")
ORDERS = ("ascending", "descending", "pairwise", "longdouble")


def ring_frames(w, ring=None):
    """the ring capacity wf_hip_create gives a handle of window w: the next power of two of max(ring, w), or of max(2 w, 4096) by
    default"""
    return 1 << ((max(ring, w) if ring else max(2 * w, 4096)) - 1).bit_length()


def geometry(w, ring):
    """(P, K) of a handle whose wf_hip_fft_size() is w and whose ring holds `ring` frames"""
    p = 1
    while 2 * p <= min(int(w), MAX_WINDOW, int(ring) // 8):
        p *= 2
    return p, min(MAX_SEGMENTS, 2 * int(ring) // p - 3)


def span_frames(p, k):
    """the frames of either channel that a read may touch, without the up to H - 1 frames behind the anchor"""
    return (k - 1) * (p // 2) + p + 2 * (p // 4)


def _sum(a, order):
    """the sum over axis 0 in one of ORDERS"""
    if order == "ascending":
        s = np.zeros(a.shape[1:], a.dtype)
        for row in a:
            s = s + row
        return s
    if order == "descending":
        return _sum(a[::-1], "ascending")
    if order == "pairwise":
        while a.shape[0] > 1:
            if a.shape[0] & 1:
                a = np.concatenate([a, np.zeros_like(a[:1])])
            a = a[0::2] + a[1::2]
        return a[0]
    wide = np.clongdouble if np.iscomplexobj(a) else np.longdouble
    return np.sum(a.astype(wide), axis=0).astype(a.dtype)


def _sums(sp, p, k, n, order):
    """Sxx, Syy, Sxy [M - 1] of the bins 1 .. M - 1 with channel 1 read n frames earlier; sp: float64 [2, span]"""
    h, l, m = p // 2, p // 4, p // 2
    w = taper(p)
    e = sp.shape[1] - l  # the index of counter frame E
    x0 = np.stack([np.fft.fft(w * sp[0, e - a * h - p:e - a * h])[1:m] for a in range(k - 1, -1, -1)])  # oldest first
    x1 = np.stack([np.fft.fft(w * sp[1, e - a * h - p - n:e - a * h - n])[1:m] for a in range(k - 1, -1, -1)])
    # (written out in real arithmetic, so that two channels of the same bits give Sxx = Syy = Re Sxy and Im Sxy = 0 exactly)
    a, b, c, d = x1.real, x1.imag, x0.real, x0.imag
    return _sum(a * a + b * b, order), _sum(c * c + d * d, order), _sum((a * c + b * d) + 1j * (a * d - b * c), order)


def correlations(g, p, order="ascending"):
    """r[n], -L <= n <= L, of the cross spectrum G [M - 1] (bins 1 .. M - 1), and max |G|"""
    m, l = p // 2, p // 4
    mag = np.abs(g)
    top = float(np.max(mag))
    lags = np.arange(-l, l + 1)
    if not top > 0.0:
        return np.zeros(lags.size), top
    a = g / np.maximum(mag, BETA * top)
    if order == "ascending":
        full = np.zeros(p, np.complex128)
        full[1:m] = a
        full[p - np.arange(1, m)] = np.conj(a)
        r_all = (np.fft.ifft(full) * p).real / (2.0 * (m - 1))
        return r_all[lags % p], top
    kk = np.arange(1, m)
    terms = (a[:, None] * np.exp(2j * np.pi * ((kk[:, None] * lags[None, :]) % p) / p)).real  # [bins, lags]
    return _sum(terms, order) / (m - 1), top


def analyse(x, w, ring, sr, lag=None, wpos=None, order="ascending"):
    """x: float32 [2, n], every frame pushed so far (or the newest of them: what is missing in front counts as the zeros of create),
    the newest last; wpos: the stream's write counter (n if None).  lag: None searches, an integer is taken as given.  (one wf_hip_xfer
    as a 0-d record, the float64 values behind its fields as a dict -- empty for an invalid record)"""
    x = np.asarray(x, np.float32)
    assert x.ndim == 2 and x.shape[0] == 2
    p, k = geometry(w, ring)
    h, l, m = p // 2, p // 4, p // 2
    wpos = x.shape[1] if wpos is None else int(wpos)
    span = span_frames(p, k)
    assert span + h - 1 < ring
    end = x.shape[1] - (wpos % h)  # just behind counter frame E + L - 1
    sp = x[:, max(end - span, 0):end]
    if sp.shape[1] < span:
        sp = np.concatenate([np.zeros((2, span - sp.shape[1]), np.float32), sp], axis=1)
    out = np.zeros((), XFER_DTYPE)
    out["window"], out["hop"], out["segments"] = p, h, k
    if not (np.all(np.isfinite(sp)) and np.any(sp[0] != 0.0) and np.any(sp[1] != 0.0)):
        return out, {}
    sp = sp.astype(np.float64)
    sxx, syy, sxy = _sums(sp, p, k, 0, order)
    r, top = correlations(sxy, p, order)
    lags = np.arange(-l, l + 1)
    if lag is not None:
        i0 = int(lag) + l
    elif top > 0.0:
        i0 = int(np.argmax(np.abs(r)))  # (the first of equal values: the scan runs from -L up)
    else:
        i0 = l
    n0 = int(lags[i0])
    if n0 != 0:
        sxx, syy, sxy = _sums(sp, p, k, n0, order)
    live = sxx > DEAD_RATIO * float(np.max(sxx))
    full = live & (syy != 0.0)
    gain, phase, coh = np.zeros(m - 1), np.zeros(m - 1), np.zeros(m - 1)
    m2 = np.abs(sxy) ** 2
    hk = np.zeros(m - 1, np.complex128)
    hk[full] = sxy[full] / sxx[full]
    with np.errstate(divide="ignore"):
        gain[full] = 10.0 * np.log10(m2[full] / sxx[full] ** 2)
    gain[live & ~full] = -np.inf
    phase[full] = np.arctan2(hk[full].imag, hk[full].real)
    coh[full] = np.minimum(m2[full] / (sxx[full] * syy[full]), 1.0)
    den = float(_sum(sxx[live], order)) if live.any() else 0.0
    vals = {
        "lag": n0, "lag_peak": float(r[i0]), "gain_db": gain, "phase": phase, "coherence": coh, "h": hk, "live": live,
        "mean_coherence": float(_sum((sxx * coh)[live], order)) / den if den > 0.0 else 0.0,
        "sxx": sxx, "syy": syy, "sxy": sxy, "r": r,
    }
    others = np.delete(np.abs(r), i0)
    vals["margin"] = abs(float(r[i0])) - float(np.max(others))  # the argmax margin: |r[n0]| - max_{n != n0} |r[n]|
    out["valid"], out["lag"], out["newest"] = 1, n0, (wpos // h) & 0xFFFFFFFF
    out["lag_peak"], out["mean_coherence"] = vals["lag_peak"], vals["mean_coherence"]  # (float32 fields: rounded once)
    for name in ("gain_db", "phase", "coherence"):
        out[name][1:m] = vals[name]
    return out, vals


def xfer(frames, w, ring, sr, lag=None, wpos=None, order="ascending"):
    """frames: float32 [streams, 2, n], the frames pushed, the newest last.  lag: None searches; an integer, or one per stream with
    None where to search, is taken as given.  wpos: the write counter of every stream, or one per stream (n if None)"""
    n = len(frames)
    lags = list(lag) if isinstance(lag, (list, tuple, np.ndarray)) else [lag] * n
    pos = list(wpos) if isinstance(wpos, (list, tuple, np.ndarray)) else [wpos] * n
    return np.array([analyse(x, w, ring, sr, lg, wp, order)[0] for x, lg, wp in zip(frames, lags, pos)], XFER_DTYPE)


def margins(frames, w, ring, sr, wpos=None):
    """the argmax margin |r[n0]| - max_{n != n0} |r[n]| of every stream (nan for an invalid one)"""
    return np.array([analyse(x, w, ring, sr, None, wpos)[1].get("margin", np.nan) for x in frames])


def zero_record(w, ring, streams):
    p, k = geometry(w, ring)
    s = np.zeros((), XFER_DTYPE)
    s["window"], s["hop"], s["segments"] = p, p // 2, k
    return np.repeat(s, streams)


def _circle(d):
    return np.abs((d + np.pi) % (2.0 * np.pi) - np.pi)


def _diff(name, g, f):
    g, f = np.asarray(g, np.float64), np.asarray(f, np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(g - f)
    d = np.where(np.isinf(f) & (g == f), 0.0, d)
    return _circle(d) if name == "phase" else d


def worst(got, want):
    """the largest |got - want| of every float field, for printing"""
    return {name: float(np.max(_diff(name, got[name], want[name]), initial=0.0)) for name in FLOAT_FIELDS}


def mismatches(got, want, float_tol=None):
    """(field, index, got, want) of everything in `got` ([streams] of wf_hip_xfer) beyond the bound (the module's docstring) of
    `want`.  float_tol: an absolute bound for every float field instead (the comparison of orderings)"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return [("shape", (), (got.shape, got.dtype), (want.shape, want.dtype))]
    bad = []

    def note(name, where, g, f):
        bad.extend((name, tuple(i), g[tuple(i)].item(), f[tuple(i)].item()) for i in np.argwhere(where)[:5])

    for name in INT_FIELDS:
        note(name, got[name] != want[name], got[name], want[name])
    for name in FLOAT_FIELDS:
        g, f = got[name], want[name]
        with np.errstate(invalid="ignore"):
            tol = np.maximum(np.spacing(np.abs(f)).astype(np.float64), 1e-6) if float_tol is None else float_tol
            tol = np.where(np.isfinite(tol), tol, 0.0)
        note(name, ~(_diff(name, g, f) <= tol), g, f)
    return bad


# ---- the signals ------------------------------------------------------------------------------------------------------------------

# nine taps, the first the largest (the PHAT peak lies on it), and no notch: |H| stays within -3.7 .. +2.6 dB, so that the worst
# error over the bins is not the luck of the few bins where a notch leaves the measured channel little to correlate with
FIR = np.array([1.0, 0.25, 0.15, -0.1, 0.08, -0.06, 0.04, -0.03, 0.02])
FIR_DELAY = 37


def fir_response(p):
    """the true response of FIR at the bins 1 .. M - 1 of a window of p frames, the delay left out"""
    kk = np.arange(1, p // 2)
    return np.exp(-2j * np.pi * kk[:, None] * np.arange(FIR.size)[None, :] / p) @ FIR


KINDS = ("fir +37", "delay -(L-1)", "inverted -6 dB", "added noise", "independent", "dual mono", "tone, measured zero", "silent reference",
         "one NaN")
INVALID = ("silent reference", "one NaN")
NO_LAG = ("independent",)  # the lag of unrelated channels is noise: exempt from the margin, compared at the device's lag


def true_lag(kind, p):
    return {"fir +37": FIR_DELAY, "delay -(L-1)": -(p // 4 - 1), "inverted -6 dB": 0, "added noise": 0, "dual mono": 0,
            "tone, measured zero": 0}.get(kind)


def stream(kind, rng, frames, p, tail=3):
    """float32 [2, frames] of one kind of stereo audio for segments of p frames: row 0 the measured channel, row 1 the reference.
    tail: the frames behind the anchor at the read (the counter mod H), for the one kind that places a sample by it"""
    pad = p // 4 + FIR_DELAY + FIR.size + 16
    n = frames + 2 * pad
    noise = lambda: 0.25 * rng.standard_normal(n)  # noqa: E731
    cut = lambda v: np.asarray(v[pad:pad + frames], np.float64).astype(np.float32)  # noqa: E731
    s = noise()
    if kind == "fir +37":
        y = np.convolve(s, FIR)[:n]
        return np.stack([cut(np.concatenate([np.zeros(FIR_DELAY), y[:n - FIR_DELAY]])), cut(s)])
    if kind == "delay -(L-1)":  # channel 0 is the earlier one
        d = p // 4 - 1
        return np.stack([cut(np.concatenate([s[d:], np.zeros(d)])), cut(s)])
    if kind == "inverted -6 dB":
        ref = cut(s)
        return np.stack([np.float32(-0.5) * ref, ref])  # (exact in float32)
    if kind == "added noise":  # noise of the reference's own power on top: coherence 1 / 2
        return np.stack([cut(s + noise()), cut(s)])
    if kind == "independent":
        return np.stack([cut(noise()), cut(s)])
    if kind == "dual mono":
        return np.stack([cut(s), cut(s)])
    if kind == "tone, measured zero":
        # the reference a tone in noise 120 dB under it; the measured channel +0.0 in every frame its segments read -- Syy is 0 in
        # live bins -- with one sample in the slack behind them, which no segment reads at lag 0 but which is part of the span:
        # neither channel is silent
        t = np.arange(frames, dtype=np.float64)
        ref = (0.5 * np.sin(2.0 * np.pi * 0.0613 * t + 0.4) + 0.5e-6 * s[pad:pad + frames]).astype(np.float32)
        meas = np.zeros(frames, np.float32)
        meas[frames - tail - 2] = 0.25
        return np.stack([meas, ref])
    if kind == "silent reference":
        return np.stack([cut(s), np.zeros(frames, np.float32)])
    if kind == "one NaN":
        out = np.stack([cut(np.concatenate([np.zeros(2), s[:n - 2]])), cut(s)])
        out[1, frames - p - p // 3] = np.nan  # inside the span
        return out
    raise ValueError(kind)


# what tests/test_gpu_xfer.py compares against the restatement: (fft_size asked for, sample rate, configuration overrides, the
# W = wf_hip_fft_size() that results, ring_frames asked for or None); test_xfer_cpu.py checks the conditions of the bound on them
GPU_SEED = 20261201
GPU_CASES = [
    (256, 48000, {}, 256, 2048),                                    # P = 256, K = 13: the fewest bins per thread, L = 64
    (800, 44100, {}, 800, None),                                    # not a power of two: P = 512 under the FFT; log2 P odd
    (4096, 48000, {}, 4096, None),                                  # the default ring of the headline shape: P = 1024
    (4096, 96000, {}, 4096, 16384),                                 # P = 2048, the cap
    (4096, 48000, {}, 4096, 65536),                                 # K = 32, the segment cap
    (1024, 48000, dict(meter=1, bars=0, meter_ms=46), 2208, None),  # a meter batch: W = 48000 * 0.046 = 2208, P = 1024
    (512, 48000, dict(stereo=0), 512, None),                        # a mono mixdown display of two captured channels
]
GEOMETRIES = [(256, 13), (512, 13), (1024, 13), (2048, 13), (2048, 32), (1024, 13), (512, 13)]  # (P, K) of the cases above


def case_id(case):
    fft, sr, kw, w, ring = case
    return f"w{w}_sr{sr}" + (f"_ring{ring}" if ring else "") + "".join(f"_{k}{v}" for k, v in kw.items() if k not in ("bars", "meter_ms"))


def case_wpos0(case):
    """the counter of a fresh stream: a spectrum batch holds W zeros, a meter batch nothing"""
    return 0 if case[2].get("meter") else case[3]


def case_audio(case):
    """the frames test_gpu_xfer.py pushes for a case, float32 [streams, 2, frames]: one ring and H + 3 frames, so that the span wraps
    the ring and the counter, wpos0 + frames, ends off the anchor"""
    fft, sr, kw, w, ring = case
    cap = ring_frames(w, ring)
    p, k = geometry(w, cap)
    rng = np.random.default_rng(GPU_SEED + w + cap)
    frames = cap + p // 2 + 3
    return np.stack([stream(name, rng, frames, p, (case_wpos0(case) + frames) % (p // 2)) for name in KINDS])


# ---- the staggered batch ------------------------------------------------------------------------------------------------------------

STAGGER_KINDS = ("fir +37", "delay -(L-1)", "inverted -6 dB", "added noise", "fir +37", "dual mono", "added noise")


def stagger_script(case):
    """tests/measure_stagger.py's plan of `case` (one of its two-channel cases) with this output's kinds in it, in the form its
    replay() takes: seven streams whose counters all differ, a packet longer than the ring, a reset, three push paths"""
    import measure_stagger as ms
    steps = ms.plan(case)
    frames = ms.totals(steps)
    p, k = geometry(case.W, case.ring_cap)
    rng = np.random.default_rng(ms.SEED + case.W)
    src = [stream(STAGGER_KINDS[s], rng, int(frames[s]), p) for s in range(ms.STREAMS)]
    at = [0] * ms.STREAMS

    def take(s, n):
        at[s] += n
        return src[s][:, at[s] - n:at[s]]

    script = []
    for st in steps:
        if st[0] == "push":
            script.append(("push", st[1], np.stack([take(s, st[3]) for s in range(st[1], st[1] + st[2])])))
        elif st[0] == "ragged":
            counts = np.asarray(st[1], np.uint32)
            x = np.zeros((ms.STREAMS, 2, int(counts.max())), np.float32)
            for s in range(ms.STREAMS):
                x[s, :, :int(counts[s])] = take(s, int(counts[s]))
            script.append(("ragged", x, counts))
        else:
            script.append(st)
    assert at == [a.shape[1] for a in src]
    return script
