"""Float64 restatement of WF_HIP_OUT_TEMPO (include/wf_hip.h, "tempo"): the onset strength of tests/onset_ref.py over up to 2048
columns, its autocorrelation, the salience of every beat period under a log-Gaussian preference around 120 BPM, the best and the
second candidate, and the beat phase on the sample counter.  The columns are onset_ref's arithmetic (numpy's rfft per channel and
column); of how the device sums this knows the stated orders alone.  Also the rule on float32 strengths alone (entries), how far
every decision is from flipping (margins), the comparison (mismatches), and the signals and cases the CPU and the device tests
share."""
import math

import numpy as np

import onset_ref

WINDOW, HOP, COLUMNS, LAGS = 1024, 256, 2048, 576  # WF_HIP_TEMPO_WINDOW, _HOP, _COLUMNS, _LAGS
P, H = WINDOW, HOP
MAX_LAG, MIN_RING, MARGIN = 287, 131072, 2.0  # WF_HIP_TEMPO_MAX_LAG, _MIN_RING, _MARGIN
BPM_FAST, BPM_SLOW, BPM_CENTRE = 240, 40, 120.0
ABS_TOL = onset_ref.ABS_TOL
FLOAT_FIELDS = ("bpm", "period", "confidence", "salience", "bpm2", "salience2", "ambiguity", "strength_max", "strength_mean")
UINT_FIELDS = ("valid", "columns", "newest", "lag_lo", "lag_hi", "lag", "lag2", "beat_age", "period_frames", "last_beat_frame",
               "next_beat_frame", "window", "hop")
DERIVED = ("acf",) + FLOAT_FIELDS + ("valid", "lag", "lag2", "beat_age", "period_frames", "last_beat_frame", "next_beat_frame")
FIELDS = ("strength", "acf") + FLOAT_FIELDS + UINT_FIELDS + ("reserved",)
TEMPO_DTYPE = np.dtype([("strength", np.float32, (COLUMNS,)), ("acf", np.float32, (LAGS,))] + [(n, np.float32) for n in FLOAT_FIELDS]
                       + [(n, np.uint32) for n in UINT_FIELDS] + [("reserved", np.uint32, (2,))])
assert (onset_ref.P, onset_ref.H) == (P, H) and MARGIN == onset_ref.MARGIN


def columns(ring_cap):
    """T: the strength columns of an entry"""
    return min(COLUMNS, (ring_cap - P) // H - 1)


def lag_range(sr, t):
    """(lag_lo, lag_hi) in columns: 240 down to 40 BPM where the columns and the rate allow it"""
    return -((-60 * sr) // (BPM_FAST * H)), min((60 * sr) // (BPM_SLOW * H), t // 4, MAX_LAG)


def served(sr, ring_cap):
    if ring_cap < MIN_RING:
        return False
    lo, hi = lag_range(sr, columns(ring_cap))
    return hi >= lo + 2


def prior(sr):
    """w[L], L = 0 .. MAX_LAG: exp(-0.5 log2(bpm(L) / 120)^2); w[0] = 0"""
    w = np.zeros(MAX_LAG + 1)
    lag = np.arange(1, MAX_LAG + 1, dtype=np.float64)
    w[1:] = np.exp(-0.5 * np.log2(60.0 * sr / (H * lag) / BPM_CENTRE) ** 2)
    return w


def strengths(hist, wpos, sr, ring_cap):
    """hist: float32 [streams, channels, L], the frames of counter positions [wpos - L, wpos), the newest last (what came before
    reads as the zeros of create).  float32 [streams, T], the total strength, age 0 first.  wpos: one counter for the whole
    batch, or [streams] of them"""
    if np.ndim(wpos):
        assert len(wpos) == len(hist)
        return np.concatenate([strengths(hist[s:s + 1], int(w), sr, ring_cap) for s, w in enumerate(wpos)])
    hist = np.asarray(hist, np.float32).astype(np.float64)
    streams, ch, length = hist.shape
    ts = columns(ring_cap) + 1
    span = (ts - 1) * H + P + (int(wpos) % H)
    if length < span:
        hist = np.concatenate([np.zeros((streams, ch, span - length)), hist], axis=2)
        length = span
    end = length - (int(wpos) % H)  # where column `newest` ends
    s = onset_ref.levels_at(hist, [end - a * H for a in range(ts - 1, -1, -1)], sr)
    return onset_ref.flux(s)[:, 0, ::-1]


def _seq(x):
    """the sum of x in ascending index order, one float64 addition at a time (numpy's own sum is pairwise)"""
    return float(np.cumsum(np.asarray(x, np.float64))[-1]) if len(x) else 0.0


def _rint_index(j, period):
    return int(np.rint(j * period))  # (j period is exact in float64: period is a multiple of 1/16; ties to even)


def analyse(o_age, wpos, sr):
    """the rule on one stream's float32 strengths by age.  (entry, vals): a TEMPO_DTYPE scalar, and the float64 values the
    decisions were made on (None when the entry is not valid)"""
    o_age = np.asarray(o_age, np.float32)
    t = len(o_age)
    lo, hi = lag_range(sr, t)
    wpos = int(wpos) % (1 << 32)
    out = np.zeros((), TEMPO_DTYPE)
    out["strength"][:t] = o_age
    out["columns"], out["newest"], out["lag_lo"], out["lag_hi"], out["window"], out["hop"] = t, wpos // H, lo, hi, P, H
    if not np.all(np.isfinite(o_age)):
        return out, None
    o = o_age[::-1].astype(np.float64)  # oldest first
    mean = _seq(o) / t
    e = o - mean
    nl = 2 * hi + 2
    r = np.array([_seq(e[L:] * e[:t - L]) / (t - L) for L in range(nl)])
    largest = float(o_age.max())
    if not (r[0] > 0.0 and largest >= MARGIN):
        return out, None
    acf = r / r[0]
    w = prior(sr)
    c = np.full(hi + 1, -np.inf)
    for L in range(lo, hi + 1):
        c[L] = (acf[L] + 0.5 * acf[2 * L]) * w[L]
    lag = int(np.argmax(c))  # (the lowest lag on ties)
    p, den = 0.0, 0.0
    if lo < lag < hi:
        den = c[lag - 1] - 2.0 * c[lag] + c[lag + 1]
        if den < 0.0:
            p = 0.5 * (c[lag - 1] - c[lag + 1]) / den
    x = lag + p
    period = float(np.rint(x * 16.0)) / 16.0
    lag2, best2 = 0, -np.inf
    for L in range(lo + 1, hi):
        if c[L] > c[L - 1] and c[L] >= c[L + 1] and abs(L - lag) > max(2, lag // 16) and c[L] > best2:
            lag2, best2 = L, c[L]
    k_end = int(math.ceil(period))
    phi = np.zeros(k_end)
    terms = np.zeros(k_end, np.int64)
    for k in range(k_end):
        idx = []
        j = 0
        while t - 1 - k - _rint_index(j, period) >= 0:
            idx.append(t - 1 - k - _rint_index(j, period))
            j += 1
        phi[k], terms[k] = _seq(e[idx]), len(idx)
    beat_age = int(np.argmax(phi))
    out["acf"][:nl] = acf
    out["valid"], out["lag"], out["beat_age"] = 1, lag, beat_age
    out["bpm"], out["period"], out["confidence"], out["salience"] = 60.0 * sr / (H * x), period, acf[lag], c[lag]
    if lag2:
        out["lag2"], out["bpm2"], out["salience2"] = lag2, 60.0 * sr / (H * float(lag2)), c[lag2]
        out["ambiguity"] = c[lag2] / c[lag] if c[lag] > 0.0 else 0.0
    out["strength_max"], out["strength_mean"] = largest, mean
    out["period_frames"] = int(period * H)
    newest_end = wpos - wpos % H
    out["last_beat_frame"] = (newest_end - beat_age * H - 3 * P // 8) % (1 << 32)
    out["next_beat_frame"] = (int(out["last_beat_frame"]) + int(out["period_frames"])) % (1 << 32)
    vals = dict(e=e, r=r, acf=acf, c=c, lag=lag, p=p, den=den, x=x, phi=phi, terms=terms, lo=lo, hi=hi, t=t, largest=largest)
    return out, vals


def entries(o, wpos, sr):
    """[streams] of wf_hip_tempo from the float32 strengths o [streams, T] by age (wpos: a scalar or [streams])"""
    o = np.asarray(o, np.float32)
    wpos = np.broadcast_to(np.asarray(wpos).astype(np.int64), (len(o),))
    return np.array([analyse(o[s], wpos[s], sr)[0] for s in range(len(o))], TEMPO_DTYPE)


def tempo(hist, wpos, sr, ring_cap):
    """[streams] of wf_hip_tempo"""
    return entries(strengths(hist, wpos, sr, ring_cap), wpos, sr)


def margins(o_age, wpos, sr):
    """how far the integer decisions of a valid entry stand from flipping, each as a multiple of what a change of every strength by
    one float32 ulp can move it (to first order, doubled): {"salience", "phase", "half", "valid"}.

    With u the ulp of the largest strength, every e[n] moves by at most 2u (its own change and the mean's), so r[L] by at most
    dr = 4u A T / (T - L) with A the mean of |e|, acf[L] by (dr + |acf[L]| dr) / r[0] <= 2 dr / r[0], and c[L] by
    dc = 1.5 w[L] 2 dr / r[0] <= 3 dr / r[0]; a sum phi[k] of m terms by 2u m.  The parabola's offset p = 0.5 (a - c) / den moves by
    at most (dc + 4 |p| dc) / |den|.  `valid` is how far the largest strength stands from the margin 2.0, in its own ulps."""
    entry, v = analyse(o_age, wpos, sr)
    if v is None:
        return None
    t, lo, hi, lag, c = v["t"], v["lo"], v["hi"], v["lag"], v["c"]
    u = float(np.spacing(np.float32(v["largest"])))
    dr = 4.0 * u * float(np.mean(np.abs(v["e"]))) * t / (t - (2 * hi + 1))
    dc = 3.0 * dr / v["r"][0]
    others = np.delete(c[lo:hi + 1], lag - lo)
    m = {"salience": float(c[lag] - others.max()) / (2.0 * 2.0 * dc)}
    phi = v["phi"]
    if len(phi) > 1:
        k = int(np.argmax(phi))
        runner = float(np.delete(phi, k).max())
        m["phase"] = (float(phi[k]) - runner) / (2.0 * 2.0 * 2.0 * u * float(v["terms"].max()))
    else:
        m["phase"] = np.inf
    dp = (dc + 4.0 * abs(v["p"]) * dc) / abs(v["den"]) if v["den"] < 0.0 else 0.0
    y = v["x"] * 16.0
    half = abs((y - math.floor(y)) - 0.5)
    m["half"] = half / (2.0 * 16.0 * dp) if dp > 0.0 else np.inf
    # (the denominator's sign and the second candidate ride on the same c: they are covered by the comparison against the rule on
    # the device's own strengths, and by `salience` where the second lies next to the first)
    m["valid"] = abs(v["largest"] - MARGIN) / u
    return m


def mismatches(got, hist, wpos, sr, ring_cap, integers=True):
    """(bad, worst): `bad` lists (field, index, got, want) of everything in `got` ([streams] of wf_hip_tempo) outside the contract
    against the restatement of `hist`; `worst` is the largest difference of a strength in float32 ulps of the restatement's.
    Every strength lies within one float32 ulp of the restatement's or within 1e-9, and reads 0 from age T on; every other float32
    field within one float32 rounding (or 1e-9) of the rule on the device's own strengths, every integer equal to it; and with
    `integers` the integer fields also equal the restatement's from its own strengths"""
    want = tempo(hist, wpos, sr, ring_cap)
    if got.shape != want.shape or got.dtype != want.dtype:
        return [("shape", (), (got.shape, got.dtype), (want.shape, want.dtype))], None
    bad = []
    t = int(want["columns"][0])
    g, w = got["strength"].astype(np.float64), want["strength"].astype(np.float64)
    ulp = np.spacing(np.abs(want["strength"])).astype(np.float64)
    err = np.abs(g - w)
    ok = np.where(want["strength"] == 0, (got["strength"] == 0) | (err <= ABS_TOL), (err <= ulp) | (err <= ABS_TOL)) & np.isfinite(g)
    ok &= ~((np.arange(COLUMNS) >= t) & ((got["strength"] != 0) | np.signbit(got["strength"])))
    bad += [("strength", tuple(i), float(got["strength"][tuple(i)]), float(want["strength"][tuple(i)])) for i in np.argwhere(~ok)[:8]]
    live = err > ABS_TOL
    worst = float((err[live] / ulp[live]).max()) if np.any(live) else 0.0
    own = entries(got["strength"][:, :t], wpos, sr) if np.all(got["columns"] == t) else want
    for name in ("acf",) + FLOAT_FIELDS:
        a, b = got[name].astype(np.float64), own[name].astype(np.float64)
        step = np.spacing(np.abs(own[name])).astype(np.float64)
        d = np.abs(a - b)
        fine = ((d <= step) | (d <= ABS_TOL)) & np.isfinite(a)
        bad += [(name + " (rule on its own strengths)", tuple(i), float(got[name][tuple(i)]), float(own[name][tuple(i)]))
                for i in np.argwhere(~fine)[:5]]
    for name in UINT_FIELDS + ("reserved",):
        for other, tag in ((own, " (rule on its own strengths)"),) + (((want, ""),) if integers else ()):
            a, b = got[name], other[name]
            bad += [(name + tag, tuple(i), a[tuple(i)].item(), b[tuple(i)].item()) for i in np.argwhere(a != b)[:5]]
    return bad, worst


# ---- the signals ------------------------------------------------------------------------------------------------------------------

def _noise(rng, db, frames):
    return rng.standard_normal(frames) * 10.0 ** (db / 20.0)


def beats(bpm, frames, sr, first=0.31):
    """the frames at which the events of a pulse train start: the first `first` periods in, none in the last 0.2 s"""
    period = 60.0 * sr / bpm
    k = np.arange(int(frames / period) + 1)
    at = np.rint((first + k) * period).astype(np.int64)
    return at[at < frames - int(0.2 * sr)], period


def kicks(rng, bpm, frames, sr=48000):
    """a 60 Hz kick with a decay of 60 ms on every beat over noise at -40 dBFS.  (float32 [frames], beat frames, period in frames)"""
    x = _noise(rng, -40.0, frames)
    at, period = beats(bpm, frames, sr)
    m = int(0.2 * sr)
    n = np.arange(m)
    for s in at:
        x[s:s + m] += 0.8 * np.sin(2 * np.pi * 60.0 * n / sr) * np.exp(-n / (0.06 * sr))
    return x.astype(np.float32), at, period


def bursts(rng, bpm, frames, sr=48000):
    """noise bursts of 50 ms at -10 dBFS on every beat over noise at -40 dBFS"""
    x = _noise(rng, -40.0, frames)
    at, period = beats(bpm, frames, sr)
    m = int(0.05 * sr)
    for s in at:
        x[s:s + m] += _noise(rng, -10.0, m)
    return x.astype(np.float32), at, period


def noise(rng, db, frames):
    return _noise(rng, db, frames).astype(np.float32)


def steady_sine(frames, sr=48000):
    return (0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(frames) / sr)).astype(np.float32)


def beat_error(frame, at, period):
    """how far `frame` lies from a true beat, modulo the true period, in frames"""
    d = (float(frame) - float(at[0])) % period
    return min(d, period - d)


# what tests/test_gpu_tempo.py compares against the restatement: (fft size asked for, sample rate, captured channels, configuration
# overrides, ring_frames, T, the kinds of its streams); test_tempo_cpu.py checks the margins on them
GPU_SEED = 20261021
GPU_CASES = [
    (1024, 48000, 2, {}, 131072, 507, ("kicks120", "bursts150", "noise")),   # eight chunks, the last of 59 columns
    (4096, 44100, 1, {}, 131072, 507, ("kicks120", "bursts150", "noise")),   # one captured channel
    (2048, 48000, 2, {}, 1 << 18, 1019, ("kicks120", "bursts150")),           # (the canary guards on)
    (1024, 48000, 1, {}, 1 << 20, 2048, ("bursts150",)),                     # T is capped: 32 full chunks
    (1024, 48000, 2, dict(meter=1, bars=0, meter_ms=46), 131072, 507, ("kicks120", "bursts150", "noise")),  # a meter batch
    (1024, 8000, 2, {}, 131072, 507, ("kicks120", "bursts150", "noise")),    # lag_lo = 8, lag_hi = 46
]


def case_id(case):
    fft, sr, ch, kw, ring, t, kinds = case
    return f"ring{ring}_sr{sr}_ch{ch}" + ("_meter" if kw.get("meter") else f"_fft{fft}")


def case_wpos0(case):
    """the write counter of a fresh handle: a spectrum batch starts with fft_size zeros, a meter batch at 0"""
    return 0 if case[3].get("meter") else case[0]


def case_audio(case):
    """the frames test_gpu_tempo.py pushes for a case, float32 [streams, channels, ring + P / 2 + 3]: the span read wraps the ring
    and the counter ends off the hop grid; the second channel is the first at a quarter of its level"""
    fft, sr, ch, kw, ring, t, kinds = case
    frames = ring + P // 2 + 3
    out = []
    for i, kind in enumerate(kinds):
        rng = np.random.default_rng(GPU_SEED + ring + sr + ch + i)
        if kind == "kicks120":
            x = kicks(rng, 120.0, frames, sr)[0]
        elif kind == "bursts150":
            x = bursts(rng, 150.0, frames, sr)[0]
        else:
            x = noise(rng, -20.0, frames)
        out.append(np.stack([x, np.float32(0.25) * x])[:ch])
    return np.stack(out)


packets = onset_ref.packets
