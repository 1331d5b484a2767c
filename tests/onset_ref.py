"""Float64 restatement of WF_HIP_OUT_ONSET (include/wf_hip.h, "onsets"): the positive change of a compressed band level between
neighbouring sonogram columns, in total and in three groups, and the onsets picked from the four float32 curves.  The columns, the
window and the filterbank are tests/sono_ref.py's arithmetic (numpy's rfft per channel and column); nothing here knows how the device
transforms or sums.  Also the picking rule on float32 values alone (pick), how far every decision is from flipping (margins), the
comparison (mismatches), and the signals and cases the CPU and the device tests share."""
import numpy as np

import sono_ref

WINDOW, HOP, COLUMNS, BANDS = 1024, 256, 128, 64  # WF_HIP_ONSET_WINDOW, _HOP, _COLUMNS, _BANDS
P, H = WINDOW, HOP
GROUPS = ((0, 16), (16, 40), (40, 64))  # low, mid, high
KNEE, MARGIN, BEFORE, AFTER, MEAN = 100.0, 2.0, 6, 3, 16
F_TOTAL, F_LOW, F_MID, F_HIGH, F_DECIDED = 1, 2, 4, 8, 0x80
NONE = 0xFFFFFFFF
MIN_RING = 8192
FIELDS = ("strength", "group", "flags", "columns", "newest", "decided_first", "decided_end", "window", "hop", "onsets", "last_age",
          "last_frame", "last_strength", "reserved")
ONSET_DTYPE = np.dtype([("strength", np.float32, (COLUMNS,)), ("group", np.float32, (3, COLUMNS)), ("flags", np.uint8, (COLUMNS,)),
                        ("columns", np.uint32), ("newest", np.uint32), ("decided_first", np.uint32), ("decided_end", np.uint32),
                        ("window", np.uint32), ("hop", np.uint32), ("onsets", np.uint32), ("last_age", np.uint32),
                        ("last_frame", np.uint32), ("last_strength", np.float32), ("reserved", np.uint32, (6,))])
ABS_TOL = 1e-9  # a strength may differ by one float32 ulp or by this much
assert (sono_ref.P, sono_ref.H, sono_ref.BANDS) == (P, H, BANDS)


def spectral(ring_cap):
    """Ts: how many spectral columns a ring of ring_cap frames always holds"""
    return min(COLUMNS + 1, (ring_cap - P) // H)


def columns(ring_cap):
    """T: the strength columns of an entry"""
    return spectral(ring_cap) - 1


def decided(t):
    """(first, end): the ages [first, end) are decided"""
    return AFTER, (t - MEAN if t > MEAN + AFTER else 0)


def levels_at(x, ends, sr):
    """x: float64 [streams, channels, L]; ends: where each column ends in x (a column is x[..., end - P:end]).
    S: float64 [streams, len(ends), 64]"""
    streams, ch, _ = x.shape
    wt = sono_ref.band_weights(sr)
    w = sono_ref.hann()
    out = np.zeros((streams, len(ends), BANDS))
    for i, end in enumerate(ends):
        spec = np.fft.rfft(w * x[:, :, end - P:end], axis=-1)[..., :P // 2]
        b = ((np.abs(spec) ** 2) @ wt.T).sum(axis=1)  # over the captured channels: no dead-channel rule
        out[:, i] = np.log1p(KNEE * np.sqrt(b * 32.0 / (3.0 * P * P * ch))) / np.log(10.0)
    return out


def flux(s):
    """s: [streams, columns oldest first, 64].  float32 [streams, 4, columns - 1]: total, low, mid, high, oldest first"""
    d = np.maximum(s[:, 1:] - s[:, :-1], 0.0)
    g = [d[:, :, lo:hi].sum(axis=-1) for lo, hi in GROUPS]
    return np.stack([(g[0] + g[1]) + g[2], g[0], g[1], g[2]], axis=1).astype(np.float32)


def strengths(hist, wpos, sr, ring_cap):
    """hist: float32 [streams, channels, L], the frames of counter positions [wpos - L, wpos), the newest last (what came before
    reads as the zeros of create).  float32 [streams, 4, T], age 0 first.  wpos: one counter for the whole batch, or [streams] of
    them, each stream's history ending at its own"""
    if np.ndim(wpos):
        assert len(wpos) == len(hist)
        return np.concatenate([strengths(hist[s:s + 1], int(w), sr, ring_cap) for s, w in enumerate(wpos)])
    hist = np.asarray(hist, np.float32).astype(np.float64)
    streams, ch, length = hist.shape
    ts = spectral(ring_cap)
    span = (ts - 1) * H + P + (int(wpos) % H)
    if length < span:
        hist = np.concatenate([np.zeros((streams, ch, span - length)), hist], axis=2)
        length = span
    end = length - (int(wpos) % H)  # where column `newest` ends
    s = levels_at(hist, [end - a * H for a in range(ts - 1, -1, -1)], sr)
    return flux(s)[:, :, ::-1]


def _conditions(o):
    """o: float32 [..., T] by age.  For the ages a = AFTER .. T - MEAN - 1: (lhs, rhs, truth, scale) of the ten comparisons that
    decide age a, each [10, ..., n]: v > the six before, v >= the three after, v >= mean + MARGIN.  `scale` is what one float32 ulp
    of the values that enter the comparison is worth (for the mean: of the largest of its twenty)"""
    o = np.asarray(o, np.float32)
    t = o.shape[-1]
    ages = np.arange(AFTER, t - MEAN)
    v = o[..., ages]
    lhs, rhs, truth = [], [], []
    for m in range(1, BEFORE + 1):  # the column m hops older has the age a + m
        lhs.append(v), rhs.append(o[..., ages + m]), truth.append(v > o[..., ages + m])
    for m in range(1, AFTER + 1):
        lhs.append(v), rhs.append(o[..., ages - m]), truth.append(v >= o[..., ages - m])
    total = o[..., ages + MEAN].astype(np.float64)
    largest = o[..., ages + MEAN]
    for i in range(1, MEAN + AFTER + 1):  # oldest first, one float64 addition at a time (numpy's own sum is pairwise)
        total = total + o[..., ages + MEAN - i].astype(np.float64)
        largest = np.maximum(largest, o[..., ages + MEAN - i])
    thr = total / float(MEAN + AFTER + 1) + MARGIN
    lhs.append(v), rhs.append(thr), truth.append(v.astype(np.float64) >= thr)
    lhs = np.stack([np.asarray(x, np.float64) for x in lhs])
    rhs = np.stack([np.asarray(x, np.float64) for x in rhs])
    scale = np.spacing(np.maximum(np.abs(lhs), np.abs(rhs)).astype(np.float32)).astype(np.float64)
    scale[-1] = np.spacing(np.maximum(largest, thr.astype(np.float32))).astype(np.float64)
    return ages, lhs, rhs, np.stack(truth), np.maximum(scale, ABS_TOL)


def pick(o):
    """the rule, on float32 values alone.  o: float32 [streams, 4, T] by age; uint8 [streams, T]: bit g = curve g has an onset at
    that age, bit 7 = decided"""
    o = np.asarray(o, np.float32)
    flags = np.zeros(o.shape[:1] + o.shape[2:], np.uint8)
    if o.shape[-1] <= MEAN + AFTER:
        return flags
    ages, _, _, truth, _ = _conditions(o)
    on = truth.all(axis=0)  # [streams, 4, n]
    flags[:, ages] = F_DECIDED
    for g in range(4):
        flags[:, ages] |= (on[:, g].astype(np.uint8) << g).astype(np.uint8)
    return flags


def margins(o):
    """the smallest distance, in float32 ulps of the strengths (1e-9 at least: what a strength may differ by), of any decision
    from flipping.  An onset stands while each of its ten comparisons does: its margin is the smallest gap among them.  A column
    that is no onset stays none while one failed comparison stays failed: its margin is the largest gap among the failed ones"""
    if np.shape(o)[-1] <= MEAN + AFTER:
        return np.inf
    _, lhs, rhs, truth, scale = _conditions(o)
    gap = np.abs(lhs - rhs) / scale
    on = truth.all(axis=0)
    m = np.where(on, gap.min(axis=0), np.where(truth, -np.inf, gap).max(axis=0))
    return float(m.min())


def entries(o, wpos):
    """[streams] of wf_hip_onset from the float32 strengths o [streams, 4, T] by age (wpos: a scalar or [streams])"""
    o = np.asarray(o, np.float32)
    streams, _, t = o.shape
    out = np.zeros(streams, ONSET_DTYPE)
    out["strength"][:, :t] = o[:, 0]
    out["group"][:, :, :t] = o[:, 1:]
    out["flags"][:, :t] = pick(o)
    newest = np.broadcast_to((np.asarray(wpos).astype(np.int64) % (1 << 32)) // H, (streams,))
    out["columns"], out["newest"], out["window"], out["hop"] = t, newest, P, H
    out["decided_first"], out["decided_end"] = decided(t)
    out["last_age"] = NONE
    for s in range(streams):
        hit = np.flatnonzero(out["flags"][s] & F_TOTAL)
        out["onsets"][s] = len(hit)
        if len(hit):
            out["last_age"][s] = hit[0]
            out["last_frame"][s] = ((int(newest[s]) - int(hit[0])) * H - 3 * P // 8) % (1 << 32)
            out["last_strength"][s] = o[s, 0, hit[0]]
    return out


def onset(hist, wpos, sr, ring_cap):
    """[streams] of wf_hip_onset"""
    return entries(strengths(hist, wpos, sr, ring_cap), wpos)


def device_strengths(got):
    t = int(got["columns"][0])
    return np.concatenate([got["strength"][:, None, :t], got["group"][:, :, :t]], axis=1)


def mismatches(got, hist, wpos, sr, ring_cap):
    """(bad, worst): `bad` lists (field, index, got, want) of everything in `got` ([streams] of wf_hip_onset) outside the contract
    against the restatement of `hist`; `worst` is the largest difference of a strength in float32 ulps of the restatement's.
    The header words, the zeros and the ages >= T are equal; every strength lies within one float32 ulp of the restatement's or
    within 1e-9; flags, onsets and last_* are bit for bit pick() of the device's own strengths, and equal to the restatement's."""
    want = onset(hist, wpos, sr, ring_cap)
    if got.shape != want.shape or got.dtype != want.dtype:
        return [("shape", (), (got.shape, got.dtype), (want.shape, want.dtype))], None
    bad = []
    t = int(want["columns"][0])
    own = entries(device_strengths(got), wpos) if np.all(got["columns"] == t) else want
    for name in FIELDS[2:]:
        for other, tag in ((own, " (pick of its own strengths)"), (want, "")):
            a, b = got[name], other[name]
            if name == "last_strength" and other is want:
                continue  # (a strength: held below)
            bad += [(name + tag, tuple(i), a[tuple(i)].item(), b[tuple(i)].item()) for i in np.argwhere(a != b)[:5]]
    worst = 0.0
    for name in ("strength", "group", "last_strength"):
        g, w = got[name].astype(np.float64), want[name].astype(np.float64)
        ulp = np.spacing(np.abs(want[name])).astype(np.float64)
        err = np.abs(g - w)
        ok = np.where(want[name] == 0, (got[name] == 0) | (err <= ABS_TOL), (err <= ulp) | (err <= ABS_TOL))
        ok &= np.isfinite(g)
        beyond = np.arange(g.shape[-1]) >= t if name != "last_strength" else False
        ok &= ~(beyond & ((got[name] != 0) | np.signbit(got[name])))
        bad += [(name, tuple(i), float(got[name][tuple(i)]), float(want[name][tuple(i)])) for i in np.argwhere(~ok)[:8]]
        live = err > ABS_TOL
        if np.any(live):
            worst = max(worst, float((err[live] / ulp[live]).max()))
    return bad, worst


# ---- the signals ------------------------------------------------------------------------------------------------------------------

KINDS = ("noise", "burst", "chirp")
CHIRP_FRAMES = 1531  # one sweep of the chirp: no multiple of the hop, so that no two columns hold the same stretch of it


def signal(kind, rng, frames, channels=2, span=None):
    """float32 [channels, frames] of one kind of audio; the burst's events lie in the newest `span` frames (None: all of them)"""
    n = np.arange(frames, dtype=np.float64)
    if kind == "noise":      # independent noise
        x = rng.standard_normal((2, frames)) * 0.2
    elif kind == "burst":    # silence, then a noise burst, silence, then two tones that step to two others; the right channel lower
        l = np.zeros(frames)
        span = frames if span is None else min(span, frames)
        q, at = span // 4, frames - span
        m = min(700, span // 5)
        l[at + q:at + q + m] = rng.standard_normal(m) * 0.3
        a, b = slice(at + 2 * q, at + 3 * q), slice(at + 3 * q, frames)
        l[a] = 0.4 * np.sin(2 * np.pi * 0.021 * n[a]) + 0.1 * np.sin(2 * np.pi * 0.13 * n[a])
        l[b] = 0.2 * np.sin(2 * np.pi * 0.047 * n[b]) + 0.3 * np.sin(2 * np.pi * 0.21 * n[b])
        x = np.stack([l, 0.25 * l])
    elif kind == "chirp":    # 100 Hz to 12 kHz (at 48 kHz) in CHIRP_FRAMES frames, over and over; the right channel late and lower
        u = (n % CHIRP_FRAMES) / CHIRP_FRAMES
        f0, f1 = 100.0 / 48000.0, 12000.0 / 48000.0
        phase = 2 * np.pi * f0 * CHIRP_FRAMES * (np.power(f1 / f0, u) - 1.0) / np.log(f1 / f0)
        x = np.stack([0.5 * np.sin(phase), 0.25 * np.sin(np.roll(phase, 100))])
    else:
        raise ValueError(kind)
    return x[:channels].astype(np.float32)


def scan(x, sr):
    """a long signal from counter 0: float32 strengths [4, N] and flags [N] of the columns n = 1 .. N (column n ends at frame n H;
    what came before frame 0 is zeros), oldest first, every column with its twenty in view decided as a read would decide it"""
    x = np.asarray(x, np.float32).astype(np.float64)
    if x.ndim == 1:
        x = x[None]
    x = np.concatenate([np.zeros((x.shape[0], P)), x], axis=1)[None]
    n = (x.shape[-1] - P) // H
    o = flux(levels_at(x, [P + i * H for i in range(n + 1)], sr))  # [1, 4, n], oldest first
    flags = pick(o[:, :, ::-1])[0, ::-1]
    return o[0], flags


# the events of the definition's prototype, 4 s at 48 kHz each: (name, builder(rng) -> (float32 [frames], the frames where events start))
SR, LONG = 48000, 4 * 48000


def _noise(rng, db, frames=LONG):
    return rng.standard_normal(frames) * 10.0 ** (db / 20.0)


def kicks(rng):
    """a 60 Hz kick with a decay of 60 ms every 0.5 s over noise at -40 dBFS"""
    x = _noise(rng, -40.0)
    starts = list(range(12000, LONG - 12000, 24000))
    n = np.arange(9600)
    for s in starts:
        x[s:s + 9600] += 0.8 * np.sin(2 * np.pi * 60.0 * n / SR) * np.exp(-n / (0.06 * SR))
    return x.astype(np.float32), starts


def bursts(rng):
    """noise bursts of 50 ms at -10 dBFS every 0.4 s over noise at -30 dBFS"""
    x = _noise(rng, -30.0)
    starts = list(range(10000, LONG - 12000, 19200))
    for s in starts:
        x[s:s + 2400] += _noise(rng, -10.0, 2400)
    return x.astype(np.float32), starts


def legato(rng):
    """notes of equal level that change every 0.5 s without a gap (three harmonics each), phase-continuous per partial"""
    notes = (220.0, 277.18, 329.63, 392.0, 440.0, 349.23, 293.66, 261.63)
    starts = list(range(24000, LONG, 24000))
    x = np.zeros(LONG)
    n = np.arange(24000)
    for i, f in enumerate(notes):
        seg = sum(a * np.sin(2 * np.pi * f * h * n / SR) for h, a in ((1, 0.3), (2, 0.15), (3, 0.08)))
        x[i * 24000:(i + 1) * 24000] = seg
    x += _noise(rng, -70.0)
    return x.astype(np.float32), starts


def stationary(rng, db):
    return _noise(rng, db).astype(np.float32), []


def steady_sine(rng):
    return (0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(LONG) / SR)).astype(np.float32), []


# what tests/test_gpu_onset.py compares against the restatement: (fft size asked for, sample rate, captured channels, configuration
# overrides, ring_frames asked for (0: the default), the ring's capacity, T); test_onset_cpu.py checks the conditions on them
GPU_SEED = 20261019
GPU_CASES = [
    (1024, 48000, 2, {}, 8192, 8192, 27),       # the smallest ring
    (4096, 48000, 1, {}, 0, 8192, 27),          # one captured channel
    (4096, 44100, 2, {}, 16384, 16384, 59),     # (the canary guards on)
    (4096, 48000, 2, {}, 32768, 32768, 123),
    (4096, 48000, 2, {}, 65536, 65536, 128),    # Ts = 129: the last round has one wave with a column
    (2048, 48000, 1, {}, 65536, 65536, 128),
    # a meter batch: a buffer of 48000 * 0.046 = 2208 frames, wpos starts at 0
    (1024, 48000, 2, dict(meter=1, bars=0, meter_ms=46), 0, 8192, 27),
]


def case_id(case):
    fft, sr, ch, kw, ring_frames, ring_cap, t = case
    return f"ring{ring_cap}_sr{sr}_ch{ch}" + ("_meter" if kw.get("meter") else f"_fft{fft}")


def case_wpos0(case):
    """the write counter of a fresh handle: a spectrum batch starts with fft_size zeros, a meter batch at 0"""
    return 0 if case[3].get("meter") else case[0]


def case_audio(case):
    """the frames test_gpu_onset.py pushes for a case, float32 [3, channels, ring_cap + P / 2 + 3]: the span read wraps the ring and
    the counter ends off the hop grid"""
    fft, sr, ch, kw, ring_frames, ring_cap, t = case
    rng = np.random.default_rng(GPU_SEED + ring_cap + ch)
    frames = ring_cap + P // 2 + 3
    return np.stack([signal(k, rng, frames, ch, t * H + P) for k in KINDS])


packets = sono_ref.packets
