"""Float64 restatement of WF_HIP_OUT_SONO (include/wf_hip.h, "sonogram"): the level in 64 bands of an eighth of an octave of
the newest T Hann windows of 1024 frames, 256 frames apart and anchored to the stream's sample counter, with numpy's rfft per
channel and column.  Nothing here knows how the device transforms or sums.  Also the signals the tests push, the cases the CPU and
the device tests share, and the comparison (mismatches)."""
import numpy as np

WINDOW, HOP, COLUMNS, BANDS = 1024, 256, 64, 64  # WF_HIP_SONO_WINDOW, _HOP, _COLUMNS, _BANDS
P, H = WINDOW, HOP
DEAD_RATIO = 2.0 ** -80  # WF_HIP_STEREO_DEAD_RATIO
EDGES_HZ = 62.5 * np.exp2(np.arange(BANDS + 1, dtype=np.float64) / 8.0)
SCALE = 32.0 / (3.0 * P * P)
FIELDS = ("db", "columns", "newest", "first_covered", "end_covered", "window", "hop", "reserved")
SONO_DTYPE = np.dtype([("db", np.float32, (2, COLUMNS, BANDS)), ("columns", np.uint32), ("newest", np.uint32), ("first_covered", np.uint32),
                       ("end_covered", np.uint32), ("window", np.uint32), ("hop", np.uint32), ("reserved", np.uint32, (2,))])
ARM1_RATIO = 1e-9   # a cell whose band power is at least this share of its column's largest is held to two float32 ulps
ARM2_SHARE = 1e-10  # the others: the linear powers differ by less than this share of the column's largest


def columns(ring_cap):
    """T: how many columns a ring of ring_cap frames always holds"""
    return min(COLUMNS, (ring_cap - P) // H)


def edges_bins(sr):
    return EDGES_HZ * P / float(sr)


def covered(sr):
    """(first_covered, end_covered)"""
    e = edges_bins(sr)
    return int(np.argmax(e[:-1] >= 0.5)), int(np.count_nonzero(e[1:] <= P / 2 - 0.5))


def band_weights(sr):
    """[64, P/2]: the share of bin k in band b; bin 0 has none"""
    e = edges_bins(sr)
    k = np.arange(P // 2, dtype=np.float64)
    w = np.maximum(np.minimum(k[None] + 0.5, e[1:, None]) - np.maximum(k[None] - 0.5, e[:-1, None]), 0.0)
    w[:, 0] = 0.0
    return w


def hann():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(P) / P)


def band_powers(hist, wpos, sr, ring_cap):
    """hist: float32 [streams, channels, L], the frames of counter positions [wpos - L, wpos), the newest last (what came before
    reads as the zeros of create).  B: float64 [streams, 2, T, 64], age 0 first, the dead-channel rule applied, channel 1 of a
    capture of one channel 0.  wpos: one counter for the whole batch, or [streams] of them, each stream's history ending at its own"""
    if np.ndim(wpos):
        assert len(wpos) == len(hist)
        return np.concatenate([band_powers(hist[s:s + 1], int(w), sr, ring_cap) for s, w in enumerate(wpos)])
    hist = np.asarray(hist, np.float32).astype(np.float64)
    streams, ch, length = hist.shape
    t = columns(ring_cap)
    span = (t - 1) * H + P + (int(wpos) % H)
    if length < span:
        hist = np.concatenate([np.zeros((streams, ch, span - length)), hist], axis=2)
        length = span
    end = length - (int(wpos) % H)  # where column `newest` ends
    wt = band_weights(sr)
    w = hann()
    out = np.zeros((streams, 2, t, BANDS))
    for a in range(t):
        seg = hist[:, :, end - a * H - P:end - a * H]
        x = np.fft.rfft(w * seg, axis=-1)[..., :P // 2]
        out[:, :ch, a] = (np.abs(x) ** 2) @ wt.T
    if ch == 2:
        a, b = out[:, 0].copy(), out[:, 1].copy()
        out[:, 0] = np.where(a > b * DEAD_RATIO, a, 0.0)
        out[:, 1] = np.where(b > a * DEAD_RATIO, b, 0.0)
    return out


def to_db(power):
    with np.errstate(divide="ignore"):
        return np.where(power > 0, 10.0 * np.log10(power * SCALE), -np.inf).astype(np.float32)


def sono(hist, wpos, sr, ring_cap):
    """[streams] of wf_hip_sono"""
    b = band_powers(hist, wpos, sr, ring_cap)
    out = np.zeros(b.shape[0], SONO_DTYPE)
    out["db"] = -np.inf
    out["db"][:, :, :b.shape[2]] = to_db(b)
    out["columns"] = b.shape[2]
    out["newest"] = (np.asarray(wpos).astype(np.int64) % (1 << 32)) // H  # (a scalar or [streams])
    out["first_covered"], out["end_covered"] = covered(sr)
    out["window"], out["hop"] = P, H
    return out


def mismatches(got, hist, wpos, sr, ring_cap):
    """(bad, arm2): `bad` lists (field, index, got, want) of everything in `got` ([streams] of wf_hip_sono) outside the contract
    against the restatement of `hist`; arm2[s] counts the cells of stream s that passed by the second arm.
    The header words are equal.  Where the restatement reads -inf -- columns >= T, bands outside the spectrum, silence, a dead
    channel -- so does `got`.  Every other cell: where the restatement's band power is at least ARM1_RATIO of the largest band
    power of its column (both channels), within two float32 ulps of the restatement's float32; else the linear powers differ by
    less than ARM2_SHARE of that largest power."""
    want = sono(hist, wpos, sr, ring_cap)
    if got.shape != want.shape or got.dtype != want.dtype:
        return [("shape", (), (got.shape, got.dtype), (want.shape, want.dtype))], None
    bad = []
    for name in FIELDS[1:]:
        bad += [(name, tuple(i), got[name][tuple(i)].item(), want[name][tuple(i)].item()) for i in np.argwhere(got[name] != want[name])[:5]]
    t = int(want["columns"][0])
    power = band_powers(hist, wpos, sr, ring_cap)                      # [streams, 2, T, 64]
    largest = power.max(axis=(1, 3), keepdims=True)                    # of the column
    g, w = got["db"], want["db"]
    empty = np.isneginf(w)
    ok = np.where(empty, g == w, False)
    gt, wn = g[:, :, :t].astype(np.float64), w[:, :, :t].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        arm1 = (power >= ARM1_RATIO * largest) & (power > 0)
        near = np.abs(gt - wn) <= 2.0 * np.spacing(np.abs(w[:, :, :t])).astype(np.float64)
        gp = np.where(np.isneginf(gt), 0.0, 10.0 ** (gt / 10.0) / SCALE)
        close = np.abs(gp - power) < ARM2_SHARE * largest
    live = ~empty[:, :, :t]
    ok[:, :, :t] |= live & np.where(arm1, near & np.isfinite(gt), close & ~np.isnan(gt) & ~np.isposinf(gt))
    bad += [("db", tuple(i), float(g[tuple(i)]), float(w[tuple(i)])) for i in np.argwhere(~ok)[:8]]
    arm2 = (live & ~arm1).sum(axis=(1, 2, 3))
    return bad, arm2


# ---- the signals ------------------------------------------------------------------------------------------------------------------

KINDS = ("noise", "burst", "chirp")
CHIRP_FRAMES = 1536  # one sweep of the chirp: six hops, so that neighbouring columns hold different stretches of it


def signal(kind, rng, frames, channels=2, span=None):
    """float32 [channels, frames] of one kind of audio; the burst's events lie in the newest `span` frames (None: all of them)"""
    n = np.arange(frames, dtype=np.float64)
    if kind == "noise":      # independent noise
        x = rng.standard_normal((2, frames)) * 0.2
    elif kind == "burst":    # silence, then a noise burst, then two tones that step to two others; the right channel dead
        l = np.zeros(frames)
        span = frames if span is None else min(span, frames)
        q, at = span // 4, frames - span
        m = min(700, span // 5)
        l[at + q:at + q + m] = rng.standard_normal(m) * 0.3
        a, b = slice(at + 2 * q, at + 3 * q), slice(at + 3 * q, frames)
        l[a] = 0.4 * np.sin(2 * np.pi * 0.021 * n[a]) + 0.1 * np.sin(2 * np.pi * 0.13 * n[a])
        l[b] = 0.2 * np.sin(2 * np.pi * 0.047 * n[b]) + 0.3 * np.sin(2 * np.pi * 0.21 * n[b])
        x = np.stack([l, np.zeros(frames)])
    elif kind == "chirp":    # 100 Hz to 12 kHz (at 48 kHz) in CHIRP_FRAMES frames, over and over; the right channel late and lower
        u = (n % CHIRP_FRAMES) / CHIRP_FRAMES
        f0, f1 = 100.0 / 48000.0, 12000.0 / 48000.0
        phase = 2 * np.pi * f0 * CHIRP_FRAMES * (np.power(f1 / f0, u) - 1.0) / np.log(f1 / f0)
        x = np.stack([0.5 * np.sin(phase), 0.25 * np.sin(np.roll(phase, 100))])
    else:
        raise ValueError(kind)
    return x[:channels].astype(np.float32)


# what tests/test_gpu_sono.py compares against the restatement: (fft size asked for, sample rate, captured channels, configuration
# overrides, ring_frames asked for (0: the default), the ring's capacity, T); test_sono_cpu.py checks the conditions on them
GPU_SEED = 20261019
GPU_CASES = [
    (128, 48000, 2, {}, 2048, 2048, 4),       # one workgroup with no idle wave
    (1024, 48000, 1, {}, 0, 4096, 12),        # one captured channel
    (4096, 44100, 2, {}, 0, 8192, 28),
    (4096, 48000, 2, {}, 32768, 32768, 64),
    (4096, 48000, 2, {}, 16384, 16384, 60),
    # a meter batch: a buffer of 48000 * 0.046 = 2208 frames, wpos starts at 0
    (1024, 48000, 2, dict(meter=1, bars=0, meter_ms=46), 0, 8192, 28),
]


def case_id(case):
    fft, sr, ch, kw, ring_frames, ring_cap, t = case
    return f"ring{ring_cap}_sr{sr}_ch{ch}" + ("_meter" if kw.get("meter") else f"_fft{fft}")


def case_wpos0(case):
    """the write counter of a fresh handle: a spectrum batch starts with fft_size zeros, a meter batch at 0"""
    return 0 if case[3].get("meter") else case[0]


def case_audio(case):
    """the frames test_gpu_sono.py pushes for a case, float32 [3, channels, ring_cap + P / 2 + 3]: the span read wraps the ring and
    the counter ends off the hop grid"""
    fft, sr, ch, kw, ring_frames, ring_cap, t = case
    rng = np.random.default_rng(GPU_SEED + ring_cap + ch)
    frames = ring_cap + P // 2 + 3
    return np.stack([signal(k, rng, frames, ch, (t - 1) * H + P) for k in KINDS])


def packets(rng, total):
    """(lo, hi) of packets of unequal odd lengths of 1 .. 699 frames that add up to `total` (an even rest goes as an odd packet and
    one frame)"""
    cuts, at = [], 0
    while at < total:
        n = min(2 * int(rng.integers(0, 350)) + 1, total - at)
        if n % 2 == 0:
            n -= 1
        cuts.append((at, at + n))
        at += n
    return cuts
