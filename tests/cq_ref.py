"""Float64 restatement of WF_HIP_OUT_CQ (include/wf_hip.h, "constant-Q spectrum"): one level per semitone and captured channel,
bin b over the newest L_b frames, as direct sums per bin with numpy.  The tests compare the device against it; nothing here
knows how the device stages, rotates or sums.  Also the test signal the device tests push (audio) and the criterion they hold
the device to (mismatches)."""
import numpy as np

BINS = 120  # WF_HIP_CQ_BINS
MAX_WINDOW = 16384  # WF_HIP_CQ_MAX_WINDOW
Q = 1.0 / (2.0 ** (1.0 / 12.0) - 1.0)
CQ_DTYPE = np.dtype([("db", np.float32, (2, BINS)), ("end_covered", np.uint32), ("first_resolved", np.uint32),
                     ("max_window", np.uint32), ("reserved", np.uint32)])


def centres():
    """f_b [120]: 440 * 2^((b - 57) / 12)"""
    return 440.0 * 2.0 ** ((np.arange(BINS) - 57.0) / 12.0)


def max_window(ring_frames):
    return min(int(ring_frames), MAX_WINDOW)


def full_windows(sr):
    """Q sr / f_b [120], before the ceil"""
    return Q * float(sr) / centres()


def geometry(sr, lmax):
    """(L [120] int, end_covered, first_resolved) of a sample rate and Lmax"""
    full = np.ceil(full_windows(sr))
    covered = centres() * 2.0 ** (1.0 / 24.0) < sr / 2.0
    end_covered = int(np.argmin(covered)) if not covered.all() else BINS
    assert covered[:end_covered].all() and not covered[end_covered:].any()  # a prefix
    resolved = full <= lmax
    first_resolved = int(np.argmax(resolved)) if resolved.any() else BINS
    return np.minimum(full, lmax).astype(np.int64), end_covered, first_resolved


def amplitudes(frames, sr, lmax):
    """frames: float32 [streams, channels, >= lmax], the newest last.  a_b, float64 [streams, channels, 120]; 0 in the uncovered
    bins"""
    x = np.asarray(frames, np.float32).astype(np.float64)
    assert x.shape[-1] >= lmax
    L, end_covered, _ = geometry(sr, lmax)
    f = centres()
    a = np.zeros(x.shape[:-1] + (BINS,))
    for b in range(end_covered):
        n = np.arange(L[b], dtype=np.float64)
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / L[b])
        s = x[..., x.shape[-1] - L[b]:] @ (w * np.exp(-2j * np.pi * f[b] * n / sr))
        a[..., b] = 4.0 * np.abs(s) / L[b]
    return a


def struct_of(a, sr, lmax):
    """the wf_hip_cq of amplitudes a [streams, 1 or 2, 120]"""
    _, end_covered, first_resolved = geometry(sr, lmax)
    out = np.zeros(a.shape[0], CQ_DTYPE)
    out["db"] = -np.inf
    with np.errstate(divide="ignore"):
        db = np.where(a > 0.0, 20.0 * np.log10(a), -np.inf)
    db[..., end_covered:] = -np.inf
    out["db"][:, :a.shape[1]] = db
    out["end_covered"], out["first_resolved"], out["max_window"] = end_covered, first_resolved, lmax
    return out


def cq(frames, sr, ring_frames):
    """frames: float32 [streams, channels, >= Lmax]: the newest frames of every captured channel's ring, the newest last"""
    lmax = max_window(ring_frames)
    return struct_of(amplitudes(frames, sr, lmax), sr, lmax)


def audio(rng, streams, frames, sr):
    """float32 [streams, 2, frames]: white Gaussian noise of rms 0.25 plus sines at 55 Hz (A1) and 440 Hz (A4) whose amplitudes
    (0.05 .. 0.2) and phases differ per channel and stream"""
    t = np.arange(frames)
    x = 0.25 * rng.standard_normal((streams, 2, frames))
    for f in (55.0, 440.0):
        amp = rng.uniform(0.05, 0.2, (streams, 2, 1))
        ph = rng.uniform(0.0, 2.0 * np.pi, (streams, 2, 1))
        x += amp * np.sin(2.0 * np.pi * f * t / sr + ph)
    return x.astype(np.float32)


def peak(frames, lmax):
    """pk [streams, channels]: max |x| over the newest Lmax frames"""
    return np.abs(np.asarray(frames, np.float32)[..., -lmax:]).max(axis=-1).astype(np.float64)


def strong(a, pk):
    """[streams, channels, 120] bool: the bins with a_b >= 1e-3 pk, which must agree to two float32 ulps"""
    return a >= 1e-3 * pk[..., None]


def mismatches(got, frames, sr, ring_frames):
    """(what, index, got, want) of everything in `got` ([streams] of wf_hip_cq) outside the contract against the restatement of
    `frames` [streams, channels, >= Lmax].  Per covered bin, either |got - want| <= 2 float32 ulps of want, or
    |10^(got / 20) - a_want| <= 1e-10 pk; a bin with a_want >= 1e-3 pk must pass the first.  The uncovered bins, a channel that
    was not captured and the four integer fields are compared exactly."""
    lmax = max_window(ring_frames)
    a = amplitudes(frames, sr, lmax)
    want = struct_of(a, sr, lmax)
    pk = peak(frames, lmax)
    ch, end = a.shape[1], int(want["end_covered"][0])
    bad = []
    for name in ("end_covered", "first_resolved", "max_window", "reserved"):
        bad += [(name, tuple(i), int(got[name][tuple(i)]), int(want[name][tuple(i)])) for i in np.argwhere(got[name] != want[name])[:5]]
    g, w = got["db"], want["db"]
    exact = np.ones(g.shape, bool)
    exact[:, :ch, :end] = False
    bad += [("db exact", tuple(i), float(g[tuple(i)]), float(w[tuple(i)])) for i in np.argwhere(exact & (g != w))[:5]]
    g, w = g[:, :ch, :end], w[:, :ch, :end]
    with np.errstate(invalid="ignore", over="ignore"):
        arm1 = np.where(np.isinf(w), g == w, np.abs(g.astype(np.float64) - w.astype(np.float64)) <= 2.0 * np.spacing(np.abs(w)).astype(np.float64))
        arm1 &= ~np.isnan(g)
        arm2 = np.abs(10.0 ** (g.astype(np.float64) / 20.0) - a[..., :end]) <= 1e-10 * pk[..., None]
    ok = arm1 | (arm2 & ~strong(a, pk)[..., :end])
    bad += [("db", tuple(i), float(g[tuple(i)]), float(w[tuple(i)])) for i in np.argwhere(~ok)[:8]]
    return bad


def worst(got, frames, sr, ring_frames):
    """for the tests' printed figures: (largest |got - want| in float32 ulps of want over the strong bins, the number of covered
    bins further than two ulps from want, the largest |10^(got/20) - a_want| / pk among those, the share of strong bins among
    the covered)"""
    lmax = max_window(ring_frames)
    a = amplitudes(frames, sr, lmax)
    want = struct_of(a, sr, lmax)
    pk = peak(frames, lmax)
    ch, end = a.shape[1], int(want["end_covered"][0])
    g, w = got["db"][:, :ch, :end].astype(np.float64), want["db"][:, :ch, :end]
    st = strong(a, pk)[..., :end]
    with np.errstate(invalid="ignore", over="ignore"):
        ulps = np.abs(g - w.astype(np.float64)) / np.spacing(np.abs(w)).astype(np.float64)
        lin = np.abs(10.0 ** (g / 20.0) - a[..., :end]) / pk[..., None]
    far = ulps > 2.0
    return float(np.max(ulps[st], initial=0.0)), int(far.sum()), float(np.max(lin[far], initial=0.0)), float(st.mean())


# what tests/test_gpu_cq.py compares against the restatement: (fft_size, sample rate, ring_frames asked for (0: the default),
# captured channels, configuration overrides, the Lmax that results); test_cq_cpu.py checks the condition of audio() on them
GPU_SEED = 20261017
GPU_CASES = [
    (128, 48000, 128, 2, {}, 128),            # nearly everything unresolved
    (2064, 44100, 0, 2, {}, 8192),            # not a power of two; the default ring of 2 * 2064 frames rounds up to 8192
    (4096, 48000, 16384, 2, {}, 16384),       # the cap
    (16384, 96000, 0, 2, {}, 16384),          # ring 32768, wider than the cap
    (1024, 8000, 0, 1, {}, 4096),             # bins above Nyquist uncovered; mono
    (1024, 48000, 0, 2, dict(meter=1, bars=0), 16384),  # a meter batch (its ring follows the meter's buffer, not fft_size)
]


def case_id(case):
    fft, sr, ring, ch, kw, _ = case
    return f"n{fft}_sr{sr}_ring{ring}_ch{ch}" + "".join(f"_{k}{v}" for k, v in kw.items() if k != "bars")


def case_audio(case, streams=3):
    """the frames test_gpu_cq.py pushes for a case: Lmax + 2 * 801 of audio(), float32 [streams, channels, frames]"""
    fft, sr, _, ch, _, lmax = case
    return audio(np.random.default_rng(GPU_SEED + fft + sr), streams, lmax + 2 * 801, sr)[:, :ch]
