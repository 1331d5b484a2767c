"""Numpy float64 restatement of WF_HIP_OUT_IMPULSE (include/wf_hip.h, "impulse response"): the response over time of captured
channel 0 (measured) against channel 1 (reference) -- ir, its energy-time curve etc_db and the up to eight strongest arrivals --
from the regularised average of the segments WF_HIP_OUT_XFER reads.  The sums, the lag and the fields the two records share come
from tests/xfer_ref.py unchanged; nothing here knows how the device transforms or reduces.  For the comparison of orderings
(tests/test_impulse_cpu.py) three more orders of the same definition: "descending" (the segments newest first), "pairwise" (every sum
over segments and over time by pairs) and "radix2" (both inverse transforms by a hand-rolled radix-2 transform instead of numpy.fft).
Also the signal kinds the tests push and the audio of the cases the CPU and the device tests share (the cases are xfer_ref.GPU_CASES).

Bound of `mismatches` -- derived, not measured: both sides work in float64 from the same float32 samples and differ only in the order
of operations.
  ir            |got - want| <= one float32 ulp of want + FLOOR max|ir|
  etc_db        in the linear domain, 10^(etc_db / 20): |got - want| <= 2^-22 |want| + FLOOR env[peak]; -inf only equals -inf
  float32 scalars and arrival fields   one float32 rounding (one ulp of the wanted value); for `frames` and delay_ms FRAC_FLOOR on
                top: the fraction is 0.5 (l - r) / curvature, a difference that cancels -- at lag 0 under a symmetric peak the whole
                field is that rounding, and no ulp of it means anything.  The envelope is good to FLOOR of the peak and the curvature
                of an arrival is at least MARGIN of it (`margins`), so the fraction is good to 2 FLOOR / MARGIN = 2e-8 frames
  integer fields, polarity             equal
FLOOR = 1e-11 of the peak rests on test_impulse_cpu.py: the four orders agree within 1e-13 of the peak in ir and the envelope on the
very seeds and shapes of the device cases (it asserts that and prints the figure), so the floor has a hundredfold margin; and no
decision is near a tie there: `margins` are at least MARGIN = 1e-3 on every stream whose lag is asserted (margins_hold has the one
exception).  (On an MI355X every float32 field of every case of tests/test_gpu_impulse.py came out equal to the restatement's.)"""
import numpy as np

import xfer_ref
from delay_ref import taper

FRAMES = 2048           # WF_HIP_IMPULSE_FRAMES
ARRIVALS = 8            # WF_HIP_IMPULSE_ARRIVALS
GUARD = 8               # WF_HIP_IMPULSE_GUARD
DIRECT = 16             # WF_HIP_IMPULSE_DIRECT
REG = 1e-6              # WF_HIP_IMPULSE_REG
ARRIVAL_RATIO = 0.031622776601683794  # WF_HIP_IMPULSE_ARRIVAL_RATIO
FLOOR = 1e-11
MARGIN = 1e-3
NOISY_TOP_MARGIN = 1e-5
FRAC_FLOOR = 2.0 * FLOOR / MARGIN
ARRIVAL_DTYPE = np.dtype([("frames", np.float32), ("level_db", np.float32), ("polarity", np.int32), ("reserved", np.uint32)])
IMPULSE_DTYPE = np.dtype([("valid", np.uint32), ("window", np.uint32), ("hop", np.uint32), ("segments", np.uint32), ("lag", np.int32),
                          ("newest", np.uint32), ("lag_peak", np.float32), ("mean_coherence", np.float32), ("count", np.uint32),
                          ("peak_index", np.uint32), ("peak_db", np.float32), ("delay_ms", np.float32), ("energy_db", np.float32),
                          ("direct_db", np.float32), ("reserved", np.uint32, (2,)), ("arrivals", ARRIVAL_DTYPE, (ARRIVALS,)),
                          ("ir", np.float32, (FRAMES,)), ("etc_db", np.float32, (FRAMES,))])
SHARED_FIELDS = ("valid", "window", "hop", "segments", "lag", "newest", "lag_peak", "mean_coherence")  # wf_hip_xfer's, bit for bit
INT_FIELDS = ("valid", "window", "hop", "segments", "lag", "newest", "count", "peak_index", "reserved")
FLOAT_SCALARS = ("lag_peak", "mean_coherence", "peak_db", "delay_ms", "energy_db", "direct_db")
ORDERS = ("ascending", "descending", "pairwise", "radix2")
_XFER_ORDER = {"ascending": "ascending", "descending": "descending", "pairwise": "pairwise", "radix2": "ascending"}


def _fft_radix2(x):
    """the forward transform of a power-of-two length, decimation in time, by recursion"""
    n = x.shape[0]
    if n == 1:
        return x.astype(np.complex128)
    even, odd = _fft_radix2(x[0::2]), _fft_radix2(x[1::2])
    tw = np.exp(-2j * np.pi * np.arange(n // 2) / n) * odd
    return np.concatenate([even + tw, even - tw])


def _inverse(spec, order):
    """y[n] = (1 / P) sum_k spec[k] e^(+j 2 pi k n / P)"""
    p = spec.shape[0]
    if order == "radix2":  # one forward transform read at (-n) mod P
        return _fft_radix2(spec)[(-np.arange(p)) % p] / p
    return np.fft.ifft(spec)


def _total(v, order):
    return float(xfer_ref._sum(np.asarray(v, np.float64).reshape(-1, 1), "pairwise" if order == "pairwise" else "ascending")[0]) if len(v) else 0.0


def _db(x, scale):
    with np.errstate(divide="ignore"):
        return scale * np.log10(x)


def pick(env):
    """the indices of the arrivals of an envelope, the peak first (empty where the envelope is all 0)"""
    p = env.shape[0]
    ipk = int(np.argmax(env))  # (the first of equal values)
    if not env[ipk] > 0.0:
        return []
    i = np.arange(1, p - 1)
    cand = i[(env[i] > env[i - 1]) & (env[i] >= env[i + 1]) & (env[i] >= ARRIVAL_RATIO * env[ipk])]
    taken = [ipk]
    while len(taken) < ARRIVALS:
        free = cand[np.all(np.abs(cand[:, None] - np.array(taken)[None, :]) > GUARD, axis=1)]
        if free.size == 0:
            break
        taken.append(int(free[np.argmax(env[free])]))  # (the first of equal values: the lower index)
    return taken


def vertex(env, i):
    if i == 0 or i == env.shape[0] - 1:
        return 0.0
    l, c, r = env[i - 1], env[i], env[i + 1]
    curv = (l - c) + (r - c)
    return float(np.clip(0.5 * (l - r) / curv, -0.5, 0.5)) if curv < 0.0 else 0.0


def analyse(x, w, ring, sr, lag=None, wpos=None, order="ascending"):
    """x, w, ring, sr, lag, wpos: as xfer_ref.analyse.  (one wf_hip_impulse as a 0-d record, the float64 values behind its fields as a
    dict -- empty for an invalid record)"""
    xrec, xv = xfer_ref.analyse(x, w, ring, sr, lag, wpos, _XFER_ORDER[order])
    out = np.zeros((), IMPULSE_DTYPE)
    for name in SHARED_FIELDS:
        out[name] = xrec[name]
    if not xv:
        return out, {}
    p = int(xrec["window"])
    m, l = p // 2, p // 4
    n0 = int(xrec["lag"])
    sxx, sxy = xv["sxx"], xv["sxy"]
    d = sxx + REG * float(np.max(sxx))
    hr = np.zeros(m - 1, np.complex128)
    ok = d > 0.0
    hr[ok] = sxy.real[ok] / d[ok] + 1j * (sxy.imag[ok] / d[ok])
    kk = np.arange(1, m)
    full = np.zeros(p, np.complex128)
    full[kk] = hr
    full[p - kk] = np.conj(hr)
    at = (np.arange(p) - l) % p
    h = _inverse(full, order).real[at]
    one = np.zeros(p, np.complex128)
    one[kk] = 2.0 * (2.0 * taper(p)[2 * kk]) * hr
    a = _inverse(one, order)[at]
    env = np.abs(a)
    taken = pick(env)
    vals = dict(xv, h=h, a=a, env=env, taken=taken, hr=hr)
    out["ir"][:p] = h
    out["etc_db"][:p] = _db(env, 20.0)
    if not taken:  # no response: the measured channel is +-0 under every segment
        out["ir"][:p] = 0.0
        return out, vals
    ipk = taken[0]
    frames = [n0 + i - l + vertex(env, i) for i in taken]
    for s, i in enumerate(taken):
        out["arrivals"][s] = (frames[s], _db(env[i] / env[ipk], 20.0), 1 if a[i].real >= 0.0 else -1, 0)
    near = np.abs(np.arange(p) - ipk) <= DIRECT
    vals.update(frames=frames, energy=_total(h * h, order), direct=_total((h * h)[near], order))
    out["count"], out["peak_index"] = len(taken), ipk
    out["peak_db"], out["delay_ms"] = _db(env[ipk], 20.0), frames[0] * 1000.0 / sr
    out["energy_db"], out["direct_db"] = _db(vals["energy"], 10.0), _db(vals["direct"], 10.0)
    return out, vals


def _each(frames, lag, wpos):
    n = len(frames)
    lags = list(lag) if isinstance(lag, (list, tuple, np.ndarray)) else [lag] * n
    pos = list(wpos) if isinstance(wpos, (list, tuple, np.ndarray)) else [wpos] * n
    return zip(frames, lags, pos)


def impulse(frames, w, ring, sr, lag=None, wpos=None, order="ascending"):
    """frames: float32 [streams, 2, n], the frames pushed, the newest last; lag and wpos as xfer_ref.xfer takes them"""
    return np.array([analyse(x, w, ring, sr, lg, wp, order)[0] for x, lg, wp in _each(frames, lag, wpos)], IMPULSE_DTYPE)


def zero_record(w, ring, streams):
    p, k = xfer_ref.geometry(w, ring)
    s = np.zeros((), IMPULSE_DTYPE)
    s["window"], s["hop"], s["segments"] = p, p // 2, k
    return np.repeat(s, streams)


def margins(frames, w, ring, sr, lag=None, wpos=None):
    """[streams, 3], how far every decision of a stream is from a tie (nan for an invalid record, inf where there is no such
    decision): the lag search's |r[n0]| - max_{n != n0} |r[n]|; the smallest gap in dB between consecutive arrivals behind the peak,
    between the last one taken and the strongest free candidate it was preferred to, and between the -30 dB rule and the arrival or
    the free local maximum nearest to it; the smallest env[i] - max(env[i - 1], env[i + 1]) of the arrivals behind the peak over
    env[peak]"""
    rows = []
    for x, lg, wp in _each(frames, lag, wpos):
        v = analyse(x, w, ring, sr, lg, wp)[1]
        if not v:
            rows.append((np.nan, np.nan, np.nan))
            continue
        env, taken = v["env"], v["taken"]
        if not taken:
            rows.append((np.inf, np.inf, np.inf))  # (no cross power in any bin: lag 0 without a search)
            continue
        top = env[taken[0]]
        level = lambda i: 20.0 * np.log10(env[i] / top)  # noqa: E731
        gaps, tops = [], []
        later = [level(i) for i in taken[1:]]
        gaps += [a - b for a, b in zip(later[:-1], later[1:])]
        i = np.arange(1, env.shape[0] - 1)
        local = i[(env[i] > env[i - 1]) & (env[i] >= env[i + 1]) & (env[i] > 0.0)]
        free = local[np.all(np.abs(local[:, None] - np.array(taken)[None, :]) > GUARD, axis=1)]
        rest = np.array([level(j) for j in free])
        if len(taken) == ARRIVALS and rest.size and later:
            gaps.append(later[-1] - float(np.max(rest)))
        gaps += [abs(v_ + 30.0) for v_ in later] + [abs(float(v_) + 30.0) for v_ in rest]
        tops = [(env[j] - max(env[j - 1], env[j + 1])) / top for j in taken[1:]]
        rows.append((v["margin"], min(gaps, default=np.inf), min(tops, default=np.inf)))
    return np.array(rows, np.float64)


def margins_hold(m, noisy=False):
    """whether one row of `margins` is far enough from a tie: MARGIN in all three figures.  A stream with noise as strong as its
    signal (NOISY) lists maxima of its floor, 25 dB under the peak -- 0.06 of it -- on an envelope whose main lobe is eight frames
    wide: such a maximum stands 1e-4 to 3e-3 of the peak above its neighbours whatever the seed, so MARGIN cannot be asked of the
    third figure there, and NOISY_TOP_MARGIN is: still a million times the bound's floor"""
    return bool(m[0] >= MARGIN and m[1] >= MARGIN and m[2] >= (NOISY_TOP_MARGIN if noisy else MARGIN))


def _lin(db):
    with np.errstate(over="ignore"):
        return np.power(10.0, np.asarray(db, np.float64) / 20.0)


def _ulp(f):
    f = np.asarray(f, np.float32)
    with np.errstate(invalid="ignore"):
        u = np.spacing(np.abs(f)).astype(np.float64)
    return np.where(np.isfinite(u), u, 0.0)


def _parts(got, want):
    """(name, |got - want|, the bound) of every float field, [streams, ...] each"""
    g64 = lambda a: np.asarray(a, np.float64)  # noqa: E731
    with np.errstate(invalid="ignore"):
        same_inf = lambda g, f: np.isinf(f) & (g == f)  # noqa: E731
        for name in FLOAT_SCALARS:
            g, f = g64(got[name]), g64(want[name])
            yield name, np.where(same_inf(g, f), 0.0, np.abs(g - f)), _ulp(want[name]) + (FRAC_FLOOR if name == "delay_ms" else 0.0)
        for name in ("frames", "level_db"):
            g, f = g64(got["arrivals"][name]), g64(want["arrivals"][name])
            yield "arrivals." + name, np.where(same_inf(g, f), 0.0, np.abs(g - f)), _ulp(want["arrivals"][name]) + (FRAC_FLOOR if name == "frames" else 0.0)
        g, f = g64(got["ir"]), g64(want["ir"])
        yield "ir", np.abs(g - f), _ulp(want["ir"]) + FLOOR * np.max(np.abs(f), axis=-1, keepdims=True)
        # the envelope in the linear domain; an entry that is -inf (or the 0 beyond P) on one side must be the same on the other
        gd, fd = g64(got["etc_db"]), g64(want["etc_db"])
        g, f = _lin(gd), _lin(fd)
        top = np.where(want["count"] > 0, _lin(want["peak_db"]), 0.0)[..., None]
        d = np.where(np.isneginf(gd) != np.isneginf(fd), np.inf, np.abs(g - f))
        yield "etc_db", d, 2.0 ** -22 * np.abs(f) + FLOOR * top


def worst(got, want):
    """the largest |got - want| of every float field (the envelope's in the linear domain), for printing"""
    return {name: float(np.max(d, initial=0.0)) for name, d, _ in _parts(got, want)}


def mismatches(got, want):
    """(field, index, got, want) of everything in `got` ([streams] of wf_hip_impulse) beyond the bound (the module's docstring) of
    `want`"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return [("shape", (), (got.shape, got.dtype), (want.shape, want.dtype))]
    bad = []
    for name in INT_FIELDS:
        bad.extend((name, tuple(i), got[name][tuple(i)].item(), want[name][tuple(i)].item()) for i in np.argwhere(got[name] != want[name])[:5])
    for name in ("polarity", "reserved"):
        g, f = got["arrivals"][name], want["arrivals"][name]
        bad.extend(("arrivals." + name, tuple(i), g[tuple(i)].item(), f[tuple(i)].item()) for i in np.argwhere(g != f)[:5])
    for name, d, tol in _parts(got, want):
        bad.extend((name, tuple(i), float(d[tuple(i)]), float(np.broadcast_to(tol, d.shape)[tuple(i)])) for i in np.argwhere(~(d <= tol))[:5])
    return bad


# ---- the signals ------------------------------------------------------------------------------------------------------------------

TAP_DELAY = 37
TAP_GAINS = (1.0, -0.5, 0.25)


def tap_offsets(p):
    """where the three taps lie behind the first: inside the first sixteenth, and just behind a quarter of the segment"""
    return (0, p // 16 + 5, p // 4 + 11)


ECHO_GAIN, ECHO_OFFSET = 0.5, 40          # the one echo of the stream with a negative lag
GUARD_DELAY = 12
GUARD_TAPS = ((0, 1.0), (20, 0.5), (6, 0.4))  # two echoes 20 frames apart, and a third inside the guard of the first

KINDS = ("three taps", "delay -(L-1), echo", "inverted -6 dB", "three taps, noise", "independent", "dual mono", "guarded echoes",
         "tone, measured zero")
LAST_KINDS = ("silent reference", "one NaN")  # the ninth stream of the cases with an even and an odd number
INVALID = LAST_KINDS
NO_LAG = ("independent",)  # the lag of unrelated channels is noise: exempt from its margin, compared at the device's lag
NO_RESPONSE = ("tone, measured zero",)
NOISY = ("three taps, noise",)  # lists maxima of its noise floor (margins_hold)


def true_lag(kind, p):
    return {"three taps": TAP_DELAY, "delay -(L-1), echo": -(p // 4 - 1), "inverted -6 dB": 0, "three taps, noise": TAP_DELAY, "dual mono": 0,
            "guarded echoes": GUARD_DELAY, "tone, measured zero": 0}.get(kind)


def _taps(s, taps, n):
    """sum_g g s(. - d) over (d, g) in taps, [n]"""
    y = np.zeros(n)
    for d, g in taps:
        y[d:] += g * s[:n - d]
    return y


def stream(kind, rng, frames, p, tail=3):
    """float32 [2, frames] of one kind of stereo audio for segments of p frames: row 0 the measured channel, row 1 the reference"""
    if kind in ("inverted -6 dB", "independent", "dual mono", "tone, measured zero", "silent reference", "one NaN"):
        return xfer_ref.stream(kind, rng, frames, p, tail)
    pad = p + 64
    n = frames + 2 * pad
    noise = lambda: 0.25 * rng.standard_normal(n)  # noqa: E731
    cut = lambda v: np.asarray(v[pad:pad + frames], np.float64).astype(np.float32)  # noqa: E731
    s = noise()
    if kind in ("three taps", "three taps, noise"):
        y = _taps(s, [(TAP_DELAY + d, g) for d, g in zip(tap_offsets(p), TAP_GAINS)], n)
        if kind == "three taps, noise":  # noise of the measured signal's own power on top
            y = y + np.sqrt(sum(g * g for g in TAP_GAINS)) * noise()
        return np.stack([cut(y), cut(s)])
    if kind == "delay -(L-1), echo":  # channel 0 is the earlier one
        d = p // 4 - 1
        y = _taps(s, [(0, 1.0), (ECHO_OFFSET, ECHO_GAIN)], n)
        return np.stack([cut(np.concatenate([y[d:], np.zeros(d)])), cut(s)])
    if kind == "guarded echoes":
        return np.stack([cut(_taps(s, [(GUARD_DELAY + d, g) for d, g in GUARD_TAPS], n)), cut(s)])
    raise ValueError(kind)


# (the first seed from 20270115 up at which every margin of every stream that is compared holds with twofold room: the condition
# of the bound, which tests/test_impulse_cpu.py asserts)
GPU_SEED = 20270117


def case_kinds(index):
    return KINDS + (LAST_KINDS[index % 2],)


def case_audio(case, index):
    """the frames test_gpu_impulse.py pushes for xfer_ref.GPU_CASES[index], float32 [9, 2, frames]: one ring and H + 3 frames, so
    that the span wraps the ring and the counter, wpos0 + frames, ends off the anchor"""
    fft, sr, kw, w, ring = case
    cap = xfer_ref.ring_frames(w, ring)
    p, k = xfer_ref.geometry(w, cap)
    rng = np.random.default_rng(GPU_SEED + w + cap)
    frames = cap + p // 2 + 3
    return np.stack([stream(name, rng, frames, p, (xfer_ref.case_wpos0(case) + frames) % (p // 2)) for name in case_kinds(index)])


# how many arrivals a kind has when the ring is full of it
TAPS_OF = {"three taps": 3, "delay -(L-1), echo": 2, "inverted -6 dB": 1, "dual mono": 1, "guarded echoes": 2}

# ---- the staggered batch ------------------------------------------------------------------------------------------------------------

STAGGER_KINDS = ("three taps", "delay -(L-1), echo", "inverted -6 dB", "guarded echoes", "three taps", "dual mono", "guarded echoes")


def stagger_script(case):
    """tests/measure_stagger.py's plan of `case` with this output's kinds in it, in the form its replay() takes (as
    xfer_ref.stagger_script makes its own)"""
    import measure_stagger as ms
    steps = ms.plan(case)
    frames = ms.totals(steps)
    p, k = xfer_ref.geometry(case.W, case.ring_cap)
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


def overlap(p, d):
    """rho(d) = sum_n w[n] w[n + d] / sum_n w[n]^2 of the periodic Hann window of p frames"""
    w = taper(p)
    return float(np.dot(w[:p - d], w[d:]) / np.dot(w, w))
