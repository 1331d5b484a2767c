"""The click detector (WF_HIP_OUT_CLICK) restated in numpy from include/wf_hip.h, "clicks": float64 with every product and every sum
rounded on its own, the float32 cast of |e| where the definition has it, the order statistics by np.sort, and r[k] summed in the
order the header fixes (256 strided partials in ascending n, six butterfly rounds within each 64 of them, the four groups in
order) -- a product of two float32 values is exact in float64, so numpy's plain sums are the device's fused ones and `r`, the
predictor and the residual are the same bits on both.  What is left to differ is log10 in the four kinds of dB field.

The bound (mismatches):
  integer fields                       equal
  float32 fields                       one float32 rounding: one ulp of the wanted value; infinities equal
It rests on conditions that tests/test_click_cpu.py asserts of every window the device test reads (margins): no judged frame's
ratio within 1e-3 of the threshold, no two listed strengths within 1e-4 dB, and the same hits with every median and g moved by one
float32 ulp either way.

Also here: the signals of both tests, and the device test's cases -- seven streams at seven write positions (gpu_script)."""
import numpy as np

from waveform_amd import binding

MAX_WINDOW = binding.CLICK_MAX_WINDOW
ORDER = binding.CLICK_ORDER
GAP = binding.CLICK_GAP
MAX_EVENTS = binding.CLICK_MAX_EVENTS
THRESHOLD = binding.CLICK_THRESHOLD
BLOCK = 256
MIN_WINDOW = 256
CLICK_DTYPE = binding.CLICK_DTYPE
CHANNEL_INT_FIELDS = ("valid", "events", "hit_frames", "listed")
CHANNEL_FLOAT_FIELDS = ("rate", "peak_db", "floor_db", "prediction_gain_db")
EVENT_INT_FIELDS = ("start", "length", "peak", "frame")
EVENT_FLOAT_FIELDS = ("strength_db", "amplitude")
RATIO_MARGIN = 1e-3
STRENGTH_MARGIN_DB = 1e-4


def window_frames(w):
    """P of a handle whose wf_hip_fft_size() is w"""
    return min(int(w), MAX_WINDOW)


def autocorrelation(x):
    """r[0 .. ORDER] of float64 x in the header's order"""
    P = len(x)
    rows = -(-P // 256)
    lanes = np.arange(64)
    r = np.zeros(ORDER + 1)
    for k in range(ORDER + 1):
        prod = np.zeros(rows * 256)
        prod[k:P] = x[k:] * x[:P - k]  # exact
        acc = np.zeros(256)
        for row in prod.reshape(rows, 256):  # partial t: n = t, t + 256, ... ascending
            acc = acc + row
        v = acc.reshape(4, 64)
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lanes ^ off]
        r[k] = ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]
    return r


def levinson(r):
    """(a[0 .. ORDER] with a[0] unused, E) of r with r[0] (1 + 1e-9), every operation in the header's order"""
    a = [0.0] * (ORDER + 1)
    E = float(r[0]) * (1.0 + 1e-9)
    for i in range(1, ORDER + 1):
        acc = float(r[i])
        for j in range(1, i):
            acc = acc - a[j] * float(r[i - j])
        k = acc / E
        nxt = list(a)
        for j in range(1, i):
            nxt[j] = a[j] - k * a[i - j]
        nxt[i] = k
        a = nxt
        E = E * (1.0 - k * k)
    return np.array(a), E


def _nudged(v, ulps):
    """float32 v moved by `ulps` float32 steps (not below 0)"""
    v = np.asarray(v, np.float32)
    if ulps == 0:
        return v
    return np.maximum(v.view(np.int32) + np.int32(ulps), 0).astype(np.int32).view(np.float32)


def analyse(x, sr=48000, wpos=None, nudge=0):
    """One channel: x float32 [P], the window.  Returns (record of CLICK_CHANNEL_DTYPE, ratio float64 [P] -- 0 for the frames not
    judged --, details).  wpos: the stream's counter at the read (default P: the window starts at position 0).  nudge: every m_b and
    g moved by that many float32 ulps, for the margin condition alone."""
    x32 = np.asarray(x, np.float32)
    P = len(x32)
    assert MIN_WINDOW <= P <= MAX_WINDOW
    wpos = P if wpos is None else int(wpos)
    rec = np.zeros((), binding.CLICK_CHANNEL_DTYPE)
    ratio = np.zeros(P)
    x = x32.astype(np.float64)
    bad = not np.all(np.isfinite(x))
    r = None if bad else autocorrelation(x)
    if bad or r[0] == 0.0:
        for name in ("peak_db", "floor_db", "prediction_gain_db"):
            rec[name] = -np.inf
        return rec, ratio, {}
    p = ORDER
    a, E = levinson(r)
    acc = np.zeros(P - p)
    for k in range(1, p + 1):
        acc = acc + a[k] * x[p - k:P - k]
    e = np.zeros(P)
    e[p:] = x[p:] - acc
    d = np.abs(e).astype(np.float32)
    judged = P - p
    nb = max(1, judged // BLOCK)
    edges = [p + b * BLOCK for b in range(nb)] + [P]
    med = _nudged([np.sort(d[edges[b]:edges[b + 1]])[(edges[b + 1] - edges[b]) // 2] for b in range(nb)], nudge).astype(np.float64)
    g = float(_nudged(np.sort(d[p:])[judged // 2], nudge))
    A = float(np.max(np.abs(x)))
    if nb == 1:  # a lone block has no neighbours: half the medians of its two halves stand in for them
        half = p + judged // 2
        med = np.concatenate([med, 0.5 * _nudged([np.sort(d[lo:hi])[(hi - lo) // 2] for lo, hi in ((p, half), (half, P))], nudge).astype(np.float64)])
    s = np.zeros(nb)
    for b in range(nb):
        s[b] = 1.4826 * max(float(np.max(med[max(0, b - 1):b + 2] if nb > 1 else med)), 0.25 * g, 2.0 ** -24 * A)
    for b in range(nb):
        ratio[edges[b]:edges[b + 1]] = d[edges[b]:edges[b + 1]].astype(np.float64) / s[b]
    hits = np.nonzero(ratio > THRESHOLD)[0]
    events = []  # [start, last, peak]
    for n in hits:
        n = int(n)
        if events and n - events[-1][1] <= GAP:
            events[-1][1] = n
            if ratio[n] > ratio[events[-1][2]]:
                events[-1][2] = n
        else:
            events.append([n, n, n])
    with np.errstate(divide="ignore"):
        strengths = [np.float32(20.0 * np.log10(ratio[pk])) for _, _, pk in events]
        order = sorted(range(len(events)), key=lambda i: (-float(strengths[i]), events[i][0]))
        rec["valid"] = 1
        rec["events"] = len(events)
        rec["hit_frames"] = len(hits)
        rec["listed"] = min(len(events), MAX_EVENTS)
        rec["rate"] = np.float32(float(len(events)) * float(sr) / float(judged))
        rec["peak_db"] = np.float32(20.0 * np.log10(np.max(ratio[p:])))
        rec["floor_db"] = np.float32(20.0 * np.log10(1.4826 * g))
        rec["prediction_gain_db"] = np.float32(10.0 * np.log10(r[0] / E))
    for slot, i in enumerate(order[:MAX_EVENTS]):
        st, last, pk = events[i]
        ev = rec["ev"][slot]
        ev["start"], ev["length"], ev["peak"] = st, last - st + 1, pk
        ev["frame"] = (wpos - P + st) & 0xFFFFFFFF
        ev["strength_db"] = strengths[i]
        ev["amplitude"] = np.float32(e[pk])
    return rec, ratio, dict(hits=hits, events=events, strengths=[float(v) for v in strengths], r=r, a=a, E=E, e=e, med=med, g=g, s=s)


def click(windows, sr=48000, wpos=None):
    """[streams] of wf_hip_click from windows, float32 [streams, channels, P] (the newest P frames of every captured channel), and
    the counters wpos [streams] at the read"""
    windows = np.asarray(windows, np.float32)
    streams, channels, P = windows.shape
    out = np.zeros(streams, CLICK_DTYPE)
    for s in range(streams):
        for c in range(channels):
            out["ch"][s, c] = analyse(windows[s, c], sr, None if wpos is None else wpos[s])[0]
    out["window"] = P
    out["order"] = ORDER
    return out


def margins(x, sr=48000):
    """the conditions the bound rests on, for one channel's window: (the least |ratio / threshold - 1| over the judged frames, the
    least difference in dB between two listed strengths, whether the hits stay the same with every m_b and g one float32 ulp up and
    one down)"""
    rec, ratio, det = analyse(x, sr)
    if not rec["valid"]:
        return np.inf, np.inf, True
    near = float(np.min(np.abs(ratio[ORDER:] / THRESHOLD - 1.0)))
    listed = np.sort(rec["ev"]["strength_db"][:int(rec["listed"])].astype(np.float64))
    apart = float(np.min(np.diff(listed))) if len(listed) > 1 else np.inf
    same = all(np.array_equal(analyse(x, sr, nudge=u)[2]["hits"], det["hits"]) for u in (-1, 1))
    return near, apart, same


def margins_hold(m):
    return m[0] >= RATIO_MARGIN and m[1] >= STRENGTH_MARGIN_DB and m[2]


def _ulp(f):
    f = np.asarray(f, np.float32)
    with np.errstate(invalid="ignore"):
        u = np.spacing(np.abs(f)).astype(np.float64)
    return np.where(np.isfinite(u), u, 0.0)


def _float_parts(got, want):
    for name in CHANNEL_FLOAT_FIELDS:
        yield "ch." + name, got["ch"][name], want["ch"][name]
    for name in EVENT_FLOAT_FIELDS:
        yield "ch.ev." + name, got["ch"]["ev"][name], want["ch"]["ev"][name]


def worst(got, want):
    """the largest |got - want| of every float field in ulps of the wanted value, for printing"""
    out = {}
    for name, g, f in _float_parts(got, want):
        with np.errstate(invalid="ignore", divide="ignore"):
            dlt = np.where(g == f, 0.0, np.abs(g.astype(np.float64) - f.astype(np.float64)) / np.maximum(_ulp(f), 1e-300))
        out[name] = float(np.max(dlt, initial=0.0))
    return out


def mismatches(got, want):
    """(field, index, got, want) of everything in `got` ([streams] of wf_hip_click) beyond the bound of `want`"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return [("shape", (), (got.shape, got.dtype), (want.shape, want.dtype))]
    bad = []

    def differ(name, g, f, where):
        bad.extend((name, tuple(i), g[tuple(i)].item(), f[tuple(i)].item()) for i in np.argwhere(where)[:5])

    for name in ("window", "order", "reserved"):
        differ(name, got[name], want[name], got[name] != want[name])
    for name in CHANNEL_INT_FIELDS:
        differ("ch." + name, got["ch"][name], want["ch"][name], got["ch"][name] != want["ch"][name])
    for name in EVENT_INT_FIELDS:
        g, f = got["ch"]["ev"][name], want["ch"]["ev"][name]
        differ("ch.ev." + name, g, f, g != f)
    for name, g, f in _float_parts(got, want):
        with np.errstate(invalid="ignore"):
            ok = (g == f) | (np.abs(g.astype(np.float64) - f.astype(np.float64)) <= _ulp(f))
        differ(name, g, f, ~ok)
    return bad


# ---- the signals ------------------------------------------------------------------------------------------------------------------

SEED = 20261020
KINDS = ("noise", "noise clicks", "sine", "sine click", "lone", "half", "crackle", "skip", "repeat", "silence", "nan")
INVALID = ("silence", "nan")
SKIP, REPEAT = 37, 64
CRACKLE_SPACING = 60


def pink(rng, n, amplitude=0.05):
    """white noise through a third-order 1/f filter, its first 200 frames dropped"""
    b = (0.049922035, -0.095993537, 0.050612699, -0.004408786)
    a = (-2.494956002, 2.017265875, -0.522189400)
    w = rng.standard_normal(n + 200)
    y = np.zeros(n + 200)
    for i in range(n + 200):
        v = b[0] * w[i]
        if i >= 1:
            v += b[1] * w[i - 1] - a[0] * y[i - 1]
        if i >= 2:
            v += b[2] * w[i - 2] - a[1] * y[i - 2]
        if i >= 3:
            v += b[3] * w[i - 3] - a[2] * y[i - 3]
        y[i] = v
    return amplitude * y[200:]


def note(n, sr=48000):
    """a sum of six decaying harmonics of 220 Hz over a little noise (what keeps the predictor from being exact)"""
    t = np.arange(n) / sr
    y = np.zeros(n)
    for h in range(1, 7):
        y += (0.3 / h) * np.sin(2.0 * np.pi * 220.0 * h * t + 0.4 * h) * np.exp(-t * (3.0 + 2.0 * h))
    return y


def crackle_positions(P):
    """up to twelve click positions at least CRACKLE_SPACING frames apart, the same for every seed of the noise under them"""
    rng = np.random.default_rng(SEED + P)
    grid = np.arange(100, P - 90, CRACKLE_SPACING)
    return np.sort(rng.choice(grid, min(12, len(grid) // 2), replace=False))


def splice_at(P):
    return P // 2 + 11


def signal(kind, P, seed=0, sr=48000):
    """float32 [P]: one window of the kind (include/wf_hip.h's table of readings, and the splices)"""
    rng = np.random.default_rng(SEED + 1000 * KINDS.index(kind) + P + 100000 * seed)
    if kind == "noise":
        y = pink(rng, P)
    elif kind == "noise clicks":
        y = pink(rng, P)
        y[P // 2] += 0.3
        y[P // 4] -= 0.2
    elif kind in ("sine", "sine click"):
        y = 0.5 * np.sin(2.0 * np.pi * 1000.0 * np.arange(P) / sr)
        if kind == "sine click":
            y[P // 3] += 0.01
    elif kind == "lone":
        y = np.zeros(P)
        y[P // 2] = 0.25
    elif kind == "half":
        y = np.concatenate([np.zeros(P // 2), pink(rng, P - P // 2)])
    elif kind == "crackle":
        y = pink(rng, P)
        pos = crackle_positions(P)
        y[pos] += 0.3 * rng.choice([-1.0, 1.0], len(pos))
    elif kind == "skip":
        y = note(P + SKIP, sr) + pink(rng, P + SKIP, 1e-4)
        c = splice_at(P)
        y = np.concatenate([y[:c], y[c + SKIP:]])
    elif kind == "repeat":
        y = note(P, sr) + pink(rng, P, 1e-4)
        c = splice_at(P)
        y = np.concatenate([y[:c], y[c - REPEAT:c], y[c:]])[:P]
    elif kind == "silence":
        y = np.zeros(P)
    elif kind == "nan":
        y = pink(rng, P)
        y[P // 5] = np.nan
    else:
        raise ValueError(kind)
    assert y.shape == (P,)
    return y.astype(np.float32)


# ---- the device test's cases ------------------------------------------------------------------------------------------------------

STREAMS = 7
# (fft_size, capture channels, further configuration, wf_hip_fft_size())
GPU_CASES = [(fft, ch, {}, fft) for fft in (256, 800, 4096, 16384) for ch in (1, 2)] + [
    # a meter batch: W = 48000 * 0.046 = 2208, no multiple of 64, and counters that start at 0
    (1024, 2, dict(meter=1, bars=0, meter_ms=46), 2208),
]
# what the final window of every stream holds, channel 0 and channel 1 (stream 2's is what follows a reset: zeros, then its tail)
GPU_KINDS = (("noise clicks", "sine"), ("sine click", "repeat"), ("half", "noise clicks"), ("lone", "silence"), ("crackle", "lone"),
             ("skip", "noise"), ("nan", "crackle"))
RESET_STREAM = 2
OVERLONG_STREAM = 3
# where a window of some case left a condition of the bound unmet, the next seed was taken: (kind, P) -> seed
SEED_STEPS = {}


def case_id(case):
    fft, ch, kw, w = case
    return f"w{w}_ch{ch}" + ("_meter" if kw.get("meter") else "")


def ring_frames(w):
    """the ring capacity wf_hip_create gives a handle of window w by default: the next power of two of max(2 w, 4096)"""
    return 1 << (max(2 * w, 4096) - 1).bit_length()


def gpu_windows(case):
    """float32 [STREAMS, channels, P]: the designed final window of every stream"""
    fft, ch, kw, w = case
    P = window_frames(w)
    return np.stack([np.stack([signal(k, P, SEED_STEPS.get((k, P), 0)) for k in GPU_KINDS[s][:ch]]) for s in range(STREAMS)])


def gpu_totals(case):
    """frames every stream is pushed, and where that leaves its window:
      0  a whole ring and P + 5 frames: the window lies flat at positions 5 .. P + 4
      1  the counter ends P / 2 + 1 frames past a whole ring: the window wraps round the ring
      2  100 frames, wf_hip_reset, then the newest P - P / 2 frames of its window: zeros, then a partial refill
      3  one packet of ring + 77 frames
      4, 5, 6  P + 1, P + 2 and 2 P + 3 frames: with stream 0 all four classes of start & 3"""
    fft, ch, kw, w = case
    P, ring = window_frames(w), ring_frames(w)
    w0 = 0 if kw.get("meter") else w
    return [ring - w0 + P + 5, 2 * ring - w0 + P // 2 + 1, P - P // 2, ring + 77, P + 1, P + 2, 2 * P + 3]


def gpu_script(case):
    """the steps in the form tests/measure_stagger.py's replay() takes: ("push", first, x [1, channels, n]) | ("reset", first, 1).
    Every stream's audio is white noise of amplitude 0.05 with its window at the end, in packets of at most half a ring and one
    frame -- but stream 3's, which is one packet"""
    fft, ch, kw, w = case
    P, ring = window_frames(w), ring_frames(w)
    win = gpu_windows(case)
    rng = np.random.default_rng(SEED + w + ch)
    steps = []
    for s, total in enumerate(gpu_totals(case)):
        if s == RESET_STREAM:
            steps.append(("push", s, rng.uniform(-0.05, 0.05, (1, ch, 100)).astype(np.float32)))
            steps.append(("reset", s, 1))
            steps.append(("push", s, np.ascontiguousarray(win[s:s + 1, :, P - total:])))
            continue
        x = np.concatenate([rng.uniform(-0.05, 0.05, (1, ch, total - P)).astype(np.float32), win[s:s + 1]], axis=2)
        step = total if s == OVERLONG_STREAM else ring // 2 + 1
        for lo in range(0, total, step):
            steps.append(("push", s, np.ascontiguousarray(x[:, :, lo:lo + step])))
    return steps


def gpu_final_windows(case):
    """float32 [STREAMS, channels, P] and the counters [STREAMS] after gpu_script, by tests/measure_stagger.py's ring model"""
    import measure_stagger as ms
    fft, ch, kw, w = case
    rings = ms.Rings(STREAMS, ch, ring_frames(w), 0 if kw.get("meter") else w)
    ms.replay(gpu_script(case), rings)
    return rings.window(window_frames(w)), rings.counter.astype(np.int64)
