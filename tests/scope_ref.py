"""Float64 restatement of WF_HIP_OUT_SCOPE (include/wf_hip.h, "oscilloscope"): the triggered min/max trace of the newest frames in
each captured channel's ring.  The trigger walk is the sequential state machine of the definition, one frame after the other;
nothing here knows how the device stages, scans or reduces.  Every step is a comparison, an exact float64 operation or one
correctly rounded IEEE operation, so the device is held to it bit for bit (mismatches).  Also the signals the tests push and the
cases the CPU and the device tests share."""
import numpy as np

MAX_WINDOW = 8192  # WF_HIP_SCOPE_MAX_WINDOW
COLUMNS = 256  # WF_HIP_SCOPE_COLUMNS
SCOPE_DTYPE = np.dtype([("lo", np.float32, (2, COLUMNS)), ("hi", np.float32, (2, COLUMNS)), ("window", np.uint32), ("view", np.uint32),
                        ("columns", np.uint32), ("start", np.uint32), ("triggered", np.uint32), ("period", np.uint32),
                        ("frac", np.float32), ("reserved", np.uint32)])
INT_FIELDS = ("window", "view", "columns", "start", "triggered", "period", "reserved")


def geometry(w):
    """(P, V, K) of a handle whose wf_hip_fft_size() is w"""
    p = min(int(w), MAX_WINDOW)
    v = p // 2
    return p, v, min(COLUMNS, v)


def column_edges(v, k):
    """[k + 1] ints: column c covers view frames edges[c] .. edges[c + 1] - 1"""
    return [c * v // k for c in range(k + 1)]


def trigger_signal(x):
    """x: float32 [channels, P].  (u [P] float64, hyst): the trigger signal less its level, and the hysteresis; hyst 0: flat"""
    x = np.asarray(x, np.float32).astype(np.float64)
    t = x[0] + x[1] if x.shape[0] == 2 else x[0]  # exact
    tmax, tmin = t.max(), t.min()
    level = (tmax + tmin) * 0.5
    hyst = (tmax - tmin) * 0.125
    return t - level, hyst


def triggers(u, hyst, end):
    """the triggers among frames 0 .. end - 1, walked one frame after the other"""
    out, armed = [], False
    if not hyst > 0.0:
        return out
    for i in range(end):
        if u[i] <= -hyst:
            armed = True
        elif u[i] >= 0.0 and armed:
            out.append(i)
            armed = False
    return out


def scope_one(x, w):
    """x: float32 [channels, >= P], the newest frame last.  One wf_hip_scope as a 0-d record"""
    p, v, k = geometry(w)
    x = np.asarray(x, np.float32)[:, x.shape[-1] - p:]
    out = np.zeros((), SCOPE_DTYPE)
    out["window"], out["view"], out["columns"] = p, v, k
    u, hyst = trigger_signal(x)
    trig = triggers(u, hyst, p - v + 1)  # start <= P - V
    start = p - v
    if trig:
        start = trig[-1]
        out["triggered"] = 1
        out["period"] = start - trig[-2] if len(trig) > 1 else 0
        out["frac"] = np.float32(u[start - 1] / (u[start - 1] - u[start]))
    out["start"] = start
    edges = column_edges(v, k)
    for ch in range(x.shape[0]):
        view = x[ch, start:start + v]
        out["lo"][ch, :k] = np.minimum.reduceat(view, edges[:-1])
        out["hi"][ch, :k] = np.maximum.reduceat(view, edges[:-1])
    return out


def scope(frames, w):
    """frames: float32 [streams, channels, >= P]: the newest frames of every captured channel's ring, the newest last"""
    return np.array([scope_one(x, w) for x in frames], SCOPE_DTYPE)


def mismatches(got, frames, w=None):
    """(field, index, got, want) of everything in `got` ([streams] of wf_hip_scope) that differs from the restatement of `frames`
    [streams, channels, >= P] (w: the handle's fft size; None: all of the frames).  The integer fields are compared exactly, lo and
    hi as values (-0 equals +0), frac exactly or within one float32 ulp (frac_outcome says which)."""
    want = scope(frames, frames.shape[-1] if w is None else w)
    bad = []
    if got.shape != want.shape:
        return [("shape", (), got.shape, want.shape)]
    for name in INT_FIELDS:
        bad += [(name, tuple(i), int(got[name][tuple(i)]), int(want[name][tuple(i)])) for i in np.argwhere(got[name] != want[name])[:5]]
    for name in ("lo", "hi"):
        bad += [(name, tuple(i), float(got[name][tuple(i)]), float(want[name][tuple(i)]))
                for i in np.argwhere(~(got[name] == want[name]))[:5]]
    g, f = got["frac"].astype(np.float64), want["frac"].astype(np.float64)
    ok = np.abs(g - f) <= np.spacing(want["frac"]).astype(np.float64)
    bad += [("frac", tuple(i), float(g[tuple(i)]), float(f[tuple(i)])) for i in np.argwhere(~ok)[:5]]
    return bad


def frac_outcome(got, frames, w=None):
    """'equal' when every frac is the restatement's float32, 'within one ulp' otherwise"""
    want = scope(frames, frames.shape[-1] if w is None else w)
    return "equal" if np.array_equal(got["frac"], want["frac"]) else "within one ulp"


def table_periodic(period, frames, phase=0):
    """float32 [frames]: a wave of integer period `period` read from one table, so every period holds the same float32 values.
    Its second harmonic is strong enough for a second, shallow pair of zero crossings per period: 0.5 sin(a) + 0.4 sin(2a + 3.1)
    rises through its mid level twice per period, once after a dip of less than an eighth of the swing."""
    a = 2.0 * np.pi * np.arange(period) / period
    table = (0.5 * np.sin(a) + 0.4 * np.sin(2.0 * a + 3.1) + 0.1).astype(np.float32)
    return table[(np.arange(frames) + phase) % period]


def rising_crossings(x):
    """upward crossings of the 50 % level of a float32 [frames] wave, without hysteresis"""
    u, _ = trigger_signal(x[None])
    return int(np.count_nonzero((u[:-1] < 0.0) & (u[1:] >= 0.0)))


def audio(rng, streams, frames, w):
    """float32 [streams, 2, frames]: per stream a fundamental whose period lies between 8 frames and (P - V) / 3 frames, so that
    at least two triggers lie at or below P - V, its second and third harmonic, a DC offset and white noise 30 dB under the
    fundamental; the channels differ in gain and in their noise"""
    p, v, _ = geometry(w)
    n = np.arange(frames)
    x = np.empty((streams, 2, frames))
    for s in range(streams):
        period = rng.uniform(8.0, (p - v) / 3.0)
        amp = rng.uniform(0.2, 0.4)
        ph = rng.uniform(0.0, 2.0 * np.pi, 3)
        wave = amp * (np.sin(2.0 * np.pi * n / period + ph[0]) + 0.3 * np.sin(4.0 * np.pi * n / period + ph[1])
                      + 0.2 * np.sin(6.0 * np.pi * n / period + ph[2]))
        dc = rng.uniform(-0.2, 0.2)
        for c in range(2):
            noise = rng.standard_normal(frames) * amp / np.sqrt(2.0) * 10.0 ** (-30.0 / 20.0)
            x[s, c] = rng.uniform(0.7, 1.0) * wave + dc + noise
    return x.astype(np.float32)


# what tests/test_gpu_scope.py compares against the restatement: (fft_size asked for, sample rate, captured channels, configuration
# overrides, the W = wf_hip_fft_size() that results); test_scope_cpu.py checks the condition of audio() on them
GPU_SEED = 20261017
GPU_CASES = [
    (128, 48000, 2, {}, 128),      # V = 64, K = 64: fewer columns than the struct holds
    (1024, 48000, 2, {}, 1024),
    (2000, 48000, 2, {}, 2000),    # V = 1000: column boundaries that are not whole frames apart
    (4096, 48000, 2, {}, 4096),
    (16384, 48000, 2, {}, 16384),  # the cap: P = 8192 of a longer window
    # a meter batch: W = 44100 * 0.05 & -16 = 2192 = 16 * 137 (the library, like the reference, rounds a meter buffer down to a
    # multiple of 16, so no W is less aligned than this), V = 1096
    (1024, 44100, 2, dict(meter=1, bars=0, meter_ms=50), 2192),
    (1024, 48000, 1, {}, 1024),    # one captured channel
]


def ring_frames(w):
    """the ring capacity wf_hip_create gives a handle of window w by default: the next power of two of max(2 w, 4096)"""
    return 1 << (max(2 * w, 4096) - 1).bit_length()


def case_id(case):
    fft, sr, ch, kw, w = case
    return f"w{w}_ch{ch}" + ("_meter" if kw.get("meter") else "")


def case_audio(case, streams=3):
    """the frames test_gpu_scope.py pushes for a case, float32 [streams, channels, frames]: one ring and P / 2 + 3 frames of
    audio(), so that the window wraps the ring and ends at an odd position"""
    fft, sr, ch, _, w = case
    return audio(np.random.default_rng(GPU_SEED + w + ch), streams, ring_frames(w) + geometry(w)[0] // 2 + 3, w)[:, :ch]
