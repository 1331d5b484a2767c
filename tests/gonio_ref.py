"""Float64 restatement of WF_HIP_OUT_GONIO (include/wf_hip.h, "vectorscope"): how many of the newest frames of captured channels
0 and 1 fall into each cell of a 64 x 64 side / mid picture that a power of two magnifies to the peak.  Nothing here knows how the
device stages, reduces or counts.  Every step is a comparison, an integer count, an exact float64 operation or one correctly
rounded IEEE operation (np.frexp / np.ldexp for the range), so the device is held to it bit for bit (mismatches).  Also the
signals the tests push and the cases the CPU and the device tests share."""
import numpy as np

GRID = 64  # WF_HIP_GONIO_GRID
MAX_WINDOW = 8192  # WF_HIP_GONIO_MAX_WINDOW
MIN_EXP = -24  # WF_HIP_GONIO_MIN_EXP
GONIO_DTYPE = np.dtype([("cell", np.uint16, (GRID, GRID)), ("window", np.uint32), ("zoom", np.int32), ("peak", np.float32),
                        ("mid_peak", np.float32), ("side_peak", np.float32), ("in_phase", np.uint32), ("out_phase", np.uint32),
                        ("occupied", np.uint32)])
FIELDS = ("cell", "window", "zoom", "peak", "mid_peak", "side_peak", "in_phase", "out_phase", "occupied")


def window_frames(w):
    """P of a handle whose wf_hip_fft_size() is w"""
    return min(int(w), MAX_WINDOW)


def exponent(peak):
    """e of a float32 peak A >= 0: 0 for A == 0, else A = f 2^e with 0.5 <= f < 1, raised to at least MIN_EXP"""
    if peak == 0:
        return 0
    return max(int(np.frexp(np.float64(peak))[1]), MIN_EXP)


def coordinates(x, e):
    """x: float32 [2, P].  (u, v) float64 [P]: side and mid, scaled by 2^-e"""
    l, r = np.asarray(x, np.float32).astype(np.float64)
    return np.ldexp((r - l) * 0.5, -e), np.ldexp((l + r) * 0.5, -e)


def index(u):
    """the cell index of a coordinate: min / max in floating point, then the conversion"""
    return np.minimum(np.maximum(np.floor((u + 1.0) * (GRID / 2)), 0.0), GRID - 1.0).astype(np.int64)


def gonio_one(x, w):
    """x: float32 [2, >= P], the newest frame last.  One wf_hip_gonio as a 0-d record"""
    p = window_frames(w)
    x = np.asarray(x, np.float32)[:, x.shape[-1] - p:]
    assert x.shape == (2, p)
    out = np.zeros((), GONIO_DTYPE)
    peak = np.abs(x).max()
    e = exponent(peak)
    u, v = coordinates(x, e)
    cell = np.zeros((GRID, GRID), np.int64)
    np.add.at(cell, (index(v), index(u)), 1)
    l, r = x.astype(np.float64)
    out["cell"] = cell
    out["window"], out["zoom"], out["peak"] = p, -e, peak
    out["mid_peak"] = np.float32(np.abs((l + r) * 0.5).max())
    out["side_peak"] = np.float32(np.abs((r - l) * 0.5).max())
    out["in_phase"] = np.count_nonzero(((l > 0) & (r > 0)) | ((l < 0) & (r < 0)))
    out["out_phase"] = np.count_nonzero(((l > 0) & (r < 0)) | ((l < 0) & (r > 0)))
    out["occupied"] = np.count_nonzero(cell)
    return out


def gonio(frames, w):
    """frames: float32 [streams, 2, >= P]: the newest frames of both rings, the newest last"""
    return np.array([gonio_one(x, w) for x in frames], GONIO_DTYPE)


def mismatches(got, frames, w=None):
    """(field, index, got, want) of everything in `got` ([streams] of wf_hip_gonio) that differs from the restatement of `frames`
    [streams, 2, >= P] (w: the handle's fft size; None: all of the frames).  Every field is compared for equality: the integers
    as integers, the three float32 peaks by their bits."""
    want = gonio(frames, frames.shape[-1] if w is None else w)
    if got.shape != want.shape or got.dtype != want.dtype:
        return [("shape", (), (got.shape, got.dtype), (want.shape, want.dtype))]
    bad = []
    for name in FIELDS:
        g, f = got[name], want[name]
        if g.dtype == np.float32:
            g, f = g.view(np.uint32), f.view(np.uint32)
        bad += [(name, tuple(i), got[name][tuple(i)].item(), want[name][tuple(i)].item()) for i in np.argwhere(g != f)[:5]]
    return bad


# ---- the signals ------------------------------------------------------------------------------------------------------------------

KINDS = ("noise", "correlated", "lissajous", "quiet", "loud", "mono", "antiphase", "left", "silence", "half")
PICTURE_KINDS = ("noise", "correlated", "lissajous", "quiet", "loud")  # a spread picture: test_gonio_cpu.py checks how spread


def signal(kind, rng, frames):
    """float32 [2, frames] of one kind of audio"""
    n = np.arange(frames)
    a, b = rng.standard_normal(frames) * 0.2, rng.standard_normal(frames) * 0.2
    if kind == "noise":                      # independent noise
        x = np.stack([a, b])
    elif kind == "correlated":               # correlation 0.8
        x = np.stack([a, 0.8 * a + 0.6 * b])
    elif kind == "lissajous":                # two tones whose ratio is no small fraction: the figure fills its rectangle
        f = rng.uniform(0.011, 0.017)
        x = np.stack([0.6 * np.sin(2 * np.pi * f * n + 0.3), 0.45 * np.sin(2 * np.pi * f * 1.618 * n + 1.1)])
    elif kind == "quiet":                    # noise at -78 dB: zoom 13 or so
        x = np.stack([a, b]) * 2.0 ** -13
    elif kind == "loud":                     # noise above full scale: a negative zoom
        x = np.stack([a, b]) * 9.0
    elif kind == "mono":                     # l = r: column GRID / 2
        x = np.stack([a, a])
    elif kind == "antiphase":                # l = -r: row GRID / 2
        x = np.stack([a, -a])
    elif kind == "left":                     # r = 0: the diagonal that points up-left
        x = np.stack([a, np.zeros(frames)])
    elif kind == "silence":
        x = np.zeros((2, frames))
    elif kind == "half":                     # peaks at exactly 0.5, every frame: zoom 0
        x = np.clip(np.stack([a, b]), -0.5, 0.5)
        x[0, 3::97] = 0.5
        x[1, 5::89] = -0.5
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


# what tests/test_gpu_gonio.py compares against the restatement: (fft_size asked for, sample rate, configuration overrides, the
# W = wf_hip_fft_size() that results, the kinds of its three streams); test_gonio_cpu.py checks the conditions on them
GPU_SEED = 20261018
GPU_CASES = [
    (128, 48000, {}, 128, ("noise", "mono", "silence")),              # P smaller than the workgroup
    (1024, 48000, {}, 1024, ("correlated", "quiet", "left")),
    (2000, 48000, {}, 2000, ("lissajous", "antiphase", "loud")),      # not a multiple of 64 or 256
    (4096, 48000, {}, 4096, ("noise", "half", "mono")),
    (16384, 48000, {}, 16384, ("loud", "left", "lissajous")),         # the cap: P = 8192 of a longer window
    # a meter batch: W = 48000 * 0.046 = 2208 = 16 * 138, no multiple of 64
    (1024, 48000, dict(meter=1, bars=0, meter_ms=46), 2208, ("quiet", "noise", "antiphase")),
]
CLAMP_SCALE = 2.0 ** -30  # tests that want the clamp of e active scale a signal by it: the peak lies below 2^-24


def ring_frames(w):
    """the ring capacity wf_hip_create gives a handle of window w by default: the next power of two of max(2 w, 4096)"""
    return 1 << (max(2 * w, 4096) - 1).bit_length()


def case_id(case):
    fft, sr, kw, w, kinds = case
    return f"w{w}" + ("_meter" if kw.get("meter") else "")


def case_audio(case):
    """the frames test_gpu_gonio.py pushes for a case, float32 [3, 2, frames]: one ring and P / 2 + 3 frames, so that the window
    wraps the ring and ends at an odd position"""
    fft, sr, kw, w, kinds = case
    rng = np.random.default_rng(GPU_SEED + w)
    frames = ring_frames(w) + window_frames(w) // 2 + 3
    return np.stack([signal(k, rng, frames) for k in kinds])
