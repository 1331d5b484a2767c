"""Numpy restatement of WF_HIP_OUT_BITS (include/wf_hip.h, "bit statistics"): per captured channel the histogram of sample values,
how often each bit of the sample on a 32-bit two's-complement grid is set, the level histogram in bits, the word length, the
over-range and below-the-grid counts and the longest run of identical samples of the newest frames.  Nothing here knows how the
device stages, ballots or counts.  Every step is a comparison, an exact float64 operation (a float32 times 2^31, floor) or an
integer operation, so the device is held to it bit for bit (mismatches).  Also the signals the tests push and the cases the CPU
and the device tests share."""
import numpy as np

MAX_WINDOW = 8192  # WF_HIP_BITS_MAX_WINDOW
BITS_CHANNEL_DTYPE = np.dtype([("hist", np.uint16, (256,)), ("ones", np.uint16, (32,)), ("mag", np.uint16, (32,)),
                               ("word_length", np.uint32), ("magnitude_bits", np.uint32), ("over", np.uint32), ("fine", np.uint32),
                               ("repeats", np.uint32), ("max_run", np.uint32), ("max_run_start", np.uint32),
                               ("max_run_value", np.float32)])
BITS_DTYPE = np.dtype([("ch", BITS_CHANNEL_DTYPE, (2,)), ("window", np.uint32), ("reserved", np.uint32, (3,))])
CHANNEL_FIELDS = BITS_CHANNEL_DTYPE.names
FIELDS = ("ch", "window", "reserved")


def window_frames(w):
    """P of a handle whose wf_hip_fft_size() is w"""
    return min(int(w), MAX_WINDOW)


def code(x):
    """x: float32 [P].  (v int64 [P] in the int32 range, over bool [P], fine bool [P])"""
    x = np.asarray(x, np.float32)
    y = x.astype(np.float64) * 2.0 ** 31  # exact: a power of two, and float64 holds every float32 times it
    over = (y >= 2.0 ** 31) | (y < -(2.0 ** 31))
    fl = np.floor(y)
    v = np.minimum(np.maximum(fl, -(2.0 ** 31)), 2.0 ** 31 - 1).astype(np.int64)
    fine = ~over & (fl != y)
    return v, over, fine


def significant_bits(v):
    """m(v): the number of significant bits of s(v) = v for v >= 0 and ~v for v < 0; 0..31"""
    s = np.where(v >= 0, v, ~v).astype(np.int64)
    m = np.zeros(s.shape, np.int64)
    for b in range(31):
        m[s >= (1 << b)] = b + 1
    return m


def bits_channel(x):
    """x: float32 [P], the whole window.  One wf_hip_bits_channel as a 0-d record"""
    x = np.ascontiguousarray(x, np.float32)
    p = x.shape[0]
    out = np.zeros((), BITS_CHANNEL_DTYPE)
    v, over, fine = code(x)
    out["hist"] = np.bincount((v >> 24) + 128, minlength=256)
    u = v & 0xffffffff  # the two's-complement pattern
    out["ones"] = [np.count_nonzero((u >> b) & 1) for b in range(32)]
    m = significant_bits(v)
    out["mag"] = np.bincount(m, minlength=32)
    orv = int(np.bitwise_or.reduce(u))
    out["word_length"] = 0 if orv == 0 else 32 - ((orv & -orv).bit_length() - 1)
    out["magnitude_bits"] = m.max()
    out["over"], out["fine"] = np.count_nonzero(over), np.count_nonzero(fine)
    pat = x.view(np.uint32)
    same = pat[1:] == pat[:-1]
    out["repeats"] = np.count_nonzero(same)
    heads = np.flatnonzero(np.concatenate([[True], ~same]))
    lengths = np.diff(np.concatenate([heads, [p]]))
    k = int(np.argmax(lengths))  # the first of the longest
    out["max_run"], out["max_run_start"], out["max_run_value"] = lengths[k], heads[k], x[heads[k]]
    return out


def bits_one(x, w):
    """x: float32 [channels (1 or 2), >= P], the newest frame last.  One wf_hip_bits as a 0-d record"""
    p = window_frames(w)
    x = np.asarray(x, np.float32)
    x = x[:, x.shape[-1] - p:]
    assert x.shape[0] in (1, 2) and x.shape[1] == p
    out = np.zeros((), BITS_DTYPE)
    for c in range(x.shape[0]):
        out["ch"][c] = bits_channel(x[c])
    out["window"] = p
    return out


def bits(frames, w):
    """frames: float32 [streams, channels, >= P]: the newest frames of the rings, the newest last"""
    return np.array([bits_one(x, w) for x in frames], BITS_DTYPE)


def mismatches(got, frames, w=None):
    """(field, index, got, want) of everything in `got` ([streams] of wf_hip_bits) that differs from the restatement of `frames`
    [streams, channels, >= P] (w: the handle's fft size; None: all of the frames).  Every field is compared for equality: the
    integers as integers, max_run_value by its bits."""
    want = bits(frames, frames.shape[-1] if w is None else w)
    if got.shape != want.shape or got.dtype != want.dtype:
        return [("shape", (), (got.shape, got.dtype), (want.shape, want.dtype))]
    bad = []
    for name in CHANNEL_FIELDS:
        g, f = got["ch"][name], want["ch"][name]
        if g.dtype == np.float32:
            g, f = g.view(np.uint32), f.view(np.uint32)
        bad += [("ch." + name, tuple(i), got["ch"][name][tuple(i)].item(), want["ch"][name][tuple(i)].item()) for i in np.argwhere(g != f)[:5]]
    for name in ("window", "reserved"):
        bad += [(name, tuple(i), got[name][tuple(i)].item(), want[name][tuple(i)].item()) for i in np.argwhere(got[name] != want[name])[:5]]
    return bad


# ---- the signals ------------------------------------------------------------------------------------------------------------------

KINDS = ("s16", "u8", "s24", "float", "clipped", "silence", "constant", "gap", "stuck", "two_runs", "run_first", "run_last")
NOISE_KINDS = ("s24", "float")  # plain noise at 0.25 rms: test_bits_cpu.py checks how spread their histograms are
RUN_KINDS = ("constant", "gap", "two_runs", "run_first", "run_last")
GAP = 300      # frames of the zero gap of "gap"
RUN = 40       # frames of the runs of "two_runs", "run_first" and "run_last"


def _quantise(x, bits_):
    """float64 in [-1, 1) onto a grid of `bits_` bits, as float32 (exact: at most 24 significant bits)"""
    q = 2.0 ** (bits_ - 1)
    return (np.clip(np.round(x * q), -q, q - 1) / q).astype(np.float32)


def _place_end(frames, p):
    """where the window of the newest p frames starts in a signal of `frames` frames"""
    return frames - p


def signal(kind, rng, frames, p=None):
    """float32 [frames] of one kind of audio; p: the window the device will read (the newest p frames), which the kinds with a
    placed run need (None: all of it)"""
    p = frames if p is None else p
    w0 = _place_end(frames, p)
    n = np.arange(frames)
    noise = rng.standard_normal(frames)
    if kind == "s16":                         # a sine plus noise on a 16-bit grid
        x = _quantise(0.5 * np.sin(2 * np.pi * n / 57.3) + 0.05 * noise, 16)
    elif kind == "u8":                        # 8-bit audio: (u - 128) / 128
        x = _quantise(0.6 * np.sin(2 * np.pi * n / 41.7) + 0.02 * noise, 8)
    elif kind == "s24":
        x = _quantise(0.25 * noise, 24)
    elif kind == "float":                     # float noise at 0.25 rms: bits below the grid wherever |x| < 2^-8
        x = (0.25 * noise).astype(np.float32)
    elif kind == "clipped":                   # a sine of amplitude 2 clipped to +-1: over-range frames and flat tops
        x = np.clip(2.0 * np.sin(2 * np.pi * n / 200.0), -1.0, 1.0).astype(np.float32)
    elif kind == "silence":
        x = np.zeros(frames, np.float32)
    elif kind == "constant":                  # one run equal to the window
        x = np.full(frames, 0.3125, np.float32)
    elif kind == "gap":                       # noise with a drop-out across a multiple of 256 (a workgroup step), where p allows
        x = (0.25 * noise).astype(np.float32)
        g = min(GAP, p // 2)
        at = w0 + (256 - g // 3 if p >= 512 else p // 4)
        x[at:at + g] = 0.0
    elif kind == "stuck":                     # s16 with bit 16 of v (the grid's least significant bit) forced to 1
        q = np.clip(np.round((0.4 * np.sin(2 * np.pi * n / 63.1) + 0.05 * noise) * 32768.0), -32768, 32767).astype(np.int64) | 1
        x = (q / 32768.0).astype(np.float32)
    elif kind == "two_runs":                  # two runs of equal length: the first must win
        x = (0.25 * noise).astype(np.float32)
        r = min(RUN, p // 8)
        a, b = w0 + p // 3, w0 + (2 * p) // 3
        x[a:a + r] = 0.125
        x[b:b + r] = -0.375
    elif kind == "run_first":                 # a run that starts at frame 0 of the window (and before it: older frames do not count)
        x = (0.25 * noise).astype(np.float32)
        r = min(RUN, p // 8)
        x[max(w0 - 5, 0):w0 + r] = 0.0625
    elif kind == "run_last":                  # a run that ends with the window
        x = (0.25 * noise).astype(np.float32)
        r = min(RUN, p // 8)
        x[frames - r:] = -0.5
    else:
        raise ValueError(kind)
    return x


# what tests/test_gpu_bits.py compares against the restatement: (fft_size asked for, sample rate, configuration overrides, the
# W = wf_hip_fft_size() that results, the kinds of its three streams -- channel 0 the kind, channel 1 the next kind of KINDS);
# test_bits_cpu.py checks the conditions on them
GPU_SEED = 20261019
GPU_CASES = [
    (128, 48000, {}, 128, ("s16", "silence", "run_first")),           # P smaller than the workgroup: two chunks
    (1024, 48000, {}, 1024, ("u8", "gap", "two_runs")),               # one workgroup step
    (2000, 48000, {}, 2000, ("s24", "clipped", "run_last")),          # not a multiple of 64 or 256
    (4096, 48000, {}, 4096, ("float", "constant", "stuck")),
    (16384, 48000, {}, 16384, ("gap", "constant", "clipped")),        # the cap: P = 8192 of a longer window
    # a meter batch: W = 48000 * 0.046 = 2208 = 16 * 138, no multiple of 64
    (1024, 48000, dict(meter=1, bars=0, meter_ms=46), 2208, ("stuck", "run_last", "float")),
]


def ring_frames(w):
    """the ring capacity wf_hip_create gives a handle of window w by default: the next power of two of max(2 w, 4096)"""
    return 1 << (max(2 * w, 4096) - 1).bit_length()


def case_id(case):
    fft, sr, kw, w, kinds = case
    return f"w{w}" + ("_meter" if kw.get("meter") else "")


def case_kinds(case):
    """[3][2]: the kinds of both channels of every stream"""
    return [(k, KINDS[(KINDS.index(k) + 1) % len(KINDS)]) for k in case[4]]


def case_audio(case):
    """the frames test_gpu_bits.py pushes for a case, float32 [3, 2, frames]: one ring and P / 2 + 3 frames, so that the window
    wraps the ring and ends at an odd position"""
    fft, sr, kw, w, kinds = case
    rng = np.random.default_rng(GPU_SEED + w)
    p = window_frames(w)
    frames = ring_frames(w) + p // 2 + 3
    return np.stack([np.stack([signal(k, rng, frames, p) for k in pair]) for pair in case_kinds(case)])
