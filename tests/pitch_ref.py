"""Float64 restatement of WF_HIP_OUT_PITCH (include/wf_hip.h, "pitch"): YIN steps 1 to 5 over the newest
P = min(fft_size, 4096) frames of every stream, from a zero-prefixed history of the frames pushed into it (signal_ref.History).

Every stream is evaluated twice, with two different orders of the float64 additions:
  order 0  numpy's pairwise sum over j for r(tau) and e(tau), a sequential running sum of d;
  order 1  64 partial sums over j = lane, lane + 64, ... added in lane order, and a running sum of d taken in blocks of 8.
In both, r(tau) and e(tau) are direct sums per lag in one and the same order of j, as the definition demands, so d(tau) is
exactly 0 where x[j + tau] == x[j] for all j.  A stream is *well conditioned* when both orders agree in lag and voiced and
differ by at most 1 float32 ulp in hz and clarity: reordering the additions moves each sum by about H 2^-53 = 2.3e-13 of its
magnitude, six orders under a float32 half-ulp, so a result moves by one rounding step at most unless a threshold decision
or the parabola's denominator sits within that distance of a tie -- which is what the second order exposes."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

MIN_LAG = 8
THRESHOLD = 0.15
MAX_WINDOW = 4096
PITCH_DTYPE = np.dtype([("hz", np.float32), ("clarity", np.float32), ("lag", np.uint32), ("voiced", np.uint32)])


def window_frames(fft_size):
    return min(int(fft_size), MAX_WINDOW)


def _sums(prod, order):
    """prod: float64 [lags, H], exact products; the sum over j of every row"""
    if order == 0:
        return prod.sum(axis=1)  # pairwise along the contiguous axis
    lags, H = prod.shape
    pad = (-H) % 64
    if pad:
        prod = np.concatenate([prod, np.zeros((lags, pad))], axis=1)  # (a zero adds nothing)
    part = prod.reshape(lags, -1, 64).sum(axis=1)  # lane l: j = l, l + 64, ... in that order
    tot = part[:, 0].copy()
    for l in range(1, 64):
        tot += part[:, l]
    return tot


def _running(d, order):
    """sum_{t=1..tau} d(t) for tau = 0 .. H (d[0] is 0)"""
    if order == 0:
        return np.cumsum(d)
    n = len(d) - 1
    pad = (-n) % 8
    body = np.concatenate([d[1:], np.zeros(pad)]).reshape(-1, 8)
    local = np.cumsum(body, axis=1)
    before = np.concatenate([[0.0], np.cumsum(local[:, -1])[:-1]])
    return np.concatenate([[0.0], (before[:, None] + local).reshape(-1)[:n]])


def pitch_one(x, sr, order=0):
    """x: float64 [P], the mixed signal of one stream.  Returns (hz, clarity, lag, voiced) with hz and clarity float32."""
    P = len(x)
    H = P // 2
    head = x[:H]
    V = sliding_window_view(x, H)[:H + 1]  # V[tau, j] = x[j + tau]
    r = _sums(V * head, order)
    e = _sums(V * V, order)
    d = np.maximum(e[0] + e - 2.0 * r, 0.0)
    d[0] = 0.0
    c = _running(d, order)
    if not c[H] > 0.0:
        return np.float32(0), np.float32(0), 0, 0
    tau = np.arange(H + 1, dtype=np.float64)
    dp = np.where(c > 0.0, d * tau / np.where(c > 0.0, c, 1.0), 1.0)
    dp[0] = 1.0
    rng = dp[MIN_LAG:H]  # lags MIN_LAG .. H - 1
    under = np.nonzero(rng < THRESHOLD)[0]
    if len(under):
        lag = MIN_LAG + int(under[0])
        while lag + 1 <= H - 1 and dp[lag + 1] < dp[lag]:
            lag += 1
        voiced = 1
    else:
        lag = MIN_LAG + int(np.argmin(rng))  # the first of equal minima
        voiced = 0
    a, b, cc = dp[lag - 1], dp[lag], dp[lag + 1]
    den = a - 2.0 * b + cc
    p = min(max(0.5 * (a - cc) / den, -0.5), 0.5) if den > 0.0 else 0.0
    return np.float32(sr / (lag + p)), np.float32(min(max(1.0 - b, 0.0), 1.0)), lag, voiced


def mix(window):
    """window: float32 [streams, channels, P] -> float64 [streams, P]: the sample, or (l + r) / 2"""
    w = np.asarray(window, np.float32).astype(np.float64)
    return w[:, 0] if w.shape[1] == 1 else (w[:, 0] + w[:, 1]) * 0.5


def pitch(window, sr, order=0):
    """window: float32 [streams, channels, P] -> PITCH_DTYPE [streams]"""
    out = np.zeros(len(window), PITCH_DTYPE)
    for s, x in enumerate(mix(window)):
        out[s] = pitch_one(x, sr, order)
    return out


def ulps(a, b):
    """distance in float32 steps between finite values"""
    def key(v):
        i = np.asarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def evaluate(window, sr):
    """the reference of every stream and whether it is well conditioned: (PITCH_DTYPE [streams], bool [streams])"""
    a, b = pitch(window, sr, 0), pitch(window, sr, 1)
    well = (a["lag"] == b["lag"]) & (a["voiced"] == b["voiced"]) & (ulps(a["hz"], b["hz"]) <= 1) & (ulps(a["clarity"], b["clarity"]) <= 1)
    return a, well


def compare(got, want, well, ulp=2):
    """the device against the reference: the indices of the well-conditioned streams that differ (lag and voiced equal, hz
    and clarity within `ulp` float32 steps), and the number of streams left out"""
    ok = (got["lag"] == want["lag"]) & (got["voiced"] == want["voiced"]) & (ulps(got["hz"], want["hz"]) <= ulp) \
        & (ulps(got["clarity"], want["clarity"]) <= ulp)
    return np.nonzero(well & ~ok)[0], int(np.count_nonzero(~well))
