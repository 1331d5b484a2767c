"""float64 reference of the loudness producer (include/wf_hip.h, "loudness"), written from ITU-R BS.1770-4 and EBU Tech 3341 /
3342: K-weighting, 100 ms sub-blocks, momentary / short-term windows, gated integrated loudness with exact gating, loudness
range with exact nearest-rank percentiles (no histogram) and true peak through the same 4x interpolator the library designs
(restated here).  The IIR runs as a numpy time loop vectorised over streams and channels."""
from __future__ import annotations

import math

import numpy as np

# BS.1770-4 Tables 1 and 2 (48 kHz)
TABLE_SHELF = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585)
TABLE_HPF = (1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621)

# the analogue prototypes behind the tables (bilinear transform with pre-warping)
SHELF_F0, SHELF_GAIN_DB, SHELF_Q, SHELF_VB_EXP = 1681.974450955533, 3.999843853973347, 0.7071752369554196, 0.4996667741545416
HPF_F0, HPF_Q = 38.13547087602444, 0.5003270373238773


def k_coefs(fs: int):
    """(shelf, hpf): each (b0, b1, b2, a1, a2) with a0 = 1"""
    K = math.tan(math.pi * SHELF_F0 / fs)
    Vh = 10.0 ** (SHELF_GAIN_DB / 20.0)
    Vb = Vh ** SHELF_VB_EXP
    a0 = 1.0 + K / SHELF_Q + K * K
    shelf = ((Vh + Vb * K / SHELF_Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / SHELF_Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / SHELF_Q + K * K) / a0)
    K = math.tan(math.pi * HPF_F0 / fs)
    a0 = 1.0 + K / HPF_Q + K * K
    hpf = (1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / HPF_Q + K * K) / a0)
    return shelf, hpf


def response_db(fs: int, f: float) -> float:
    """|H| of the K-weighting cascade at f Hz, dB"""
    z = np.exp(-2j * np.pi * f / fs)
    h = 1.0
    for b0, b1, b2, a1, a2 in k_coefs(fs):
        h *= (b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z)
    return float(20.0 * np.log10(abs(h)))


def fir_taps() -> np.ndarray:
    """[4 phases][12 taps]: 48-tap Kaiser (beta 7) windowed sinc, cut-off at the input Nyquist, each phase at unit DC gain;
    y[4m + r] = sum_k taps[r, k] x[m - k]"""
    n = np.arange(48)
    c = 23.5
    h = np.sinc((n - c) / 4.0) * np.kaiser(48, 7.0)
    ph = h.reshape(12, 4).T
    return ph / ph.sum(axis=1, keepdims=True)


def kweight(x: np.ndarray, fs: int) -> np.ndarray:
    """x: [..., frames] -> K-weighted, float64 (direct form II transposed, zero initial state)"""
    x = np.asarray(x, np.float64)
    lead = x.shape[:-1]
    flat = x.reshape(-1, x.shape[-1])
    y = np.empty_like(flat)
    (b0, b1, b2, a1, a2), (c0, c1, c2, d1, d2) = k_coefs(fs)
    s0 = np.zeros(flat.shape[0]); s1 = np.zeros_like(s0); s2 = np.zeros_like(s0); s3 = np.zeros_like(s0)
    for t in range(flat.shape[1]):
        xt = flat[:, t]
        y1 = b0 * xt + s0
        s0 = b1 * xt - a1 * y1 + s1
        s1 = b2 * xt - a2 * y1
        yt = c0 * y1 + s2
        s2 = c1 * y1 - d1 * yt + s3
        s3 = c2 * y1 - d2 * yt
        y[:, t] = yt
    return y.reshape(lead + (x.shape[-1],))


def _lufs(ms):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(ms)


def true_peak(x: np.ndarray) -> np.ndarray:
    """x: [streams, channels, frames] -> dBTP per stream (the 4 phases of the interpolator and the samples themselves)"""
    x = np.asarray(x, np.float64)
    taps = fir_taps()
    pad = np.concatenate([np.zeros(x.shape[:-1] + (11,)), x], axis=-1)
    n = x.shape[-1]
    peak = np.abs(x).max(axis=(1, 2)) if n else np.zeros(x.shape[0])
    for r in range(4):
        acc = np.zeros(x.shape)
        for k in range(12):
            acc += taps[r, k] * pad[..., 11 - k:11 - k + n]
        peak = np.maximum(peak, np.abs(acc).max(axis=(1, 2)))
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(peak)


def measure(x: np.ndarray, fs: int) -> dict:
    """x: [streams, channels, frames] (channels of weight 1.0) -> readings per stream, as wf_hip_loudness defines them"""
    x = np.asarray(x, np.float64)
    S, _, n = x.shape
    B = fs // 10
    y = kweight(x, fs)
    nsub = n // B
    e = (y[..., :nsub * B] ** 2).reshape(S, y.shape[1], nsub, B).sum(axis=(1, 3))  # [S, nsub]
    out = {k: np.full(S, -np.inf) for k in ("momentary", "short_term", "integrated", "true_peak")}
    out["range"] = np.zeros(S)
    out["frames"] = np.full(S, n, np.uint64)
    out["true_peak"] = true_peak(x)
    for s in range(S):
        if nsub >= 4:
            m = np.convolve(e[s], np.ones(4), "valid") / (4 * B)  # the 400 ms blocks, one per completed sub-block
            out["momentary"][s] = _lufs(m[-1])
            L = _lufs(m)
            g = m[L > -70.0]
            if g.size:
                gate = _lufs(g.mean()) - 10.0
                sel = m[(L > -70.0) & (L > gate)]
                if sel.size:
                    out["integrated"][s] = _lufs(sel.mean())
        if nsub >= 30:
            st = np.convolve(e[s], np.ones(30), "valid") / (30 * B)
            out["short_term"][s] = _lufs(st[-1])
            L = _lufs(st)
            g = st[L > -70.0]
            if g.size:
                gate = _lufs(g.mean()) - 20.0
                v = np.sort(L[(L > -70.0) & (L > gate)])
                if v.size:
                    p10 = v[max(math.ceil(0.10 * v.size), 1) - 1]
                    p95 = v[max(math.ceil(0.95 * v.size), 1) - 1]
                    out["range"][s] = p95 - p10
    return out
