"""Float64 restatement of WF_HIP_OUT_BANDS (include/wf_hip.h, "band levels"): third-octave band levels (IEC 61260-1, base
ten) and the Z / A / C weighted level (IEC 61672-1) of spectrum rows, from the rows, the window table, the sample rate and the
FFT size alone.  The tests compare the device against it; nothing here knows how the device sums."""
import numpy as np

NUM_BANDS = 31
BANDS_DTYPE = np.dtype([("band_db", np.float32, (NUM_BANDS,)), ("covered", np.uint32), ("total_db", np.float32), ("a_db", np.float32),
                        ("c_db", np.float32), ("reserved", np.uint32)])
DB_MIN = np.float32(-758.5955810546875)  # wf_hip_db_min(): 20.0f * std::log10(FLT_MIN) as the C library rounds it


def centres_hz():
    return 1000.0 * 10.0 ** ((np.arange(NUM_BANDS) - 17) / 10.0)


def edges_hz():
    """e[0..31]: band b lies between e[b] and e[b + 1]"""
    j = np.arange(NUM_BANDS + 1)
    return 1000.0 * 10.0 ** ((2 * (j - 17) - 1) / 20.0)


def edges_bins(sr, n):
    return edges_hz() * float(n) / float(sr)


def enbw(window, n):
    """equivalent noise bandwidth in bins of the float32 window table (None or empty: no window, 1)"""
    if window is None or len(window) == 0:
        return 1.0
    s1 = s2 = 0.0
    for w in np.asarray(window, np.float32).astype(np.float64):  # (index order, float64 sums, as the definition says)
        s1 += w
        s2 += w * w
    return float(n) * s2 / (s1 * s1)


def ra(f):
    f2 = np.asarray(f, np.float64) ** 2
    return 12194.0 ** 2 * f2 ** 2 / ((f2 + 20.6 ** 2) * np.sqrt((f2 + 107.7 ** 2) * (f2 + 737.9 ** 2)) * (f2 + 12194.0 ** 2))


def rc(f):
    f2 = np.asarray(f, np.float64) ** 2
    return 12194.0 ** 2 * f2 / ((f2 + 20.6 ** 2) * (f2 + 12194.0 ** 2))


def a_weight(f):
    """the squared A weighting, exactly 1 at 1000 Hz"""
    return (ra(f) / ra(1000.0)) ** 2


def c_weight(f):
    return (rc(f) / rc(1000.0)) ** 2


def bin_weights(sr, n):
    """[NUM_BANDS, M]: the length of the overlap of [k - 0.5, k + 0.5] with [E[b], E[b + 1]]"""
    m = n // 2
    e = edges_bins(sr, n)
    k = np.arange(m, dtype=np.float64)
    return np.maximum(np.minimum(k[None] + 0.5, e[1:, None]) - np.maximum(k[None] - 0.5, e[:-1, None]), 0.0)


def covered(sr, n):
    e = edges_bins(sr, n)
    m = n // 2
    bits = 0
    for b in range(NUM_BANDS):
        if e[b] >= 0.5 and e[b + 1] <= m - 0.5:
            bits |= 1 << b
    return bits


def powers(rows):
    """P[..., k] of float32 rows [..., M]"""
    rows = np.asarray(rows, np.float32)
    p = 10.0 ** (rows.astype(np.float64) / 10.0)
    p[rows <= DB_MIN] = 0.0
    p[..., 0] = 0.0
    return p


def _db(s):
    with np.errstate(divide="ignore"):
        return np.where(s == 0.0, -np.inf, 10.0 * np.log10(np.where(s == 0.0, 1.0, s))).astype(np.float32)


def bands_of_powers(p, window, sr, n, reverse=False):
    """the struct of rows whose powers are p [..., M] (float64); reverse: the sums taken in the opposite order of k"""
    m = n // 2
    assert p.shape[-1] == m
    q = enbw(window, n)
    w = bin_weights(sr, n)
    f = np.arange(m, dtype=np.float64) * float(sr) / float(n)
    wa, wc = a_weight(f), c_weight(f)
    if reverse:
        p, w, wa, wc = p[..., ::-1], w[:, ::-1], wa[::-1], wc[::-1]
    out = np.zeros(p.shape[:-1], BANDS_DTYPE)
    for b in range(NUM_BANDS):
        out["band_db"][..., b] = _db(np.sum(p * w[b], axis=-1) / q)
    out["covered"] = covered(sr, n)
    out["total_db"] = _db(np.sum(p, axis=-1) / q)
    out["a_db"] = _db(np.sum(p * wa, axis=-1) / q)
    out["c_db"] = _db(np.sum(p * wc, axis=-1) / q)
    return out


def bands(rows, window, sr, n, reverse=False):
    """rows: float32 [..., M] as WF_HIP_OUT_DECIBELS returns them; window: the float32 table WF_HIP_TABLE_WINDOW (None: no window)"""
    return bands_of_powers(powers(rows), window, sr, n, reverse)


def ulps(a, b):
    """distance of two float32 values in representable steps (equal infinities: 0)"""
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def mismatches(got, want):
    """(field, index) of every value outside the contract's bound: |got - want| <= max(1 float32 ulp of want, 1e-9 dB), -INFINITY
    exactly where `want` has it, `covered` and `reserved` equal"""
    bad = []
    for name in ("band_db", "total_db", "a_db", "c_db"):
        g, w = got[name], want[name]
        inf = np.isneginf(w)
        with np.errstate(invalid="ignore"):
            ok = np.where(inf, np.isneginf(g), np.abs(g.astype(np.float64) - w.astype(np.float64))
                          <= np.maximum(np.spacing(np.abs(w)).astype(np.float64), 1e-9))
        ok &= np.isfinite(g) | inf
        bad += [(name, tuple(i), float(g[tuple(i)]), float(w[tuple(i)])) for i in np.argwhere(~ok)[:5]]
    for name in ("covered", "reserved"):
        bad += [(name, tuple(i), int(got[name][tuple(i)]), int(want[name][tuple(i)])) for i in np.argwhere(got[name] != want[name])[:5]]
    return bad
