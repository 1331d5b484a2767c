"""Float64 restatement of WF_HIP_OUT_SIGNAL (include/wf_hip.h, "signal statistics"): level, DC, clipping and stereo phase of
the newest W = fft_size frames of every stream, from a zero-prefixed history of the frames pushed into it."""
import numpy as np

FULL_SCALE = np.float32(0.999969482421875)  # 32767 / 32768


class History:
    """What the rings of `streams` streams hold, as far as the window can see: the newest W frames of every captured
    channel, zeros where nothing has been pushed since create or reset."""

    def __init__(self, streams, capture_channels, W):
        self.W = W
        self.x = np.zeros((streams, capture_channels, W), np.float32)

    def push(self, samples, first=0, frames=None):
        """samples: float32 [count, capture_channels, n]; frames: per-stream counts of a ragged push (the first frames[i] of
        stream i's block)"""
        samples = np.asarray(samples, np.float32)
        for i in range(samples.shape[0]):
            n = samples.shape[2] if frames is None else int(frames[i])
            if n == 0:
                continue
            s = first + i
            self.x[s] = np.concatenate([self.x[s], samples[i, :, :n]], axis=1)[:, -self.W:]

    def reset(self, first, count):
        self.x[first:first + count] = 0.0

    def window(self):
        return self.x


def _db(ratio, scale):
    ratio = np.asarray(ratio, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(ratio > 0, scale * np.log10(np.where(ratio > 0, ratio, 1.0)), -np.inf)


def signal(window):
    """window: float32 [streams, capture_channels, W].  Returns a dict of float64 arrays: rms_db, peak_db, dc, clipped
    ([streams, 2]; peak_db is 20 log10 of the float32 maximum), correlation, balance_db, mid_db, side_db ([streams])."""
    w = np.asarray(window, np.float32)
    streams, cap, W = w.shape
    x = w.astype(np.float64)
    s1 = x.sum(axis=2)
    s2 = (x * x).sum(axis=2)
    mx = np.abs(w).max(axis=2).astype(np.float64)
    out = dict(rms_db=np.full((streams, 2), -np.inf), peak_db=np.full((streams, 2), -np.inf), dc=np.zeros((streams, 2)),
               clipped=np.zeros((streams, 2), np.int64), correlation=np.zeros(streams), balance_db=np.zeros(streams),
               mid_db=np.full(streams, -np.inf), side_db=np.full(streams, -np.inf))
    out["rms_db"][:, :cap] = _db(s2 / W, 10.0)
    out["peak_db"][:, :cap] = _db(mx, 20.0)
    out["dc"][:, :cap] = s1 / W
    out["clipped"][:, :cap] = (np.abs(w) >= FULL_SCALE).sum(axis=2)
    if cap == 2:
        l, r = x[:, 0], x[:, 1]
        l2, r2 = s2[:, 0], s2[:, 1]
        slr = (l * r).sum(axis=1)
        both = (l2 > 0) & (r2 > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            out["correlation"] = np.where(both, np.clip(slr / np.sqrt(l2 * r2), -1.0, 1.0), 0.0)
            out["balance_db"] = np.where(both, 10.0 * np.log10(r2 / l2),
                                         np.where(l2 > 0, -np.inf, np.where(r2 > 0, np.inf, 0.0)))
        out["mid_db"] = _db((((l + r) / 2) ** 2).sum(axis=1) / W, 10.0)
        out["side_db"] = _db((((l - r) / 2) ** 2).sum(axis=1) / W, 10.0)
    return out


DB_TOL = 1e-4  # dB, of rms_db, balance_db, mid_db and side_db


def mismatches(got, want):
    """(field, stream index, got, want) of everything in `got` ([streams] of wf_hip_signal) beyond the bound of `want` (signal()'s
    dict): rms_db, balance_db, mid_db and side_db within 1e-4 dB, infinities equal; peak_db (the maximum is one of the samples) and
    clipped exact; dc within 1e-7 + 1e-6 |want|; correlation within 1e-6"""
    bad = []

    def note(name, ok, g, w):
        bad.extend((name, tuple(i), np.asarray(g)[tuple(i)].item(), np.asarray(w)[tuple(i)].item()) for i in np.argwhere(~np.asarray(ok))[:5])

    def db_close(g, w):
        g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
        with np.errstate(invalid="ignore"):
            return np.where(np.isinf(w), g == w, np.abs(g - w) <= DB_TOL)

    ch = got["ch"]
    note("ch.rms_db", db_close(ch["rms_db"], want["rms_db"]), ch["rms_db"], want["rms_db"])
    note("ch.peak_db", ch["peak_db"] == want["peak_db"].astype(np.float32), ch["peak_db"], want["peak_db"])
    note("ch.clipped", ch["clipped"] == want["clipped"], ch["clipped"], want["clipped"])
    d, w = ch["dc"].astype(np.float64), want["dc"]
    note("ch.dc", np.abs(d - w) <= 1e-7 + 1e-6 * np.abs(w), d, w)
    c = got["correlation"].astype(np.float64)
    note("correlation", np.abs(c - want["correlation"]) <= 1e-6, c, want["correlation"])
    for f in ("balance_db", "mid_db", "side_db"):
        note(f, db_close(got[f], want[f]), got[f], want[f])
    return bad
