"""Structured test audio for the spectrum tick -- tones, DC, square waves, lone samples -- with the rows they must produce in closed
form, and the accuracy criterion the tone tests use.  numpy only.

Every parity test before this module fed the tick uniform noise or digital silence.  Noise cannot see a share of a window that
drops out of the silence scan (every thread holds a non-zero sample) and it hides the round-off of a transform (every bin sits
near the frame's peak).  The generators here are addressed by the ABSOLUTE sample index, so packets of any size join up: a spec
is a small dict, `render(spec, start, frames)` its samples [start, start + frames) as float32.

  sine(n, f_bins, amp, phase)   amp * sin(2 pi f_bins i / n + phase): f_bins in bins of an n-point transform
  dc(level)
  square(n, f_bins, amp)        +amp over the first half of every period of n / f_bins samples, -amp over the second
  two_tone(n)                   0.5 at 100.37 bins plus 1e-4 at 901.5 bins of a 4096-point transform, scaled to n
                                (the same two frequencies in Hz at every n: a strong line and one 74 dB under it)
  impulses([(pos, value), ...]) zeros but for the listed absolute positions
Every spec takes an optional "offset": the signal advanced by that many samples (how two streams of a batch hear different
audio from one spec).

Closed forms (float64), with the window `w` and its sum taken from the restatement (OracleSource.window()):
  lone_sample_row      one sample a at window position p: every bin reads 20 log10(|a| w[p] 2 / sum) (times the slope table)
  two_sample_row       a at p and b at q, no window: bin k reads |a + b e^{-2 pi i k (q - p) / n}| 2 / n

assert_no_worse_than_reference: see its docstring; why tones need it is DESIGN.md section 5.
"""
from __future__ import annotations

import numpy as np

TWO_TONE_N = 4096  # two_tone's frequencies are given in bins of this size


def sine(n, f_bins, amp=1.0, phase=0.0, offset=0):
    return dict(kind="sine", n=int(n), f_bins=float(f_bins), amp=float(amp), phase=float(phase), offset=int(offset))


def dc(level, offset=0):
    return dict(kind="dc", level=float(level), offset=int(offset))


def square(n, f_bins, amp=1.0, offset=0):
    return dict(kind="square", n=int(n), f_bins=float(f_bins), amp=float(amp), offset=int(offset))


def two_tone(n, offset=0):
    return dict(kind="two_tone", n=int(n), offset=int(offset))


def impulses(points, offset=0):
    return dict(kind="impulses", points=[(int(p), float(np.float32(v))) for p, v in points], offset=int(offset))


def _turns(n, f_bins, idx):
    """f_bins * idx / n modulo 1 in float64; idx is exact (int64), the product is reduced modulo n first where f_bins is whole"""
    if float(f_bins).is_integer():
        return ((int(f_bins) * idx) % n).astype(np.float64) / n
    t = f_bins * idx.astype(np.float64) / n
    return t - np.floor(t)


def render(spec, start: int, frames: int) -> np.ndarray:
    """float32 [frames]: samples [start, start + frames) of `spec` (None: zeros)"""
    if spec is None:
        return np.zeros(frames, np.float32)
    idx = np.arange(frames, dtype=np.int64) + int(start) + int(spec.get("offset", 0))
    kind = spec["kind"]
    if kind == "sine":
        x = spec["amp"] * np.sin(2.0 * np.pi * _turns(spec["n"], spec["f_bins"], idx) + spec["phase"])
    elif kind == "dc":
        x = np.full(frames, spec["level"], np.float64)
    elif kind == "square":
        x = np.where(_turns(spec["n"], spec["f_bins"], idx) < 0.5, spec["amp"], -spec["amp"])
    elif kind == "two_tone":
        s = spec["n"] / TWO_TONE_N
        x = (0.5 * np.sin(2.0 * np.pi * _turns(spec["n"], 100.37 * s, idx)) + 1e-4 * np.sin(2.0 * np.pi * _turns(spec["n"], 901.5 * s, idx)))
    elif kind == "impulses":
        out = np.zeros(frames, np.float32)
        first = int(idx[0]) if frames else 0
        for p, v in spec["points"]:
            if first <= p < first + frames:
                out[p - first] = np.float32(v)
        return out
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def render_channels(spec, channels: int, start: int, frames: int) -> np.ndarray:
    """float32 [channels, frames]; `spec` is one spec for every channel, or a list / tuple of one spec (or None) per channel"""
    per = list(spec) if isinstance(spec, (list, tuple)) else [spec] * channels
    assert len(per) >= channels, (len(per), channels)
    return np.stack([render(per[c], start, frames) for c in range(channels)])


# ---- closed forms -------------------------------------------------------------------------------------------------------------
def lone_sample_row(a, p, window, window_sum, bins, slope=None, db_min=None):
    """float64 [bins]: the row of a window that holds the one sample `a` at position p.  window: float32 [n] or None (no window:
    w = 1, sum = n).  slope: the restatement's slope table or None.  A magnitude of zero (w[p] == 0) reads db_min."""
    w = 1.0 if window is None else float(window[p])
    mag = np.full(bins, abs(float(np.float32(a))) * w * 2.0 / float(window_sum), np.float64)
    if slope is not None:
        mag = mag * np.asarray(slope, np.float64)
    out = np.full(bins, np.nan if db_min is None else float(db_min), np.float64)
    np.log10(mag, out=out, where=mag > 0.0)
    out[mag > 0.0] *= 20.0
    return out


def two_sample_row(a, p, b, q, n, slope=None):
    """float64 [n / 2]: a at p and b at q of an n-sample window, no window function"""
    k = np.arange(n // 2, dtype=np.int64)
    ang = -2.0 * np.pi * ((k * (int(q) - int(p))) % n).astype(np.float64) / n
    mag = np.abs(float(np.float32(a)) + float(np.float32(b)) * np.exp(1j * ang)) * 2.0 / n
    if slope is not None:
        mag = mag * np.asarray(slope, np.float64)
    return 20.0 * np.log10(mag)


# ---- the accuracy criterion for concentrated spectra --------------------------------------------------------------------------
def _linear(db, off):
    return 10.0 ** ((np.asarray(db, np.float32).astype(np.float64) + off) / 20.0)


def reference_error(ref_db, truth_db, undo_db=None):
    """E_ref per frame (last axis): the largest |ref - truth| in linear magnitude, float64, shape [..., 1]"""
    off = 0.0 if undo_db is None else np.asarray(undo_db, np.float64)
    return np.abs(_linear(ref_db, off) - _linear(truth_db, off)).max(axis=-1, keepdims=True)


def assert_no_worse_than_reference(got_db, ref_db, truth_db, k, what="", undo_db=None):
    """Rows of dB values (last axis = the bins of one frame) of a float transform, judged by how far the REFERENCE's float
    transform is from the truth on the same frame:

      truth   the restatement's row: the DFT in double, rounded once
      ref     the reference's row (its float FFTW)
      E_ref   the frame's largest |ref - truth|, in linear magnitude
      q[bin]  the linear size of half a float32 ulp of that bin's dB value, the larger of the two sides: the rows are float32 dB,
              which near a -20 dB peak is already 1e-7 relative, so `got` and `truth` each carry up to q of rounding
      a bin passes if   |got - truth| <= k * E_ref + 2 q[bin]

    undo_db (per bin) is added to all three rows before the conversion, as assert_db_close does.  Returns the worst frame's
    ratio max|got - truth| / E_ref (0 where both are 0).  Counts nothing in helpers.ARM_STATS: the linear arm of
    assert_db_close, whose rarity test_zz_display_arm_stays_rare bounds, is not involved."""
    off = 0.0 if undo_db is None else np.asarray(undo_db, np.float64)
    t32 = np.asarray(truth_db, np.float32)
    g, r, t = _linear(got_db, off), _linear(ref_db, off), _linear(t32, off)
    assert g.shape == r.shape == t.shape, (g.shape, r.shape, t.shape)
    assert np.isfinite(g).all(), f"{what}: non-finite values"
    e_ref = np.abs(r - t).max(axis=-1, keepdims=True)
    half = 0.5 * np.spacing(np.abs(t32)).astype(np.float64)
    t64 = t32.astype(np.float64) + off
    q = np.maximum(10.0 ** ((t64 + half) / 20.0) - t, t - 10.0 ** ((t64 - half) / 20.0))
    err = np.abs(g - t)
    bad = err > k * e_ref + 2.0 * q if k is not None else np.zeros(err.shape, bool)
    worst = err.max(axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(worst > 0.0, worst / e_ref, 0.0)
    if bad.any():
        i = int(np.argmax(np.where(bad, err - k * e_ref - 2.0 * q, -np.inf)))
        frame = i // g.shape[-1]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} bins farther from the double DFT than {k} x the reference is; worst at "
                             f"flat index {i}: |got - truth| {err.flat[i]:.3e}, E_ref {e_ref.flat[frame]:.3e}, q {q.flat[i]:.3e} "
                             f"(frame peak {t.reshape(-1, t.shape[-1])[frame].max():.3e}); worst frame ratio {float(ratio.max()):.2f}")
    return float(ratio.max())


def needed_k(got_db, ref_db, truth_db, undo_db=None):
    """the smallest k with which assert_no_worse_than_reference passes: the largest (|got - truth| - 2 q) / E_ref over all bins --
    unlike the ratio it returns, the number the bound is about (a peak bin one dB ulp off shows in the ratio and not here)"""
    off = 0.0 if undo_db is None else np.asarray(undo_db, np.float64)
    t32 = np.asarray(truth_db, np.float32)
    g, r, t = _linear(got_db, off), _linear(ref_db, off), _linear(t32, off)
    e_ref = np.abs(r - t).max(axis=-1, keepdims=True)
    half = 0.5 * np.spacing(np.abs(t32)).astype(np.float64)
    t64 = t32.astype(np.float64) + off
    q = np.maximum(10.0 ** ((t64 + half) / 20.0) - t, t - 10.0 ** ((t64 - half) / 20.0))
    over = np.maximum(np.abs(g - t) - 2.0 * q, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(over > 0.0, over / e_ref, 0.0).max())


def assert_within_peak(got_db, truth_db, eps, what="", undo_db=None):
    """every bin within eps of the frame's largest magnitude (last axis) of `truth`, in linear magnitude: the linear arm of
    assert_db_close (eps = helpers.LIN_EPS) alone and uncounted -- the stated fallback of the tone tests"""
    off = 0.0 if undo_db is None else np.asarray(undo_db, np.float64)
    g, t = _linear(got_db, off), _linear(truth_db, off)
    assert np.isfinite(g).all(), f"{what}: non-finite values"
    err, peak = np.abs(g - t), t.max(axis=-1, keepdims=True)
    bad = err > eps * peak
    if bad.any():
        i = int(np.argmax(np.where(bad, err / peak, -np.inf)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} bins off by more than {eps:g} of the frame's peak; worst at flat index {i}: "
                             f"{(err / peak).flat[i]:.3e}")
