"""Transfer function (WF_HIP_OUT_XFER) without a device: the structured dtype against the C layout, the appended output number, P
and K of every (fft size, ring) the library makes with the span they need (wf::host::xfer_window / xfer_segments, compiled into a
program of their own), the restatement (tests/xfer_ref.py) against an independent Welch estimate, how well the definition measures
a known system, the conditions of the device comparison on its own seeds and shapes, and a gfx950 compile of the read kernel with no
scratch and no spilled vector registers."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
import measure_stagger as ms
import xfer_ref as ref
from kernel_usage import kernel_usage

OUT_XFER = binding.OUT_XFER  # (the output these tests are about: a library without it fails every one of them)
ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "waveform_amd" / "csrc"
SR = 48000
# (fft size, ring) of the committed geometries (P, K) = (256, 13), (512, 13), (1024, 13), (2048, 13), (2048, 32)
GEOMETRIES = ((256, 2048), (512, 4096), (1024, 8192), (2048, 16384), (2048, 65536))


def test_xfer_dtype_matches_the_c_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wf_hip.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %d %d %d %d %d", sizeof(wf_hip_xfer), (int)WF_HIP_OUT_XFER, (int)WF_HIP_OUT_ONSET,\n'
                   "         (int)WF_HIP_XFER_MAX_WINDOW, (int)WF_HIP_XFER_MAX_SEGMENTS, (int)WF_HIP_XFER_BINS);\n"
                   + "".join(f'  printf(" %zu", offsetof(wf_hip_xfer, {n}));\n' for n in ref.FIELDS) +
                   '  printf(" %d %.17g", (int)WF_HIP_ABI_VERSION, WF_HIP_STEREO_DEAD_RATIO);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    text = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    got = [int(v) for v in text[:-1]]
    dt = binding.XFER_DTYPE
    assert got == [dt.itemsize, binding.OUT_XFER, binding.OUT_ONSET, binding.XFER_MAX_WINDOW, binding.XFER_MAX_SEGMENTS, binding.XFER_BINS] \
        + [dt.fields[n][1] for n in ref.FIELDS] + [13]
    assert float(text[-1]) == ref.DEAD_RATIO
    assert dt.itemsize == 12336 and dt.itemsize % 16 == 0 and dt == ref.XFER_DTYPE
    assert dt.names == ("valid", "window", "hop", "segments", "lag", "newest", "lag_peak", "mean_coherence", "reserved", "gain_db", "phase",
                        "coherence")
    assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 48, 48 + 4096, 48 + 8192]
    assert dt.fields["lag"][0] == np.int32 and dt.fields["reserved"][0].shape == (4,)
    for n in ("gain_db", "phase", "coherence"):
        assert dt.fields[n][0].shape == (1024,) and dt.fields[n][0].base == np.float32
    assert (ref.MAX_WINDOW, ref.MAX_SEGMENTS, ref.BINS) == (binding.XFER_MAX_WINDOW, binding.XFER_MAX_SEGMENTS, binding.XFER_BINS) == (2048, 32, 1024)


# ---- P and K of every ring the library makes ----------------------------------------------------------------------------------------

PROGRAM = r"""
#include <cstdio>
#include "wf_measure_tables.hpp"
using namespace wf::host;
int main() {
  // every fft size the output serves, with every ring wf_hip_create can give it: a power of two >= the fft size, from 512 frames
  for(unsigned w = 256; w <= 65536; w += 16)
    for(unsigned ring = 512; ring <= (1u << 22); ring *= 2) {
      if(ring < w) continue;
      const unsigned p = xfer_window(w, ring), k = xfer_segments(p, ring);
      std::printf("%u %u %u %u\n", w, ring, p, k);
    }
  // the tables are the delay finder's at this P
  for(unsigned p : {64u, 256u, 2048u}) {
    const DelayTables t = delay_tables(p);
    if(t.P != p || t.tab.size() != 2 * (size_t)p || (1u << t.log2p) != p) return 2;
  }
  return 0;
}
"""


def _build_and_run(directory, name, extra=()):
    src = directory / "xfer_sizes_main.cpp"
    src.write_text(PROGRAM)
    exe = directory / name
    subprocess.run(["g++", "-std=c++20", "-O2", *extra, "-I", str(CSRC), "-I", str(ROOT / "include"), str(src),
                    str(CSRC / "wf_measure_tables.cpp"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout


@pytest.fixture(scope="module")
def sizes(tmp_path_factory):
    return _build_and_run(tmp_path_factory.mktemp("xfer_sizes"), "sizes")


def test_window_and_segments_of_every_ring(sizes):
    """P the largest power of two <= min(W, 2048, R / 8), K = min(32, 2 R / P - 3) >= 13, and the span with its slack and the
    frames behind the anchor inside the ring: (K - 1) H + P + 2 L + (H - 1) < R"""
    rows = np.array([[int(v) for v in line.split()] for line in sizes.splitlines()])
    assert rows.shape[0] == 32526 and rows[:, 0].min() == 256 and rows[:, 0].max() == 65536
    seen = set()
    for w, ring, p, k in rows:
        assert (p, k) == ref.geometry(w, ring), (w, ring, p, k)
        assert p & (p - 1) == 0 and 64 <= p <= min(w, 2048, ring // 8) < 2 * p
        assert 13 <= k <= 32 and k == min(32, 2 * ring // p - 3)
        h, l = p // 2, p // 4
        assert (k - 1) * h + p + 2 * l + (h - 1) < ring and ref.span_frames(p, k) == (k - 1) * h + p + 2 * l
        seen.add((p, k))
    assert {(64, 13), (256, 13), (512, 13), (1024, 13), (2048, 13), (2048, 29), (2048, 32)} <= seen
    # the default rings: the next power of two of max(2 W, 4096)
    assert [ref.geometry(w, ref.ring_frames(w)) for w in (256, 800, 2208, 4096, 16384, 65536)] == \
        [(256, 29), (512, 13), (1024, 13), (1024, 13), (2048, 29), (2048, 32)]


def test_the_sizes_program_is_clean_under_the_sanitizers(sizes, tmp_path):
    """the same program with -fsanitize=address,undefined, run directly: exit 0 and the same output"""
    assert _build_and_run(tmp_path, "sizes_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")) == sizes


# ---- the restatement against an independent Welch estimate -------------------------------------------------------------------------

def _welch(sp, p, k, n):
    """H and coherence of the bins 1 .. M - 1 by scipy.signal's Welch estimate over the very frames the K segments cover, channel 1
    read n frames earlier; a plain loop over the segments with math.fsum where scipy is not installed"""
    h, l, m = p // 2, p // 4, p // 2
    e = sp.shape[1] - l
    first, last = e - (k - 1) * h - p, e
    y, x = sp[0, first:last].astype(np.float64), sp[1, first - n:last - n].astype(np.float64)
    w = ref.taper(p)
    try:
        from scipy import signal
    except ImportError:
        import math
        sxx, syy, sxy = [], [], []
        for kk in range(1, m):
            c = np.exp(-2j * np.pi * kk * np.arange(p) / p)
            xs = [complex(np.dot(w * x[a * h:a * h + p], c)) for a in range(k)]
            ys = [complex(np.dot(w * y[a * h:a * h + p], c)) for a in range(k)]
            sxx.append(math.fsum(abs(v) ** 2 for v in xs))
            syy.append(math.fsum(abs(v) ** 2 for v in ys))
            sxy.append(complex(math.fsum((v.conjugate() * u).real for v, u in zip(xs, ys)),
                               math.fsum((v.conjugate() * u).imag for v, u in zip(xs, ys))))
        sxx, syy, sxy = np.array(sxx), np.array(syy), np.array(sxy)
        return sxy / sxx, np.abs(sxy) ** 2 / (sxx * syy)
    kw = dict(fs=1.0, window=w, nperseg=p, noverlap=p - h, detrend=False)
    _, pxy = signal.csd(x, y, **kw)  # conj(X) Y
    _, pxx = signal.welch(x, **kw)
    _, coh = signal.coherence(x, y, **kw)
    return (pxy / pxx)[1:m], coh[1:m]


@pytest.mark.parametrize("w,ring", GEOMETRIES)
def test_the_restatement_is_a_welch_estimate(w, ring):
    p, k = ref.geometry(w, ring)
    rng = np.random.default_rng(77 + p + k)
    n = ring + p // 2 + 3
    for kind in ("fir +37", "added noise", "delay -(L-1)"):
        x = ref.stream(kind, rng, n, p)
        r, v = ref.analyse(x, w, ring, SR)
        assert v["lag"] == ref.true_lag(kind, p)
        sp = x[:, n - (n % (p // 2)) - ref.span_frames(p, k):n - (n % (p // 2))]
        hk, coh = _welch(sp, p, k, v["lag"])
        d_h = float(np.max(np.abs(v["h"] - hk) / np.abs(hk)))
        d_c = float(np.max(np.abs(v["coherence"] - np.minimum(coh, 1.0))))
        print(f"P {p}, K {k}, {kind}: H against Welch's {d_h:.3g} relative, coherence {d_c:.3g}")
        assert d_h <= 1e-12 and d_c <= 1e-12


# ---- physics on the restatement -----------------------------------------------------------------------------------------------------

# measured with seed 1000 (the figures the docstring below quotes): worst |gain_db error| dB, worst |phase error| rad, 1 - mean_coherence
FIR_MEASURED = {(256, 13): (0.0915, 0.01341, 1.30e-4), (512, 13): (0.0455, 0.00489, 3.1e-5), (1024, 13): (0.0267, 0.00301, 8e-6),
                (2048, 13): (0.0100, 0.00153, 2e-6), (2048, 32): (0.0089, 0.00112, 2e-6)}
# the mean over the bins of the coherence over the seeds 1000 .. 1015: (least, largest) with noise of the reference's power added to
# the measured channel, and of two independent channels read at lag 0
NOISE_MEASURED = {(256, 13): ((0.4884, 0.5596), (0.0672, 0.0909)), (512, 13): ((0.5065, 0.5521), (0.0721, 0.0913)),
                  (1024, 13): ((0.5117, 0.5396), (0.0740, 0.0853)), (2048, 13): ((0.5081, 0.5302), (0.0767, 0.0863)),
                  (2048, 32): ((0.5013, 0.5142), (0.0312, 0.0349))}


def _fir_errors(w, ring, seed):
    p, k = ref.geometry(w, ring)
    x = ref.stream("fir +37", np.random.default_rng(seed), ring + p // 2 + 3, p)
    r, v = ref.analyse(x, w, ring, SR)
    truth = ref.fir_response(p)
    assert v["live"].all()
    gain = float(np.max(np.abs(v["gain_db"] - 20.0 * np.log10(np.abs(truth)))))
    phase = float(np.max(np.abs(np.angle(v["h"] * np.conj(truth)))))
    return r, gain, phase, 1.0 - v["mean_coherence"]


@pytest.mark.parametrize("w,ring", GEOMETRIES)
def test_a_known_system_is_measured(w, ring):
    """white noise through the nine taps of xfer_ref.FIR and a delay of 37 frames: lag 37, and over the live bins the worst error of
    gain_db and of phase against the filter's true response -- the leakage bias of a finite window and the noise that K segments
    leave.  Measured with seed 1000: 0.0915 dB and 0.0134 rad at (P, K) = (256, 13), 0.0455 and 0.0049 at (512, 13), 0.0267 and
    0.0030 at (1024, 13), 0.0100 and 0.0015 at (2048, 13), 0.0089 and 0.0011 at (2048, 32); 1 - mean_coherence 1.3e-4, 3.1e-5,
    8e-6, 2e-6, 2e-6.  Asserted: twice those; the margin is for other seeds of the same family, and the three seeds after it stay
    under it (over 1000 .. 1015 the largest ratio to the first seed's figure was 1.77)"""
    p, k = ref.geometry(w, ring)
    g0, p0, c0 = FIR_MEASURED[(p, k)]
    for seed in (1000, 1001, 1002, 1003):
        r, gain, phase, deficit = _fir_errors(w, ring, seed)
        print(f"(P, K) = ({p}, {k}), seed {seed}: gain_db within {gain:.4f} dB (measured {g0}), phase within {phase:.5f} rad ({p0}), "
              f"1 - mean_coherence {deficit:.3g} ({c0}), lag {int(r['lag'])}, lag_peak {float(r['lag_peak']):.3f}")
        assert r["valid"] == 1 and r["lag"] == 37 and r["window"] == p and r["segments"] == k
        if seed == 1000:
            assert abs(gain - g0) <= 0.02 * g0 and abs(phase - p0) <= 0.02 * p0  # the quoted figures are this seed's
        assert gain <= 2.0 * g0 and phase <= 2.0 * p0 and deficit <= 2.0 * c0


@pytest.mark.parametrize("w,ring", GEOMETRIES)
def test_noise_lowers_the_coherence(w, ring):
    """noise of the reference's own power on the measured channel reads a coherence near 1 / 2, two independent channels one near
    the floor of K averages, 1 / K and somewhat more for the half overlap (a mean of 0.081 at K = 13, 0.033 at K = 32).  The bands:
    least / 1.5 .. largest * 1.5 of the mean over the bins that the restatement gave over the seeds 1000 .. 1015 (NOISE_MEASURED);
    four fresh seeds must lie in them"""
    p, k = ref.geometry(w, ring)
    (a_lo, a_hi), (i_lo, i_hi) = NOISE_MEASURED[(p, k)]
    assert a_lo < 0.5 * 1.2 and a_hi > 0.5 and 1.0 / k < i_hi < 1.3 / k and i_lo > 0.8 / k
    n = ring + p // 2 + 3
    for seed in (2000, 2001, 2002, 2003):
        rng = np.random.default_rng(seed)
        a = ref.analyse(ref.stream("added noise", rng, n, p), w, ring, SR)[1]
        i = ref.analyse(ref.stream("independent", rng, n, p), w, ring, SR, lag=0)[1]
        ca, ci = float(np.mean(a["coherence"])), float(np.mean(i["coherence"]))
        print(f"(P, K) = ({p}, {k}), seed {seed}: added noise {ca:.4f} in [{a_lo / 1.5:.4f}, {a_hi * 1.5:.4f}], independent {ci:.4f} in "
              f"[{i_lo / 1.5:.4f}, {i_hi * 1.5:.4f}]")
        assert a["lag"] == 0 and a_lo / 1.5 <= ca <= a_hi * 1.5
        assert i_lo / 1.5 <= ci <= i_hi * 1.5


def test_an_inverted_half_reads_minus_six_decibels_and_pi():
    w, ring = 1024, 8192
    rng = np.random.default_rng(5)
    r, v = ref.analyse(ref.stream("inverted -6 dB", rng, ring + 515, 1024), w, ring, SR)
    assert r["valid"] == 1 and r["lag"] == 0 and r["lag_peak"] == -1.0
    assert np.all(np.abs(v["gain_db"] - 20.0 * np.log10(0.5)) <= 1e-12) and abs(20.0 * np.log10(0.5) + 6.0206) < 1e-5
    assert np.all(np.abs(np.abs(v["phase"]) - np.pi) <= 1e-12) and np.all(v["coherence"] == 1.0) and r["mean_coherence"] == 1.0
    dual, d = ref.analyse(ref.stream("dual mono", rng, ring + 515, 1024), w, ring, SR)
    assert dual["lag"] == 0 and dual["lag_peak"] == 1.0 and not d["gain_db"].any() and not d["phase"].any() and np.all(d["coherence"] == 1.0)


def test_the_other_direction_is_coherence_over_h():
    """H_01 = coherence / H_10 to 1e-9 relative, on streams of lag 0 (the same segments read either way)"""
    w, ring = 1024, 8192
    rng = np.random.default_rng(6)
    for kind in ("added noise", "inverted -6 dB"):
        x = ref.stream(kind, rng, ring + 515, 1024)
        fwd = ref.analyse(x, w, ring, SR)[1]
        back = ref.analyse(x[::-1], w, ring, SR, lag=0)[1]
        assert fwd["lag"] == 0
        d = float(np.max(np.abs(back["h"] - fwd["coherence"] / fwd["h"]) / np.abs(back["h"])))
        print(f"{kind}: H_01 against coherence / H_10: {d:.3g} relative")
        assert d <= 1e-9 and np.max(np.abs(back["coherence"] - fwd["coherence"])) <= 1e-12


def test_dead_bins_silent_bins_and_validity():
    w, ring = 512, 4096
    p, k = ref.geometry(w, ring)
    n = ring + p // 2 + 3
    # a period of four frames, exact in float32: all of it in bin P / 4 and the taper's two neighbours, every other bin is rounding
    tone = np.tile(np.array([0.0, 0.5, 0.0, -0.5], np.float32), n // 4 + 1)[:n]
    r, v = ref.analyse(np.stack([np.float32(0.25) * tone, tone]), w, ring, SR, lag=0)
    live = v["live"]
    q = p // 4 - 1  # (v's index of bin P / 4)
    assert r["valid"] == 1 and np.flatnonzero(live).tolist() == [q - 1, q, q + 1]
    assert np.all(np.abs(v["gain_db"][live] - 20.0 * np.log10(0.25)) < 1e-9) and np.all(np.abs(v["coherence"][live] - 1.0) < 1e-12)
    for name in ("gain_db", "phase", "coherence"):
        assert not v[name][~live].any() and not r[name][0] and not r[name][p // 2:].any()
    # live bins with Syy == 0: -inf, 0, 0, and a mean coherence of 0
    rng = np.random.default_rng(8)
    x = ref.stream("tone, measured zero", rng, n, p, n % (p // 2))
    r, v = ref.analyse(x, w, ring, SR)
    assert r["valid"] == 1 and v["live"].all() and np.all(np.isneginf(v["gain_db"])) and not v["phase"].any() and not v["coherence"].any()
    assert r["lag"] == 0 and r["lag_peak"] == 0.0 and r["mean_coherence"] == 0.0 and not v["syy"].any()
    # without the sample in the slack the measured channel's span is all zeros: the zero record
    x[0] = 0.0
    zero = ref.zero_record(w, ring, 1)
    assert ref.analyse(x, w, ring, SR)[0].tobytes() == zero[0].tobytes()
    x = ref.stream("fir +37", rng, n, p)
    span = ref.span_frames(p, k)
    for bad in (np.nan, np.inf, -np.inf):
        for c in (0, 1):
            y = x.copy()
            y[c, n - 3 - span] = bad  # the oldest frame of the span
            assert ref.analyse(y, w, ring, SR)[0].tobytes() == zero[0].tobytes()
            y = x.copy()
            y[c, n - 4 - span] = bad  # one frame older: not in it
            assert ref.analyse(y, w, ring, SR)[0]["valid"] == 1
    y = x.copy()
    y[1] = -0.0
    assert ref.analyse(y, w, ring, SR)[0].tobytes() == zero[0].tobytes()
    assert zero["window"][0] == p and zero["hop"][0] == p // 2 and zero["segments"][0] == k and zero["valid"][0] == 0


def test_reads_within_a_hop_are_the_same():
    """the segments are anchored to the counter: frames pushed behind the anchor change nothing until the next one is reached"""
    w, ring = 1024, 8192
    p, k = ref.geometry(w, ring)
    h = p // 2
    rng = np.random.default_rng(9)
    x = ref.stream("fir +37", rng, ring + 2 * h, p)
    base = ref.analyse(x[:, :ring], w, ring, SR)[0]
    for extra in (1, 3, h - 1):
        assert ref.analyse(x[:, :ring + extra], w, ring, SR)[0].tobytes() == base.tobytes()
    moved = ref.analyse(x[:, :ring + h], w, ring, SR)[0]
    assert moved["newest"] == base["newest"] + 1 and moved.tobytes() != base.tobytes()
    older = x[:, :ring + 3].copy()
    older[:, :ring - ref.span_frames(p, k)] = 7.0  # only the span counts
    assert ref.analyse(older, w, ring, SR)[0].tobytes() == base.tobytes()


def test_mismatches_applies_the_bound():
    case = ref.GPU_CASES[1]
    want = ref.xfer(ref.case_audio(case)[:7], case[3], ref.ring_frames(case[3], case[4]), case[1], wpos=ref.case_wpos0(case) + 4096 + 259)
    assert ref.mismatches(want, want) == [] and np.all(want["valid"] == 1)
    for name in ref.FLOAT_FIELDS:
        where = (0, 3) if want[name].ndim == 2 else (0,)
        got = want.copy()
        f = got[name]
        f[where] = np.nextafter(f[where], np.float32(1e9))  # one ulp: inside
        assert ref.mismatches(got, want) == [], name
        f[where] = f[where] + max(3.0 * float(np.spacing(np.abs(f[where]))), 3e-6)  # three: outside
        assert [m[0] for m in ref.mismatches(got, want)] == [name]
    for name in ref.INT_FIELDS:
        got = want.copy()
        got[name][1] += 1
        assert {m[0] for m in ref.mismatches(got, want)} == {name}
    got = want.copy()
    got["phase"][2, 5] = -got["phase"][2, 5]  # the inverted stream: +pi and -pi are one angle
    assert abs(abs(float(want["phase"][2, 5])) - np.pi) < 1e-6 and ref.mismatches(got, want) == []
    got["gain_db"][0, 7] = np.nan
    assert [m[0] for m in ref.mismatches(got, want)] == ["gain_db"]
    got = want.copy()
    got["gain_db"][6, 9] = 0.0  # -inf is wanted there
    assert np.isneginf(want["gain_db"][6, 9]) and [m[0] for m in ref.mismatches(got, want)] == ["gain_db"]
    assert ref.mismatches(want[:1], want)[0][0] == "shape"


# ---- the conditions of the device comparison ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ref.GPU_CASES, ids=ref.case_id)
def test_the_gpu_cases_meet_the_conditions_of_the_bound(case):
    """on the very seeds and shapes of tests/test_gpu_xfer.py: the argmax margin |r[n0]| - max |r[n != n0]| is at least 1e-3 on every
    stream whose lag is asserted -- independent noise is exempt: its lag is noise, and the device comparison hands the device's lag to
    the restatement; so is the stream without any cross power, whose lag is 0 by definition --, and the four orders of the sums agree
    to 1e-9 in every field at the same lag.  With these, one float32 rounding is all that can separate the device from the
    restatement"""
    fft, sr, kw, w, ring = case
    cap = ref.ring_frames(w, ring)
    p, k = ref.geometry(w, cap)
    assert (p, k) == ref.GEOMETRIES[ref.GPU_CASES.index(case)]
    x = ref.case_audio(case)
    wpos = ref.case_wpos0(case) + x.shape[-1]
    assert x.shape == (9, 2, cap + p // 2 + 3) and wpos % (p // 2) in (3, 35)
    margin = ref.margins(x, w, cap, sr, wpos)
    base = ref.xfer(x, w, cap, sr, wpos=wpos)
    assert base["valid"].tolist() == [1] * 7 + [0, 0] and base[7:].tobytes() == ref.zero_record(w, cap, 2).tobytes()
    for s, name in enumerate(ref.KINDS):
        if name in ref.INVALID:
            assert np.isnan(margin[s])
            continue
        print(f"{ref.case_id(case)} stream {s} {name}: lag {int(base['lag'][s])}, lag_peak {float(base['lag_peak'][s]):+.4f}, argmax margin "
              f"{margin[s]:.3g}, mean coherence {float(base['mean_coherence'][s]):.4f}")
        if name in ref.NO_LAG or name == "tone, measured zero":
            continue
        assert margin[s] >= 1e-3 and base["lag"][s] == ref.true_lag(name, p), (name, margin[s])
        assert margin[s] >= 0.1  # (0.37 was the smallest when the cases were written)
    overall = 0.0
    for o in ref.ORDERS[1:]:
        other = ref.xfer(x, w, cap, sr, lag=base["lag"].tolist(), wpos=wpos, order=o)
        bad = ref.mismatches(other, base, float_tol=1e-9)
        figures = ref.worst(other, base)
        overall = max(overall, max(figures.values()))
        assert not bad, (o, bad[:4])
    print(f"{ref.case_id(case)}: the four orders agree to {overall:.3g} over every field")


@pytest.mark.parametrize("case", [c for c in ms.CASES if c.channels == 2], ids=lambda c: c.name)
def test_the_staggered_script_meets_the_margin(case):
    """every valid stream of every read of the staggered batch (test_gpu_xfer.py plays the same script into the device): the argmax
    margin is at least 1e-3, and the counters all differ at the end"""
    rings = ms.Rings.of(case)
    least = []

    def on_read(i, tag):
        hist, wpos = rings.histories(), rings.counter.astype(np.int64)
        m = [ref.analyse(hist[s], case.W, case.ring_cap, case.sr, wpos=wpos[s])[1].get("margin") for s in range(ms.STREAMS)]
        print(f"{case.name} {tag}: margins {[None if v is None else round(v, 3) for v in m]}")
        least.extend(v for v in m if v is not None)

    reads = ms.replay(ref.stagger_script(case), rings, (), on_read)
    assert reads >= 5 and min(least) >= 1e-3 and len(set(rings.counter.tolist())) == ms.STREAMS


def test_xfer_kernel_has_no_scratch():
    res = kernel_usage("wf_hip_measure", "xfer_read_kernel")
    assert len(res) == 1, res
    for name, r in res.items():
        print(name, r)
        assert r.get("ScratchSize [bytes/lane]") == 0 and r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
        assert r.get("LDS Size [bytes/block]") <= 2048, (name, r)  # the cross-wave hand-overs; the transforms' LDS is dynamic
    src = (CSRC / "wf_xfer.hpp").read_text()
    assert "asm" not in src and "atomic" not in src.replace("no atomics", "")
    # at the cap a region, half a region and one slot: 48 KB and 16 bytes, what a workgroup gets without asking
    assert (binding.XFER_MAX_WINDOW + binding.XFER_MAX_WINDOW // 2 + 1) * 16 == 48 * 1024 + 16 < 64 * 1024
