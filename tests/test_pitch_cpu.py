"""Pitch (WF_HIP_OUT_PITCH) without a device: the structured dtype against the C layout, the appended output number,
the float64 reference (tests/pitch_ref.py) against analytic cases, every seeded input of the GPU tests shown to be well
conditioned for the reference alone, and a gfx950 compile of the read kernel with no scratch."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from waveform_amd import binding
import pitch_cases as cases
import pitch_ref as ref
from signal_ref import History
from kernel_usage import kernel_usage

ROOT = Path(__file__).resolve().parents[1]
SR = cases.SR


def test_pitch_dtype_matches_the_c_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wf_hip.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %d %d %d", sizeof(wf_hip_pitch), (int)WF_HIP_OUT_PITCH, (int)WF_HIP_PITCH_MIN_LAG, (int)WF_HIP_PITCH_MAX_WINDOW);\n'
                   '  printf(" %zu %zu %zu %zu", offsetof(wf_hip_pitch, hz), offsetof(wf_hip_pitch, clarity), offsetof(wf_hip_pitch, lag),\n'
                   "         offsetof(wf_hip_pitch, voiced));\n"
                   '  printf(" %.17g", (double)WF_HIP_PITCH_THRESHOLD);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    got, threshold = [int(v) for v in out[:-1]], float(out[-1])
    dt = binding.PITCH_DTYPE
    assert got == [dt.itemsize, binding.OUT_PITCH, binding.PITCH_MIN_LAG, binding.PITCH_MAX_WINDOW] \
        + [dt.fields[n][1] for n in ("hz", "clarity", "lag", "voiced")]
    assert dt.itemsize == 16 and dt == ref.PITCH_DTYPE
    assert threshold == 0.15 == binding.PITCH_THRESHOLD == ref.THRESHOLD
    assert (binding.PITCH_MIN_LAG, binding.PITCH_MAX_WINDOW) == (ref.MIN_LAG, ref.MAX_WINDOW) == (8, 4096)


def test_pitch_output_is_appended_after_signal():
    assert binding.OUT_PITCH == binding.OUT_SIGNAL + 1 == 13  # the existing outputs keep their numbers


def _one(x, order=0):
    """the reference of one mono stream: x float32 [P]"""
    return ref.pitch(np.asarray(x, np.float32)[None, None], SR, order)[0]


def test_reference_reads_sines_close_to_the_truth():
    """Sines at 55, 110, 440, 997.3 and 3000 Hz, 48 kHz, P = 4096, amplitude 0.5.  How close is a property of YIN's parabola
    through d', which reads high at short lags.  Measured relative errors of the reference (both orders alike):
    55 Hz 3.47e-7 (lag 873), 110 Hz 1.32e-6 (436), 440 Hz 3.92e-5 (109), 997.3 Hz 2.10e-4 (48), 3000 Hz 1.89e-3 (16).
    Each is asserted with a factor 2 over that."""
    measured = {55.0: 3.47e-7, 110.0: 1.32e-6, 440.0: 3.92e-5, 997.3: 2.10e-4, 3000.0: 1.89e-3}
    lags = {55.0: 873, 110.0: 436, 440.0: 109, 997.3: 48, 3000.0: 16}
    for hz in cases.SINES:
        for order in (0, 1):
            r = _one(cases.sine(hz, 4096), order)
            err = abs(float(r["hz"]) - hz) / hz
            print(f"sine {hz} Hz order {order}: hz {r['hz']:.6f} rel err {err:.3e} clarity {r['clarity']:.7f} lag {r['lag']}")
            assert r["voiced"] == 1 and r["clarity"] > 0.99 and r["lag"] == lags[hz], (hz, r)
            assert err <= 2 * measured[hz], (hz, err)
    # a period of whole frames is found exactly: d(16) is 0, not a rounding residue
    r = _one(cases.sine(3000.0, 4096))
    assert r["clarity"] == 1.0
    assert _one(cases.sine(3000.0, 128))["lag"] == 16  # the shortest window of a spectrum batch


def test_reference_on_unpitched_and_degenerate_input():
    P = 4096
    c = cases.analytic(P)
    r = _one(c["missing_fundamental"])
    assert r["voiced"] == 1 and r["lag"] == 218 and abs(float(r["hz"]) - 220.0) < 0.01 and r["clarity"] > 0.999, r
    r = _one(c["noise"])
    assert r["voiced"] == 0 and r["clarity"] < 0.5 and ref.MIN_LAG <= r["lag"] <= P // 2 - 1, r
    zero = np.zeros(1, ref.PITCH_DTYPE)[0]
    assert _one(c["silence"]) == zero
    for order in (0, 1):
        assert _one(c["constant"], order) == zero  # direct sums in one order of j: d is exactly 0
    x = cases.sine(440.0, P)
    assert ref.pitch(np.stack([x, -x])[None], SR)[0] == zero  # l = -r mixes to nothing
    both = ref.pitch(np.stack([x, x])[None], SR)[0]
    assert both == _one(x)  # (l + l) / 2 is l


def test_window_follows_the_fft_size():
    assert [ref.window_frames(w) for w in (128, 800, 4096, 4112, 16384, 65536)] == [128, 800, 4096, 4096, 4096, 4096]
    h = History(1, 1, ref.window_frames(16384))
    x = cases.sine(440.0, 16384)
    h.push(x[None, None])
    assert ref.pitch(h.window(), SR)[0] == _one(x[-4096:])  # the newest 4096 frames


def test_ulps():
    one = np.float32(1.0)
    assert ref.ulps(one, np.nextafter(one, np.float32(2))) == 1 and ref.ulps(np.float32(0.0), np.float32(-0.0)) == 0
    assert ref.ulps(np.float32(1e-45), np.float32(-1e-45)) == 2


def test_analytic_and_headline_inputs_are_well_conditioned():
    P = 4096
    c = cases.analytic(P)
    w = np.stack([v[None] for v in c.values()])
    _, well = ref.evaluate(w, SR)
    assert well.all(), [k for k, ok in zip(c, well) if not ok]
    from tools import synth
    idx = list(range(32)) + list(range(4096 - 32, 4096))
    w = np.concatenate([synth.block(cases.SEED, s, 1, 2, 1601, P) for s in idx])  # what test_headline_shape compares
    _, well = ref.evaluate(w, SR)
    assert well.all(), np.nonzero(~well)[0]


@pytest.mark.parametrize("fft,cap,kw,ring", cases.FUZZ, ids=cases.FUZZ_IDS)
def test_fuzz_inputs_are_well_conditioned(fft, cap, kw, ring):
    """every read of every fuzz script the GPU test replays: the two orders of the reference agree, so the GPU test's count of
    skipped streams is 0 before a device is involved"""
    hist = History(cases.FUZZ_STREAMS, cap, ref.window_frames(fft))
    bad = []

    def on_read(i):
        want, well = ref.evaluate(hist.window(), SR)
        bad.extend((i, int(s)) for s in np.nonzero(~well)[0])
    reads = cases.replay(cases.fuzz_script(fft, cap, kw, ring), hist, on_read)
    assert reads == 9 and not bad, bad


def test_pitch_kernel_has_no_scratch():
    res = kernel_usage("wf_hip_measure", "pitch_read_kernel")
    assert len(res) == 2, res  # mono and stereo capture
    for name, r in res.items():
        assert r.get("ScratchSize [bytes/lane]") == 0 and r.get("VGPRs Spill") == 0, (name, r)
        assert r.get("Occupancy [waves/SIMD]") == 4, (name, r)  # WF_PITCH_OCC: four workgroups in a CU's LDS
