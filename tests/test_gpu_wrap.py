"""Every reader of the 32-bit sample counters (d_wpos, d_rend, d_mend, d_cend) and every push path that advances them, carried
across the 2^32 wrap a day of audio at 48 kHz brings: tests/wrap_child.py ages one of two twin handles to just below 2^32
(wf_hip_debug_age) and walks both through the wrap in small hops, with an A/V-sync delay -- so that WF_STREAM_WRAPPED, which alone
tells "wrapped" from "not enough audio for the delay yet", decides what the aged handle shows.  The twins must agree bit for bit at
every tick.  One child process per kind, on the development build of the library (the release library has no test aids)."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

# fft sizes of spectrum_delay_<fft>, by the kernel family each is there for (wrap_child.GEOMETRIES confirms it from kernel_name())
GEOMETRIES = (512, 800, 1120, 2096, 4096, 8192, 32768, 65536, 16400, 32000)
KINDS = [(f"spectrum_delay_{n}", 60) for n in GEOMETRIES] + [
    ("push_paths", 120),  # (seven twin pairs, and torch for the device-memory path)
    ("reset_after_wrap", 60), ("meter_delay", 60), ("rms_feed", 60), ("waveform", 60), ("measure", 90)]


@pytest.mark.parametrize("kind,limit", KINDS, ids=[k for k, _ in KINDS])
def test_wrap(kind, limit):
    env = dict(os.environ, WF_HIP_LIB=str(ROOT / "waveform_amd" / "libwaveform_hip_dev.so"))
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "wrap_child.py"), kind], capture_output=True, text=True, timeout=limit, env=env)
    assert r.returncode == 0 and "wrapped ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
