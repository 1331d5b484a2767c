"""Every tick family on several lanes, at the slice boundaries.

wf_hip_tick cuts a spectrum batch into up to four slices of streams, each on a HIP stream of its own, and on a lane every kernel
of the tick adds stream_base to whatever it indexes: the tick kernel's clamped spare spectrum and its pairs of spectra per
workgroup, the rows / columns / epilogue kernels beyond a CU's LDS, big_outputs_kernel, vertex_fill_kernel, the verdict words, the
per-lane copies of the bars mirrors.  The lanes rule fires from thousands of streams on, so the small batches of the other modules
run on one lane.  tests/lanes_child.py plays the mixed batches of tests/test_gpu_mixed_states.py on the development build of the
library with WF_HIP_LANES = 1, 2, 3 and 4 (above 16384 samples: 1 and 4) -- slices of one and two streams with odd bases --, demands the one-lane bits from
every lane count and holds the four-lane records against every stream's own reference; it says in its docstring what else it
asserts.  One child process per case, so that a failure names its case."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

import lanes_child

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
LIMIT = 120  # seconds, as the larger children of tests/test_gpu_wrap.py (a case takes about a second)


@pytest.mark.parametrize("kind", lanes_child.KINDS)
def test_lanes(kind):
    env = dict(os.environ, WF_HIP_LIB=str(ROOT / "waveform_amd" / "libwaveform_hip_dev.so"))
    env.pop("WF_HIP_LANES", None)
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "lanes_child.py"), kind], capture_output=True, text=True, timeout=LIMIT, env=env)
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith("TOTALS")))
    assert r.returncode == 0 and "lanes ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
