"""The compiler's resource-usage remarks of one translation unit of the library, for the CPU tests that pin a kernel's scratch,
spills, LDS and occupancy.  The remarks come from the Makefile's own `usage-<unit>` target, so the flags are the ones the
library is built with; a unit is compiled once per process however many tests look at it."""
from __future__ import annotations

import functools
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


@functools.lru_cache(maxsize=None)
def _remarks(unit: str) -> dict | None:
    hipcc = Path("/opt/rocm/bin/hipcc")
    if not hipcc.exists():
        found = shutil.which("hipcc")
        if found is None:
            return None
        hipcc = Path(found)
    r = subprocess.run(["make", "-s", "-C", str(ROOT / "waveform_amd" / "csrc"), f"usage-{unit}", f"HIPCC={hipcc}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    res, name = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        m = re.search(r"remark:\s+([^:]+): (\d+) \[", line)
        if m and name:
            res[name][m.group(1)] = int(m.group(2))
    return res


def kernel_usage(unit: str, kernel: str) -> dict:
    """{mangled name: {field: value}} of the kernels of `unit` (a .hip file's stem) whose name contains `kernel`, the fields named
    as the compiler prints them ("ScratchSize [bytes/lane]", "VGPRs Spill" ...).  Skips the calling test where there is no hipcc."""
    res = _remarks(unit)
    if res is None:
        pytest.skip("hipcc not found")
    return {name: dict(fields) for name, fields in res.items() if kernel in name}
