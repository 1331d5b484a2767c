"""The plugin binding (host/wav_source_hip.cpp) without a device and without a sanitizer: a behaviour record.

The reference harness (oracle/_ref/libwfref.so) runs WAVSourceHIP over the plain build of the host-only stand-in for
libwaveform_hip.so (tests/mock/mock_wf_hip.cpp -> build/libwfhip_mock_plain.so).  The stand-in's rows are an exact integer
function of the audio a stream received since its reset, and it keeps a running hash over every call the binding makes: entry
point, scalar arguments, the contents of every array (staged audio, state masks, delays, timestamps, RMS values, squared peaks,
tick parameters), never an address.  Every script below plays ten sources over groups of four -- stalls, hide / show, a capture
timeout, a source ticked twice in a frame, a source destroyed and a new one taking its slot, update() into another group and
back into the same one -- and records
  trace      the stand-in's call hash at the end,
  digest     SHA-256 over every observation (rows, silent flag, display values) of the sources still on the device path -- after
             a fallback the rows are the reference's FFTW results, which need not be the same bits on another machine,
  using_hip  who is still on the device path, and
  fallbacks  the ticks handed to the CPU class.
These are compared for equality with tests/golden/host_groups_mock.json: what the binding hands to the library, and what it
hands back to the reference's members, is pinned call by call.  A restructuring of the binding leaves the file alone.

Every script is a plain child process (the binding loads its library once per process and reads its environment at create):
  python tests/test_host_groups_mock_cpu.py --play NAME     one script, one JSON line
  python tests/test_host_groups_mock_cpu.py --record        rewrites the fixture from the binding as it is"""
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
MOCK = ROOT / "build" / "libwfhip_mock_plain.so"
REF = ROOT / "oracle" / "_ref" / "libwfref.so"
FIXTURE = ROOT / "tests" / "golden" / "host_groups_mock.json"

SOURCES, CAPACITY, FRAMES = 10, 4, 24

# display kind -> (wf_config overrides, the update() that moves a member into another group, audio sync offset in ms, environment)
KINDS = {
    "spectrum_rows": (dict(fft_size=1024, stereo=1, slope=1.0, bars=1, interp_mode=1), dict(fft_size=2048), 0, {"WF_HIP_RENDER": "0"}),
    "spectrum_bars": (dict(fft_size=1024, stereo=1, slope=1.0, bars=1, interp_mode=1, vertices=1), dict(fft_size=2048), 0, {}),
    "spectrum_stepped": (dict(fft_size=1024, stereo=0, bars=1, interp_mode=2, channel_spacing=6, vertices=3), dict(fft_size=512), 0, {}),
    "spectrum_curve": (dict(fft_size=1024, stereo=1, curve=1, interp_mode=2, mirror_freq_axis=1, width=600, vertices=1), dict(fft_size=2048), 0, {}),
    "spectrum_sync": (dict(fft_size=1024, stereo=1, capture_channels=1), dict(fft_size=2048), 20, {}),
    "meter": (dict(meter=1, meter_ms=20), dict(meter_ms=30), 0, {}),
    "meter_sync": (dict(meter=1, meter_ms=50, capture_channels=1), dict(meter_ms=30), 15, {}),
    "waveform": (dict(waveform=1, stereo=1, width=400), dict(width=320), 10, {}),
    "normalize": (dict(fft_size=1024, stereo=1, normalize_volume=1), dict(fft_size=2048), 0, {}),
    "normalize_feed": (dict(fft_size=1024, stereo=1, normalize_volume=1, bars=1, vertices=1), dict(fft_size=2048), 5, {"WF_MOCK_RMS_FEED": "1"}),
    "waveform_normalize": (dict(waveform=1, stereo=1, width=400, normalize_volume=1), dict(width=320), 10, {}),
}
# a tick of the library that fails: in batched mode a whole group fails and its members fall back one by one, in synchronous mode
# one source does (the N-th wf_hip_tick of the process, chosen to fall in the middle of the script)
FAILING = {
    "spectrum_bars": {"batched": 20, "synchronous": 70},
    "meter": {"batched": 20, "synchronous": 70},
    "waveform": {"batched": 20, "synchronous": 70},
    "normalize_feed": {"batched": 20},
}
SCRIPTS = {}
for _kind in KINDS:
    for _mode in ("batched", "synchronous"):
        SCRIPTS[f"{_kind}-{_mode}"] = (_kind, _mode, None)
for _kind, _modes in FAILING.items():
    for _mode, _nth in _modes.items():
        SCRIPTS[f"{_kind}-{_mode}-failing_tick"] = (_kind, _mode, _nth)


def _environment(name):
    kind, mode, nth = SCRIPTS[name]
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD" and not k.startswith(("WF_HIP_", "WF_MOCK_"))}
    env.update(KINDS[kind][3], WF_HIP_LIBRARY=str(MOCK), WF_HIP_BATCHED="1" if mode == "batched" else "0", WF_HIP_BATCH_CAPACITY=str(CAPACITY))
    if nth is not None:
        env["WF_MOCK_FAIL_TICK"] = str(nth)
    return env


def _run(name):
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--play", name], capture_output=True, text=True, timeout=120,
                       env=_environment(name), cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def golden():
    if not REF.exists():
        pytest.skip(f"{REF} not built")
    if not MOCK.exists():
        subprocess.run(["make", "-C", str(ROOT / "tests" / "mock"), str(Path("..") / ".." / "build" / MOCK.name)], capture_output=True)
    if not MOCK.exists():
        pytest.skip(f"{MOCK} not built")
    return json.loads(FIXTURE.read_text())


@pytest.mark.parametrize("name", list(SCRIPTS))
def test_the_binding_makes_the_recorded_calls_and_shows_the_recorded_frames(name, golden):
    got = _run(name)
    assert got == golden[name], f"{name}: the binding's calls into the library (trace) or what its sources show (digest) changed"
    failing = SCRIPTS[name][2] is not None
    assert (got["fallbacks"] > 0) == failing and all(got["using_hip"]) != failing, got


def test_the_scripts_and_the_fixture_name_the_same_cases(golden):
    assert sorted(golden) == sorted(SCRIPTS)


# ---- the child -------------------------------------------------------------------------------------------------------------
def _play(name):
    import ctypes as C
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    import numpy as np
    import scenarios
    from oracle import wfref
    from tools import synth

    os.environ.update(_environment(name))  # (as _run sets it: the script also plays when started by hand)
    kind, _, _ = SCRIPTS[name]
    overrides, elsewhere, sync_ms, _ = KINDS[kind]
    cfg = scenarios.make_config(overrides)
    mock = C.CDLL(os.environ["WF_HIP_LIBRARY"])  # the library instance the binding dlopen()s
    mock.wf_hip_mock_trace.restype = C.c_uint64
    digest = hashlib.sha256()

    def create():
        be = scenarios.RefBackend(cfg, isa="hip")
        if sync_ms:
            be.set_sync_ms(sync_ms)  # re-runs update(): the source leaves its slot and takes it again
        assert be.src.using_hip, "the source did not reach the stand-in library"
        return be

    def observe(be, tag):
        rec = be.observe()
        if not be.src.using_hip:
            return  # on the CPU class: FFTW's results
        digest.update(tag.encode())
        for key in sorted(rec):
            parts = rec[key] if isinstance(rec[key], list) else [rec[key]]
            digest.update(key.encode())
            for v in parts:
                digest.update(b"none" if v is None else np.ascontiguousarray(v).tobytes())

    srcs = [create() for _ in range(SOURCES)]
    stream = list(range(300, 300 + SOURCES))
    pos = [0] * SOURCES
    for f in range(FRAMES):
        if f == 8:
            srcs[6].src.close()  # its slot is freed in the middle of the run ...
            srcs[6], stream[6], pos[6] = create(), 400, 0  # ... and taken by a new source
        if f == 12:
            srcs[4].update(elsewhere)  # another configuration: another group
        if f == 15:
            srcs[2].update({})  # the same settings: back into its own slot
        for i, be in enumerate(srcs):
            if i % 7 == 3 and f in (9, 10):
                continue  # no packet and no tick in these frames
            if i % 5 == 1 and f == 6:
                be.set_hidden(True)
            if i % 5 == 1 and f == 11:
                be.set_hidden(False)
            hop = (800, 441, 1024, 960)[i % 4] if f % 3 != 2 or i % 2 else 0  # some frames bring no packet at all
            if i % 11 == 4 and f == 14:
                be.timeout()
            elif hop:
                a = synth.block(scenarios.SEED, stream[i], 1, 2, pos[i], hop)[0][: be.capture_channels] * np.float32(1.0 if i % 3 else 0.05)
                pos[i] += hop
                be.push(a, muted=(i == 8 and f == 16))
            be.tick(1.0 / 60.0)
            if i == 2 and f == 5:
                be.tick(1.0 / 60.0)  # twice in one frame: its group's frame is sent off incomplete
            observe(be, f"{f}/{i}")
    using = [bool(be.src.using_hip) for be in srcs]
    fallbacks = wfref.hip_fallback_ticks()
    for be in srcs:
        be.src.close()
    print(json.dumps(dict(trace=f"{mock.wf_hip_mock_trace():016x}", digest=digest.hexdigest(), using_hip=using, fallbacks=fallbacks)))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--play"]:
        _play(sys.argv[2])
    elif sys.argv[1:] == ["--record"]:
        FIXTURE.write_text(json.dumps({name: _run(name) for name in SCRIPTS}, indent=1, sort_keys=True) + "\n")
        print(f"recorded {len(SCRIPTS)} scripts into {FIXTURE}")
    else:
        sys.exit(__doc__)
