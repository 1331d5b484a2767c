"""wf_hip_push_pcm without a device: the ctypes mirror of struct wf_hip_pcm against the C layout, the numpy restatement of the
conversions at their edges, the exports, argument checking on a NULL handle, and a gfx950 compile of every instantiation of
the append kernel with no scratch."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
from pcm_convert import to_float, captured
from kernel_usage import kernel_usage

ROOT = Path(__file__).resolve().parents[1]


def test_ctypes_pcm_matches_the_c_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wf_hip.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu", sizeof(wf_hip_pcm));\n'
                   + "".join(f'  printf(" %zu", offsetof(wf_hip_pcm, {n}));\n' for n, _ in binding.Pcm._fields_)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(binding.Pcm)] + [getattr(binding.Pcm, n).offset for n, _ in binding.Pcm._fields_]
    assert got == want


def test_format_values_are_libobs_audio_format():
    h = (ROOT / "include" / "wf_hip.h").read_text()
    names = re.search(r"typedef enum wf_hip_pcm_format \{(.*?)\}", h, re.S).group(1)
    order = re.findall(r"WF_HIP_PCM_(\w+)", names)
    assert order == ["U8", "S16", "S32", "F32", "U8_PLANAR", "S16_PLANAR", "S32_PLANAR", "F32_PLANAR"]
    assert "WF_HIP_PCM_U8 = 1" in names
    obs = (ROOT / "oracle" / "ref" / "fake_obs" / "obs-module.h").read_text()
    fmt = re.search(r"enum audio_format \{(.*?)\}", obs, re.S).group(1)
    assert [f.strip() for f in fmt.split(",")][1:] == ["AUDIO_FORMAT_U8BIT", "AUDIO_FORMAT_16BIT", "AUDIO_FORMAT_32BIT", "AUDIO_FORMAT_FLOAT",
                                                       "AUDIO_FORMAT_U8BIT_PLANAR", "AUDIO_FORMAT_16BIT_PLANAR", "AUDIO_FORMAT_32BIT_PLANAR",
                                                       "AUDIO_FORMAT_FLOAT_PLANAR"]
    assert list(binding.PCM_FORMAT.values()) == [1, 2, 3, 4]


def test_conversion_edges():
    assert to_float(np.array([0, 128, 255], np.uint8)).tolist() == [-1.0, 0.0, 127.0 / 128.0]
    assert to_float(np.array([-32768, 0, 32767], np.int16)).tolist() == [-1.0, 0.0, 32767.0 / 32768.0]
    i32 = to_float(np.array([-2 ** 31, 2 ** 31 - 1, 0, 2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1)], np.int32))
    # INT32_MAX rounds up to 2^31 (nearest even of 2^31 - 1 at 24 bits): +1.0; 2^24 + 1 is a tie, to the even 2^24
    assert i32.tolist() == [-1.0, 1.0, 0.0, 2.0 ** 24 * 2.0 ** -31, (2.0 ** 24 + 4) * 2.0 ** -31, -(2.0 ** 24) * 2.0 ** -31]
    f = np.array([np.nan, -0.0, np.inf, 1e-40], np.float32)
    assert to_float(f).view(np.uint32).tolist() == f.view(np.uint32).tolist()  # the bits, NaN and denormal included
    for x in (np.arange(256, dtype=np.uint8), np.arange(-32768, 32768, dtype=np.int16)):
        assert to_float(x).dtype == np.float32 and np.all(np.abs(to_float(x)) <= 1.0)


def test_channel_pick():
    pkt = np.arange(2 * 3 * 6, dtype=np.int16).reshape(2, 3, 6)  # interleaved [count][frames][channels]
    got = captured(pkt, True, 3, 1)
    assert got.shape == (2, 1, 3)
    assert (got * 32768).astype(np.int64)[1, 0].tolist() == [18 + 3, 24 + 3, 30 + 3]
    planar = np.ascontiguousarray(pkt.transpose(0, 2, 1))
    np.testing.assert_array_equal(captured(planar, False, 0, 2), captured(pkt, True, 0, 2))


def test_new_symbols_exported_and_null_handle_refused():
    so = ROOT / "waveform_amd" / "libwaveform_hip.so"
    nm = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert {"wf_hip_push_pcm", "wf_hip_multi_push_pcm"} <= exported
    L = wf.lib()
    pkt = np.zeros((1, 4, 2), np.int16)
    pcm = binding.Pcm(data=pkt.ctypes.data, format=2, channels=2, channel_base=0, frames=4, memory=binding.PCM_HOST)
    assert L.wf_hip_push_pcm(None, 0, 1, C.byref(pcm)) == -1  # WF_HIP_ERR_INVALID, no device needed
    assert L.wf_hip_push_pcm(None, 0, 1, None) == -1
    assert L.wf_hip_multi_push_pcm(None, 0, 1, C.byref(pcm)) == -1


def test_append_kernel_has_no_scratch():
    scratch = {name: r.get("ScratchSize [bytes/lane]") for name, r in kernel_usage("wf_hip", "ring_push_pcm_kernel").items()}
    assert len(scratch) == 16, sorted(scratch)  # 4 sample types x interleaved / planar x ragged or not
    assert all(v == 0 for v in scratch.values()), scratch
