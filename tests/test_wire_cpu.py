"""The wire formats of wf_hip_push_pcm (packed 24-bit, big-endian, G.711) without a device: the header's enum against the
binding, the numpy restatement of the conversions at their edges, the format facts of wf_pcm_formats.hpp compiled on their own
(plain and under the sanitizers), the exports, argument checking on a NULL handle, and a gfx950 compile of every instantiation
of the append kernel with no scratch and no spills."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import waveform_amd as wf
from waveform_amd import binding
from pcm_convert import to_float
from wire_convert import BYTES, WIRES, captured, decode, decode_int, random_packet
from kernel_usage import kernel_usage

ROOT = Path(__file__).resolve().parents[1]


def _byte(v):
    return np.array([[v]], np.uint8)


def test_header_values_match_the_binding(tmp_path):
    names = [w.upper() for w in binding.WIRE_FORMAT]
    src = tmp_path / "wire.c"
    src.write_text('#include <stdio.h>\n#include "wf_hip.h"\nint main(void) {\n'
                   + "".join(f'  printf("%d %d ", (int)WF_HIP_WIRE_{n}, (int)WF_HIP_WIRE_{n}_PLANAR);\n' for n in names)
                   + '  printf("%zu %d", sizeof(wf_hip_pcm), (int)WF_HIP_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "wire"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for v in binding.WIRE_FORMAT.values():
        want += [v, v + 8]
    assert got == want + [C.sizeof(binding.Pcm), 13]
    assert binding.WIRE_FORMAT == {"s24": 16, "s24_be": 17, "s16_be": 18, "ulaw": 19, "alaw": 20}
    assert binding.WIRE_BYTES == BYTES and tuple(binding.WIRE_FORMAT) == WIRES
    assert C.sizeof(binding.Pcm) == 40 and [n for n, _ in binding.Pcm._fields_] == ["data", "format", "channels", "channel_base", "frames",
                                                                                    "frames_per_stream", "memory", "slot"]
    assert list(binding.PCM_FORMAT.values()) == [1, 2, 3, 4]


def test_g711_anchors_and_tables():
    ulaw = {0x00: -32124, 0x80: 32124, 0xFF: 0, 0x7F: 0, 0xFE: 8}
    alaw = {0xD5: 8, 0x55: -8, 0xAA: 32256, 0x2A: -32256}
    for code, v in ulaw.items():
        assert decode_int(_byte(code), "ulaw")[0] == v, hex(code)
    for code, v in alaw.items():
        assert decode_int(_byte(code), "alaw")[0] == v, hex(code)
    codes = np.arange(256, dtype=np.uint8)[:, None]
    u, a = decode_int(codes, "ulaw"), decode_int(codes, "alaw")
    assert len(np.unique(u)) == 255 and len(np.unique(a)) == 256
    # odd symmetry: flipping the sign bit of the code negates the value (mu-law's two zero codes both read 0)
    assert np.array_equal(u[:128], -u[128:]) and np.array_equal(a[:128], -a[128:])
    assert np.flatnonzero(u == 0).tolist() == [0x7F, 0xFF] and not np.any(a == 0)
    fu = decode(codes, "ulaw")
    assert fu.dtype == np.float32 and fu[[0x7F, 0xFF]].view(np.uint32).tolist() == [0, 0]  # +0.0f, both
    assert np.array_equal(fu.astype(np.float64) * 2.0 ** 15, u) and np.array_equal(decode(codes, "alaw").astype(np.float64) * 2.0 ** 15, a)
    assert np.abs(u).max() == 32124 and np.abs(a).max() == 32256


def test_s24_and_s16_be_edges():
    vals = np.array([-2 ** 23, -1, 0, 1, 2 ** 23 - 1], np.int64)
    le = np.stack([(vals >> s) & 0xFF for s in (0, 8, 16)], axis=-1).astype(np.uint8)
    assert decode_int(le, "s24").tolist() == vals.tolist()
    f = decode(le, "s24")
    assert f.dtype == np.float32 and f.tolist() == [-1.0, -2.0 ** -23, 0.0, 2.0 ** -23, float.fromhex("0x1.fffffcp-1")]
    rng = np.random.default_rng(1)
    codes = rng.integers(0, 256, (100000, 3), dtype=np.uint8)
    want = codes[:, 0].astype(np.int64) | codes[:, 1].astype(np.int64) << 8 | codes[:, 2].astype(np.int64) << 16
    want = np.where(want >= 2 ** 23, want - 2 ** 24, want)
    assert np.array_equal(decode(codes, "s24").astype(np.float64) * 2.0 ** 23, want)  # every 24-bit integer is a float32
    assert np.array_equal(decode(codes[:, ::-1], "s24_be").view(np.uint32), decode(codes, "s24").view(np.uint32))
    be = rng.integers(0, 256, (100000, 2), dtype=np.uint8)
    be[:4] = [[0x80, 0x00], [0x7F, 0xFF], [0xFF, 0xFF], [0x00, 0x01]]
    swapped = np.ascontiguousarray(be[:, ::-1]).view("<i2")[:, 0]
    assert swapped[:4].tolist() == [-32768, 32767, -1, 1]
    assert np.array_equal(decode(be, "s16_be").view(np.uint32), to_float(swapped.astype(np.int16)).view(np.uint32))


def test_random_packet_and_channel_pick():
    rng = np.random.default_rng(2)
    for wire in WIRES:
        pkt = random_packet(rng, wire, 2, 6, 50, True)
        assert pkt.dtype == np.uint8 and pkt.shape == (2, 50, 6, BYTES[wire])
        ints = decode_int(pkt, wire)
        if wire in ("s24", "s24_be"):
            assert ints.min() == -2 ** 23 and ints.max() == 2 ** 23 - 1
        elif wire in ("ulaw", "alaw"):
            assert len(np.unique(pkt)) == 256
        got = captured(pkt, wire, True, 3, 2)
        assert got.shape == (2, 2, 50) and got.dtype == np.float32
        assert np.array_equal(got[1, 1], decode(pkt[1, :, 4], wire))
        planar = np.ascontiguousarray(pkt.transpose(0, 2, 1, 3))
        assert np.array_equal(captured(planar, wire, False, 3, 2), got)
    assert random_packet(rng, "s24", 1, 1, 1, False).shape == (1, 1, 1, 3)  # fewer samples than edges


FORMATS_MAIN = """
#include <cstdio>
#include "wf_pcm_formats.hpp"
int main()
{
    for(uint32_t f = 0; f <= 40; ++f)
        std::printf("%u %d %u %d %u %u\\n", f, (int)wf::pcm_format_valid(f), wf::pcm_sample_bytes(f), (int)wf::pcm_is_interleaved(f),
                    wf::pcm_device_alignment(f), wf::pcm_sample_kind(f));
    return 0;
}
"""


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_format_facts_header_on_its_own(tmp_path, flags):
    src = tmp_path / "formats_main.cpp"
    src.write_text(FORMATS_MAIN)
    exe = tmp_path / "formats_main"
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", str(ROOT / "include"),
                    "-I", str(ROOT / "waveform_amd" / "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    # (valid, bytes, interleaved, alignment, kind) by format value; everything else is no format
    table = {}
    for kind, (nbytes, align) in {1: (1, 1), 2: (2, 2), 3: (4, 4), 4: (4, 4)}.items():
        table[kind] = (1, nbytes, 1, align, kind)
        table[kind + 4] = (1, nbytes, 0, align, kind)
    for wire, kind in binding.WIRE_FORMAT.items():
        align = 2 if wire == "s16_be" else 1
        table[kind] = (1, BYTES[wire], 1, align, kind)
        table[kind + 8] = (1, BYTES[wire], 0, align, kind)
    assert sorted(table) == list(range(1, 9)) + list(range(16, 21)) + list(range(24, 29))
    assert got == [(f,) + table.get(f, (0, 0, 0, 0, 0)) for f in range(41)]
    for f in range(1, 9):  # what the code computed before the header existed
        base = (f - 1) & 3
        assert got[f][2] == (1 if base == 0 else 2 if base == 1 else 4) and got[f][3] == int(f <= 4) and got[f][4] == got[f][2]


def test_wire_kernel_instantiations_have_no_scratch_and_no_spills():
    wire = kernel_usage("wf_hip", "ring_push_wire_kernel")
    assert len(wire) == 20, sorted(wire)  # 5 sample types x interleaved / planar x ragged or not
    for name, r in wire.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        assert r["LDS Size [bytes/block]"] == 2 * (8192 + 32), (name, r)
    pcm = kernel_usage("wf_hip", "ring_push_pcm_kernel")
    assert len(pcm) == 16 and not set(pcm) & set(wire), sorted(pcm)


def test_null_handle_refused_exports_and_abi_unchanged():
    L = wf.lib()
    pkt = np.zeros((1, 4, 2, 3), np.uint8)
    for fmt in (16, 20, 24, 28):
        pcm = binding.Pcm(data=pkt.ctypes.data, format=fmt, channels=2, channel_base=0, frames=4, memory=binding.PCM_HOST)
        assert L.wf_hip_push_pcm(None, 0, 1, C.byref(pcm)) == -1  # WF_HIP_ERR_INVALID, no device needed
        assert L.wf_hip_multi_push_pcm(None, 0, 1, C.byref(pcm)) == -1
    assert L.wf_hip_abi_version() == 13
    so = ROOT / "waveform_amd" / "libwaveform_hip.so"
    nm = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line and line.split()[-1].startswith("wf_hip_")}
    assert len(exported) == 75, sorted(exported)  # no new entry point


def test_binding_builds_the_descriptor_and_refuses_wrong_shapes():
    pkt = np.zeros((3, 10, 2, 3), np.uint8)
    pcm, count, _ = binding._pcm(pkt, True, 0, None, None, "s24")
    assert (pcm.format, pcm.channels, pcm.frames, count, pcm.memory) == (16, 2, 10, 3, binding.PCM_HOST)
    pcm, count, _ = binding._pcm(pkt, False, 1, None, None, "s24_be")
    assert (pcm.format, pcm.channels, pcm.frames, pcm.channel_base) == (25, 10, 2, 1)
    assert binding._pcm(np.zeros((3, 10, 2, 1), np.uint8), True, 0, None, None, "alaw")[0].format == 20
    for bad, wire in [(np.zeros((3, 10, 2, 2), np.uint8), "s24"), (np.zeros((3, 10, 6), np.uint8), "s24"), (np.zeros((3, 10, 2, 3), np.int8), "s24"),
                      (np.zeros((3, 10, 2), np.uint8), "ulaw"), (np.zeros((3, 10, 2, 2), np.int16), "s16_be"), (pkt, "s20")]:
        with pytest.raises(ValueError):
            binding._pcm(bad, True, 0, None, None, wire)
    assert binding._pcm(np.zeros((3, 10, 2), np.uint8), True, 0, None, None)[0].format == 1  # without `wire`, as before
