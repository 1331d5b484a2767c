"""child process of tests/test_gpu_wire.py::test_device_tensor_at_every_byte_offset (needs a GPU): wf_hip_push_pcm reading the
wire formats from torch tensors on the handle's device in place.  s24_be planar with the data pointer advanced by 0..15 bytes
(a packed 24-bit packet needs no alignment), every other wire format once, and s16_be at an odd address refused.  A process of
its own because torch brings its own HIP runtime and has to be imported before libwaveform_hip.so is loaded."""
import sys
from pathlib import Path

import numpy as np
import torch  # before libwaveform_hip.so: one HIP runtime per process

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import waveform_amd as wf  # noqa: E402
from wire_convert import captured, random_packet  # noqa: E402
from test_gpu_pcm import _assert_same, _cfg  # noqa: E402

torch.cuda.set_device(0)
streams, frames = 6, 801


def at_offset(pkt, offset):
    """the packet's bytes in device memory, `offset` bytes past an allocation's start (torch allocations are 256-B aligned)"""
    buf = torch.zeros(pkt.size + 16, dtype=torch.uint8, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    d = buf[offset:offset + pkt.size]
    d.copy_(torch.from_numpy(pkt.reshape(-1)))
    d = d.view(pkt.shape)
    torch.cuda.synchronize()
    assert d.is_contiguous() and d.data_ptr() % 16 == offset
    return d, buf


rng = np.random.default_rng(7)
with wf.SpectrumBatch(_cfg(2), streams) as b, wf.SpectrumBatch(_cfg(2), streams) as twin:
    for offset in range(16):
        pkt = random_packet(rng, "s24_be", streams, 2, frames, False)
        d, buf = at_offset(pkt, offset)
        b.push_pcm(d, interleaved=False, wire="s24_be")
        twin.push_audio(captured(pkt, "s24_be", False, 0, 2))
        b.tick()
        twin.tick()
        b.sync()  # the tensor may go
        _assert_same(b, twin, f"device s24_be planar at +{offset}")
    print("s24_be planar at +0..15: ok", flush=True)

CASES = [("s24", True, (6, 2, 0), 5), ("s24", False, (6, 1, 3), 1), ("s16_be", True, (6, 2, 0), 2), ("s16_be", False, (6, 1, 5), 6),
         ("ulaw", True, (2, 2, 0), 7), ("alaw", False, (6, 1, 3), 9), ("s24_be", True, (1, 1, 0), 11)]
for wire, interleaved, (channels, cap, base), offset in CASES:
    with wf.SpectrumBatch(_cfg(cap), streams) as b, wf.SpectrumBatch(_cfg(cap), streams) as twin:
        for t in range(3):
            pkt = random_packet(rng, wire, streams, channels, frames, interleaved)
            d, buf = at_offset(pkt, offset)
            b.push_pcm(d, interleaved=interleaved, channel_base=base, wire=wire)
            twin.push_audio(captured(pkt, wire, interleaved, base, cap))
            b.tick()
            twin.tick()
            b.sync()
            _assert_same(b, twin, f"device {wire} {'interleaved' if interleaved else 'planar'} step {t}")
        if wire == "s16_be":  # 2-B samples need a 2-B aligned address; the handle stays usable
            d, buf = at_offset(pkt, 3)
            try:
                b.push_pcm(d, interleaved=interleaved, channel_base=base, wire=wire)
            except wf.WfHipError as e:
                assert e.code == -1, e
            else:
                raise AssertionError("s16_be device data at an odd address was accepted")
            b.tick()
            twin.tick()
            b.sync()
            _assert_same(b, twin, "after the refused odd address")
    print(f"{wire} {'interleaved' if interleaved else 'planar'} {channels}ch base {base} at +{offset}: ok", flush=True)
print("wire device ok", flush=True)
