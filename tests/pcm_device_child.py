"""child process of tests/test_gpu_pcm.py::test_device_tensor (needs a GPU): wf_hip_push_pcm reading torch tensors on the
handle's device in place.  A process of its own because torch brings its own HIP runtime and has to be imported before
libwaveform_hip.so is loaded."""
import sys
from pathlib import Path

import numpy as np
import torch  # before libwaveform_hip.so: one HIP runtime per process

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import waveform_amd as wf  # noqa: E402
from pcm_convert import captured, random_packet  # noqa: E402
from test_gpu_pcm import _assert_same, _cfg  # noqa: E402

torch.cuda.set_device(0)
CASES = [(np.int16, True, (6, 2, 0)), (np.uint8, False, (6, 1, 3)), (np.int32, False, (2, 2, 0)), (np.float32, True, (1, 1, 0)),
         (np.int16, False, (6, 1, 5))]
for dtype, interleaved, (channels, cap, base) in CASES:
    streams, frames = 6, 801
    rng = np.random.default_rng(7)
    with wf.SpectrumBatch(_cfg(cap), streams) as b, wf.SpectrumBatch(_cfg(cap), streams) as twin:
        for t in range(4):
            pkt = random_packet(rng, dtype, streams, channels, frames, interleaved)
            d = torch.from_numpy(pkt).to("cuda:0")
            torch.cuda.synchronize()
            b.push_pcm(d, interleaved=interleaved, channel_base=base)
            twin.push_audio(captured(pkt, interleaved, base, cap))
            b.tick()
            twin.tick()
            b.sync()  # the tensor may go
            _assert_same(b, twin, f"device {np.dtype(dtype)} {'interleaved' if interleaved else 'planar'} step {t}")
    print(f"{np.dtype(dtype)} {'interleaved' if interleaved else 'planar'} {channels}ch base {base}: ok", flush=True)
print("pcm device ok", flush=True)
